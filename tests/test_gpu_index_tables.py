"""Every entry of the index's derived device tables against the numpy model of tests/index_tables_model.py.

The search kernels start from tables that gs_index.hip and gs_pairtab.hip derive from the text and the suffix array; several
of their fields are filters (mask bits, selected rows, filter sets, blind flags, exception flags) whose errors only lose
hits of guides nobody sampled.  Here the arrays themselves are read back (gs_debug_index_layout / gs_debug_index_array) and
compared entry by entry, exactly: no sampling, no tolerance, nothing left out but the uninitialised padding behind ctx16.
The suffix array the model is fed is the handle's own, proved in the same test by verify_sa(samples="all").

Each text is the smallest that reaches its branch, and says so with an assert on the MODEL's numbers before the device is
looked at.  One exception, stated where it applies: the first row of a deep-table entry WITHOUT rows is not compared (the
builder leaves there wherever its Occ steps ended; no reader looks at the first row of an empty interval).

Run on the GPU box with `pytest -m gpu`."""
import time
from importlib import import_module

import numpy as np
import pytest

import index_tables_model as M
import oracle_lib as ol
import sa_model
from test_gpu_low_memory import built
from test_gpu_parity import gpu_hits_as_records, oracle_hits_as_records

api = import_module("guidescan-cli_amd.api")
synth = import_module("guidescan-cli_amd.synth")

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", np.uint8)
STRAND_NAMES = ("blocks", "sa", "ptab", "ptab_rot", "ctx", "ctx16", "isa", "exc_row", "exc_sym", "run_start", "run_cum", "xr_seg",
                "xr_start", "xr_cum", "C256")
SLOT_NAMES = ("tab", "rot", "c16", "ctx", "rowid", "deep", "sp_off", "sp_rows")
COMPARED = set()      # (kind, array, strand) of every device array that was present and found equal to the model
TIMES = {}


@pytest.fixture(autouse=True)
def timed(request):
    t0 = time.perf_counter()
    yield
    TIMES[request.node.name] = time.perf_counter() - t0
    print(f"[index tables] {request.node.name}: {TIMES[request.node.name]:.2f} s, file so far {sum(TIMES.values()):.2f} s")


def rand_text(rng, n):
    return ACGT[rng.integers(0, 4, n)].copy()


def rc(b):
    return synth.reverse_complement_bytes(np.asarray(b, dtype=np.uint8))


def check_strands(gidx, text, k, *, mask_off=None, ctx=True, isa=True, rot_copies=None, small_sa=True, want=None):
    """both strands of a handle against the model; `want(strand, model, t, sa)` states what the text was built to reach.
    -> the models"""
    models = []
    n = int(text.shape[0]) + 1
    for strand in (0, 1):
        if isa:   # (the check of every row reads the inverse suffix array: a handle without one is proved by sa_model below)
            rep = gidx.verify_sa(text, strand=strand, samples="all")
            assert rep == dict(rows=n, not_permutation=0, sampled=n - 1, out_of_order=0, undecided=0, bwt_mismatch=0), rep
        assert isa or small_sa
        t = sa_model.strand_text(text, strand)
        dev_sa = gidx.debug_array(strand, "sa")
        assert np.array_equal(dev_sa, gidx.suffix_array(strand))
        sa = dev_sa.astype(np.int64)
        if small_sa:
            M.compare_exact("sa", strand, dev_sa, sa_model.suffix_array(t[:-1]).astype(np.uint32))
            COMPARED.add(("strand", "sa", strand))
        lay = gidx.debug_layout(strand)
        want_off = (M.default_mask_off(k) if mask_off is None else mask_off) if ctx else 0
        assert lay["mask_off"] == want_off and lay["k"] == k, lay
        m = M.strand_tables(t, sa, k, want_off, ctx=ctx)
        if want is not None:
            want(strand, m, t, sa)
        for key, v in m["layout"].items():
            assert lay[key] == v, (key, strand, lay, m["layout"])
        if not isa:
            m["isa"] = None
        r = m["_rows"]
        for name in STRAND_NAMES:
            if name in ("sa", "ptab_rot"):
                continue
            got = gidx.debug_array(strand, name)
            if name == "ptab" and ctx:   # what loses hits, by itself: every true pair of every occurrence has its bit
                M.check_mask_soundness("ptab", strand, got, r["rcode"], r["w"][r["vrows"]], r["nib"][r["vrows"]],
                                       M.mask_offsets(want_off))
            if name == "exc_row":
                M.check_strictly_ascending("exc_row", strand, got)
            M.compare_exact(name, strand, got, m[name])
            if got is not None:
                COMPARED.add(("strand", name, strand))
        rot = gidx.debug_array(strand, "ptab_rot")
        if rot_copies is not None:
            assert (lay["rot_copies"], lay["rot_first"]) == ((rot_copies, 3) if rot_copies else (0, 31)), lay
        M.compare_rotated("ptab_rot", strand, rot, m["ptab"], k, lay["rot_first"], lay["rot_copies"])
        if rot is not None:
            # the same index as the library's own statement of the permutation
            for j in range(lay["rot_copies"]):
                idx = np.random.default_rng(j).integers(0, 4 ** k, 64)
                perm = M.rot_perm(k, lay["rot_first"] + j)
                assert [api.rot_index(int(i), k, lay["rot_first"] + j) for i in idx] == [int(perm[i]) for i in idx]
            COMPARED.add(("strand", "ptab_rot", strand))
        models.append(m)
    return models


def cheap_batch(gidx, text, L=20):
    """two guides, one mismatch, no PAM-pair tables: the batch that makes gs_strand_rot_ensure build the rotated copies"""
    gidx.set_option("GS_NO_PAIRTAB", "1")
    seqs, pams, _, _ = synth.sample_guides(text, 2, seed=1, L=L)
    gidx.enumerate(seqs, pams, mismatches=1)


def two_chromosomes():
    rng = np.random.default_rng(21)
    # (bases of unequal frequency: at depth 6, 16 rows per k-mer on average, some k-mers still have one row or none)
    text = ACGT[rng.choice(4, size=40_000 + 25_000, p=(0.4, 0.1, 0.1, 0.4))].copy()
    text[18_000:18_700] = ord("N")
    text[40_000 - 40:40_000 + 40] = ord("N")   # the chromosomes' ends
    return text


@pytest.mark.parametrize("k,env", [(6, {}), (8, {}), (6, dict(GS_NO_ISA="1")), (6, dict(GS_NO_CTX="1")),
                                   (8, dict(GS_MASK_OFFSETS="1,3,6,9"))],
                         ids=["k6", "k8", "k6-no-isa", "k6-no-ctx", "k8-mask-offsets"])
def test_strand_tables_two_chromosomes(k, env):
    text = two_chromosomes()
    ctx = "GS_NO_CTX" not in env
    # the rotated copies need the context arrays and, in the builder's plan, the inverse suffix array's switch left alone
    copies = k - 1 - 3 if ctx else 0

    def want(strand, m, t, sa):
        cnt = m["ptab"][:, 1] & 0x7FFFFFFF
        assert (cnt == 0).any() and (cnt == 1).any() and (cnt > 1).any(), "k-mers with 0, 1 and more rows must all occur"
        if ctx:
            assert m["layout"]["n_exc"] > 0 and (m["ptab"][:, 1] >> 31).any() and m["layout"]["nruns"] > 0
    with built(dict(text=text), GS_PREFIX_K=str(k), **env) as gidx:
        cheap_batch(gidx, text)
        check_strands(gidx, text, k, mask_off=(1 | 3 << 4 | 6 << 8 | 9 << 12) if "GS_MASK_OFFSETS" in env else None, ctx=ctx,
                      isa="GS_NO_ISA" not in env and ctx, rot_copies=copies, want=want)


def edge_text():
    """k-mers at 0..17 and at the very end, bytes of class 5, single N with clean A,C,G,T for 40 symbols on either side"""
    rng = np.random.default_rng(22)
    text = rand_text(rng, 3_000)
    n_at = (500, 1_000, 1_500)
    for p in n_at:
        text[p] = ord("N")
    for p, ch in ((2_000, "R"), (2_100, "Y"), (2_200, "a"), (2_201, "c"), (2_300, "g"), (2_301, "t"), (2_400, "R")):
        text[p] = ord(ch)
    return text, n_at


@pytest.mark.parametrize("k", (4, 6))
def test_strand_tables_edges(k):
    text, n_at = edge_text()
    ln = int(text.shape[0])

    def want(strand, m, t, sa):
        isa = np.empty(sa.shape[0], dtype=np.int64)
        isa[sa] = np.arange(sa.shape[0])
        r = m["_rows"]
        code, valid = M.kmer_codes(t, k)
        exc_rows = set(int(x) for x in m["exc_row"])
        # positions 0..17: valid k-mers; the text start within 16 symbols flags 0..15 and not 16, 17
        assert valid[:18].all()
        for p in range(18):
            row = int(isa[p])
            nib = int(r["nib"][row])
            assert [(nib >> (4 * (j - 1))) & 15 == 6 for j in range(1, 17)] == [p < j for j in range(1, 17)], p
            assert (row in exc_rows) == (p < 16), p
        # a k-mer ending exactly at the last symbol; the window one further runs into the sentinel
        assert valid[ln - k] and not valid[ln - k + 1:].any() and int(m["ptab"][code[ln - k], 1] & 0x7FFFFFFF) >= 1
        # an N at distance 1 and 16 flags, at 17 it does not (strand 1: the same places seen from the other end)
        for p in n_at:
            q = p if strand == 0 else ln - 1 - p
            assert t[q] == ord("N")
            for dist, flagged in ((1, True), (16, True), (17, False)):
                assert valid[q + dist] and (int(isa[q + dist]) in exc_rows) == flagged, (p, dist)
        # class 5 among the exception symbols, and its runs in the general path's lists
        syms = np.concatenate([(m["exc_sym"] >> np.uint64(4 * j)) & np.uint64(15) for j in range(16)])
        assert set(int(x) for x in np.unique(syms)) == {0, 1, 2, 3, 4, 5, 6}
        present = set(int(c) for c in np.nonzero(m["xr_seg"][:, 1])[0])
        assert present == {ord(c) for c in "NRYacgt"}, present   # (the other strand swaps a/t and c/g: the same set)
    with built(dict(text=text), GS_PREFIX_K=str(k)) as gidx:
        check_strands(gidx, text, k, rot_copies=0, want=want)


@pytest.mark.parametrize("rows", (128 * 20 - 1, 128 * 20, 128 * 20 + 1))
def test_strand_tables_last_occ_block(rows):
    text = rand_text(np.random.default_rng(rows), rows - 1)
    text[700] = ord("N")

    def want(strand, m, t, sa):
        assert m["layout"]["n"] == rows and m["layout"]["blocks"] == (rows >> 7) + 1
        ex_last = m["blocks"][-1, 12:16]
        pad = 128 * m["layout"]["blocks"] - rows
        assert pad in (128, 127, 1)   # rows at and beyond n in the last block are marked in ex
        assert all((int(ex_last[(128 - 1 - j) >> 5]) >> ((128 - 1 - j) & 31)) & 1 for j in range(pad))
    with built(dict(text=text), GS_PREFIX_K="4") as gidx:
        check_strands(gidx, text, 4, rot_copies=0, want=want)


def test_strand_tables_second_exception_pass():
    """more than 2^16 exception rows per strand: k_ctx_build runs a second time with the counted capacity"""
    rng = np.random.default_rng(24)
    text = rand_text(rng, 300_000)
    text[30:300_000:60][:5_000] = ord("N")
    assert int((text == ord("N")).sum()) == 5_000

    def want(strand, m, t, sa):
        assert m["layout"]["n_exc"] > 65_536, m["layout"]
    with built(dict(text=text), GS_PREFIX_K="6") as gidx:
        check_strands(gidx, text, 6, rot_copies=0, want=want)


def test_strand_tables_run_list_retry():
    """N, R and Y head more than 2^20 runs of the BWT: k_x_runs is launched again with the counted capacity"""
    rng = np.random.default_rng(25)
    text = rand_text(rng, 3_200_000)
    special = rng.random(text.shape[0]) < 0.41
    text[special] = np.frombuffer(b"NRY", np.uint8)[rng.integers(0, 3, int(special.sum()))]
    text[:64] = rand_text(rng, 64)

    def want(strand, m, t, sa):
        runs = int(m["xr_seg"][:, 1].sum())
        assert runs > 1 << 20 and m["layout"]["xr_entries"] == runs + 3, runs
    with built(dict(text=text), GS_PREFIX_K="6") as gidx:
        check_strands(gidx, text, 6, rot_copies=0, small_sa=False, want=want)


# ---------------------------------------------------------------------------------------------- pair, deep, spaced tables
PK = 10            # the smallest depth at which a batch gets pair, deep and spaced tables with BOTH deep-table widths:
# two-sided seeding needs v_rem + 1 <= k, so 16-mers at the most (NGG + NAG: v_rem 9, deep tables over 8 and 9 guide symbols);
# 15-mers behind TTN (--start) give another v_rem (8).  Two mismatches: the spaced tables' class needs m <= k - |X| = 2 or 3
L_END, L_START, M_BUDGET = 16, 15, 2
CODE = dict(NGG=5, NAG=7, TTN=15)   # the pair as the strand's consumption sees it, first | second << 2 (C,C / T,C / T,T)


def plant(text, at, s, strand):
    s = np.asarray(s, dtype=np.uint8)
    text[at:at + s.shape[0]] = s if strand == 0 else rc(s)
    return at + s.shape[0] + 1


def site(rng, kmer, v_rem, code, n_at=None):
    """what a selected row of strand text looks like, left to right: the pair (farther symbol first), v_rem - 2 free symbols,
    the k-mer; n_at: distance before the k-mer of an N (beyond v_rem: in front of the pair)"""
    free = rand_text(rng, v_rem - 2)
    s = np.concatenate([rand_text(rng, 16 - v_rem), ACGT[[code >> 2, code & 3]], free, kmer])
    if n_at is not None:
        s[s.shape[0] - kmer.shape[0] - n_at] = ord("N")
    return s


@pytest.fixture(scope="module")
def pair_world():
    rng = np.random.default_rng(26)
    text = rand_text(rng, 240_000)
    for _ in range(6):
        at = int(rng.integers(150_000, 236_000))
        text[at:at + int(rng.integers(1, 60))] = ord("N")
    at = 2_000
    fams = {}
    # repeats of one k-mer behind the pair: 62, 63, 64 and 300 selected rows, both strands, NGG's pair; 63 and 64 for NAG, TTN
    for pam, v_rem, counts in (("NGG", L_END + 3 - PK, (62, 63, 64, 300)), ("NAG", L_END + 3 - PK, (63,)),
                               ("TTN", L_START + 3 - PK, (64,))):
        for strand in (0, 1):
            for c in counts:
                kmer = rand_text(rng, PK)
                fams[(pam, strand, c)] = kmer
                for _ in range(c):
                    at = plant(text, at, site(rng, kmer, v_rem, CODE[pam]), strand)
            if pam == "NGG":   # exception symbols in a selected interval: nearer than v_rem (left out), farther (kept)
                kmer = rand_text(rng, PK)
                fams[("exc", strand, 7)] = kmer
                for n_at in (None, 3, v_rem - 2, v_rem + 1, 16, None, None, None, None):
                    at = plant(text, at, site(rng, kmer, v_rem, CODE[pam], n_at=n_at), strand)
    fams_end = at
    # deep-table intervals of exactly 4,096 (strand 0) and 4,097 (strand 1) rows: nine guide symbols, a base, GG
    for strand, c in ((0, 4_096), (1, 4_097)):
        unit = np.concatenate([rand_text(rng, 9), np.frombuffer(b"AGG", np.uint8)])
        fams[("deep", strand, c)] = unit
        for _ in range(c):
            at = plant(text, at, unit, strand)
    assert at < 150_000
    # guides from the pair families' stretch and from the plain stretch behind the plants, none from the 4,096-fold repeats: a
    # guide whose own k-mer heads thousands of rows sends the batch to the sharing form, which builds no spaced tables
    fam_end = 2_000 + 36_000
    assert fams_end <= fam_end
    tt = np.nonzero((text[:-40] == ord("T")) & (text[1:-39] == ord("T")))[0]
    tt = tt[(tt < fam_end - 40) | (tt > 150_000)]
    tt = tt[np.all(np.isin(np.stack([text[tt + 2 + j] for j in range(1 + L_START)]), ACGT), axis=0)]
    start_seqs = np.stack([text[p + 3:p + 3 + L_START] for p in tt[np.linspace(0, tt.shape[0] - 1, 24).astype(int)]])
    seqs = {False: np.concatenate([synth.sample_guides(text[:fam_end], 12, seed=3, L=L_END)[0],
                                   synth.sample_guides(text[150_000:], 12, seed=4, L=L_END)[0]]), True: start_seqs}
    return dict(text=text, fams=fams, seqs=seqs)


def pair_batch(gidx, w, pam, alt, L, start, kb):
    gidx.set_options(GS_SPACED_FROM="1", GS_DEEP_SYMBOLS=str(kb))
    seqs = w["seqs"][start]
    pams = np.tile(np.frombuffer(pam.encode(), np.uint8), (seqs.shape[0], 1))
    return seqs, gidx.enumerate(seqs, pams, mismatches=M_BUDGET, alt_pams=alt, start=start)


def strand_model(gidx, w, strand, cache):
    if strand not in cache:
        n = int(w["text"].shape[0]) + 1
        rep = gidx.verify_sa(w["text"], strand=strand, samples="all")
        assert rep == dict(rows=n, not_permutation=0, sampled=n - 1, out_of_order=0, undecided=0, bwt_mismatch=0), rep
        t = sa_model.strand_text(w["text"], strand)
        sa = gidx.debug_array(strand, "sa").astype(np.int64)
        cache[strand] = (t, M.strand_tables(t, sa, PK))
        M.compare_exact("ptab", strand, gidx.debug_array(strand, "ptab"), cache[strand][1]["ptab"])
    return cache[strand]


def slot_model(t, st, v_rem, code, kb, lay):
    """the tables of one slot and strand, and what they show (for the asserts on what the text was planted to reach)"""
    pt = M.pair_tables(st, PK, v_rem, code)
    deep = M.deep_table(t, st, PK, 3, kb, code)
    spaced = M.spaced_table(pt, PK, lay["sp_x"], lay["sp_g"], lay["sp_rem"], lay["d"])
    r = st["_rows"]
    sel = np.zeros(st["layout"]["n"], dtype=bool)
    sel[pt["rowid"][pt["_slot"]]] = True
    coded = ((r["w"][r["vrows"]].astype(np.int64) >> (2 * (v_rem - 2))) & 15) == code
    facts = dict(cnt=pt["_cnt"], kept_exc=int((sel[r["vrows"]] & r["exc"][r["vrows"]]).sum()),
                 left_out=int((coded & ~sel[r["vrows"]]).sum()), deep_cnt=deep[:, 1] & 0x7FFFFFFF, deep_flag=deep[:, 1] >> 31,
                 deep_masks=deep[:, 2:])
    return pt, deep, spaced, facts


def check_slots(gidx, w, want_slots, kb, L, facts, cache):
    """every array of every slot and strand against the model; facts: what the model's tables show, for the caller's asserts"""
    seen = {}
    for slot in (0, 1):
        for strand in (0, 1):
            lay = gidx.debug_layout(strand, slot=slot)
            if not lay["valid"]:
                continue
            seen[lay["code"]] = slot
            v_rem, code = lay["v_rem"], lay["code"]
            assert lay["k"] == PK and v_rem == L + 3 - PK and code in want_slots, lay
            assert lay["deep"] and (lay["deep_P"], lay["deep_kb"]) == (3, kb), lay
            assert lay["spaced"] and (lay["sp_x"], lay["sp_g"]) == (L - kb, L - PK), lay
            assert lay["sp_rem"] + lay["d"] == 2 * (lay["sp_x"] + lay["sp_g"]), lay
            t, st = strand_model(gidx, w, strand, cache)
            pt, deep, (key, rows, off), f = slot_model(t, st, v_rem, code, kb, lay)
            facts.setdefault(code, []).append(f)
            assert lay["n_slots"] == pt["n_slots"], (lay, pt["n_slots"])
            what = f"slot {slot} (pair {code}, v_rem {v_rem})"
            for name in ("tab", "c16", "ctx", "rowid"):
                M.compare_exact(f"{what} {name}", strand, gidx.debug_array(strand, name, slot=slot), pt[name])
                COMPARED.add(("slot", name, strand))
            rot = gidx.debug_array(strand, "rot", slot=slot)
            assert (lay["rot_copies"] == 0) == (lay["rot_first"] == 31) == (rot is None), lay
            M.compare_rotated(f"{what} rot", strand, rot, pt["tab"], PK, lay["rot_first"], lay["rot_copies"])
            if rot is not None:
                COMPARED.add(("slot", "rot", strand))
            got = gidx.debug_array(strand, "deep", slot=slot).copy()
            got[(got[:, 1] & 0x7FFFFFFF) == 0, 0] = 0   # the first row of an entry without rows: not compared (see the head)
            M.compare_exact(f"{what} deep", strand, got, deep)
            COMPARED.add(("slot", "deep", strand))
            assert lay["sp_rows"] == rows.shape[0] == int(pt["_cnt"].sum())   # every row once; header slots are no rows
            M.compare_spaced(what, strand, gidx.debug_array(strand, "sp_rows", slot=slot),
                             gidx.debug_array(strand, "sp_off", slot=slot), key, rows, off, lay["sp_rem"])
            COMPARED.update({("slot", "sp_off", strand), ("slot", "sp_rows", strand)})
    assert sorted(seen) == sorted(want_slots), (seen, want_slots)


def hits_equal_oracle(w, seqs, result, pam, alt, start):
    offsets, hits, _ = result
    oidx = ol.OracleIndex(w["text"])
    try:
        opts = ol.make_opts(mismatches=M_BUDGET, alt_pams=alt, start=start)
        total = 0
        for i in range(seqs.shape[0]):
            g = seqs[i].tobytes().decode()
            want = oracle_hits_as_records(oidx, g, pam, opts, 3, start)[0]
            assert gpu_hits_as_records(offsets, hits, i, g, 3, start) == want, (pam, i)
            total += len(want)
        assert total >= seqs.shape[0]
    finally:
        oidx.close()


def assert_planted(w, facts):
    """the NGG + NAG batch's tables hold, by the model's count, what the text was planted to reach"""
    ngg = facts[CODE["NGG"]]
    counts = np.concatenate([f["cnt"] for f in ngg])
    for c in (1, 2, 62, 63, 64):
        assert (counts == c).any(), f"no pair-table entry with exactly {c} selected rows"
    assert ((counts > 200) & (counts < 1_000)).any()
    for (pam, strand, c), kmer in w["fams"].items():
        if pam == "NGG":
            e = int(sum(int(np.searchsorted(ACGT, b)) << (2 * i) for i, b in enumerate(kmer)))
            assert int(ngg[strand]["cnt"][e]) == c, (pam, strand, c)
    assert (np.concatenate([f["cnt"] for f in facts[CODE["NAG"]]]) >= 63).any()
    assert sum(f["kept_exc"] for f in ngg) >= 2 and sum(f["left_out"] for f in ngg) >= 2, ngg
    dc = np.concatenate([f["deep_cnt"] for f in ngg])
    df = np.concatenate([f["deep_flag"] for f in ngg])
    dm = np.concatenate([f["deep_masks"] for f in ngg])
    assert ((dc == 4_096) & (df == 0) & dm.any(axis=1)).any() and ((dc == 4_097) & (df == 1) & ~dm.any(axis=1)).any()
    assert ((dc > 0) & (dc <= 4_096) & (df == 1)).any()   # flagged through the depth-k interval it descends from


@pytest.mark.parametrize("kb", (PK - 2, PK - 1))   # both legal widths: one and two Occ steps beyond the depth-k interval in k_pb_build
def test_pair_deep_and_spaced_tables_ngg_nag(pair_world, kb):
    """(a handle per width: what a handle has seen of its first batch may send the second to the sharing form, which
    builds no spaced tables)"""
    w = pair_world
    with built(dict(text=w["text"]), GS_PREFIX_K=str(PK)) as gidx:
        before = gidx.resident()
        lay = gidx.debug_layout(0)
        assert gidx.debug_array(0, "ptab").shape == (4 ** PK, 4) and lay["n"] == 240_001
        assert gidx.resident() == before   # the readers change nothing
        seqs, result = pair_batch(gidx, w, "NGG", ("NAG",), L_END, False, kb)
        facts = {}
        res = gidx.resident()
        check_slots(gidx, w, (CODE["NGG"], CODE["NAG"]), kb, L_END, facts, {})
        assert gidx.resident() == res
        assert_planted(w, facts)
        hits_equal_oracle(w, seqs, result, "NGG", ("NAG",), False)


def test_pair_deep_and_spaced_tables_start_ttn(pair_world):
    w = pair_world
    with built(dict(text=w["text"]), GS_PREFIX_K=str(PK)) as gidx:
        seqs, result = pair_batch(gidx, w, "TTN", (), L_START, True, PK - 2)
        facts = {}
        check_slots(gidx, w, (CODE["TTN"],), PK - 2, L_START, facts, {})
        ttn = facts[CODE["TTN"]]
        assert all(int(f["cnt"].max()) >= 64 for f in ttn) and (np.concatenate([f["cnt"] for f in ttn]) == 64).any()
        hits_equal_oracle(w, seqs, result, "TTN", (), True)


@pytest.mark.parametrize("bits,rem", [("32", 0), ("1", 23)], ids=["whole-key", "smallest"])
def test_pair_deep_and_spaced_tables_key_split(pair_world, bits, rem):
    """the same comparison under GS_SPACED_BITS: the whole 24-bit key of this geometry (|X| = 7, |R| = 5) in the offsets and
    no key bits with the row - what a genome of hg38's size gets -, and one bit in the offsets, the other 23 with the row"""
    w = pair_world
    with built(dict(text=w["text"]), GS_PREFIX_K=str(PK)) as gidx:
        gidx.set_option("GS_SPACED_BITS", bits)
        seqs, result = pair_batch(gidx, w, "TTN", (), L_START, True, PK - 2)
        for strand in (0, 1):
            lay = gidx.debug_layout(strand, slot=0)
            assert lay["spaced"] and (lay["sp_rem"], lay["d"]) == (rem, 24 - rem), lay
        check_slots(gidx, w, (CODE["TTN"],), PK - 2, L_START, {}, {})
        assert gidx.last_counters()["spaced_items"] == 2 * seqs.shape[0]
        hits_equal_oracle(w, seqs, result, "TTN", (), True)


def test_every_array_was_compared():
    """a table that silently was not built fails here: every array name, both strands, was present and equal at least once"""
    missing = [(kind, name, s) for kind, names in (("strand", STRAND_NAMES), ("slot", SLOT_NAMES)) for name in names
               for s in (0, 1) if (kind, name, s) not in COMPARED]
    assert not missing, missing
    print("[index tables] seconds per test:", {k: round(v, 2) for k, v in TIMES.items()}, "total", round(sum(TIMES.values()), 2))
