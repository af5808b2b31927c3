"""The scoring model of tests/score_model.py held to every reference there is on the CPU - the oracle's text
lines, the files the reference binary wrote, the host decoder and the host formatter - and the conditions on the
synthesized batches that make tests/test_gpu_score_synth.py able to tell a wrong kernel from a right one.  A
failure of the GPU test then points at the kernel, not at the model."""
import numpy as np
import pytest

import oracle_lib as ol
import score_model as sm
from test_gpu_score_kmers import SCORE_CASES, fmt_f, golden_specificities

api = sm.api


@pytest.fixture(scope="module")
def toy_oracle(toy):
    oidx = ol.OracleIndex(toy["text"])
    yield toy, oidx
    oidx.close()


@pytest.fixture(scope="module")
def ladder():
    b = sm.build_ladder()
    return b, sm.batch_facts(b["seqs"], 3, b["offsets"], b["hits"], b["lengths"])


@pytest.fixture(scope="module")
def maxoff():
    b = sm.build_maxoff()
    return b, sm.batch_facts(b["seqs"], 3, b["offsets"], b["hits"], b["lengths"])


def _guide_str(batch, g):
    return batch["seqs"][g].tobytes().decode()


@pytest.mark.parametrize("cfg", SCORE_CASES, ids=lambda c: "-".join(f"{k}{v}" for k, v in c.items()))
def test_model_equals_the_oracles_lines_and_the_golden_files(toy_oracle, cfg):
    toy, oidx = toy_oracle
    m, sam, alt = cfg["m"], cfg.get("sam", False), cfg.get("alt", ())
    start, max_off = cfg.get("start", False), cfg.get("max_off", -1)
    gold = golden_specificities(toy["dir"] / cfg["golden"], sam) if "golden" in cfg else None
    opts = ol.make_opts(mismatches=m, alt_pams=alt, start=start, max_off_targets=max_off)
    checked = checked_gold = 0
    for k in toy["kmers"]:
        L, P = len(k.sequence), len(k.pam)
        ohits, _, raw = oidx.enumerate(k.sequence, k.pam, opts)
        text = ol.text_lines("sam" if sam else "csv", toy["names"], toy["lengths"], k.id, k.sequence, k.pam,
                             k.positive, opts, raw)
        ol.lib().gso_free(raw[0])
        d, cfd, dropped, perfect, keys = [], [], [], [], []
        for pos, mm, index, sequence, _ in ohits:
            key, ms = sm.encode_hit(k.sequence, sm.subs_of(sequence, L), sequence[L:], mm, index, start)
            assert ms == sequence   # under --start this is the host decoder against the oracle's search
            assert sm.match_sequence(k.sequence, P, key, start) == sequence
            c, pf = sm.hit_facts(k.sequence, P, key, start)
            d.append(mm), cfd.append(c), perfect.append(pf), keys.append(key)
            dropped.append(sm.resolve_absolute(toy["lengths"], pos, L, P) is None)
        assert keys == sorted(keys)   # ascending key == the reference's order
        spec = (sm.specificity_sam if sam else sm.specificity_csv)(d, cfd, dropped, perfect, max_off)
        lines = text.splitlines()
        if sam:
            osp = {[c for c in ln.split("\t") if c.startswith("sp:f:")][0][5:] for ln in lines}
        else:
            osp = {ln.split(",")[-1] for ln in lines}
        if osp and osp != {"1.0"}:   # "1.0" is the literal of the no-hit CSV row (printer.hpp:189-199)
            assert osp == {fmt_f(spec)}, (k.id, osp, spec)
            checked += 1
        if gold is not None and k.id in gold and gold[k.id] != "1.0":
            assert gold[k.id] == fmt_f(spec), (k.id, gold[k.id], spec)
            checked_gold += 1
    assert checked >= 1 and (gold is None or checked_gold >= 1)


@pytest.mark.parametrize("L,P,start", [(20, 3, False)] + sm.SHAPES, ids=lambda v: str(int(v)))
def test_encoder_round_trip_through_the_host_decoder(L, P, start):
    rng = np.random.default_rng(1000 + 10 * L + P)
    for _ in range(200):
        guide = sm._guide(rng, L)
        q = sm.query_chars(guide, start)
        nsub = int(rng.integers(0, 5))
        subs = {int(t): [b for b in sm.BASES if b != q[t]][rng.integers(3)] for t in rng.choice(L, nsub, replace=False)}
        pam = "".join(rng.choice(list(sm.PAM_SYMBOLS), P))
        key, ms = sm.encode_hit(guide, subs, pam, nsub, int(rng.integers(2)), start)
        assert api.decode_sequence(guide, P, key, api.GS_FLAG_PAM_AT_START if start else 0) == ms
        assert len(ms) == L + P and ms[L:] == pam
        assert {t for t in range(L) if ms[t].islower()} == set(subs)
        for t in range(L):
            assert ms[t] == (subs[t].lower() if t in subs else q[t])
        assert key >> 61 == nsub and key & 1 == 0


def _host_specificity(gs, batch, g, sam, max_off):
    a, b = int(batch["offsets"][g]), int(batch["offsets"][g + 1])
    hits = batch["hits"][a:b]
    mism = int(hits["key"].max() >> np.uint64(61)) if b > a else 0
    text = api.format_guide(gs, f"g{g}", _guide_str(batch, g), "N" * batch["P"], True, hits, mism, sam=sam,
                            start=batch["start"], max_off_targets=max_off)
    lines = [ln for ln in text.splitlines() if ln]
    if sam:
        return {[c for c in ln.split("\t") if c.startswith("sp:f:")][0][5:] for ln in lines}
    return {ln.split(",")[-1] for ln in lines}


@pytest.mark.parametrize("sam", [False, True], ids=["csv", "sam"])
@pytest.mark.parametrize("max_off", [-1, 1, 2, 64, 100])
def test_model_equals_the_host_formatter_on_synthesized_lists(maxoff, sam, max_off):
    batch, facts = maxoff
    gs = api.make_genome_structure([f"c{i}" for i in range(len(batch["lengths"]))], batch["lengths"])
    spec = sm.specificity_batch(batch["offsets"], *facts, max_off=max_off, sam=sam)
    checked = 0
    for g in range(batch["seqs"].shape[0]):
        if int(batch["offsets"][g + 1] - batch["offsets"][g]) > 6000:
            continue
        got = _host_specificity(gs, batch, g, sam, max_off)
        if got and got != {"1.0"}:
            assert got == {fmt_f(spec[g])}, (g, got, spec[g])
            checked += 1
    assert checked >= 8


@pytest.mark.parametrize("L,P,start", sm.SHAPES, ids=lambda v: str(int(v)))
def test_model_equals_the_host_formatter_on_every_shape(L, P, start):
    batch = sm.build_shape(L, P, start)
    gs = api.make_genome_structure(["a", "b"], batch["lengths"])
    facts = sm.batch_facts(batch["seqs"], P, batch["offsets"], batch["hits"], batch["lengths"], start)
    # the reference scores nothing but 20-mers with three PAM symbols behind them
    if L != 20 or L + P < 23:
        assert (facts[1] == np.float32(1.0)).all()
    else:
        assert len(set(facts[1].tolist())) > 10
    # positions 21 and 22 read GG in some distance-0 hits and not in others; a shorter sequence has no perfect hit
    if L + P >= 23:
        assert facts[3].any() and (~facts[3][facts[0] == 0]).any()
    else:
        assert not facts[3].any()
    for sam, max_off in ((False, -1), (True, -1), (False, 3), (True, 3)):
        spec = sm.specificity_batch(batch["offsets"], *facts, max_off=max_off, sam=sam)
        assert np.array_equal(spec.view(np.uint32),
                              sm.specificity_loops(batch["offsets"], *facts, max_off=max_off, sam=sam).view(np.uint32))
        checked = 0
        for g in range(batch["seqs"].shape[0]):
            got = _host_specificity(gs, batch, g, sam, max_off)
            if got:   # (a guide without a distance-0 hit has no SAM line)
                assert got == {fmt_f(spec[g])}, (g, sam, max_off, got, spec[g])
                checked += 1
        assert checked >= 3


def test_sentinel_forms_agree_with_each_other_and_the_oracle():
    lib = ol.lib()
    import ctypes as C
    for name, lengths, joins in sm.geometry_structures():
        batch = sm.build_geometry(lengths, joins)
        pos = batch["hits"]["pos"]
        fast = sm.dropped_batch(lengths, pos, 20, 3)
        slow = np.array([sm.resolve_absolute(lengths, int(p), 20, 3) is None for p in pos])
        assert np.array_equal(fast, slow), name
        arr = np.asarray(lengths, dtype=np.uint64)
        s, st = C.c_int64(), C.c_char()
        orc = np.array([lib.gso_resolve_absolute(arr.ctypes.data, len(lengths), int(p), 20, 3, C.byref(s), C.byref(st)) < 0
                        for p in pos])
        assert np.array_equal(slow, orc), name
        if lengths:
            assert fast.any() and (~fast).any(), name
        else:
            assert fast.all()


def test_batch_aggregation_equals_the_loops(ladder, maxoff):
    for batch, facts in (ladder, maxoff):
        for sam in (False, True):
            for max_off in [-1] + sm.MAXOFF_VALUES:
                a = sm.specificity_batch(batch["offsets"], *facts, max_off=max_off, sam=sam)
                b = sm.specificity_loops(batch["offsets"], *facts, max_off=max_off, sam=sam)
                assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (sam, max_off)
    t = sm.build_tickets(5000, n_heavy=6)
    facts = sm.batch_facts(t["seqs"], 3, t["offsets"], t["hits"], t["lengths"])
    for sam, max_off in ((False, -1), (False, 1), (True, 1)):
        a = sm.specificity_batch(t["offsets"], *facts, max_off=max_off, sam=sam)
        b = sm.specificity_loops(t["offsets"], *facts, max_off=max_off, sam=sam)
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), (sam, max_off)


# ---- the inputs can tell --------------------------------------------------------------------------

def test_ladder_has_the_shape_the_kernels_edges_need(ladder):
    batch, facts = ladder
    off = batch["offsets"].astype(np.int64)
    counts = np.diff(off)
    assert set(sm.LADDER_COUNTS) <= set(counts.tolist())
    assert counts[0] == 0 and counts[-1] == 0
    with_hits = np.flatnonzero(counts)
    assert counts[with_hits[-1]] < 8   # the unguarded loads of the last guide run past the end of the array
    # a prefix sum on a multiple of 4,096, then empty guides, then a guide with hits
    assert any(off[g] % 4096 == 0 and off[g] > 0 and counts[g] == 0 and counts[g - 1] > 0 and counts[g + 1] == 0
               for g in range(1, len(counts) - 1))
    assert sum(1 for g in with_hits if off[g] // 4096 != (off[g + 1] - 1) // 4096) >= 8   # straddle a chunk edge
    assert max(np.diff(np.flatnonzero(np.concatenate([[1], counts, [1]]))) - 1) >= 3      # a run of empty guides
    d, cfd, dropped, perfect = facts
    g = batch["named"]["perfect_at_chunk_end"]
    assert off[g] % 4096 == 4095 and perfect[off[g]] and not perfect[off[g] + 1:off[g + 1]].any()
    assert not perfect[off[g - 1]:off[g]].any() and not perfect[off[g + 1]:off[g + 2]].any()
    g = batch["named"]["perfect_dropped"]
    assert perfect[off[g]] and dropped[off[g]] and cfd[off[g]] == 1.0
    g = batch["named"]["perfect_reverse_only"]
    sel = slice(off[g], off[g + 1])
    assert [(int(k) >> 60) & 1 for k in batch["hits"]["key"][sel][perfect[sel]]] == [1]
    g = batch["named"]["only_xAG"]
    assert (d[off[g]:off[g + 1]] == 0).sum() == 2 and not perfect[off[g]:off[g + 1]].any()
    # CFDs spread over orders of magnitude, zeros (an N in the PAM) among them; both kinds of guide
    pos_cfd = cfd[cfd > 0]
    assert (cfd == 0).any() and pos_cfd.max() / pos_cfd.min() > 1e4
    has_perfect = np.bincount(np.repeat(np.arange(len(counts)), counts)[perfect], minlength=len(counts)) > 0
    assert has_perfect[with_hits].any() and (~has_perfect[with_hits]).any()
    assert dropped.any()


def test_order_of_addition_shows_in_the_heaviest_guide(ladder):
    batch, facts = ladder
    d, cfd, dropped, perfect = facts
    g = batch["heaviest"]
    a, b = int(batch["offsets"][g]), int(batch["offsets"][g + 1])
    assert b - a == 70000
    terms = cfd[a:b][~dropped[a:b]]
    seq = np.float32(0.0)
    for x in terms:   # the reference's loop itself
        seq = np.float32(seq + x)
    assert np.cumsum(terms, dtype=np.float32)[-1].view(np.uint32) == seq.view(np.uint32)
    assert np.sum(terms, dtype=np.float32).view(np.uint32) != seq.view(np.uint32)             # pairwise
    assert np.float32(np.sum(terms.astype(np.float64))).view(np.uint32) != seq.view(np.uint32)   # rounded once
    # and in blocks of 64 or 512 partial sums, the orders a wavefront would find convenient
    for blk in (64, 512):
        part = [np.cumsum(terms[i:i + blk], dtype=np.float32)[-1] for i in range(0, len(terms), blk)]
        assert np.cumsum(np.array(part, np.float32), dtype=np.float32)[-1].view(np.uint32) != seq.view(np.uint32)


def test_cuts_show_in_the_max_off_batch(maxoff):
    batch, facts = maxoff
    d, cfd, dropped, perfect = facts
    for max_off in sm.MAXOFF_VALUES:
        csv = sm.specificity_batch(batch["offsets"], *facts, max_off=max_off, sam=False)
        sam = sm.specificity_batch(batch["offsets"], *facts, max_off=max_off, sam=True)
        if max_off >= 1:
            assert (csv.view(np.uint32) != sam.view(np.uint32)).any(), max_off
        # and the cut itself: some guide differs from the uncut result
        assert (csv.view(np.uint32) != sm.specificity_batch(batch["offsets"], *facts).view(np.uint32)).any()
    # the perfect hit beyond the cut
    g = batch["named"]["aag_tgg_agg"]
    a, b = int(batch["offsets"][g]), int(batch["offsets"][g + 1])
    assert list(perfect[a:a + 3]) == [False, True, True]
    cut = sm.specificity_csv(d[a:b], cfd[a:b], dropped[a:b], perfect[a:b], 1)
    assert cut != sm.specificity_csv(d[a:b], cfd[a:b], dropped[a:b], np.array([True] + [False] * (b - a - 1)), 1)
    g = batch["named"]["aag_dropped_cag_agg"]
    a, b = int(batch["offsets"][g]), int(batch["offsets"][g + 1])
    assert dropped[a] and not dropped[a + 1]
    assert sm.specificity_csv(d[a:b], cfd[a:b], dropped[a:b], perfect[a:b], 1) != \
        sm.specificity_sam(d[a:b], cfd[a:b], dropped[a:b], perfect[a:b], 1)
    # dropped hits at the first and last place of a 64-hit block, and class boundaries on block boundaries
    g = batch["named"]["blocks_64_64_200"]
    a = int(batch["offsets"][g])
    assert all(dropped[a + i] for i in (0, 63, 64, 127, 128))
    assert d[a + 63] != d[a + 64] and d[a + 127] != d[a + 128]
    for name, n in (("list_of_64", 64), ("list_of_128", 128)):
        g = batch["named"][name]
        assert int(batch["offsets"][g + 1] - batch["offsets"][g]) == n


def test_dropped_hits_show_in_every_geometry():
    for name, lengths, joins in sm.geometry_structures():
        batch = sm.build_geometry(lengths, joins)
        facts = sm.batch_facts(batch["seqs"], 3, batch["offsets"], batch["hits"], batch["lengths"])
        d, cfd, dropped, perfect = facts
        for sam, max_off in ((False, -1), (True, 5)):
            real = sm.specificity_batch(batch["offsets"], d, cfd, dropped, perfect, max_off=max_off, sam=sam)
            kept = sm.specificity_batch(batch["offsets"], d, cfd, np.zeros_like(dropped), perfect, max_off=max_off, sam=sam)
            differ = real.view(np.uint32) != kept.view(np.uint32)
            assert differ.any(), name
            assert np.array_equal(differ, dropped), name   # one hit per guide: every fate shows
        if name == "beyond_2_to_32":
            assert (np.abs(batch["hits"]["pos"]) > 2 ** 32).any()


def test_tickets_batch_is_what_the_issue_describes():
    t = sm.build_tickets(20000, n_heavy=40)
    counts = np.diff(t["offsets"].astype(np.int64))
    light = np.delete(counts, t["heavy"])
    assert set(light.tolist()) == {0, 1, 2, 3}
    assert ((counts[t["heavy"]] >= 1000) & (counts[t["heavy"]] <= 3000)).all()
    keys = t["hits"]["key"]
    gid = np.repeat(np.arange(len(counts)), counts)
    assert ((keys[1:] >= keys[:-1]) | (gid[1:] != gid[:-1])).all()   # canonical order inside every guide
    facts = sm.batch_facts(t["seqs"], 3, t["offsets"], t["hits"], t["lengths"])
    spec = sm.specificity_batch(t["offsets"], *facts)
    assert len(set(spec.view(np.uint32).tolist())) > 1000   # a stale or misplaced value would not pass for its neighbour's
