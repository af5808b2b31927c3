"""Candidate ids and kmers-file rows encoded in HBM (gs_kmers.hip: gs_kmers_encode_ids, gs_kmers_get_ids, gs_kmers_csv,
gs_kmers_concat), the text encoder over ids that are on the device already (gs_format_device_ids) and the fused entry
point over device pointers (gs_enumerate_text_device).

Expected ids and rows are built from the reference script's own rows (tests/golden/kmers) or from the numpy restatement
that tests/test_kmers.py pins on them (kmers.find_all_kmers / write_kmers_csv(device=None)); the device-id encoder is
compared with gs_format_device given the same ids from the host, the fused entry with gs_enumerate_text on downloaded
copies.  What the API lets a test see of a buffer's surroundings is the terminator behind gs_kmers_csv's text: the
device buffers are allocated by the library after the lengths are known, so no canary can be laid behind them; their
contents are compared byte for byte over exactly offsets[n] bytes instead.  GPU only."""
import ctypes as C
import io
from importlib import import_module

import numpy as np
import pytest

from kmers_golden import expected_rows, golden_cases

api = import_module("guidescan-cli_amd.api")
kmers = import_module("guidescan-cli_amd.kmers")
synth = import_module("guidescan-cli_amd.synth")

pytestmark = pytest.mark.gpu

CASES = golden_cases()
# (prefix, chromosome name): no prefix and a 1-byte name, a 40-byte prefix and a 64-byte name
NAMINGS = [("", "c"), ("p" * 39 + "_", "scaffold_" + "x" * 55)]


def _hip():
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return hip


def from_device(ptr, n):
    out = np.empty(n, dtype=np.uint8)
    if n:
        assert _hip().hipMemcpy(out.ctypes.data, ptr, n, 2) == 0
    return out.tobytes()


def expected_text(rows, pam, prefix, name):
    """(ids, their offsets, senses as 0/1, the kmers-file rows) for (sequence, position, sense) triples"""
    ids = [f"{prefix}{name}:{pos}:{sense}" for _, pos, sense in rows]
    off = np.zeros(len(ids) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(i) for i in ids], dtype=np.uint64)
    text = "".join(f"{i},{seq},{pam},{name},{pos},{sense}\n" for i, (seq, pos, sense) in zip(ids, rows))
    return "".join(ids).encode(), off, np.array([s == "+" for _, _, s in rows], dtype=np.uint8), text.encode()


def csv_with_terminator(km, prefix, name):
    """gs_kmers_csv through ctypes: the text, and the byte behind it"""
    out, ln = C.c_void_p(), C.c_uint64()
    assert api.lib().gs_kmers_csv(km._h, prefix.encode(), name.encode(), C.byref(out), C.byref(ln)) == 0
    raw = C.string_at(out, ln.value + 1)
    api.lib().gs_free(out)
    return raw[:-1], raw[-1]


def check_against(km, rows, pam, prefix, name):
    want_ids, want_off, want_sense, want_rows = expected_text(rows, pam, prefix, name)
    assert km.n == len(rows)
    km.encode_ids(prefix, name)
    ids, off, sp = km.ids_to_host()
    assert np.array_equal(off, want_off)
    assert int(off[-1]) == len(want_ids) and ids == want_ids
    assert np.all(off[1:] > off[:-1])  # strictly ascending: no id is empty
    assert np.array_equal(sp, want_sense)
    # the same arrays as they lie in HBM
    assert from_device(km.ids_ptr, len(want_ids)) == want_ids
    assert from_device(km.id_offsets_ptr, 8 * (km.n + 1)) == want_off.tobytes()
    assert from_device(km.sense_positive_ptr, km.n) == want_sense.tobytes()
    text, term = csv_with_terminator(km, prefix, name)
    assert text == want_rows and term == 0
    assert km.csv(prefix, name) == want_rows


@pytest.mark.parametrize("naming", NAMINGS, ids=["short", "long"])
@pytest.mark.parametrize("case", CASES, ids=lambda c: c["name"])
def test_ids_and_rows_equal_the_reference_scripts_rows(case, naming):
    assert len(CASES) == 12 and len(naming[0]) in (0, 40) and len(naming[1]) in (1, 64)
    km = api.generate_kmers(case["record"].encode(), case["pam"], case["k"], case["start"], device=0)
    try:
        check_against(km, expected_rows(case), case["pam"], *naming)
    finally:
        km.close()


def chromosome_with(n_sites, seed):
    """a seeded random chromosome cut to the length at which it has exactly n_sites NGG candidates"""
    for s in range(seed, seed + 50):
        rng = np.random.default_rng(s)
        full = rng.choice(np.frombuffer(b"ACGT", np.uint8), size=30 + 12 * n_sites + 200)
        count = lambda ln: len(kmers.find_all_kmers(full[:ln], "NGG", 20, False))
        lo, hi = 0, full.shape[0]  # smallest length with at least n_sites candidates
        if count(hi) < n_sites:
            continue
        while lo < hi:
            mid = (lo + hi) // 2
            if count(mid) >= n_sites:
                hi = mid
            else:
                lo = mid + 1
        if count(lo) == n_sites:  # a position can add two sites at once: then the next seed
            return full[:lo]
    raise AssertionError(f"no chromosome with {n_sites} candidates")


@pytest.mark.parametrize("n_sites", [1, 63, 64, 65, 255, 256, 257, 5000])
def test_record_counts_at_the_wave_and_block_edges(n_sites):
    """(n = 0 is the `empty_record` golden above)"""
    chrm = chromosome_with(n_sites, 1000 + n_sites)
    rows = kmers.find_all_kmers(chrm, "NGG", 20, False)
    assert len(rows) == n_sites
    km = api.generate_kmers(chrm, "NGG", 20, False, device=0)
    try:
        check_against(km, rows, "NGG", "lib_", "chr7")
    finally:
        km.close()


def test_positions_of_one_to_seven_digits():
    chrm = np.random.default_rng(77).choice(np.frombuffer(b"ACGT", np.uint8), size=1_200_000)
    buf = io.StringIO()
    n = kmers.write_kmers_csv(buf, [("chr1", chrm)], "NGG", 20, False, "")
    want = buf.getvalue().split("\n", 1)[1].encode()
    digits = {len(line.split(b",")[4]) for line in want.splitlines()}
    assert digits == {1, 2, 3, 4, 5, 6, 7} or digits == {2, 3, 4, 5, 6, 7}, digits  # the first site may lie past position 9
    km = api.generate_kmers(chrm, "NGG", 20, False, device=0)
    try:
        assert km.n == n
        assert km.csv("", "chr1") == want
        km.encode_ids("", "chr1")
        ids, off, _ = km.ids_to_host()
        assert ids == b"".join(line.split(b",")[0] for line in want.splitlines())
        assert int(off[-1]) == len(ids) and np.all(off[1:] > off[:-1])
    finally:
        km.close()


def test_positions_of_nine_and_ten_digits():
    """a chromosome of 1,000,000,200 bytes made on the device, all N but for planted sites in its first 100 bytes and at its
    end.  The last 200 bytes begin at position 1,000,000,001; so that 999,999,9xx occurs as well the planted end is the
    last 300 bytes (it contains the last 200).  The expected rows come from the planted text alone: between the two
    pieces nothing but N, which no candidate touches."""
    import torch
    total, head_n, tail_n, gap = 1_000_000_200, 100, 300, 40
    rng = np.random.default_rng(91)
    piece = lambda n: rng.choice(np.frombuffer(b"ACGGT", np.uint8), size=n)  # G-rich: many NGG / CCN sites
    head, tail = piece(head_n), piece(tail_n)
    small = np.concatenate([head, np.full(gap, ord("N"), np.uint8), tail])
    shift = total - tail_n - (head_n + gap)
    rows = [(s, p if p <= head_n + gap else p + shift, z) for s, p, z in kmers.find_all_kmers(small, "NGG", 20, False)]
    widths = {len(str(p)) for _, p, _ in rows}
    assert {9, 10} <= widths and min(widths) <= 2, widths
    assert any(999_999_900 <= p <= 999_999_999 for _, p, _ in rows) and any(1_000_000_000 <= p < 1_000_000_100 for _, p, _ in rows)
    d = torch.full((total,), ord("N"), dtype=torch.uint8, device="cuda")
    d[:head_n] = torch.from_numpy(head).cuda()
    d[total - tail_n:] = torch.from_numpy(tail).cuda()
    torch.cuda.synchronize()
    km = api.generate_kmers(None, "NGG", 20, False, device=0, chrm_device_ptr=d.data_ptr(), chrm_len=total)
    try:
        check_against(km, rows, "NGG", "", "chrBig")
    finally:
        km.close()
        del d


# ---- gs_format_device_ids / gs_enumerate_text_device ---------------------------------------------------------------
class Candidates:
    """every candidate of a genome in one device stream (scan per chromosome, ids, concatenation) beside its index"""

    def __init__(self, text, names, lengths, start=False, prefix=""):
        assert sum(lengths) == text.shape[0]
        self.gs = api.make_genome_structure(names, lengths)
        self.index = api.GenomeIndex.build(text, device=0)
        parts, off = [], 0
        for name, ln in zip(names, lengths):
            km = api.generate_kmers(text[off:off + ln], "NGG", 20, start, device=0)
            km.encode_ids(prefix, name)
            parts.append(km)
            off += ln
        self.part_sizes = [p.n for p in parts]
        self.all = api.concat_kmers(parts)
        for p in parts:
            p.close()
        self.start = start
        seqs, pams, _, _ = self.all.to_host()
        self.seqs, self.pams = seqs, pams
        self.ids_blob, self.id_off, self.sense = self.all.ids_to_host()

    def close(self):
        self.all.close()
        self.index.close()

    def ids(self, lo, n):
        return [self.ids_blob[int(self.id_off[g]):int(self.id_off[g + 1])] for g in range(lo, lo + n)]


def toy_candidates(toy, **kw):
    return Candidates(np.ascontiguousarray(toy["text"], dtype=np.uint8), toy["names"], toy["lengths"], **kw)


@pytest.fixture(scope="module")
def toy_set(toy):
    c = toy_candidates(toy, prefix="t_")
    yield c
    c.close()


@pytest.fixture(scope="module")
def toy_set_start(toy):
    c = toy_candidates(toy, start=True)
    yield c
    c.close()


@pytest.fixture(scope="module")
def big_set():
    text, names, lengths = synth.make_genome([900_000, 700_000, 400_000], seed=33)
    c = Candidates(text, names, lengths)
    yield c
    c.close()


def test_concatenation_keeps_every_part(toy, toy_set):
    want_ids, want_rows, off = [], [], 0
    text = np.ascontiguousarray(toy["text"], dtype=np.uint8)
    for name, ln in zip(toy["names"], toy["lengths"]):
        rows = kmers.find_all_kmers(text[off:off + ln], "NGG", 20, False)
        want_ids += [f"t_{name}:{p}:{s}".encode() for _, p, s in rows]
        want_rows += rows
        off += ln
    assert toy_set.all.n == len(want_rows) > 0 and len(toy_set.part_sizes) == len(toy["names"])
    assert toy_set.ids(0, toy_set.all.n) == want_ids
    assert [r.tobytes().decode() for r in toy_set.seqs] == [s for s, _, _ in want_rows]
    assert np.array_equal(toy_set.sense, np.array([s == "+" for _, _, s in want_rows], np.uint8))
    assert int(toy_set.id_off[0]) == 0 and np.all(toy_set.id_off[1:] > toy_set.id_off[:-1])


def both_texts(c, lo, n, m, skip=None, sam=False, complete=True, max_off_targets=-1):
    """the text of candidates [lo, lo + n) by gs_format_device (ids from the host) and by gs_format_device_ids (ids in
    HBM, offsets beginning at id_off[lo]), each with its per-guide text offsets"""
    import torch
    L, P, km, g = 20, 3, c.all, c.index
    d_g, d_p = km.seqs_ptr + lo * L, km.pams_ptr + lo * P
    d_spec = torch.empty(n, dtype=torch.float32, device="cuda")
    with g.locked():
        d_off, d_hits, stats = g.enumerate_device(d_g, n, L, d_p, P, mismatches=m, start=c.start)
        g.score_device(c.gs, d_g, n, L, P, d_off, d_hits, None, d_spec.data_ptr(), sam=sam, start=c.start,
                       max_off_targets=max_off_targets)
        cfg = dict(sam=sam, complete=complete, start=c.start, max_off_targets=max_off_targets)
        d_text, ln = g.format_device(c.gs, d_g, n, L, d_p, P, c.ids(lo, n), list(c.sense[lo:lo + n]), skip, d_off, d_hits,
                                     d_spec.data_ptr(), m, **cfg)
        host_ids = from_device(d_text, ln), g.last_text_offsets(n)
        d_text, ln = g.format_device_ids(c.gs, d_g, n, L, d_p, P, km.ids_ptr, km.id_offsets_ptr + 8 * lo,
                                         km.sense_positive_ptr + lo, skip, d_off, d_hits, d_spec.data_ptr(), m, **cfg)
        dev_ids = from_device(d_text, ln), g.last_text_offsets(n)
    return host_ids, dev_ids, stats


FORMATS = [dict(complete=False), dict(), dict(sam=True, complete=False), dict(sam=True), dict(max_off_targets=2),
           dict(sam=True, max_off_targets=2)]
fmt_id = lambda c: "-".join(f"{k}{v}" for k, v in c.items()) or "default"


@pytest.mark.parametrize("cfg", FORMATS, ids=fmt_id)
def test_device_ids_give_the_text_of_host_ids_on_the_toy_genome(toy_set, cfg):
    n = toy_set.all.n
    for lo, cnt, skip in ((0, n, None), (5, n - 9, None), (3, n - 3, (np.arange(n - 3) % 3 == 1))):
        (want, want_off), (got, got_off), stats = both_texts(toy_set, lo, cnt, 3, skip=skip, **cfg)
        assert got == want and np.array_equal(got_off, want_off)
        assert stats["n_hits"] > 0 and (len(want) > 200 or cfg.get("sam"))
        assert toy_set.id_off[lo] != 0 or lo == 0


def test_device_ids_with_the_pam_at_the_start(toy_set_start):
    n = toy_set_start.all.n
    assert n > 10
    for cfg in (dict(), dict(sam=True)):
        (want, want_off), (got, got_off), _ = both_texts(toy_set_start, 2, n - 2, 2, **cfg)
        assert got == want and len(want) > 200 and np.array_equal(got_off, want_off)


@pytest.mark.parametrize("cfg", FORMATS[:4], ids=fmt_id)
def test_device_ids_give_the_text_of_host_ids_across_chromosomes(big_set, cfg):
    """a range that holds the tail of the first chromosome, the second one's head, with a skip mask: N runs lie around
    both ends"""
    n0 = big_set.part_sizes[0]
    assert len(big_set.part_sizes) == 3 and min(big_set.part_sizes) > 10_000
    lo, cnt = n0 - 3000, 6000
    skip = np.arange(cnt) % 7 == 3
    (want, want_off), (got, got_off), stats = both_texts(big_set, lo, cnt, 2, skip=skip, **cfg)
    assert got == want and np.array_equal(got_off, want_off)
    assert b"chr1:" in want and b"chr2:" in want and stats["n_hits"] >= cnt - 10 and int(big_set.id_off[lo]) > 0


def test_descending_id_offsets_are_refused_by_the_device(toy_set):
    import torch
    n, L, P, km, g = 4, 20, 3, toy_set.all, toy_set.index
    d_spec = torch.empty(n, dtype=torch.float32, device="cuda")
    bad = torch.from_numpy(np.array([0, 9, 4, 12, 20], np.int64)).cuda()
    torch.cuda.synchronize()
    with g.locked():
        d_off, d_hits, _ = g.enumerate_device(km.seqs_ptr, n, L, km.pams_ptr, P, mismatches=1)
        g.score_device(toy_set.gs, km.seqs_ptr, n, L, P, d_off, d_hits, None, d_spec.data_ptr())
        with pytest.raises(api.GsError) as e:
            g.format_device_ids(toy_set.gs, km.seqs_ptr, n, L, km.pams_ptr, P, km.ids_ptr, bad.data_ptr(), None, None, d_off, d_hits,
                                d_spec.data_ptr(), 1)
    assert e.value.status == 1


@pytest.mark.parametrize("cfg", [dict(), dict(sam=True), dict(complete=False, max_off_targets=2)], ids=fmt_id)
def test_fused_entry_equals_enumerate_text_on_downloaded_copies(toy_set, big_set, cfg):
    for c, lo, n, m in ((toy_set, 0, toy_set.all.n, 3), (toy_set, 7, 20, 3), (big_set, big_set.part_sizes[0] - 500, 1500, 2)):
        km, skip = c.all, (np.arange(n) % 5 == 2)
        for sk in (None, skip):
            want = c.index.enumerate_text(c.seqs[lo:lo + n], c.pams[lo:lo + n], c.ids(lo, n), list(c.sense[lo:lo + n]), c.gs,
                                          mismatches=m, skip=sk, **cfg)
            got = c.index.enumerate_text_device(km.seqs_ptr + lo * 20, n, 20, km.pams_ptr + lo * 3, 3, km.ids_ptr,
                                                km.id_offsets_ptr + 8 * lo, km.sense_positive_ptr + lo, c.gs, mismatches=m,
                                                skip=sk, **cfg)
            assert got == want and len(want) > 100


def test_fused_entry_serves_the_raw_counts_of_a_threshold_pass(toy_set):
    n = toy_set.all.n
    got = toy_set.index.raw_counts_device(toy_set.all.seqs_ptr, n, 20, toy_set.all.pams_ptr, 3, toy_set.gs, 1)
    want = toy_set.index.enumerate(toy_set.seqs, toy_set.pams, mismatches=1, raw_counts=True)[2]["raw_hits"]
    assert want is not None and np.array_equal(got, np.asarray(want, np.uint32))
    assert got.min() >= 1  # every candidate was cut from this genome


def test_fused_entry_answers_unsupported_beyond_the_key(toy, toy_set):
    """L = 25, P = 4: 2L + 3P = 62 > 59"""
    km = api.generate_kmers(np.ascontiguousarray(toy["text"], dtype=np.uint8)[:toy["lengths"][0]], "TTTN", 25, True, device=0)
    try:
        assert km.n > 0
        km.encode_ids("", toy["names"][0])
        out, ln = C.c_void_p(), C.c_uint64(5)
        rc = api.lib().gs_enumerate_text_device(toy_set.index._h, km.seqs_ptr, km.n, 25, km.pams_ptr, 4, None, 0, 2,
                                                api.GS_FLAG_PAM_AT_START, -1, C.byref(toy_set.gs), km.ids_ptr, km.id_offsets_ptr,
                                                km.sense_positive_ptr, None, C.byref(out), C.byref(ln), None, None)
        assert rc == 3 and out.value is None and ln.value == 0
    finally:
        km.close()
