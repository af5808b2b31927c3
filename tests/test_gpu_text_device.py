"""The CSV / SAM encoder on the device (gs_textdev.hip: gs_format_device, gs_enumerate_text) against the host encoder
(gs_format_guides_scored), byte for byte: the synthetic branches of tests/test_text_batch.py, the "%f" of the
specificity on ties and near-ties, real searches with chromosome-boundary hits and guides without hits, a guide with
more than 2^16 hits, and the fallback for a guide the fast path does not encode.  GPU only."""
import ctypes as C
from importlib import import_module

import numpy as np
import pytest

from test_text_batch import random_batch

api = import_module("guidescan-cli_amd.api")
synth = import_module("guidescan-cli_amd.synth")

pytestmark = pytest.mark.gpu

CFGS = [dict(), dict(complete=False), dict(start=True), dict(max_off_targets=2), dict(max_off_targets=0, complete=False),
        dict(sam=True), dict(sam=True, start=True)]  # the seven option sets of tests/test_text_batch.py
cfg_id = lambda c: "-".join(f"{k}{v}" for k, v in c.items()) or "default"


def _hip():
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return hip


@pytest.fixture(scope="module")
def handle(toy):
    """any handle: gs_format_device uses its workspace, not its index"""
    g = api.GenomeIndex.build(toy["text"], device=0)
    yield g
    g.close()


def device_text(gidx, gs, ids, seqs, pams, senses, offs, hits, spec, m, skip=None, **cfg):
    """format_device on uploaded arrays -> the text's bytes"""
    import torch
    n = len(ids)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    d_g = up(np.frombuffer("".join(seqs).encode(), np.uint8))
    d_p = up(np.frombuffer("".join(pams).encode(), np.uint8))
    d_o, d_s = up(np.asarray(offs, np.uint64)), up(np.asarray(spec, np.float32))
    hits = np.ascontiguousarray(hits, dtype=api.HIT_DTYPE)
    d_h = up(hits) if hits.shape[0] else None
    torch.cuda.synchronize()
    with gidx.locked():  # the text stays in the handle's buffer until it is copied
        d_text, ln = gidx.format_device(gs, d_g.data_ptr(), n, len(seqs[0]), d_p.data_ptr(), len(pams[0]), ids, senses, skip,
                                        d_o.data_ptr(), d_h.data_ptr() if d_h is not None else None, d_s.data_ptr(), m, **cfg)
        out = np.empty(ln, dtype=np.uint8)
        if ln:
            assert _hip().hipMemcpy(out.ctypes.data, d_text, ln, 2) == 0
    return out.tobytes()


@pytest.mark.parametrize("cfg", CFGS, ids=cfg_id)
def test_synthetic_branches_equal_the_host_encoder(handle, cfg):
    rng = np.random.default_rng(11)
    gs, ids, seqs, pams, senses, offs, hits, spec = random_batch(rng, 300)
    skip = (rng.random(300) < 0.1).astype(np.uint8)
    want = api.format_guides(gs, ids, seqs, pams, senses, offs, hits, spec, 3, skip=skip, **cfg)
    got = device_text(handle, gs, ids, seqs, pams, senses, offs, hits, spec, 3, skip=skip, **cfg)
    assert got == want
    assert want.count(b"\n") > 50
    # a sub-range whose offsets do not start at zero
    s = slice(100, 200)
    want2 = api.format_guides(gs, ids[s], seqs[s], pams[s], senses[s], offs[100:201], hits, spec[s], 3, **cfg)
    got2 = device_text(handle, gs, ids[s], seqs[s], pams[s], senses[s], offs[100:201], hits, spec[s], 3, **cfg)
    assert got2 == want2 and want2.count(b"\n") > 10


def _one_hit_batch(values):
    """a guide per value, each with one perfect hit inside chrA: every row prints its guide's specificity"""
    n = len(values)
    gs = api.make_genome_structure(["chrA", "chrB"], [5000, 3000])
    rng = np.random.default_rng(5)
    ids = [f"v{i}" for i in range(n)]
    seqs = ["".join(rng.choice(list("ACGT"), 20)) for _ in range(n)]
    pams = ["NGG"] * n
    senses = [bool(i & 1) for i in range(n)]
    offs = np.arange(n + 1, dtype=np.uint64)
    hits = np.zeros(n, dtype=api.HIT_DTYPE)
    hits["pos"] = rng.integers(100, 4000, n)
    hits["key"] = (2 << (59 - 2 * 20 - 3 + 1)) | (2 << (59 - 2 * 20 - 6 + 1)) | (2 << (59 - 2 * 20 - 9 + 1))  # PAM GGG, distance 0
    return gs, ids, seqs, pams, senses, offs, hits, np.asarray(values, np.float32)


def test_specificity_is_printed_as_printf_prints_it(handle):
    f32 = np.float32
    vals = [f32(0), f32(1), f32(0.5), f32(1) / f32(3), np.frombuffer(np.uint32(1).tobytes(), f32)[0]]
    # k * 1e-6 + 5e-7 with k = 7812 (2 j + 1) + j is (2 j + 1) / 128: a float, and an exact tie of the sixth decimal
    ties = [f32((2 * j + 1) / 128.0) for j in range(64)]
    assert all(float(t) * 1e6 % 1 == 0.5 for t in ties)
    near = [f32(0.9999995)]
    for v in ties + near:
        vals += [np.nextafter(v, f32(0)), v, np.nextafter(v, f32(2))]
    # ... and of decimal ties that are no floats: the two floats around k * 1e-6 + 5e-7
    for k in np.random.default_rng(7).integers(0, 999_999, 64):
        v = f32(k * 1e-6 + 5e-7)
        vals += [np.nextafter(v, f32(0)), v, np.nextafter(v, f32(2))]
    vals += list(np.random.default_rng(8).random(4096, dtype=np.float32))
    vals = np.asarray(vals, np.float32)
    assert vals.min() >= 0 and vals.max() <= 1
    b = _one_hit_batch(vals)
    for cfg in (dict(), dict(sam=True, complete=False)):
        want = api.format_guides(*b, 3, **cfg)
        got = device_text(handle, *b, 3, **cfg)
        assert want.count(b"\n") == len(vals)
        if got != want:
            w, g = want.split(b"\n"), got.split(b"\n")
            bad = [(float(vals[i]), w[i], g[i]) for i in range(min(len(w), len(g)) - 1) if w[i] != g[i]][:5]
            raise AssertionError(f"{len(bad)}+ rows differ, e.g. {bad}")
    assert b"0.007812\n" in want and b"0.023438\n" in want  # 7812.5 and 23437.5: half to even


@pytest.mark.parametrize("bad", [1.5, -0.25, float("nan")])
def test_a_specificity_outside_the_unit_interval_is_refused(handle, bad):
    b = list(_one_hit_batch([0.25, bad, 0.5]))
    with pytest.raises(api.GsError) as e:
        device_text(handle, *b, 3)
    assert e.value.status == 1  # GS_ERR_ARG, reported by the device


# ---- argument checks on a live handle: every one must answer GS_ERR_ARG, and before it reads an array -------------
BAD_ARGS = [dict(gs=None), dict(out=None), dict(out_len=None), dict(L=0), dict(L=32), dict(L=28, P=2), dict(P=9), dict(m=8),
            dict(max_off=-2), dict(n=1 << 31), dict(guides=None), dict(pams=None), dict(ids=None), dict(id_off=None),
            dict(id_off="falling"), dict(chr_names=None)]
bad_id = lambda k: "-".join(f"{a}_{b}" for a, b in k.items())


def _abi_args(kw):
    """the arguments both entries share, all valid (two 20-mers, ids "a" and "bc") unless kw says otherwise"""
    v = dict(gs=True, out=True, out_len=True, L=20, P=3, m=3, max_off=-1, n=2, guides=True, pams=True, ids=True, id_off=True,
             chr_names=True)
    unknown = set(kw) - set(v)
    assert not unknown, unknown
    v.update(kw)
    names = (C.c_char_p * 1)(b"c")
    lens = (C.c_uint64 * 1)(100000)
    g = api.GsGenomeStructure(names if v["chr_names"] else None, lens, 1)
    v["keep"] = (names, lens, g, C.create_string_buffer(b"abc"),
                 np.array([0, 3, 1] if v["id_off"] == "falling" else [0, 1, 3], np.uint64),
                 C.create_string_buffer(b"ACGTACGTACGTACGTACGTTGCATGCATGCATGCATGCA"), C.create_string_buffer(b"NGGNGG"))
    v["gs_p"] = C.byref(g) if v["gs"] else None
    v["ids_p"] = C.addressof(v["keep"][3]) if v["ids"] else None
    v["id_off_p"] = v["keep"][4].ctypes.data if v["id_off"] is not None else None
    return v


@pytest.mark.parametrize("kw", BAD_ARGS, ids=bad_id)
def test_null_and_bad_size_arguments_of_format_device(handle, kw):
    import torch
    v = _abi_args(kw)
    d_g = torch.from_numpy(np.frombuffer(v["keep"][5].raw[:40], np.uint8).copy()).cuda()
    d_p = torch.from_numpy(np.frombuffer(b"NGGNGG", np.uint8).copy()).cuda()
    d_o = torch.zeros(3, dtype=torch.int64, device="cuda")  # no hits
    d_s = torch.full((2,), 0.5, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    d_text, ln = C.c_void_p(), C.c_uint64()

    def call(v):
        return api.lib().gs_format_device(handle._h, v["gs_p"], d_g.data_ptr() if v["guides"] else None, v["n"], v["L"],
                                          d_p.data_ptr() if v["pams"] else None, v["P"], v["ids_p"], v["id_off_p"], None, None,
                                          d_o.data_ptr(), None, d_s.data_ptr(), v["m"], 0, v["max_off"], None,
                                          C.byref(d_text) if v["out"] else None, C.byref(ln) if v["out_len"] else None)
    assert call(v) == 1  # GS_ERR_ARG
    assert call(_abi_args({})) == 0 and ln.value > 0  # the same call with nothing wrong: two NA rows


@pytest.mark.parametrize("kw", BAD_ARGS, ids=bad_id)
def test_null_and_bad_size_arguments_of_enumerate_text(handle, kw):
    text, ln = C.c_void_p(), C.c_uint64()

    def call(v):
        return api.lib().gs_enumerate_text(handle._h, C.addressof(v["keep"][5]) if v["guides"] else None, v["n"], v["L"],
                                           C.addressof(v["keep"][6]) if v["pams"] else None, v["P"], None, 0, v["m"], 0,
                                           v["max_off"], v["gs_p"], v["ids_p"], v["id_off_p"], None, None,
                                           C.byref(text) if v["out"] else None, C.byref(ln) if v["out_len"] else None, None)
    assert call(_abi_args(kw)) == 1  # GS_ERR_ARG
    assert text.value is None
    assert call(_abi_args({})) == 0 and ln.value > 0  # the same call with nothing wrong
    api.lib().gs_free(text)


def test_alt_pams_without_a_pointer_are_refused(handle):
    v = _abi_args({})
    text, ln = C.c_void_p(), C.c_uint64()
    assert api.lib().gs_enumerate_text(handle._h, C.addressof(v["keep"][5]), 2, 20, C.addressof(v["keep"][6]), 3, None, 1, 3, 0, -1,
                                       v["gs_p"], v["ids_p"], v["id_off_p"], None, None, C.byref(text), C.byref(ln), None) == 1


def test_what_only_the_device_can_see_is_refused_too(handle):
    gs, ids, seqs, pams, senses, offs, hits, spec = _one_hit_batch([0.5, 0.5])
    with pytest.raises(api.GsError) as e:  # a distance beyond `mismatches`
        h2 = hits.copy()
        h2["key"] |= np.uint64(3) << np.uint64(61)
        device_text(handle, gs, ids, seqs, pams, senses, offs, h2, spec, 2)
    assert e.value.status == 1


def test_text_offsets_per_guide(handle):
    """gs_index_last_text_offsets: text[off[g]:off[g+1]] is guide g's own text, in CSV and in SAM"""
    rng = np.random.default_rng(12)
    gs, ids, seqs, pams, senses, offs, hits, spec = random_batch(rng, 200)
    skip = (rng.random(200) < 0.1).astype(np.uint8)
    for cfg in (dict(), dict(sam=True), dict(max_off_targets=1, complete=False)):
        with handle.locked():
            got = device_text(handle, gs, ids, seqs, pams, senses, offs, hits, spec, 3, skip=skip, **cfg)
            off = handle.last_text_offsets(200)
        assert off[0] == 0 and off[-1] == len(got) and (np.diff(off.astype(np.int64)) >= 0).all()
        for g in range(200):
            want = b"" if skip[g] else api.format_guide(gs, ids[g], seqs[g], pams[g], senses[g], hits[offs[g]:offs[g + 1]], 3,
                                                        specificity=spec[g], **cfg).encode()
            assert got[int(off[g]):int(off[g + 1])] == want, (cfg, g)
    with pytest.raises(api.GsError):
        handle.last_text_offsets(199)


# ---- real searches ----------------------------------------------------------------------------------------------
RUNS = [dict(), dict(complete=False), dict(sam=True), dict(sam=True, complete=False), dict(start=True),
        dict(alt_pams=("NAG",)), dict(sam=True, alt_pams=("NAG",)), dict(max_off_targets=0), dict(max_off_targets=2),
        dict(sam=True, max_off_targets=0), dict(sam=True, max_off_targets=2), dict(sam=True, start=True, max_off_targets=2)]


def host_text(gidx, gs, seqs, pams, ids, senses, m, skip=None, alt_pams=(), start=False, sam=False, complete=True,
              max_off_targets=-1):
    """enumerate + score + the host encoder -> (text, hits of the batch, rows or lines written)"""
    offsets, hits, st = gidx.enumerate(seqs, pams, mismatches=m, alt_pams=alt_pams, start=start)
    assert not st["needs_general"]
    _, spec = gidx.score(gs, seqs, pams.shape[1], offsets, hits, sam=sam, start=start, max_off_targets=max_off_targets,
                         want_cfd=False)
    s = [r.tobytes().decode() for r in seqs]
    p = [r.tobytes().decode() for r in pams]
    text = api.format_guides(gs, ids, s, p, senses, offsets, hits, spec, m, sam=sam, complete=complete, start=start,
                             max_off_targets=max_off_targets, skip=skip)
    return text, offsets, hits


def _check_genome(text, names, lengths, seqs, pams, ids, senses):
    gs = api.make_genome_structure(names, lengths)
    gidx = api.GenomeIndex.build(text, device=0)
    seen = dict(dropped=0, na=0, lines=0)
    try:
        n = seqs.shape[0]
        skip = np.zeros(n, np.uint8)
        skip[3::11] = 1
        for m in (0, 3):
            for i, run in enumerate(RUNS):
                for sk in ((None, skip) if not run else (skip if i & 1 else None,)):
                    want, offsets, hits = host_text(gidx, gs, seqs, pams, ids, senses, m, skip=sk, **run)
                    got = gidx.enumerate_text(seqs, pams, ids, senses, gs, mismatches=m, skip=sk, **run)
                    assert got == want, (m, run, sk is not None)
                    seen["lines"] += want.count(b"\n")
                    if not run and sk is None:
                        # rows the CSV printer left out: hits dropped at a chromosome boundary; NA rows: guides without hits
                        na = want.count(b",NA,NA,NA,0,")
                        seen["na"] += na
                        seen["dropped"] += int(hits.shape[0]) - (want.count(b"\n") - na)
                        assert na == int((np.diff(offsets.astype(np.int64)) == 0).sum())
    finally:
        gidx.close()
    return seen


def test_real_searches_on_the_toy_genome(toy):
    km = [k for k in toy["kmers"] if len(k.sequence) == 20 and len(k.pam) == 3 and set(k.sequence) <= set("ACGT")]
    assert len(km) >= 4
    seqs = np.array([np.frombuffer(k.sequence.encode(), np.uint8) for k in km])
    pams = np.array([np.frombuffer(k.pam.encode(), np.uint8) for k in km])
    # a guide without hits among them
    seqs = np.vstack([seqs, np.frombuffer(b"ACGTTGCAACGTTGCAACGT", np.uint8)])
    pams = np.vstack([pams, pams[:1]])
    ids = [k.id for k in km] + ["nohit"]
    senses = [k.positive for k in km] + [False]
    seen = _check_genome(toy["text"], toy["names"], toy["lengths"], seqs, pams, ids, senses)
    assert seen["lines"] > 100 and seen["na"] >= 1


def test_real_searches_across_short_chromosomes():
    """chromosomes of 70 bases: guides drawn from the concatenated text often straddle two of them, so their hits are
    dropped by resolve_absolute (CSV: no row; SAM: a line with an empty RNAME)"""
    lengths = [70] * 150 + [4000, 2500]
    text, names, lengths = synth.make_genome(lengths, seed=21)
    seqs, pams, _, strands = synth.sample_guides(text, 96, seed=22)
    seqs = np.vstack([seqs, np.frombuffer(b"ACGTTGCAACGTTGCAACGT", np.uint8)])
    pams = np.vstack([pams, pams[:1]])
    n = seqs.shape[0]
    ids = [f"guide_{i}:{'x' * (i % 7)}" for i in range(n)]
    senses = [bool(s == ord("+")) for s in strands] + [True]
    seen = _check_genome(text, names, lengths, seqs, pams, ids, senses)
    assert seen["dropped"] >= 1, "no hit was dropped at a chromosome boundary: the test proves less than it claims"
    assert seen["na"] >= 1, "no guide without hits"
    assert seen["lines"] > 1000


def test_a_guide_with_more_than_2_16_hits():
    """rows are the unit of work, not guides: one guide's 70,000 hits (eight perfect ones, the rest at one to three
    substitutions) spread over the chip like any others.  The host encoder's own output is the expected text."""
    rng = np.random.default_rng(31)
    guide = np.frombuffer(b"GATTACAGGCTCATTGCAGT", np.uint8)
    copies, unit = 70_000, 32
    block = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (copies, unit))].copy()
    block[:, :20] = guide
    subs, col0 = rng.integers(1, 4, copies - 8), rng.integers(0, 20, copies - 8)
    for k in (1, 2, 3):  # one to three substitutions, at distinct positions, in all but eight copies
        rows = np.arange(8, copies)[subs >= k]
        cols = (col0[subs >= k] + 7 * k) % 20
        block[rows, cols] = np.frombuffer(b"ACGT", np.uint8)[(rng.integers(1, 4, rows.shape[0]) +
                                                              np.searchsorted(np.frombuffer(b"ACGT", np.uint8), block[rows, cols])) % 4]
    block[:, 21:23] = ord("G")
    text = np.ascontiguousarray(block.reshape(-1))
    names, lengths = ["r1", "r2"], [copies * unit // 2, copies * unit // 2]
    gs = api.make_genome_structure(names, lengths)
    seqs = np.vstack([guide, np.frombuffer(b"ACGTTGCAACGTTGCAACGT", np.uint8)])
    pams = np.tile(np.frombuffer(b"NGG", np.uint8), (2, 1))
    ids, senses = ["many", "few"], [True, False]
    gidx = api.GenomeIndex.build(text, device=0)
    try:
        for run in (dict(), dict(sam=True), dict(sam=True, complete=False), dict(max_off_targets=5), dict(sam=True, max_off_targets=5)):
            want, offsets, hits = host_text(gidx, gs, seqs, pams, ids, senses, 3, **run)
            assert int(offsets[1] - offsets[0]) >= 1 << 16
            got = gidx.enumerate_text(seqs, pams, ids, senses, gs, mismatches=3, **run)
            assert len(got) == len(want) and got == want, run
            if not run:
                assert want.count(b"\n") >= 1 << 16
    finally:
        gidx.close()


def test_a_guide_outside_the_fast_path_is_left_to_the_caller(toy, handle):
    gs = api.make_genome_structure(toy["names"], toy["lengths"])
    km = [k for k in toy["kmers"] if len(k.sequence) == 20 and set(k.sequence) <= set("ACGT")][:3]
    seqs = np.array([np.frombuffer(k.sequence.encode(), np.uint8) for k in km] + [np.frombuffer(b"ACGTNGCAACGTTGCAACGT", np.uint8)])
    pams = np.tile(np.frombuffer(b"NGG", np.uint8), (4, 1))
    with pytest.raises(api.GsError) as e:
        handle.enumerate_text(seqs, pams, ["a", "b", "c", "n"], [True] * 4, gs, mismatches=2)
    assert e.value.status == 3  # GS_ERR_UNSUPPORTED: nothing is returned
    assert handle.enumerate_text(seqs[:3], pams[:3], ["a", "b", "c"], [True] * 3, gs, mismatches=2).count(b"\n") >= 3


TILE_LDS = 12288   # the bytes of a wave's slice (GS_ROW_LDS, csrc/gs_rowtext.h)


@pytest.mark.parametrize("cfg", [dict(), dict(sam=True)], ids=cfg_id)
def test_a_tile_at_the_border_of_the_lds_slice(handle, cfg):
    """A tile is composed in the wave's slice while a0 + total <= 12288 (a0: the tile's offset in the text mod 16) and
    straight in HBM beyond.  The second tile of a batch of one-hit guides - 32 rows, a row per hit slot - is padded with
    long ids to 12288 - 24 bytes; then one guide's id grows byte by byte over 48 values, so the tile's total passes the
    border whatever a0 is.  With sam=True every line carries an of:H: field, the span the wave copies afterwards."""
    n, lo, swept = 74, 32, 45   # tiles of 32 guides: [0, 32) short rows, [32, 64) the padded tile, [64, 74) a partial tile
    gs, ids, seqs, pams, senses, offs, hits, spec = _one_hit_batch(np.linspace(0.0, 1.0, n))

    def rows_of_tile(ids):
        lines = api.format_guides(gs, ids, seqs, pams, senses, offs, hits, spec, 3, **cfg).split(b"\n")[:-1]
        assert len(lines) == n
        return sum(len(x) + 1 for x in lines[lo:lo + 32])

    extra = TILE_LDS - 24 - rows_of_tile(ids)   # an id stands once in its row
    assert extra > 32 * 100
    ids = [x + "p" * (extra // 32 + (extra % 32 if i == swept else 0)) if lo <= i < lo + 32 else x for i, x in enumerate(ids)]
    totals = []
    for j in range(48):
        grown = [x + "q" * j if i == swept else x for i, x in enumerate(ids)]
        want = api.format_guides(gs, grown, seqs, pams, senses, offs, hits, spec, 3, **cfg)
        totals.append(rows_of_tile(grown))
        assert device_text(handle, gs, grown, seqs, pams, senses, offs, hits, spec, 3, **cfg) == want, f"id grown by {j}"
    assert totals == list(range(TILE_LDS - 24, TILE_LDS + 24))
