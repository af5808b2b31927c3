"""`guidescan controls` on the GPU: gs_controls_generate (k_ct_generate, k_ct_gather, the search, k_ct_keep, k_ct_old,
k_ct_walk, k_ct_count and the id passes of csrc/gs_controls.hip) against the host twin fed the oracle's targeting bits,
which tests/test_controls_model.py holds to tests/controls_model.py: kept counters, rows byte for byte and every count of
the report, at the round sizes and N on the edges of the kernels' steps.  Every case asserts that it decides something."""
from importlib import import_module

import numpy as np
import pytest

import controls_cases as cc
import controls_model as cm

api = import_module("guidescan-cli_amd.api")

pytestmark = pytest.mark.gpu

GC_TTTT = dict(gc=(40, 70), exclude_motifs=("TTTT",))


@pytest.fixture(scope="module")
def index():
    ix = api.GenomeIndex.build(cc.genome()[0], device=0)
    yield ix
    ix.close()


@pytest.fixture(scope="module")
def bare():
    """an index over a genome with no NGG site on either strand: 20,000 random bases with every GG and CC broken up"""
    rng = np.random.default_rng(11)
    t = bytearray(rng.choice(np.frombuffer(b"ACGT", dtype=np.uint8), 20000).tobytes())
    for i in range(1, len(t)):
        if t[i] == t[i - 1] and t[i] in b"GC":
            t[i] = ord("A") if t[i] == ord("G") else ord("T")
    text = np.frombuffer(bytes(t), dtype=np.uint8)
    assert b"GG" not in bytes(t) and b"CC" not in bytes(t) and len(set(bytes(t))) == 4
    ix = api.GenomeIndex.build(text, device=0)
    yield ix
    ix.close()


def twin(bits, n, rule=None, **kw):
    for k in ("round", "alt_pams", "start", "mismatches"):
        kw.pop(k, None)
    kw.setdefault("L", cc.L)
    kw.setdefault("seed", cc.SEED)
    kw.setdefault("max_candidates", len(bits))
    return api.controls_host_model(bits, n, seq_rule=api.SeqRule(**rule) if rule else None, **kw)


def check(ix, bits, n, rule=None, **kw):
    """the device against the twin over the same candidates -> (report, kept counters)"""
    want = twin(bits, n, rule, **dict(kw))
    kw.setdefault("L", cc.L)
    kw.setdefault("seed", cc.SEED)
    kw.setdefault("mismatches", cc.M)
    kw.setdefault("max_candidates", len(bits))
    km, rep = api.controls(ix, n, seq_rule=api.SeqRule(**rule) if rule else None, **kw)
    try:
        counters = km.control_counters()
        assert counters.tolist() == want[0].tolist()
        assert km.controls_rows() == want[1]
        assert {k: rep[k] for k in cc.COUNTS} == {k: want[2][k] for k in cc.COUNTS}
        assert km.n == rep["kept"] == len(counters) and rep["rounds"] >= 1
        seqs, pams, pos, sense = km.to_host()
        rows = want[1].decode().splitlines()
        assert pos is None and sense.tobytes() == b"+" * km.n
        assert [f"{i},{bytes(s).decode()},{bytes(p).decode()},NA,0,+" for i, s, p in
                zip((f"{kw.get('prefix', 'control_')}{c}" for c in counters), seqs, pams)] == rows
        ids, off, sp = km.ids_to_host()
        assert [ids[off[i]:off[i + 1]].decode() for i in range(km.n)] == [r.split(",")[0] for r in rows] and sp.tolist() == [1] * km.n
    finally:
        km.close()
    return rep, counters


def test_the_device_is_the_twin_with_the_oracle_s_bits(index):
    bits = cc.targeting()
    rep, _ = check(index, bits[:2048], 5000)
    assert rep["kept"] == 1346 and cc.decides(rep, "targeting")
    rep, _ = check(index, bits, 5000, min_distance=4)
    assert (rep["kept"], rep["close"]) == (1772, 913) and cc.decides(rep, "targeting", "close")
    rep, _ = check(index, bits, 5000, GC_TTTT, min_distance=4)
    assert (rep["kept"], rep["close"]) == (1419, 638) and cc.decides(rep, "gc", "targeting", "close") and rep["motif"] > 0
    rep, _ = check(index, bits, 5000, dict(max_run=2, exclude_sites=("GGATC",)), min_distance=3, prefix="ctl:")
    assert rep["run"] > 400 and cc.decides(rep, "targeting")


@pytest.mark.parametrize("rounds", [63, 64, 65, 255, 256, 257, 4096])
def test_the_round_size_changes_nothing(index, rounds):
    bits = cc.targeting()
    rep, _ = check(index, bits, 5000, GC_TTTT, min_distance=4, round=rounds)
    assert rep["rounds"] == -(-4096 // rounds) and (rep["kept"], rep["close"]) == (1419, 638)
    rep, _ = check(index, bits, 700, min_distance=4, round=rounds)
    assert rep["kept"] == 700 and rep["looked_at"] < 4096 and cc.decides(rep, "targeting") and rep["close"] > 100


def test_n_on_the_edges_of_a_round_and_of_the_walk_s_step(index):
    bits = cc.targeting()
    kept = twin(bits, 5000)[0]
    in_first = int((kept < 256).sum())
    assert 100 < in_first < 256 and kept[in_first] >= 256
    # the N-th control is the last non-targeting candidate of round 1, then the first of round 2
    rep, got = check(index, bits, in_first, round=256)
    assert rep["rounds"] == 1 and rep["last_counter"] == int(got[-1]) < 256 and not bits[int(got[-1])]
    assert bits[int(got[-1]) + 1:256].all()
    rep, got = check(index, bits, in_first + 1, round=256)
    assert rep["rounds"] == 2 and rep["last_counter"] == int(got[-1]) >= 256 and bits[256:int(got[-1])].all()
    # the walk's kept set crosses its step of 64 inside one round
    for n in (64, 65, 257):
        for h in (1, 4):
            rep, got = check(index, bits, n, min_distance=h, round=4096)
            assert rep["kept"] == n and rep["rounds"] == 1 and rep["last_counter"] == int(got[-1])
    # H = 4 with N across two and three rounds: both distance kernels decide
    kept4 = twin(bits, 5000, min_distance=4)[0]
    for rounds_wanted in (2, 3):
        n = int((kept4 < 1024 * (rounds_wanted - 1)).sum()) + 50
        rep, got = check(index, bits, n, min_distance=4, round=1024)
        assert rep["rounds"] == rounds_wanted and rep["kept"] == n and rep["close"] > 100 and cc.decides(rep, "targeting")
        later = cm.walk(bits, n, cc.L, seed=cc.SEED, min_distance=4)[3][1024 * (rounds_wanted - 1):rep["looked_at"]]
        assert later.count(cm.CLOSE) > 10                                # the last round charges the distance rule too


def test_alt_pams_start_and_counters_near_two_to_the_32(index):
    nag = cc.targeting(alt=("NAG",))
    rep, _ = check(index, nag[:2048], 5000, alt_pams=("NAG",))
    assert rep["kept"] == 806 and cc.decides(rep, "targeting")
    start = cc.targeting(n=2048, start=True)
    assert (start != cc.targeting()[:2048]).sum() > 200                  # another search, not the same bits
    rep, _ = check(index, start, 5000, start=True, min_distance=3, round=1000)
    assert cc.decides(rep, "targeting") and rep["close"] > 0
    first = 2 ** 32 - 100
    high = cc.targeting(first=first, n=256)
    rep, got = check(index, high, 5000, first=first, min_distance=3, round=64)
    assert cc.decides(rep, "targeting") and got.min() < 2 ** 32 <= got.max() and rep["last_counter"] == first + 255


def test_none_kept(index):
    bits = cc.targeting()
    j = int(np.flatnonzero(bits)[0])
    rep, got = check(index, bits[j:j + 1], 5, first=j)
    assert (rep["kept"], rep["looked_at"], rep["targeting"], len(got)) == (0, 1, 1, 0)
    # and a round in which nothing passes the sequence rule is not searched at all
    rep, got = check(index, bits[:300], 5, dict(exclude_motifs=("N",)), round=100)
    assert (rep["kept"], rep["looked_at"], rep["motif"], rep["rounds"]) == (0, 300, 300, 3)


def test_generator_and_distance_without_the_search_deciding(bare):
    none = np.zeros(4096, dtype=np.uint8)
    words = cm.sequences(cc.SEED, 0, 4096, 6)
    for rounds in (0, 100, 4096):
        rep, got = check(bare, none, 5000, L=6, round=rounds)
        assert rep["targeting"] == 0 and rep["kept"] == len(set(words)) and rep["close"] == 4096 - rep["kept"] > 1000
    rep, _ = check(bare, none, 5000, L=6, min_distance=0, round=1000)
    assert rep["kept"] == 4096
    rep, _ = check(bare, none, 5000, L=6, min_distance=7, round=1000)
    assert (rep["kept"], rep["close"]) == (1, 4095)
    rep, _ = check(bare, none[:1024], 5000, L=6, min_distance=3, round=100)
    assert 10 < rep["kept"] < 400
    rep, _ = check(bare, none, 5000, L=20, pam="NGG", min_distance=9, round=1000)       # 2L + 3P = 49
    assert rep["kept"] > 100 and rep["close"] > 100
    # L = 31 is beyond the fast path's key with any PAM (2L + 3P <= 59): refused, with the message
    with pytest.raises(api.GsError) as e:
        api.controls(bare, 5, L=31, max_candidates=10)
    assert e.value.status == 3 and "2L + 3P > 59" in str(e.value)


def test_n_is_bounded_by_what_the_walk_holds_in_lds(bare):
    """N <= 16,384 for every H: the bound on N is what bounds the quadratic distance passes"""
    for h in (0, 1, 2):
        with pytest.raises(api.GsError) as e:
            api.controls(bare, 16385, L=9, min_distance=h, max_candidates=10)
        assert e.value.status == 1
    none = np.zeros(600, dtype=np.uint8)
    rep, _ = check(bare, none, 16384, L=9, round=256)                      # the largest N, far from filled
    assert rep["kept"] + rep["close"] == 600 and rep["rounds"] == 3


def test_the_controls_go_into_the_database_encoder(index):
    text, names, lengths = cc.genome()
    gs = api.make_genome_structure(names, lengths)
    km, rep = api.controls(index, 300, L=cc.L, seed=cc.SEED, mismatches=cc.M, min_distance=3, round=2048)
    try:
        assert rep["kept"] == 300
        got = index.enumerate_text_device(km.seqs_ptr, km.n, km.k, km.pams_ptr, km.P, km.ids_ptr, km.id_offsets_ptr, km.sense_positive_ptr, gs,
                                          mismatches=cc.M)
        seqs = km.to_host()[0]
        want = "".join(f"control_{c},{bytes(s).decode()}NGG,NA,NA,NA,0,NA,NA,NA,1.0\n" for c, s in zip(km.control_counters(), seqs))
        assert got.decode() == want
        with pytest.raises(api.GsError):
            km.encode_ids("x", "chr1")
        with pytest.raises(api.GsError):
            km.csv("x", "chr1")
    finally:
        km.close()
