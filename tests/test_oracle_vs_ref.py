"""Pin the oracle's FM-index primitives and helpers against the REFERENCE'S OWN SOURCES
compiled in place (oracle/_ref, built by oracle/Makefile where the reference tree can be read):
sdsl::wt_huff rank / inverse_select, byte_alphabet C/char2comp, int_vector I/O,
genomics::resolve_absolute, (reverse_)complement, Doench tables.  CPU only.
Each comparison holds against oracle/_ref where it was built, and always against the sha256 of the
reference's values recorded in tests/golden/reference/primitives.json (tools/make_ref_goldens.py);
the index-file round trip needs oracle/_ref itself and is skipped without it."""
import ctypes as C
import hashlib
import itertools
import json
import tempfile
from importlib import import_module

import numpy as np
import pytest

import oracle_lib as ol

ref = ol.ref()
needs_ref = pytest.mark.skipif(ref is None, reason="oracle/_ref not built (no reference tree)")
REF_DIGESTS = ol.ROOT / "tests" / "golden" / "reference" / "primitives.json"


def digest(values):
    return hashlib.sha256(np.ascontiguousarray(values).tobytes()).hexdigest()


def pinned(name, got, want=None):
    """the oracle's values `got` equal the reference's: `want` (live, where oracle/_ref was built) and the recorded digest"""
    if want is not None:
        assert got.dtype == want.dtype and got.shape == want.shape
        bad = np.nonzero(got != want)[0] if got.ndim == 1 else np.nonzero((got != want).any(axis=tuple(range(1, got.ndim))))[0]
        assert bad.size == 0, (name, bad[:10])
    assert digest(got) == json.loads(REF_DIGESTS.read_text())[name], name


def make_ref_index(oidx_handle, n):
    L = ol.lib()
    bwt = np.array([L.gso_bwt(oidx_handle, i) for i in range(n)], dtype=np.uint8)
    sa = np.empty(n, dtype=np.uint32)
    L.gso_copy_sa(oidx_handle, sa.ctypes.data)
    tmp = tempfile.NamedTemporaryFile(delete=False, suffix=".sdsl")
    tmp.close()
    h = ref.ref_index_build(bwt.ctypes.data, sa.ctypes.data, n, tmp.name.encode())
    return h, bwt, sa


@pytest.fixture(scope="module")
def pair(toy):
    oidx = ol.OracleIndex(toy["text"])
    n = toy["text"].shape[0] + 1
    refs = None
    if ref is not None:
        rf, _, _ = make_ref_index(oidx.fwd, n)
        rr, _, _ = make_ref_index(oidx.rev, n)
        refs = (rf, rr)
    yield oidx, n, refs
    if refs is not None:
        ref.ref_index_free(refs[0])
        ref.ref_index_free(refs[1])
    oidx.close()


# ---- the values each test compares: the oracle's side and the reference's side, built the same way ----
RANK_SYMBOLS = b"\x00ACGNTXacgt"


def rank_rows(n):
    rng = np.random.default_rng(0)
    return np.unique(np.concatenate([rng.integers(0, n + 1, 3000), np.arange(0, 700),
                                     np.arange(n - 700, n + 1), [5000, 5500, 12345]]))


def rank_values(rank, handles, n):
    rows = rank_rows(n)
    return np.array([[[rank(h, int(i), c) for c in RANK_SYMBOLS] for i in rows] for h in handles], dtype=np.uint64)


def c_values(fn, handles):
    return np.array([[fn(h, c) for c in range(256)] for h in handles], dtype=np.uint64)


def locate_values(fn, handles, n):
    return np.array([[fn(h, i) for i in range(0, n, 3)] for h in handles], dtype=np.uint64)


def inverse_select_ref(rh, n):
    r, c = C.c_uint64(), C.c_uint8()
    out = []
    for i in range(0, n, 11):
        ref.ref_inverse_select(rh, i, C.byref(r), C.byref(c))
        out.append((r.value, c.value))
    return np.array(out, dtype=np.uint64)


def inverse_select_oracle(oh, n):
    L = ol.lib()
    out = []
    for i in range(0, n, 11):
        c = L.gso_bwt(oh, i)
        out.append((L.gso_rank_bwt(oh, i, c), c))
    return np.array(out, dtype=np.uint64)


def exotic_text():
    """a text with IUPAC symbols, lowercase and a long run"""
    rng = np.random.default_rng(4)
    text = rng.choice(np.frombuffer(b"ACGTNRYKMacgt", np.uint8), 5000,
                      p=[.2, .2, .2, .2, .05, .02, .02, .02, .02, .0175, .0175, .0175, .0175])
    text[1000:1400] = ord("N")
    return text


EXOTIC_SYMBOLS = b"\x00ACGTNRYKMacgtZ"


def exotic_values(C_fn, rank_fn, locate_fn, h, n):
    cs = np.array([C_fn(h, c) for c in range(256)], dtype=np.uint64)
    ranks = np.array([[rank_fn(h, i, c) for c in EXOTIC_SYMBOLS] for i in list(range(0, n + 1, 13)) + [n]], dtype=np.uint64)
    locs = np.array([locate_fn(h, i) for i in range(0, n, 7)], dtype=np.uint64)
    return np.concatenate([cs, ranks.ravel(), locs])


RESOLVE_LENS = np.array([100, 57, 23, 300], dtype=np.uint64)


def resolve_values(fn):
    """(status, start, strand) over every interesting coordinate incl. boundaries, -0, both strands; start and strand only
    where the status says they are set"""
    total = int(RESOLVE_LENS.sum())
    out = []
    for seq_len, pam_len in ((20, 3), (20, 0), (23, 3), (5, 2)):
        for a in range(-total - 3, total + 3):
            if abs(a) >= total:
                # beyond the genome the reference hits an assert compiled out in Release; the
                # oracle returns the sentinel.  Not a reachable input (SA values < total).
                continue
            s, t = C.c_int64(-9), C.c_char(b"?")
            c = fn(RESOLVE_LENS.ctypes.data, 4, a, seq_len, pam_len, C.byref(s), C.byref(t))
            out.append((c, s.value, t.value[0]) if c >= 0 else (c, 0, 0))
    return np.array(out, dtype=np.int64)


def complement_inputs():
    rng = np.random.default_rng(2)
    alphabet = np.frombuffer(b"ACGTNacgtnRYxz.-", np.uint8)
    return [rng.choice(alphabet, rng.integers(1, 40)).tobytes() for _ in range(200)]


def complement_ref():
    out = []
    for s in complement_inputs():
        buf = C.create_string_buffer(64)
        ref.ref_reverse_complement(s, buf)
        out.append(buf.value)
    return np.frombuffer(b"\n".join(out), dtype=np.uint8)


def complement_oracle():
    synth = import_module("guidescan-cli_amd.synth")
    out = [synth.reverse_complement_bytes(np.frombuffer(s, np.uint8)).tobytes() for s in complement_inputs()]
    return np.frombuffer(b"\n".join(out), dtype=np.uint8)


CFD_GUIDE = "ACGTACGTACGTACGTACGT"


def cfd_cases():
    """every (rna, dna, position) whose guide / target pair has exactly that mismatch at that position"""
    for pos in range(20):
        for r in "ACGU":
            for d in "ACGT":
                guide_base = "T" if r == "U" else r
                target_base = {"A": "T", "C": "G", "G": "C", "T": "A"}[d]  # d = complement(target)
                if target_base != guide_base:
                    yield pos, r, d, guide_base, target_base


def cfd_ref():
    """the reference's std::maps as the oracle's float32 CFD must reproduce them: every mismatch entry, then every PAM pair"""
    mm = [np.float32(np.float64(np.float32(1.0)) * ref.ref_mm_score(r.encode(), d.encode(), pos + 1))
          for pos, r, d, _, _ in cfd_cases()]
    pam = [np.float32(ref.ref_pam_score(a.encode(), b.encode())) for a, b in itertools.product("ACGT", repeat=2)]
    return np.array(mm + pam, dtype=np.float32)


def cfd_oracle():
    L = ol.lib()
    g = CFD_GUIDE
    mm = []
    for pos, r, d, guide_base, target_base in cfd_cases():
        guide = g[:pos] + guide_base + g[pos + 1:]
        target = guide[:pos] + target_base.lower() + guide[pos + 1:]
        mm.append(L.gso_calculate_cfd(guide.encode(), target.encode(), b"AGG"))
    pam = [L.gso_calculate_cfd(g.encode(), g.encode(), ("A" + a + b).encode()) for a, b in itertools.product("ACGT", repeat=2)]
    return np.array(mm + pam, dtype=np.float32)


# ---- the tests ----
def test_rank_bwt_all_symbols(pair):
    oidx, n, refs = pair
    L = ol.lib()
    got = rank_values(L.gso_rank_bwt, (oidx.fwd, oidx.rev), n)
    pinned("rank_bwt_all_symbols", got, rank_values(ref.ref_rank_bwt, refs, n) if refs else None)


def test_C_and_char2comp(pair):
    oidx, n, refs = pair
    L = ol.lib()
    if refs:
        for rh in refs:
            assert ref.ref_sigma(rh) == 6  # \0 A C G N T
    pinned("C", c_values(L.gso_C, (oidx.fwd, oidx.rev)), c_values(ref.ref_C, refs) if refs else None)


def test_locate_every_row(pair):
    """csa[i] for every row: oracle LF walk == walk over the real wt_huff/inverse_select == SA"""
    oidx, n, refs = pair
    L = ol.lib()
    got = locate_values(L.gso_locate, (oidx.fwd, oidx.rev), n)
    for k, which in enumerate(("fwd", "rev")):
        assert np.array_equal(got[k], oidx.sa(which)[0:n:3].astype(np.uint64))
    pinned("locate_every_third_row", got, locate_values(ref.ref_locate, refs, n) if refs else None)


def test_inverse_select_is_bwt_and_rank(pair):
    oidx, n, refs = pair
    pinned("inverse_select", inverse_select_oracle(oidx.fwd, n), inverse_select_ref(refs[0], n) if refs else None)


def test_exotic_alphabet():
    """a text with IUPAC symbols, lowercase and a long run: ranks and C agree"""
    text = exotic_text()
    oidx = ol.OracleIndex(text)
    n = text.shape[0] + 1
    L = ol.lib()
    rh = make_ref_index(oidx.fwd, n)[0] if ref is not None else None
    try:
        got = exotic_values(L.gso_C, L.gso_rank_bwt, L.gso_locate, oidx.fwd, n)
        want = exotic_values(ref.ref_C, ref.ref_rank_bwt, ref.ref_locate, rh, n) if rh is not None else None
        pinned("exotic_alphabet", got, want)
    finally:
        if rh is not None:
            ref.ref_index_free(rh)
        oidx.close()


def test_resolve_absolute_grid():
    """structures.cxx:7-52 over every interesting coordinate incl. boundaries, -0, both strands"""
    L = ol.lib()
    pinned("resolve_absolute_grid", resolve_values(L.gso_resolve_absolute),
           resolve_values(ref.ref_resolve_absolute) if ref is not None else None)


def test_complement_and_reverse_complement():
    pinned("reverse_complement", complement_oracle(), complement_ref() if ref is not None else None)


def test_cfd_tables_match_doench_header():
    """every (rna, dna, position) and PAM pair the reference's std::maps hold"""
    if ref is not None:
        # the entries the maps hold are exactly the mismatches cfd_cases() builds: 240 of them, every PAM pair
        held = [(pos, r, d) for pos in range(20) for r in "ACGU" for d in "ACGT" if ref.ref_mm_score(r.encode(), d.encode(), pos + 1) >= 0]
        assert held == [(pos, r, d) for pos, r, d, _, _ in cfd_cases()] and len(held) == 240
        assert all(ref.ref_pam_score(a.encode(), b.encode()) >= 0 for a, b in itertools.product("ACGT", repeat=2))
    pinned("cfd_tables", cfd_oracle(), cfd_ref() if ref is not None else None)


@needs_ref
def test_reference_format_index_file_roundtrip(pair, tmp_path):
    """the shim writes a file in csa_wt::serialize order with each part's own serialize();
    the toy index files produced by the survey build have the same size (same layout)."""
    oidx, n, refs = pair
    p = tmp_path / "toy.forward"
    assert ref.ref_write_index_file(refs[0], str(p).encode()) == 0
    golden = ol.ROOT / "tests" / "golden" / "toy" / "toy.idx.forward"
    assert p.stat().st_size == golden.stat().st_size
    assert p.read_bytes() == golden.read_bytes()


def reference_digests(toy_text):
    """the digests of primitives.json, from oracle/_ref (tools/make_ref_goldens.py)"""
    out = {}
    oidx = ol.OracleIndex(toy_text)
    n = toy_text.shape[0] + 1
    refs = (make_ref_index(oidx.fwd, n)[0], make_ref_index(oidx.rev, n)[0])
    try:
        out["rank_bwt_all_symbols"] = digest(rank_values(ref.ref_rank_bwt, refs, n))
        out["C"] = digest(c_values(ref.ref_C, refs))
        out["locate_every_third_row"] = digest(locate_values(ref.ref_locate, refs, n))
        out["inverse_select"] = digest(inverse_select_ref(refs[0], n))
    finally:
        for h in refs:
            ref.ref_index_free(h)
        oidx.close()
    text = exotic_text()
    oidx = ol.OracleIndex(text)
    n = text.shape[0] + 1
    rh = make_ref_index(oidx.fwd, n)[0]
    try:
        out["exotic_alphabet"] = digest(exotic_values(ref.ref_C, ref.ref_rank_bwt, ref.ref_locate, rh, n))
    finally:
        ref.ref_index_free(rh)
        oidx.close()
    out["resolve_absolute_grid"] = digest(resolve_values(ref.ref_resolve_absolute))
    out["reverse_complement"] = digest(complement_ref())
    out["cfd_tables"] = digest(cfd_ref())
    return out
