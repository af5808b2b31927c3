"""The BGZF inflater's host/device header (csrc/gs_bgzf_inflate.h) through its host-only entry points: the function a
lane of k_bgzf_inflate runs against Python's zlib on members of every block type, and the member table's walk.  No GPU.
(`make -C guidescan-cli_amd/csrc inflate-check` runs the same header under the sanitizers.)"""
import random
import struct
import zlib
from importlib import import_module
from pathlib import Path

import pytest

import bam_make

api = import_module("guidescan-cli_amd.api")
DAMAGED = Path(__file__).resolve().parent / "golden" / "bgzf_inflate" / "damaged.txt"


def make_member(raw, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=None, extra=b"", extra_first=True):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    if flush_at is None:
        data = c.compress(raw) + c.flush()
    else:
        data = c.compress(raw[:flush_at]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(raw[flush_at:]) + c.flush()
    size = 12 + 6 + len(extra) + len(data) + 8
    bc = b"BC\2\0" + struct.pack("<H", size - 1)
    xfield = extra + bc if extra_first else bc + extra
    assert size <= 65536
    return (bytes([31, 139, 8, 4, 0, 0, 0, 0, 0, 255]) + struct.pack("<H", len(xfield)) + xfield + data +
            struct.pack("<II", zlib.crc32(raw), len(raw)))


def families():
    rng = random.Random(7)
    text = "".join(rng.choice(["guide", "scan", "ACGTTGCA", "NGG", "\t", "0123456789abcdef", "\n"]) for _ in range(9000)).encode()
    period = bytes(rng.choice(b"0123456789abcdef") for _ in range(32769))
    period = (period * 2)[:65536]
    fib, w = bytearray(), [1, 2]
    while len(w) < 17:   # the histogram of tests/test_bgzf_model.py: each count the two before it and one more
        w.append(w[-1] + w[-2] + 1)
    for s, c in enumerate(w):   # 10,926 bytes: one block, so the code is built from these very counts
        fib += bytes([65 + s]) * c
    rng.shuffle(fib)
    return {"text": text[:60000], "zeros": bytes(65536), "period_32769": period, "random": rng.randbytes(0xff00),
            "empty": b"", "one_byte": b"x", "fibonacci": bytes(fib), "run": b"a" * 65536}


FAMILIES = families()


@pytest.mark.parametrize("name", sorted(FAMILIES))
def test_the_lane_function_equals_zlib(name):
    raw = FAMILIES[name]
    fits = raw[:0xff00]
    forms = [(fits, dict(level=0)), (fits, dict(level=0, flush_at=len(fits) // 2)), (raw, dict(level=1)), (raw, dict(level=6)),
             (raw, dict(level=9)), (raw, dict(strategy=zlib.Z_FIXED)), (raw, dict(flush_at=len(raw) // 2)),
             (fits[:0x8000], dict(strategy=zlib.Z_HUFFMAN_ONLY, flush_at=len(fits[:0x8000]) // 3))]
    if name == "random":
        forms = [(r[:0xf000], kw) for r, kw in forms]  # (random bytes grow under a Huffman code)
    for data, kw in forms:
        m = make_member(data, **kw)
        assert zlib.decompress(m, 31) == data
        out, reason = api.inflate_member(m)
        assert reason == 0 and out == data, (name, kw)


def test_block_types_and_long_codes_are_what_the_families_hold():
    """the families do reach the cases: a stored, a fixed and a dynamic first block, and a dynamic code with 15-bit symbols"""
    def btype(m):
        return (m[18] >> 1) & 3
    assert btype(make_member(FAMILIES["text"], level=0)) == 0
    assert btype(make_member(FAMILIES["text"], strategy=zlib.Z_FIXED)) == 1
    assert btype(make_member(FAMILIES["text"])) == 2
    # Fibonacci-like counts force the longest codes: with no matches taken the literals' code is cut off at 15 bits
    m = make_member(FAMILIES["fibonacci"], strategy=zlib.Z_HUFFMAN_ONLY)
    ll, _ = bam_make.dynamic_code_lengths(m[18:-8])
    assert max(ll) == 15
    # and the repeat symbols of the code-length code are in use there (runs of unused literals)
    assert ll.count(0) > 200 and len(FAMILIES["fibonacci"]) == 10926


def test_listed_damaged_members_give_their_reasons():
    rows = [ln.split() for ln in DAMAGED.read_text().splitlines() if ln and not ln.startswith("#")]
    assert len(rows) >= 6
    for reason, hexs, name in rows:
        out, got = api.inflate_member(bytes.fromhex(hexs))
        assert got == int(reason), name


def test_member_table_walk():
    a, b = bam_make.member(b"first member"), bam_make.member(b"the second one")
    members, reason = api.bgzf_members(a + bam_make.EOF_BLOCK + b + bam_make.EOF_BLOCK)
    assert reason == 0 and members == [(0, 12), (len(a), 0), (len(a) + 28, 14), (len(a) + 28 + len(b), 0)]
    # the BC subfield behind another subfield, and in front of one
    for first in (True, False):
        m = make_member(b"extra subfields", extra=b"XY\5\0hello", extra_first=first)
        assert zlib.decompress(m, 31) == b"extra subfields"
        assert api.bgzf_members(a + m + b) == ([(0, 12), (len(a), 15), (len(a) + len(m), 14)], 0)
        assert api.inflate_member(m) == (b"extra subfields", 0)
    # BSIZE past the end of the data
    cut = (a + b)[:-1]
    members, reason = api.bgzf_members(cut)
    assert reason == 17 and members == [(0, 12)]
    # no BC subfield: another subfield only
    no_bc = bytearray(make_member(b"no bc", extra=b"XY\2\0zz"))
    i = no_bc.index(b"BC\2\0")
    no_bc[i:i + 2] = b"BD"
    members, reason = api.bgzf_members(a + bytes(no_bc))
    assert reason == 16 and members == [(0, 12)]
    # not a BGZF header at all (plain gzip has FLG 0), and ISIZE above 65,536
    import gzip
    assert api.bgzf_members(gzip.compress(b"plain"))[1] == 15
    big = bytearray(a)
    big[-4:] = struct.pack("<I", 65537)
    assert api.bgzf_members(bytes(big))[1] == 18
    with pytest.raises(api.GsError) as e:
        api._check(api.lib().gs_debug_bgzf_members(cut, len(cut), None, None, 0, api.C.byref(api.C.c_uint64()), api.C.byref(api.C.c_uint32())))
    assert e.value.status == 6 and f"member 1 at byte {len(a)}" in str(e.value) and "BSIZE" in str(e.value)
