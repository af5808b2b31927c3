"""BGZF on the device (gs_bgzf.hip: gs_bgzf_compress, gs_bgzf_compress_device) against independent inflaters (Python's
gzip / zlib) and the framing reader of tests/bam_reader.py: every input comes back byte for byte, one member per 0xff00
bytes, no member beyond 64 KiB or its piece + 31, the same bytes on every call and for every piece by itself; matches are
found (equal bytes, the window's edge), dynamic codes are used (hex digits beat Z_FIXED), what does not compress is
stored.  GPU only."""
import ctypes as C
import gzip
import struct
import subprocess
import zlib
from importlib import import_module

import numpy as np
import pytest

import bam_reader
import oracle_lib as ol

api = import_module("guidescan-cli_amd.api")

pytestmark = pytest.mark.gpu

PIECE = 0xff00
CLI = ol.ROOT / "guidescan-cli_amd" / "bin" / "guidescan"
GOLD = ol.ROOT / "tests" / "golden" / "toy"


@pytest.fixture(scope="module")
def handle(toy):
    """any handle: the compressor uses its workspace, not its index"""
    g = api.GenomeIndex.build(toy["text"], device=0)
    yield g
    g.close()


def fib_bytes():
    """the 20-symbol histogram of tests/test_bgzf_model.py as 46,345 shuffled bytes: its Huffman tree is 20 deep"""
    w = [1, 2]
    while len(w) < 20:
        w.append(w[-1] + w[-2] + 1)
    b = np.repeat(np.arange(20, dtype=np.uint8) + 65, w)
    np.random.default_rng(3).shuffle(b)
    assert b.size == 46345
    return b.tobytes()


def code_edges():
    """segments "d random bytes, then their repetition up to d + l": d the lowest and highest distance of each distance
    code that fits, l the lowest and highest length of each length code"""
    rng = np.random.default_rng(4)
    dists, base = [], 1
    for code in range(30):
        extra = 0 if code < 4 else (code >> 1) - 1
        dists += [base, base + (1 << extra) - 1]
        base += 1 << extra
    assert dists[-1] == 32768 and len(dists) == 60
    lbase = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
    lens = sorted(set(lbase + [b - 1 for b in lbase[1:28]] + [257]))
    assert lens[0] == 3 and lens[-1] == 258
    segs = []
    for i, d in enumerate(sorted(set(dists))):
        seg = rng.integers(0, 256, d, dtype=np.uint8)
        for l in (lens[(2 * i) % len(lens)], lens[(2 * i + 1) % len(lens)], 3, 258)[:4 if d < 2048 else 2]:
            segs.append(np.concatenate([seg, np.resize(seg, l)]))
    for d in (1, 2, 3, 4, 5, 7, 64, 65, 200):  # every length at short distances as well
        seg = rng.integers(0, 256, d, dtype=np.uint8)
        segs += [np.concatenate([rng.integers(0, 256, 3, dtype=np.uint8), seg, np.resize(seg, l)]) for l in lens]
    out, at = [], 0
    for sg in segs:  # a match cannot cross a piece's end: no segment does
        if at % PIECE + sg.size > PIECE:
            pad = PIECE - at % PIECE
            out.append(rng.integers(0, 256, pad, dtype=np.uint8))
            at += pad
        out.append(sg)
        at += sg.size
    return np.concatenate(out).tobytes()


def window_edge(filler):
    rng = np.random.default_rng(5)
    head = rng.integers(0, 256, 100, dtype=np.uint8)
    # a filler of one byte value: it offers no other source for the 100 random bytes
    fill = np.full(filler, 0, np.uint8)
    return np.concatenate([head, fill, head]).tobytes()


def toy_records():
    """the alignment records of the toy database (the reference's SAM file through the host's BAM writer)"""
    import tempfile
    with tempfile.TemporaryDirectory() as t:
        out = f"{t}/o.bam"
        subprocess.run([str(CLI), "sam2bam", str(GOLD / "ref_m3_sam.sam"), out], check=True, timeout=60)
        b = gzip.decompress(open(out, "rb").read())
    at = 8 + struct.unpack_from("<i", b, 4)[0]
    n_ref = struct.unpack_from("<i", b, at)[0]
    at += 4
    for _ in range(n_ref):
        at += 4 + struct.unpack_from("<i", b, at)[0] + 4
    assert len(b) - at > 1000
    return b[at:]


def make_inputs():
    rng = np.random.default_rng(1)
    text = lambda n: rng.choice(np.frombuffer(b"ACGT\tchr01:+-,;\n", np.uint8), n).tobytes()
    inp = {f"len{n}": text(n) for n in (0, 1, 2, 3, 258, 259, PIECE - 1, PIECE, PIECE + 1, 2 * PIECE + 5)}
    inp["equal"] = b"\x55" * PIECE
    inp["random"] = rng.integers(0, 256, PIECE, dtype=np.uint8).tobytes()
    inp["hex"] = rng.choice(np.frombuffer(b"0123456789abcdef", np.uint8), PIECE).tobytes()
    inp["dist32768"] = window_edge(32668)
    inp["dist32769"] = window_edge(32669)
    inp["fib20"] = fib_bytes()
    inp["code_edges"] = code_edges()
    inp["toy_records"] = toy_records()
    return inp


INPUTS = None


def inputs():
    global INPUTS
    if INPUTS is None:
        INPUTS = make_inputs()
    return INPUTS


NAMES = [f"len{n}" for n in (0, 1, 2, 3, 258, 259, PIECE - 1, PIECE, PIECE + 1, 2 * PIECE + 5)] + [
    "equal", "random", "hex", "dist32768", "dist32769", "fib20", "code_edges", "toy_records"]


def members(out):
    sizes, eof = bam_reader.bgzf_blocks(out) if out else ([], False)
    assert not eof or not out
    res, at = [], 0
    for s in sizes:
        res.append(out[at:at + s])
        at += s
    assert at == len(out)
    return res


def block_types(member):
    """BTYPE of the member's first deflate block, and whether it is the final one"""
    b = member[18]
    return (b >> 1) & 3, b & 1


@pytest.mark.parametrize("name", NAMES)
def test_round_trip_framing_and_determinism(handle, name):
    raw = inputs()[name]
    out = handle.bgzf_compress(raw)
    ms = members(out)
    print(f"{name}: {len(raw)} -> {len(out)} bytes in {len(ms)} members, first block types {[block_types(m)[0] for m in ms]}")
    assert len(ms) == (len(raw) + PIECE - 1) // PIECE
    assert (gzip.decompress(out) if out else b"") == raw
    for k, m in enumerate(ms):
        piece = raw[k * PIECE:(k + 1) * PIECE]
        assert len(m) <= 0x10000 and len(m) <= len(piece) + 31
        # every member by an inflater that stops at the deflate stream's end: nothing behind the final block but the trailer
        z = zlib.decompressobj(-15)
        assert z.decompress(m[18:]) == piece and z.eof and len(z.unused_data) == 8
        assert struct.unpack("<II", z.unused_data) == (zlib.crc32(piece), len(piece))
        assert block_types(m)[1] == 1
    assert handle.bgzf_compress(raw) == out


def test_equal_bytes_need_matches(handle):
    m = members(handle.bgzf_compress(inputs()["equal"]))[0]
    assert block_types(m)[0] == 2
    assert len(m) < 8160  # one bit per byte: no coder without matches gets below it


def test_random_bytes_are_stored(handle):
    m = members(handle.bgzf_compress(inputs()["random"]))[0]
    assert block_types(m)[0] == 0 and len(m) == PIECE + 31


def test_hex_digits_need_dynamic_codes(handle):
    raw = inputs()["hex"]
    m = members(handle.bgzf_compress(raw))[0]
    z = zlib.compressobj(9, zlib.DEFLATED, -15, 9, zlib.Z_FIXED)
    fixed = len(z.compress(raw) + z.flush())
    print(f"hex: member {len(m)}, Z_FIXED stream {fixed}")
    assert block_types(m)[0] == 2
    assert len(m) < fixed


def test_the_window_ends_at_32768(handle):
    at, beyond = (len(members(handle.bgzf_compress(inputs()[k]))[0]) for k in ("dist32768", "dist32769"))
    print(f"window edge: {at} bytes with the repeat at 32,768, {beyond} one beyond")
    # inside the window the second 100 random bytes are one match; beyond it they are literals again
    assert beyond - at > 60


def test_every_piece_compresses_as_by_itself(handle):
    inp = inputs()
    raw = inp["hex"][:PIECE] + inp["code_edges"][:PIECE].ljust(PIECE, b"x") + inp["fib20"][:1234]
    ms = members(handle.bgzf_compress(raw))
    assert len(ms) == 3
    for k, m in enumerate(ms):
        assert handle.bgzf_compress(raw[k * PIECE:(k + 1) * PIECE]) == m


def test_device_pointer_entry_gives_the_same_bytes(handle):
    import torch
    raw = inputs()["len%d" % (2 * PIECE + 5)]
    want = handle.bgzf_compress(raw)
    d = torch.from_numpy(np.frombuffer(raw, np.uint8).copy()).cuda()
    torch.cuda.synchronize()
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    with handle.locked():  # the members stay in the handle's buffer until they are copied
        ptr, ln = handle.bgzf_compress_device(d.data_ptr(), len(raw))
        out = np.empty(ln, np.uint8)
        assert hip.hipMemcpy(out.ctypes.data, ptr, ln, 2) == 0
    assert out.tobytes() == want
    assert handle.bgzf_compress_device(None, 0) == (None, 0)
