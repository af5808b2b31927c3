"""BGZF inflate on the device (gs_bgzf_inflate.hip: gs_bgzf_inflate, gs_bgzf_inflate_device) against Python's zlib: the
members of every shape a BGZF writer may emit come back byte for byte, files of 1 to 257 members, the members our own
compressor makes as a round trip; the listed damaged members (those `make inflate-check` has answered with a reason under
the sanitizers, tests/golden/bgzf_inflate/damaged.txt) give GS_ERR_FORMAT naming the member, and the decoder works on
after one.  GPU only."""
import random
import struct
import zlib
from importlib import import_module
from pathlib import Path

import numpy as np
import pytest

import bam_make
import decode_golden as dg

api = import_module("guidescan-cli_amd.api")
pytestmark = pytest.mark.gpu

EOF = bam_make.EOF_BLOCK
DAMAGED = [ln.split() for ln in (Path(__file__).resolve().parent / "golden" / "bgzf_inflate" / "damaged.txt").read_text().splitlines()
           if ln and not ln.startswith("#")]
REASON_WORDS = {1: "block type 3", 3: "over-subscribed", 7: "before the member's first byte", 8: "runs out of bytes",
                9: "longer than ISIZE", 10: "shorter than ISIZE", 13: "CRC-32"}


def raw_member(raw, **kw):
    """a member by zlib with the compressobj arguments kw, or flush_at: a full flush there (two blocks or more)"""
    flush_at = kw.pop("flush_at", None)
    c = zlib.compressobj(kw.pop("level", 6), zlib.DEFLATED, -15, 8, kw.pop("strategy", zlib.Z_DEFAULT_STRATEGY))
    data = c.compress(raw) + c.flush() if flush_at is None else (
        c.compress(raw[:flush_at]) + c.flush(zlib.Z_FULL_FLUSH) + c.compress(raw[flush_at:]) + c.flush())
    size = 18 + len(data) + 8
    assert size <= 65536
    return (bytes([31, 139, 8, 4, 0, 0, 0, 0, 0, 255, 6, 0, 66, 67, 2, 0]) + struct.pack("<H", size - 1) + data +
            struct.pack("<II", zlib.crc32(raw), len(raw)))


def inflate_all(data):
    """Python's zlib over a series of gzip members"""
    out = b""
    while data:
        d = zlib.decompressobj(31)
        out += d.decompress(data)
        data = d.unused_data
    return out


def shapes():
    rng = random.Random(11)
    text = "".join(rng.choice(["guide", "scan", "ACGTTGCA", "NGG", "\t", "0123456789abcdef", "\n"]) for _ in range(16000)).encode()
    far = bytes(rng.choice(b"0123456789abcdef") for _ in range(32768))  # repeats at distance 32,768 exactly
    fib, w = bytearray(), [1, 2]
    while len(w) < 17:   # the histogram of tests/test_bgzf_model.py: each count the two before it and one more
        w.append(w[-1] + w[-2] + 1)
    for s, c in enumerate(w):   # 10,926 bytes: one block, so the code is built from these very counts
        fib += bytes([65 + s]) * c
    rng.shuffle(fib)
    out = {
        "eof_alone": EOF,
        "eof_between": bam_make.member(b"before") + EOF + bam_make.member(b"behind") + EOF,
        "one_byte": bam_make.member(b"x"),
        "stored_ff00": raw_member(rng.randbytes(0xff00), level=0),
        "full_65536": raw_member(text[:65536]),
        "one_run": raw_member(b"r" * 65536),
        "distance_32768": raw_member((far * 2)[:65536], level=9),
        "fifteen_bit_codes": raw_member(bytes(fib), strategy=zlib.Z_HUFFMAN_ONLY),
        "fixed": raw_member(text[:30000], strategy=zlib.Z_FIXED),
        "several_blocks": raw_member(text[:60000], flush_at=20000) + raw_member(text[:0xff00], level=0, flush_at=777),
    }
    assert len(text) >= 65536
    return out


SHAPES = shapes()


def test_the_shapes_are_what_they_claim():
    m = SHAPES["one_run"]
    assert len(m) < 400   # 65,535 bytes out of matches: distance 1, length 258 over and over
    ll, dd = bam_make.dynamic_code_lengths(SHAPES["fifteen_bit_codes"][18:-8])
    assert max(ll) == 15
    assert (SHAPES["stored_ff00"][18] >> 1) & 3 == 0 and (SHAPES["fixed"][18] >> 1) & 3 == 1
    ll, dd = bam_make.dynamic_code_lengths(SHAPES["distance_32768"][18:-8])
    assert len(dd) == 30 and dd[29] > 0   # distance code 29: 24,577..32,768


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_members_equal_zlib(name):
    data = SHAPES[name]
    assert api.inflate_bgzf(data) == inflate_all(data)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_files_of_n_members(n):
    rng = random.Random(n)
    parts = []
    for k in range(n):
        size = rng.choice([0, 1, 17, 300, 5000]) if k % 16 else 40000
        raw = bytes(rng.choice(b"ACGT0123\t\n") for _ in range(size))
        parts.append(bam_make.member(raw, level=rng.choice([0, 1, 6])) if size else EOF)
    data = b"".join(parts)
    assert api.inflate_bgzf(data) == inflate_all(data)


def test_more_members_than_workgroups():
    """65,536 workgroups at most: a file of more members is taken by workgroups that go round"""
    a, b = bam_make.member(b"the first of many"), bam_make.member(b"and the last")
    data = a + EOF * 65_600 + b
    assert api.inflate_bgzf(data) == b"the first of manyand the last"
    bad = bytes.fromhex(next(d[1] for d in DAMAGED if d[2] == "wrong_crc"))
    with pytest.raises(api.GsError) as e:
        api.inflate_bgzf(a + EOF * 65_600 + bad)
    assert f"member 65601 at byte {len(a) + 28 * 65_600}" in str(e.value)


def test_round_trip_of_our_own_members(toy):
    """200 KB of BAM records through gs_bgzf_compress and back"""
    sq, recs, fasta = dg.synthetic()
    raw = b""
    for r in recs:
        if len(raw) >= 200_000:
            break
        if r.hex and len(r.hex) < 20000:
            raw += bam_make.record(0, r.pos0, 16 if r.reverse else 0, r.id, r.seq, bam_make.tag_of(r.hex))
    assert len(raw) >= 200_000
    g = api.GenomeIndex.build(toy["text"], device=0)
    try:
        members = g.bgzf_compress(np.frombuffer(raw, dtype=np.uint8))
    finally:
        g.close()
    assert len(members) < len(raw) // 2
    assert api.inflate_bgzf(members) == raw


@pytest.fixture(scope="module")
def decoder():
    sq, recs, fasta = dg.loaded("hand")
    d = api.Decoder(sq, fasta, device=0)
    yield d
    d.close()


def test_the_decoder_keeps_a_tail_in_front(decoder):
    a, b = bam_make.member(b"0123456789"), bam_make.member(b"abcdef") + EOF
    assert decoder.inflate_bgzf(a) == b"0123456789" and decoder.last_members == 1
    assert decoder.inflate_bgzf(b, keep=3) == b"789abcdef" and decoder.last_members == 2
    assert decoder.inflate_bgzf(b"", keep=9) == b"789abcdef"
    with pytest.raises(api.GsError) as e:
        decoder.inflate_bgzf(a, keep=10)
    assert e.value.status == 1


@pytest.mark.parametrize("reason,hexs,name", DAMAGED, ids=[d[2] for d in DAMAGED])
def test_listed_damaged_members(decoder, reason, hexs, name):
    good = bam_make.member(b"a sound member in front")
    bad = bytes.fromhex(hexs)
    for call in (api.inflate_bgzf, decoder.inflate_bgzf):
        with pytest.raises(api.GsError) as e:
            call(good + EOF + bad + good)
        assert e.value.status == 6
        assert f"member 2 at byte {len(good) + 28}" in str(e.value) and REASON_WORDS[int(reason)] in str(e.value)
        # and the next call is sound
        assert call(good + good) == b"a sound member in front" * 2


def test_the_listed_members_cover_the_cases():
    assert {int(d[0]) for d in DAMAGED} >= {13, 10, 9, 1, 3, 7, 8}
