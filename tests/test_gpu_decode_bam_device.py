"""BAM databases read on the device (gs_bgzf_inflate.hip, gs_bamsplit.hip: gs_decode_bam): BAM files built here from the
decode fixtures' SAM files (tests/bam_make.py) give the committed CSVs and what gs_decode_sam gives for the same records,
wherever the members and the groups of members are cut; record contents that take every branch of the field walk;
the fixtures the script raises on give the SAM route's error; malformed records give decode_bam_file's words with the
record's index.  GPU only."""
import gzip
import struct
from functools import lru_cache
from importlib import import_module

import pytest

import bam_make as bm
import decode_golden as dg

pytestmark = pytest.mark.gpu
api = import_module("guidescan-cli_amd.api")
decode = dg.decode
HEADER = {"succinct": decode.SUCCINCT_HEADER + "\n", "complete": decode.COMPLETE_HEADER + "\n"}


@lru_cache(maxsize=None)
def as_bam(name):
    """a fixture's SAM file as (header bytes, [record bytes]), or None when BAM cannot hold its SEQ symbols"""
    return bm.from_sam(dg.paths(name)[0].read_text())


GOOD = [(n, m) for n, m in dg.GOOD if as_bam(n) is not None]
RAISING = [(n, m) for n, m in dg.RAISING if as_bam(n) is not None]


@pytest.fixture(scope="module")
def decoders():
    made = {}

    def get(sq, fasta_name):
        key = (tuple(sq), fasta_name)
        if key not in made:
            made[key] = api.Decoder(sq, decode.parse_fasta_records(dg.DIR / fasta_name), device=0)
        return made[key]

    yield get
    for d in made.values():
        d.close()


def through(dec, head, recs, complete, cuts=(), groups=None, first_record=0, piece=0xff00, eof=True, tails=None):
    """the file head + recs, its members cut at `cuts` (offsets into the inflated bytes), handed over in groups of
    `groups` members (None: all at once) -> the rows.  tails: a list that takes the tail each call reports"""
    raw = head + b"".join(recs)
    members = bm.members(raw, cuts, piece) + ([bm.EOF_BLOCK] if eof else [])
    sq, ref_to_sq, skip = decode.bam_header(raw)
    # the first group holds the header
    n_head, got = 0, 0
    while got < skip:
        got += struct.unpack("<I", members[n_head][-4:])[0]
        n_head += 1
    sizes = groups or [len(members)]
    out, done, k, call = [], first_record, 0, 0
    while k < len(members):
        take = sizes[min(call, len(sizes) - 1)]
        if call == 0:
            take = max(take, n_head)
        part = members[k:k + take]
        k += len(part)
        text, n, tail = dec.decode_bam(b"".join(part), skip=skip if call == 0 else 0, ref_to_sq=ref_to_sq, complete=complete,
                                       first_record=done, end=k >= len(members), on_device=call % 2 == 1)
        out.append(text)
        done += n
        call += 1
        if tails is not None:
            tails.append(tail)
    assert done - first_record == len(recs)
    return "".join(out)


@pytest.mark.parametrize("name,mode", GOOD)
def test_fixtures_as_bam_equal_the_goldens_and_the_sam_route(decoders, name, mode):
    head, recs = as_bam(name)
    sq, _, _ = dg.loaded(name)
    dec = decoders(sq, dg.CASES[name]["fasta"])
    want = dg.expected(name, mode).decode()
    assert dec.decode_sam(dg.paths(name)[0].read_bytes(), complete=mode == "complete") == want
    assert HEADER[mode] + through(dec, head, recs, mode == "complete") == want
    # one record per member
    starts = [len(head) + sum(len(r) for r in recs[:i]) for i in range(len(recs))]
    assert HEADER[mode] + through(dec, head, recs, mode == "complete", cuts=starts, groups=[3]) == want


def test_the_fixtures_are_not_all_filtered_out():
    assert len(GOOD) >= 6 and len(RAISING) >= 6


@pytest.fixture(scope="module")
def hand(decoders):
    sq, index, rows, sam = bm.hand_database()
    dec = decoders(sq, "hand.fa")
    head_text = "@HD\tVN:1.0\n" + "".join(f"@SQ\tSN:{n}\tLN:{ln}\n" for n, ln in sq)
    want = {mode: dec.decode_sam(sam.encode(), complete=mode == "complete", header=False) for mode in dg.MODES}
    assert all(w.count("\n") >= len(rows) for w in want.values())
    return dict(sq=sq, index=index, rows=rows, dec=dec, head=bm.header(head_text, sq), recs=bm.build(rows, index), want=want)


@pytest.mark.parametrize("mode", dg.MODES)
def test_record_contents(hand, mode):
    assert through(hand["dec"], hand["head"], hand["recs"], mode == "complete") == hand["want"][mode]
    assert ",None,7,+," in hand["want"]["succinct"]


@pytest.mark.parametrize("mode", dg.MODES)
def test_member_cuts(hand, mode):
    head, recs, dec, want = hand["head"], hand["recs"], hand["dec"], hand["want"][mode]
    starts = [len(head) + sum(len(r) for r in recs[:i]) for i in range(len(recs))]
    big = [r[3] for r in hand["rows"]].index("big")
    assert len(recs[big]) > 65536   # a record longer than one member
    cuts = {"one record per member": starts,
            "inside block_size": [s + 2 for s in starts],
            "inside the fixed part": [s + 4 + 17 for s in starts],
            "inside a tag": [s + len(r) - 9 for s, r in zip(starts, recs)],
            "small members": []}
    for what, c in cuts.items():
        piece = 1000 if what == "small members" else 0xff00
        assert through(dec, head, recs, mode == "complete", cuts=c, piece=piece) == want, what
        # a group of a single member each
        assert through(dec, head, recs, mode == "complete", cuts=c, piece=piece, groups=[1]) == want, what


@pytest.mark.parametrize("tail", [1, 3, 4])
def test_group_cuts_leave_a_tail(hand, tail):
    head, recs, dec = hand["head"], hand["recs"], hand["dec"]
    at = len(head) + len(recs[0]) + len(recs[1])
    n_first = len(bm.members((head + b"".join(recs))[:at + tail], [at + tail]))
    for mode in dg.MODES:
        tails = []
        got = through(dec, head, recs, mode == "complete", cuts=[at + tail], groups=[n_first, 10_000], tails=tails)
        assert got == hand["want"][mode]
        assert tails == [tail, 0]


@pytest.mark.parametrize("mode", dg.MODES)
def test_block_size_across_the_tile_border_of_the_start_walk(hand, mode):
    """k_bs_starts reads a size as two words of its LDS ring: records that start 1, 2 and 3 bytes before a multiple of
    16,384 put the size across two tiles, the second time (32,768) across the ring's wrap"""
    head, recs, dec = hand["head"], hand["recs"], hand["dec"]
    a_row, b_row = hand["rows"][0], hand["rows"][7]
    file_recs, sam, at = [], "", len(head)
    base = len(bm.record(-1, 0, 0, "pad", "ACGT", b"xzZ\0"))
    for m, d in zip(range(1, 10), (1, 2, 3) * 3):   # starts at 16384 m - d: both slots of the ring, every split of the four bytes
        fill = 16384 * m - d - at   # a padding record whose text tag fills up to the wanted start
        assert fill >= base
        pad = bm.record(-1, 0, 0, "pad", "ACGT", b"xzZ" + b"p" * (fill - base) + b"\0")
        row = a_row if m % 2 else b_row
        file_recs += [pad, bm.build([row], hand["index"])[0]]
        at += len(pad)
        assert (at + d) % 16384 == 0
        at += len(file_recs[-1])
        sam += bm.sam_line("pad", 0, None, 0, "ACGT") + bm.sam_line(row[3], row[2], row[0], row[1], row[4], row[6])
    want = dec.decode_sam(sam.encode(), complete=mode == "complete", header=False)
    assert through(dec, head, file_recs, mode == "complete") == want
    assert through(dec, head, file_recs, mode == "complete", piece=5000, groups=[4]) == want


def test_header_forms(decoders, hand):
    """no @SQ lines in the text header: the binary list names the chromosomes; an @SQ order that differs from it"""
    sq, rows, index = hand["sq"], hand["rows"], hand["index"]
    dec = hand["dec"]
    no_sq = bm.header("@HD\tVN:1.0\n", sq)
    assert decode.bam_header(no_sq)[:2] == (list(sq), list(range(len(sq))))
    assert through(dec, no_sq, hand["recs"], False) == hand["want"]["succinct"]
    turned = list(reversed(sq)) + [("extra", 500)]
    t_index = {n: i for i, (n, _) in enumerate(turned)}
    head = bm.header("@HD\tVN:1.0\n" + "".join(f"@SQ\tSN:{n}\tLN:{ln}\n" for n, ln in sq), turned)
    _, ref_to_sq, _ = decode.bam_header(head)
    assert ref_to_sq == [len(sq) - 1 - i for i in range(len(sq))] + [-1]
    recs = bm.build(rows, t_index) + [bm.record(len(turned) - 1, 9, 0, "stray", "ACGTACGTACGTACGTACGTAGG")]
    want = hand["want"]["succinct"] + "stray,ACGTACGTACGTACGTACGTAGG,None,9,+,0,0,0,0,\n"
    assert through(dec, head, recs, False) == want


@pytest.mark.parametrize("name,mode", RAISING)
def test_raising_fixtures_give_the_sam_routes_error(decoders, hand, name, mode):
    head, recs = as_bam(name)
    sq, _, _ = dg.loaded(name)
    dec = decoders(sq, dg.CASES[name]["fasta"])
    with pytest.raises(api.GsError) as s:
        dec.decode_sam(dg.paths(name)[0].read_bytes(), complete=mode == "complete")
    with pytest.raises(api.GsError) as e:
        through(dec, head, recs, mode == "complete")
    assert e.value.status == s.value.status == 6 and str(e.value) == str(s.value)
    # the decoder works on
    assert through(hand["dec"], hand["head"], hand["recs"], mode == "complete") == hand["want"][mode]


def malformed_records(hand):
    good = hand["recs"][0]
    n_ref = len(hand["sq"])
    body = bytearray(good[4:])

    def with_body(b):
        return struct.pack("<i", len(b)) + bytes(b)

    fields = bytearray(body)
    fields[16:20] = struct.pack("<i", 1 << 20)   # l_seq beyond the record
    ref = bytearray(body)
    ref[0:4] = struct.pack("<i", n_ref)
    return {
        "a record shorter than its fixed part": struct.pack("<i", 20) + bytes(20),
        "a record's fields outrun it": with_body(fields),
        "a record's reference is beyond the list": with_body(ref),
        "a text tag without its end": with_body(body + b"xzZno end"),
        "an array tag": with_body(body + b"xbBc\1\0"),
        "a tag of unknown type": with_body(body + b"xqq\1\0\0\0"),
        "a tag outruns its record": with_body(body + b"xii\1\0\0"),
    }


def test_malformed_records_give_the_host_routes_words(hand):
    dec, head, recs = hand["dec"], hand["head"], hand["recs"]
    for words, bad in malformed_records(hand).items():
        for cuts in ((), [len(head) + len(recs[0]) + 3]):
            with pytest.raises(api.GsError) as e:
                through(dec, head, [recs[0], recs[1], bad, recs[2]], False, cuts=cuts, first_record=10)
            assert e.value.status == 6 and f"record 12: {words}" in str(e.value), words
    # the first in file order is the one reported
    bads = list(malformed_records(hand).values())
    with pytest.raises(api.GsError) as e:
        through(dec, head, [recs[0], bads[3], bads[1], bads[0]], True)
    assert "record 1: a text tag without its end" in str(e.value)
    # a record cut by the end of the data, and one whose size is
    for keep, words in ((len(recs[1]) - 5, "a record is cut"), (2, "a record's size")):
        with pytest.raises(api.GsError) as e:
            through(dec, head, [recs[0], recs[1][:keep]], False, first_record=5)
        assert e.value.status == 6 and f"record 6: {words}" in str(e.value)
    assert through(dec, head, recs, False) == hand["want"]["succinct"]


def test_python_wrapper_reads_a_file(hand, tmp_path):
    """decode.decode_bam: header on the host, the rest on the device, in groups of two members"""
    path = tmp_path / "db.bam"
    path.write_bytes(b"".join(bm.members(hand["head"] + b"".join(hand["recs"]), piece=3000)) + bm.EOF_BLOCK)
    assert gzip.decompress(path.read_bytes()) == hand["head"] + b"".join(hand["recs"])
    for mode in dg.MODES:
        want = HEADER[mode] + hand["want"][mode]
        assert decode.decode_bam(path, dg.DIR / "hand.fa", mode) == want
        assert decode.decode_bam(path, dg.DIR / "hand.fa", mode, group_members=2) == want
    assert decode.inflate_bgzf(path.read_bytes()) == hand["head"] + b"".join(hand["recs"])
