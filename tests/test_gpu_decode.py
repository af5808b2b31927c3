"""The device decoder (csrc/gs_decode.hip) and `guidescan decode`: the reference script's own output for the fixtures
byte for byte, GS_ERR_FORMAT with the record named where the script raises, a synthetic database against the model
(decode.py) in both modes with nothing left out, the same text however the records are cut into batches, and the
command on a database our own `enumerate` wrote, as SAM and as BAM.  GPU only."""
import subprocess
from importlib import import_module

import pytest

import decode_golden as dg

pytestmark = pytest.mark.gpu
api = import_module("guidescan-cli_amd.api")
decode = dg.decode
CLI = dg.ROOT / "guidescan-cli_amd" / "bin" / "guidescan"
HEADER = {"succinct": decode.SUCCINCT_HEADER + "\n", "complete": decode.COMPLETE_HEADER + "\n"}


@pytest.fixture(scope="module")
def decoders():
    """one decoder per (@SQ, FASTA) of the fixtures, closed at the end"""
    made = {}

    def get(name):
        sq, recs, fasta = dg.loaded(name)
        key = (tuple(sq), dg.CASES[name]["fasta"])
        if key not in made:
            made[key] = api.Decoder(sq, fasta, device=0)
        return made[key]

    yield get
    for d in made.values():
        d.close()


@pytest.mark.parametrize("name,mode", dg.GOOD)
def test_goldens_through_both_entry_points(decoders, name, mode):
    dec = decoders(name)
    sq, recs, fasta = dg.loaded(name)
    want = dg.expected(name, mode).decode()
    assert dec.decode_sam(dg.paths(name)[0].read_bytes(), complete=mode == "complete") == want
    got = dec.decode_records(recs, complete=mode == "complete", on_device=True)
    assert HEADER[mode] + got == want
    assert dec.last_rows == want.count("\n") - 1


@pytest.mark.parametrize("name,mode", dg.RAISING)
def test_format_error_names_the_record(decoders, name, mode):
    dec = decoders(name)
    with pytest.raises(api.GsError) as e:
        dec.decode_sam(dg.paths(name)[0].read_bytes(), complete=mode == "complete")
    sq, recs, fasta = dg.loaded(name)
    first = 0 if name == "raise_chromosome" else 1
    assert e.value.status == 6 and f"record {first} ({recs[first].id})" in str(e.value)
    # the record's number counts from first_record: a later batch names the record of the whole database
    with pytest.raises(api.GsError) as e:
        dec.decode_records(recs, complete=mode == "complete", first_record=100)
    assert f"record {100 + first} (" in str(e.value)


def test_negative_distance_fails_in_succinct_mode_only(decoders):
    dec = decoders("hand")
    sq, recs, fasta = dg.loaded("hand")
    delim = -(sum(n for _, n in sq) + 1)
    bad = decode.Record("neg", recs[0].seq, False, "chrA", 100, dg.hexw([122, -1, delim]))
    with pytest.raises(api.GsError) as e:
        dec.decode_records([recs[0], bad], complete=False)
    assert e.value.status == 6 and "record 1 (neg)" in str(e.value) and "distance" in str(e.value)
    want = "\n".join(decode.Decoder(sq, fasta, dg.TABLES).rows([recs[0], bad], complete=True)) + "\n"
    assert dec.decode_records([recs[0], bad], complete=True) == want


def test_a_stored_sequence_beyond_32_symbols_is_refused_like_the_model(decoders):
    dec = decoders("hand")
    sq, recs, fasta = dg.loaded("hand")
    model = decode.Decoder(sq, fasta, dg.TABLES)
    for hexs in (None, recs[0].hex):
        long = decode.Record("long", "ACGT" * 8 + "A", False, "chrA", 100, hexs)
        for complete in (False, True):
            with pytest.raises(decode.DecodeError) as m:
                model.rows([recs[0], long], complete=complete)
            with pytest.raises(api.GsError) as e:
                dec.decode_records([recs[0], long], complete=complete)
            assert e.value.status == 6 and "record 1 (long)" in str(e.value) and decode.REASONS[m.value.reason] in str(e.value)
    fits = [decode.Record("fits", "ACGT" * 8, False, "chrA", 100, recs[0].hex)]
    assert dec.decode_records(fits, complete=True) == "".join(r + "\n" for r in model.rows(fits, complete=True))


@pytest.fixture(scope="module")
def synthetic():
    sq, recs, fasta = dg.synthetic()
    model = decode.Decoder(sq, fasta, dg.TABLES)
    dec = api.Decoder(sq, fasta, device=0)
    want = {mode: "".join(r + "\n" for r in model.rows(recs, complete=mode == "complete")) for mode in dg.MODES}
    yield dec, recs, want
    dec.close()


@pytest.mark.parametrize("mode", dg.MODES)
def test_synthetic_database_equals_the_model(synthetic, mode):
    dec, recs, want = synthetic
    assert len(recs) == 3000 and max(len(r.hex or "") for r in recs) // 16 > 70_001
    got = dec.decode_records(recs, complete=mode == "complete", on_device=True)
    assert got == want[mode]
    if mode == "succinct":
        # the ordered fold is looked at: the records made for it (65, 257 and 70,001 off-targets, all with a CFD, the
        # first distance-0 one in the middle of a chunk; test_decode_model shows another order prints other digits)
        # do print a specificity
        spec = {row.split(",", 1)[0]: row.rsplit(",", 1)[1] for row in got.splitlines()}
        assert all(spec[name] for name in dg.FOLD)
    if mode == "complete":
        assert dec.last_rows == want[mode].count("\n") > 100_000


@pytest.mark.parametrize("mode", dg.MODES)
@pytest.mark.parametrize("batch", [7, 1000])
def test_batches_change_nothing(synthetic, mode, batch):
    dec, recs, want = synthetic
    parts = [dec.decode_records(recs[i:i + batch], complete=mode == "complete", first_record=i)
             for i in range(0, len(recs), batch)]
    assert "".join(parts) == want[mode]


def test_cli_decodes_what_enumerate_wrote(toy, tmp_path):
    d = tmp_path
    fa = toy["dir"] / "toy.fa"
    subprocess.run([str(CLI), "index", "--index", str(d / "toy"), str(fa)], check=True, timeout=120)
    for fmt in ("sam", "bam"):
        subprocess.run([str(CLI), "enumerate", str(d / "toy"), "-f", str(toy["dir"] / "kmers.csv"), "-o", str(d / f"db.{fmt}"),
                        "-m", "3", "--format", fmt, "-n", "1"], check=True, timeout=300, capture_output=True)
    assert (d / "db.sam").read_bytes() == (toy["dir"] / "ref_m3_sam.sam").read_bytes()
    for mode in dg.MODES:
        want = dg.expected("toy_ref_m3_sam", mode)
        for fmt in ("sam", "bam"):
            out = d / f"{fmt}.{mode}.csv"
            subprocess.run([str(CLI), "decode", "--mode", mode, "-o", str(out), str(d / f"db.{fmt}"), str(fa)], check=True, timeout=120)
            assert out.read_bytes() == want, (fmt, mode)
        r = subprocess.run([str(CLI), "decode", "--mode", mode, "--batch-size", "5", str(d / "db.bam"), str(fa)], check=True,
                           timeout=120, capture_output=True)
        assert r.stdout == want
    # a database the script fails on: exit status 1, the record named, no output file left
    sam, hand_fa = dg.paths("raise_pam")
    r = subprocess.run([str(CLI), "decode", "-o", str(d / "bad.csv"), str(sam), str(hand_fa)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "record 1 (r)" in r.stderr and not (d / "bad.csv").exists()


def test_cli_bam_reference_without_sq_line_and_without_eof_block(tmp_path):
    """a BAM whose binary reference list has a reference that the text header's @SQ lines do not name: the record on
    it prints None, as in the model; the file lacks the BGZF end-of-file block, which is a warning and no failure"""
    sq, recs, fasta = dg.loaded("hand")
    fa = dg.paths("hand")[1]
    head = "@HD\tVN:1.0\n" + "".join(f"@SQ\tSN:{n}\tLN:{ln}\n" for n, ln in sq)
    with_of = next(r for r in recs if r.hex and not r.reverse and r.seq.isupper() and r.rname == sq[0][0])
    bam = tmp_path / "db.bam"
    bam.write_bytes(dg.tiny_bam(head, [("extra", 500)] + list(sq), [(0, 7, 0, "stray", "ACGTACGTACGTACGTACGTAGG", None),
                                                                    (1, with_of.pos0, 0, with_of.id, with_of.seq, with_of.hex)]))
    for mode in dg.MODES:
        r = subprocess.run([str(CLI), "decode", "--mode", mode, str(bam), str(fa)], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "no BGZF end-of-file block" in r.stderr
        assert r.stdout == decode.decode_database(bam, fa, mode, tables=dg.TABLES)
    assert ",None,7,+," in r.stdout or mode == "complete"
