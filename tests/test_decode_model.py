"""decode.py, the plain restatement of the reference's scripts/decode_database.py, against the script's own output
(tests/golden/decode) byte for byte, and against the CSV database of the same toy run."""
import csv

import pytest

import decode_golden as dg

decode = dg.decode


@pytest.mark.parametrize("name,mode", dg.GOOD)
def test_model_reproduces_the_script(name, mode):
    sam, fa = dg.paths(name)
    assert decode.decode_database(sam, fa, mode, tables=dg.TABLES).encode() == dg.expected(name, mode)


@pytest.mark.parametrize("name,mode", dg.RAISING)
def test_model_raises_where_the_script_raises(name, mode):
    sam, fa = dg.paths(name)
    with pytest.raises(decode.DecodeError) as e:
        decode.decode_database(sam, fa, mode, tables=dg.TABLES)
    assert e.value.record == (0 if name == "raise_chromosome" else 1)


def test_negative_distance_is_refused_in_succinct_mode():
    """Python would index the counters from the end: not reproduced"""
    sq, recs, fasta = dg.loaded("hand")
    delim = -(sum(n for _, n in sq) + 1)
    bad = decode.Record("neg", recs[0].seq, False, "chrA", 100, dg.hexw([122, -1, delim]))
    with pytest.raises(decode.DecodeError) as e:
        decode.Decoder(sq, fasta, dg.TABLES).rows([recs[0], bad], complete=False)
    assert (e.value.record, e.value.reason) == (1, decode.ERR_DISTANCE)
    assert decode.Decoder(sq, fasta, dg.TABLES).rows([bad], complete=True)[0].startswith("neg,0,")


def test_complete_rows_are_the_csv_database_rows(toy):
    """the SAM database decoded = the CSV database of the same run, as sets of (id, chromosome, sense, distance,
    sequence), over the ids that have a SAM line"""
    sam, fa = dg.paths("toy_ref_m3_sam")
    rows = list(csv.reader(decode.decode_database(sam, fa, "complete", tables=dg.TABLES).splitlines()))[1:]
    got = {(r[0], r[3], r[5], r[6], r[2]) for r in rows}
    ids = {r[0] for r in rows}
    with open(toy["dir"] / "ref_m3_csv.csv") as f:
        want = {(r["id"], r["match_chrm"], r["match_strand"], r["match_distance"], r["match_sequence"].upper())
                for r in csv.DictReader(f) if r["match_chrm"] != "NA" and r["id"] in ids}
    assert got == want and len(got) == 60
    assert not {"polyA", "absent"} & ids


@pytest.mark.parametrize("name", ["toy_ref_m3_sam", "toy_ref_m3_sam_nag"])  # (BAM holds no lower-case SEQ: not `hand`)
def test_model_reads_bam_like_sam(name, tmp_path):
    """the same database as BAM (packed by the command's own `sam2bam`, host only) decodes to the same text"""
    import subprocess
    sam, fa = dg.paths(name)
    bam = tmp_path / "db.bam"
    subprocess.run([str(dg.ROOT / "guidescan-cli_amd" / "bin" / "guidescan"), "sam2bam", str(sam), str(bam)], check=True, timeout=60)
    for mode in dg.MODES:
        assert decode.decode_database(bam, fa, mode, tables=dg.TABLES).encode() == dg.expected(name, mode)


def test_fold_records_carry_a_sum_whose_order_shows():
    """what the GPU tests lean on: synthetic()'s FOLD records print a specificity, every off-target of theirs has a
    CFD, the first distance-0 one is neither the list's first word nor the first of a 64-word chunk, and at 257 and
    70,001 off-targets a sum taken 64 at a time prints other digits, at 70,001 a sum taken backwards does too"""
    sq, recs, fasta = dg.synthetic()
    model = decode.Decoder(sq, fasta, dg.TABLES)
    fold = [r for r in recs if r.id in dg.FOLD]
    assert sorted(r.id for r in fold) == sorted(dg.FOLD)
    for rec in fold:
        ots = model.off_targets(rec, 0)
        cfds, dist = [o[5] for o in ots], [o[0] for o in ots]
        assert len(ots) == dg.FOLD[rec.id] and all(c is not None for c in cfds)
        first0 = dist.index(0)
        assert first0 > 0 and (first0 + 2) % 64 and dist.count(0) > 3      # + 2: the distance and delimiter words before it
        row = model.rows([rec], complete=False)[0]
        printed = row.rsplit(",", 1)[1]
        left = 0.0
        for c in cfds:
            left = left + c
        assert printed == repr(1 / (1 + (left - cfds[first0])))
        if len(ots) > 256:
            chunked = sum(sum(cfds[i:i + 64]) for i in range(0, len(cfds), 64))
            others = {repr(1 / (1 + (chunked - cfds[first0]))), repr(1 / (1 + (left - cfds[0])))}
            if len(ots) > 70_000:
                others.add(repr(1 / (1 + (sum(reversed(cfds)) - cfds[first0]))))
            assert printed not in others and len(ots) // 64 > first0 // 64


def test_a_stored_sequence_beyond_32_symbols_is_refused():
    """this project's own limit (the device gathers into 32 symbols), kept by the model too so that both paths of
    decode_database() agree: the record is refused whether or not it has off-targets"""
    sq, recs, fasta = dg.loaded("hand")
    model = decode.Decoder(sq, fasta, dg.TABLES)
    for hexs in (None, recs[0].hex):
        long = decode.Record("long", "ACGT" * 8 + "A", False, "chrA", 100, hexs)
        for complete in (False, True):
            with pytest.raises(decode.DecodeError) as e:
                model.rows([recs[0], long], complete=complete)
            assert (e.value.record, e.value.reason) == (1, decode.ERR_LONG)
    ok = decode.Record("fits", "ACGT" * 8, False, "chrA", 100, None)
    assert model.rows([ok], complete=False) == ["fits," + "ACGT" * 8 + ",chrA,100,+,0,0,0,0,"]


def test_bam_reference_that_no_sq_line_names_is_unmapped(tmp_path):
    """refID counts the binary reference list; the chromosomes are the text header's @SQ lines when it has them, and a
    record on a reference they do not name prints None, as a SAM line with such an RNAME does"""
    sq, recs, fasta = dg.loaded("hand")
    head = "@HD\tVN:1.0\n" + "".join(f"@SQ\tSN:{n}\tLN:{ln}\n" for n, ln in sq)
    refs = [("extra", 500)] + list(sq)
    with_of = next(r for r in recs if r.hex and not r.reverse and r.seq.isupper() and r.rname == sq[0][0])
    bam = tmp_path / "db.bam"
    bam.write_bytes(dg.tiny_bam(head, refs, [(0, 7, 0, "stray", "ACGTACGTACGTACGTACGTAGG", None),
                                             (1, with_of.pos0, 0, with_of.id, with_of.seq, with_of.hex)]))
    got_sq, got = decode.read_database(bam)
    assert got_sq == sq and [r.rname for r in got] == [None, sq[0][0]]
    text = decode.decode_database(bam, dg.paths("hand")[1], "succinct", tables=dg.TABLES).splitlines()
    assert text[1] == "stray,ACGTACGTACGTACGTACGTAGG,None,7,+,0,0,0,0,"
    assert text[2] == decode.Decoder(sq, fasta, dg.TABLES).rows([with_of], complete=False)[0]
    # without @SQ lines the binary list is the genome
    bam.write_bytes(dg.tiny_bam("@HD\tVN:1.0\n", refs, [(0, 7, 0, "stray", "ACGTACGTACGTACGTACGTAGG", None)]))
    got_sq, got = decode.read_database(bam)
    assert got_sq == refs and got[0].rname == "extra"
