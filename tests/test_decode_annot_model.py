"""`decode --annotate` in the pure-Python path of decode.py (decode_database(device=None), Decoder.rows, decode_text) over
the fixtures of tests/golden/decode: the table is the reference script's own output (the committed CSV) with the feature
columns that tests/annot_model.py gives each row from the fields it prints.  The BED file is written against each
fixture's @SQ names.  The C-ABI argument checks that touch no device are here too.  CPU only."""
import ctypes as C
from importlib import import_module

import pytest

import annot_model as am
import decode_annot_cases as dac
import decode_golden as dg

decode = dg.decode
BOTH = sorted({n for n, _ in dg.GOOD if (n, "succinct") in dg.GOOD and (n, "complete") in dg.GOOD})
COMPLETE = sorted(n for n, m in dg.GOOD if m == "complete")


def bed_of(name, tmp_path):
    """a BED file over the fixture's chromosomes, the last one left out when there are several"""
    sq, _, _ = dg.loaded(name)
    text = dac.generic_bed(sq, skip=[sq[-1][0]] if len(sq) > 1 else [])
    path = tmp_path / f"{name}.bed"
    path.write_text(text)
    return path, text


@pytest.mark.parametrize("name", COMPLETE)
def test_complete_mode_gains_the_column(name, tmp_path):
    sq, recs, _ = dg.loaded(name)
    sam, fa = dg.paths(name)
    bed, bed_text = bed_of(name, tmp_path)
    want, feats = dac.expected_complete(dg.expected(name, "complete"), sq, recs, bed_text)
    got = decode.decode_database(sam, fa, "complete", tables=dg.TABLES, annotate=bed).encode("latin-1")
    assert got == want
    assert got.split(b"\n")[0].endswith(b",distance,cfd,match_features")
    # without the option nothing has changed
    assert decode.decode_database(sam, fa, "complete", tables=dg.TABLES).encode("latin-1") == dg.expected(name, "complete")
    if name.startswith("toy") and feats:      # (a succinct database has no off-target lists)
        assert any(feats) and not all(feats) and any(len(f) > 1 for f in feats)


@pytest.mark.parametrize("name", COMPLETE)
def test_features_only_leaves_out_the_other_rows_and_keeps_match_number(name, tmp_path):
    sq, recs, _ = dg.loaded(name)
    sam, fa = dg.paths(name)
    bed, bed_text = bed_of(name, tmp_path)
    full, feats = dac.expected_complete(dg.expected(name, "complete"), sq, recs, bed_text)
    want, _ = dac.expected_complete(dg.expected(name, "complete"), sq, recs, bed_text, features_only=True)
    got = decode.decode_database(sam, fa, "complete", tables=dg.TABLES, annotate=bed, features_only=True).encode("latin-1")
    assert got == want
    rows, kept = full.split(b"\n")[1:-1], got.split(b"\n")[1:-1]
    assert kept == [r for r, f in zip(rows, feats) if f] and all(not r.endswith(b",NA") for r in kept)
    assert set(kept) <= set(rows)     # every field, match_number among them, is the full table's


@pytest.mark.parametrize("name", BOTH)
def test_succinct_mode_gains_the_four_counts(name, tmp_path):
    sq, recs, _ = dg.loaded(name)
    sam, fa = dg.paths(name)
    bed, bed_text = bed_of(name, tmp_path)
    want = dac.expected_succinct(dg.expected(name, "succinct"), dg.expected(name, "complete"), sq, recs, bed_text)
    got = decode.decode_database(sam, fa, "succinct", tables=dg.TABLES, annotate=bed).encode("latin-1")
    assert got == want
    assert got.split(b"\n")[0].endswith(b",specificity,distance_0_feature_matches,distance_1_feature_matches,"
                                        b"distance_2_feature_matches,distance_3_feature_matches")
    assert decode.decode_database(sam, fa, "succinct", tables=dg.TABLES).encode("latin-1") == dg.expected(name, "succinct")


def test_the_synthetic_database_of_the_gpu_tests_holds_what_it_claims():
    """both clips, one-base footprints, a footprint over several segments with a repeated group, a chromosome without
    intervals, a chromosome without off-targets, a tile of 64 rows without a feature"""
    recs, fasta, bed = dac.small_records(), dac.small_genome(), dac.small_bed()
    plain = decode.decode_text(dac.SQ, recs, fasta, "complete", dg.TABLES).encode("latin-1")
    want, feats = dac.expected_complete(plain, dac.SQ, recs, bed)
    got = decode.decode_text(dac.SQ, recs, fasta, "complete", dg.TABLES, decode.parse_bed(bed, dac.SQ)).encode("latin-1")
    assert got == want
    rows = [dac.split_complete(r) for r in plain.decode().split("\n")[1:-1]]
    names, _ = am.bed_lines(bed)
    by = {(f[0], f[3], int(f[4]), f[5]): [names[g] for g in ft] for f, ft in zip(rows, feats)}
    assert by["edges", "cB", 0, "+"] == ["head"] and by["edges", "cB", 0, "-"] == ["head", "dot_a", "dot_b"]   # [-22, 1) clipped; [0, 23)
    assert by["edges", "cA", 21, "+"] == ["first_base", "base_21"] and by["edges", "cA", 22, "+"] == ["first_base", "base_21"]
    assert by["edges", "cA", 96, "-"] == ["last_base"] and by["edges", "cB", 63, "-"] == ["last_base"]  # one base after the clip
    assert by["edges", "cB", 63, "+"] == ["last_base"] and by["edges", "cC", 39, "-"] == []
    assert by["merge", "cA", 52, "+"] == ["rep", "mid", "tail", "gene", "exon"]
    assert by["short20", "cA", 19, "+"] == ["first_base"]                                           # [0, 20): base 21 is outside
    assert all(not ft for f, ft in zip(rows, feats) if f[3] == "cC") and not any(f[3] == "cD" for f in rows)
    # the tile of 64 complete-mode slots that lies inside `desert` has no feature at all
    ids = [f[0] for f in rows]
    assert ids.count("desert") == 130 and ids.count("big200") == 204
    # short and wrapped printed sequences are annotated by where they lie
    assert any(len(f[2]) < dac.N and ft for f, ft in zip(rows, feats))


def test_argument_checks_of_the_python_path(tmp_path):
    name = "hand"
    sam, fa = dg.paths(name)
    bed, _ = bed_of(name, tmp_path)
    with pytest.raises(ValueError):
        decode.decode_database(sam, fa, "succinct", tables=dg.TABLES, annotate=bed, features_only=True)
    with pytest.raises(ValueError):
        decode.decode_database(sam, fa, "complete", tables=dg.TABLES, features_only=True)
    sq, recs, fasta = dg.loaded(name)
    with pytest.raises(ValueError):
        decode.Decoder(sq, fasta, dg.TABLES, decode.parse_bed(bed.read_text(), sq)).rows(recs, complete=False, features_only=True)
    with pytest.raises(ValueError):
        decode.decode_bam(sam, fa, "succinct", annotate=bed, features_only=True)      # before the file is read
    # the refusals of the BED reader: the library's reasons, with the 1-based line
    chrom, ln = sq[0]
    for text, message in ((f"{chrom}\t0\t5\tok\n{chrom}\t9\t4\tg\n", "annotation line 2: start >= end"),
                          (f"{chrom}\t0\t{ln + 1}\n", "annotation line 1: end beyond the chromosome's length"),
                          (f"# c\n\nnowhere\t0\t5\n", "annotation line 3: no such chromosome"),
                          (f"{chrom}\t0\t5\tgene;exon\n", "gene;exon"),
                          (f"{chrom}\t0\n", "annotation line 1: fewer than three fields"),
                          ("# nothing\n", "no interval")):
        with pytest.raises(ValueError, match=message.replace("'", ".")):
            decode.parse_bed(text, sq)
    # the script's failures stay what they are with the option
    for raising, mode in dg.RAISING:
        rsam, rfa = dg.paths(raising)
        rsq, _, _ = dg.loaded(raising)
        rbed = tmp_path / "raising.bed"
        rbed.write_text(dac.generic_bed(rsq))
        with pytest.raises(decode.DecodeError) as plain:
            decode.decode_database(rsam, rfa, mode, tables=dg.TABLES)
        with pytest.raises(decode.DecodeError) as annotated:
            decode.decode_database(rsam, rfa, mode, tables=dg.TABLES, annotate=rbed)
        assert (annotated.value.record, annotated.value.reason) == (plain.value.record, plain.value.reason)


def test_c_abi_argument_checks_that_need_no_device():
    """gs_decoder_set_annotation and gs_debug_decode_annot_ms refuse a missing handle before anything else; the flag has
    the value the header gives it and collides with no other text or decode flag"""
    api = import_module("guidescan-cli_amd.api")
    L = api.lib()
    assert L.gs_decoder_set_annotation(None, None) == 1
    ms = C.c_double()
    assert L.gs_debug_decode_annot_ms(None, C.byref(ms)) == 1
    header = (dg.ROOT / "include" / "guidescan_amd.h").read_text()
    assert "#define GS_DECODE_FEATURES_ONLY 0x8000u" in header and api.GS_DECODE_FEATURES_ONLY == 0x8000
    flags = [api.GS_TEXT_SAM, api.GS_TEXT_COMPLETE, api.GS_TEXT_BAM, api.GS_TEXT_BGZF, api.GS_TEXT_FEATURES, api.GS_DECODE_NO_HEADER,
             api.GS_DECODE_BAM_END, api.GS_DECODE_FEATURES_ONLY]
    assert len(set(flags)) == len(flags) and all(f & (f - 1) == 0 for f in flags)
