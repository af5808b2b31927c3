"""The device decoder with an annotation attached (gs_decoder_set_annotation, GS_TEXT_FEATURES, GS_DECODE_FEATURES_ONLY):
byte comparison against the decoder's own output WITHOUT the flag plus the column tests/annot_model.py gives each row from
the fields it prints (tests/decode_annot_cases.py) - never against text the code under test made.  A synthetic database of
four chromosomes (97, 64, 40 and 50 bases) with both clips, one-base footprints, a footprint over six segments, lists of
more than 64 words, a chromosome without intervals and one without off-targets; a row longer than the wave's LDS slice;
features-only; batch cuts; every entry point; the errors; and `enumerate --annotate` against `decode --annotate` on one
genome.  GPU only."""
import csv
import os
import subprocess
from collections import Counter
from importlib import import_module

import numpy as np
import pytest

import bam_make as bm
import decode_annot_cases as dac
import decode_golden as dg

pytestmark = pytest.mark.gpu
api = import_module("guidescan-cli_amd.api")
decode = dg.decode
CLI = dg.ROOT / "guidescan-cli_amd" / "bin" / "guidescan"
DC_LDS = 12288   # the bytes of a wave's slice in k_dc_write (GS_ROW_LDS, csrc/gs_rowtext.h)
HEADER = {"succinct": decode.SUCCINCT_HEADER + "\n", "complete": decode.COMPLETE_HEADER + "\n"}   # the script's, without the option


def annotation(bed, sq=dac.SQ, device=0):
    rg = api.Regions.parse(bed.encode(), ([n for n, _ in sq], [ln for _, ln in sq]))
    try:
        return api.Annotation.build(rg, device)
    finally:
        rg.close()


@pytest.fixture(scope="module")
def small():
    """the decoder of the synthetic database with its annotation attached, the records, the tables without the flag (with
    their header lines) and the expected tables with it"""
    recs, fasta, bed = dac.small_records(), dac.small_genome(), dac.small_bed()
    dec = api.Decoder(dac.SQ, fasta, device=0)
    plain = {m: (HEADER[m] + dec.decode_records(recs, complete=m == "complete")).encode("latin-1") for m in dg.MODES}
    an = annotation(bed)
    dec.set_annotation(an)
    want_complete, feats = dac.expected_complete(plain["complete"], dac.SQ, recs, bed)
    want = {"complete": want_complete, "succinct": dac.expected_succinct(plain["succinct"], plain["complete"], dac.SQ, recs, bed),
            "only": dac.expected_complete(plain["complete"], dac.SQ, recs, bed, features_only=True)[0]}
    yield dict(dec=dec, recs=recs, plain=plain, want=want, feats=feats, bed=bed, fasta=fasta)
    dec.close()
    an.close()


def body(table):
    return table.split(b"\n", 1)[1].decode("latin-1")


@pytest.mark.parametrize("mode", dg.MODES)
def test_synthetic_database(small, mode):
    dec, recs = small["dec"], small["recs"]
    # the attached annotation changes nothing without the flag, and the tables without it are the model's
    model = decode.Decoder(dac.SQ, small["fasta"], dg.TABLES)
    assert body(small["plain"][mode]) == "".join(r + "\n" for r in model.rows(recs, complete=mode == "complete"))
    assert dec.decode_records(recs, complete=mode == "complete") == body(small["plain"][mode])
    got = dec.decode_records(recs, complete=mode == "complete", features=True)
    assert got == body(small["want"][mode])
    if mode == "complete":
        assert dec.last_rows == len(small["feats"]) and any(small["feats"]) and not all(small["feats"])
        assert max(len(f) for f in small["feats"]) >= 5
        assert dec.annot_ms() > 0.0
    else:
        assert dec.last_rows == len(recs)
        counts = [tuple(int(v) for v in row.rsplit(",", 4)[1:]) for row in got.splitlines()]
        assert sum(map(sum, counts)) == sum(1 for f in small["feats"] if f) and sum(c != (0, 0, 0, 0) for c in counts) >= 6
        assert counts[[r.id for r in recs].index("desert")] == (0, 0, 0, 0)


def test_an_empty_stored_sequence_has_no_feature(small):
    """with x < LN a footprint of n >= 1 bases always keeps the base x: only n == 0 leaves none"""
    dec = small["dec"]
    recs = [decode.Record("empty", "", False, "cA", 5, dac.hex_list([(0, [dac.word("cA", 0, "-"), dac.word("cA", 36, "+")])]))]
    plain = (HEADER["complete"] + dec.decode_records(recs, complete=True)).encode()
    want, feats = dac.expected_complete(plain, dac.SQ, recs, small["bed"])
    assert feats == [[], []] and plain.count(b"\n") == 3
    assert dec.decode_records(recs, complete=True, features=True) == body(want)
    assert dec.decode_records(recs, complete=True, features=True, features_only=True) == "" and dec.last_rows == 0


def test_a_row_longer_than_the_lds_slice(small):
    """70 groups with names of 200 bytes over one base: the one row of an off-target there has 14 kB of names, more than
    the slice, and goes straight to HBM; the other rows of its tile are short"""
    names = [f"g{i:03d}_" + "x" * 195 for i in range(70)]
    bed = "".join(f"cD\t25\t26\t{n}\n" for n in names) + "cA\t0\t10\tshort\n"
    recs = [decode.Record("wide", "ACGTTGCAAGCTTGCATGCAAGG", False, "cD", 7,
                          dac.hex_list([(0, [dac.word("cA", 5, "+"), dac.word("cD", 25, "+")]), (2, [dac.word("cD", 26, "-"), dac.word("cD", 2, "-")])])),
            decode.Record("next", "ACGTTGCAAGCTTGCATGCAAGG", True, "cA", 9, dac.hex_list([(1, [dac.word("cD", 48, "+"), dac.word("cA", 3, "-")])]))]
    dec = api.Decoder(dac.SQ, small["fasta"], device=0)
    an = annotation(bed)
    try:
        dec.set_annotation(an)
        plain = (HEADER["complete"] + dec.decode_records(recs, complete=True)).encode()
        want, feats = dac.expected_complete(plain, dac.SQ, recs, bed)
        rows = want.split(b"\n")[1:-1]
        assert [len(f) for f in feats] == [1, 70, 0, 0, 0, 1] and max(map(len, rows)) > DC_LDS and sorted(map(len, rows))[-2] < 100
        for on_device in (False, True):
            assert dec.decode_records(recs, complete=True, features=True, on_device=on_device) == body(want)
        only, _ = dac.expected_complete(plain, dac.SQ, recs, bed, features_only=True)
        assert dec.decode_records(recs, complete=True, features=True, features_only=True) == body(only) and dec.last_rows == 3
        succinct = (HEADER["succinct"] + dec.decode_records(recs, complete=False)).encode()
        assert dec.decode_records(recs, complete=False, features=True) == body(dac.expected_succinct(succinct, plain, dac.SQ, recs, bed))
    finally:
        dec.close()
        an.close()


def test_features_only(small):
    dec, recs = small["dec"], small["recs"]
    got = dec.decode_records(recs, complete=True, features=True, features_only=True)
    assert got == body(small["want"]["only"])
    kept = [f for f in small["feats"] if f]
    assert dec.last_rows == len(kept) == got.count("\n") and 0 < len(kept) < len(small["feats"])
    # match_number is the unfiltered table's: every row stands in the full table as it is
    full = set(body(small["want"]["complete"]).splitlines())
    assert all(row in full for row in got.splitlines())
    # a whole tile of 64 slots without a row: the off-targets of `desert` are slots [a, a + 130) and none has a feature
    words = np.cumsum([0] + [len(r.hex or "") // 16 for r in recs])
    at = [r.id for r in recs].index("desert")
    a, b = int(words[at]), int(words[at + 1])
    assert any(a <= t * 64 and (t + 1) * 64 <= b - 2 for t in range(b // 64 + 1))
    assert not any(row.startswith("desert,") for row in got.splitlines())


@pytest.mark.parametrize("batch", [1, 7])
def test_batch_cuts_change_nothing(small, batch):
    dec, recs = small["dec"], small["recs"]
    for key, kw in (("complete", dict(complete=True)), ("succinct", dict(complete=False)), ("only", dict(complete=True, features_only=True))):
        parts = [dec.decode_records(recs[i:i + batch], first_record=i, features=True, **kw) for i in range(0, len(recs), batch)]
        assert "".join(parts) == body(small["want"][key]), key


@pytest.mark.parametrize("mode", dg.MODES)
def test_entry_points(small, mode):
    dec, recs = small["dec"], small["recs"]
    complete = mode == "complete"
    want = small["want"][mode].decode("latin-1")
    sam = dac.sam_text(recs)
    assert dec.decode_sam(sam.encode(), complete=complete, features=True) == want                       # with the header line
    assert dec.decode_sam(sam.encode(), complete=complete, features=True, header=False) == body(small["want"][mode])
    assert dec.decode_sam(sam.encode(), complete=complete) == small["plain"][mode].decode("latin-1")
    assert dec.decode_records(recs, complete=complete, features=True, on_device=True) == body(small["want"][mode])
    head, records = bm.from_sam(sam)
    raw = head + b"".join(records)
    for piece in (0xff00, 700):
        bgzf = b"".join(bm.members(raw, piece=piece)) + bm.EOF_BLOCK
        for on_device in (True, False):
            text, n, tail = dec.decode_bam(bgzf, skip=len(head), ref_to_sq=range(len(dac.SQ)), complete=complete, end=True,
                                           on_device=on_device, features=True)
            assert (text, n, tail) == (body(small["want"][mode]), len(recs), 0)
    # in two groups of members, a record cut between them
    parts = bm.members(raw, piece=700)
    cut = len(parts) // 2
    t1, n1, tail = dec.decode_bam(b"".join(parts[:cut]), skip=len(head), ref_to_sq=range(len(dac.SQ)), complete=complete, on_device=True,
                                  features=True)
    t2, n2, _ = dec.decode_bam(b"".join(parts[cut:]), ref_to_sq=range(len(dac.SQ)), complete=complete, first_record=n1, end=True,
                               on_device=True, features=True)
    assert t1 + t2 == body(small["want"][mode]) and n1 + n2 == len(recs) and tail > 0
    if complete:
        text, _, _ = dec.decode_bam(b"".join(parts) + bm.EOF_BLOCK, skip=len(head), ref_to_sq=range(len(dac.SQ)), complete=True, end=True,
                                    on_device=True, features=True, features_only=True)
        assert text == body(small["want"]["only"])


def test_errors(small):
    dec, recs = small["dec"], small["recs"]
    # a bad hex word: the same record and reason with the flag as without it, in every mode
    bad = decode.Record("badhex", recs[0].seq, False, "cA", 1, recs[0].hex[:-3] + "xyz")
    batch = recs[:3] + [bad] + recs[3:]
    for kw in (dict(complete=False), dict(complete=True), dict(complete=True, features_only=True)):
        with pytest.raises(api.GsError) as plain:
            dec.decode_records(batch, complete=kw["complete"], first_record=40)
        with pytest.raises(api.GsError) as flagged:
            dec.decode_records(batch, first_record=40, features=True, **kw)
        assert flagged.value.status == plain.value.status == 6 and str(flagged.value) == str(plain.value)
        assert "record 43 (badhex)" in str(flagged.value) and decode.REASONS[decode.ERR_HEX] in str(flagged.value)
    with pytest.raises(api.GsError) as e:
        dec.decode_sam(dac.sam_text(batch).encode(), complete=True, features=True)
    assert e.value.status == 6 and "record 3 (badhex)" in str(e.value)
    # GS_DECODE_FEATURES_ONLY without GS_TEXT_FEATURES | GS_TEXT_COMPLETE
    for kw in (dict(complete=False, features=True, features_only=True), dict(complete=True, features_only=True)):
        with pytest.raises(api.GsError) as e:
            dec.decode_records(recs, **kw)
        assert e.value.status == 1
        with pytest.raises(api.GsError) as e:
            dec.decode_sam(b"", **kw)
        assert e.value.status == 1
    # the annotation of another structure, of the host only; the flag without an annotation
    other = [(n, ln + (1 if n == "cB" else 0)) for n, ln in dac.SQ]
    for make in (lambda: annotation(small["bed"], other), lambda: annotation(small["bed"], dac.SQ[:3] + [("cD", 50), ("cE", 9)]),
                 lambda: annotation(small["bed"], device=None)):
        an = make()
        with pytest.raises(api.GsError) as e:
            dec.set_annotation(an)
        assert e.value.status == 1
        an.close()
    assert dec.decode_records(recs, complete=True, features=True) == body(small["want"]["complete"])   # the attachment stands
    bare = api.Decoder(dac.SQ, small["fasta"], device=0)
    try:
        sam = dac.sam_text(recs).encode()
        head, records = bm.from_sam(sam.decode())
        bgzf = b"".join(bm.members(head + b"".join(records))) + bm.EOF_BLOCK
        for call in (lambda: bare.decode_records(recs, complete=True, features=True), lambda: bare.decode_records(recs, features=True, on_device=True),
                     lambda: bare.decode_sam(sam, features=True), lambda: bare.decode_sam(b"", features=True),
                     lambda: bare.decode_bam(bgzf, skip=len(head), ref_to_sq=range(4), end=True, features=True),
                     lambda: bare.decode_bam(bgzf, skip=len(head), ref_to_sq=range(4), end=True, features=True, on_device=True)):
            with pytest.raises(api.GsError) as e:
                call()
            assert e.value.status == 1
        assert bare.decode_records(recs, complete=True) == body(small["plain"]["complete"])
        # attached and detached again
        an = annotation(small["bed"])
        bare.set_annotation(an)
        assert bare.decode_records(recs, complete=False, features=True) == body(small["want"]["succinct"])
        bare.set_annotation(None)
        with pytest.raises(api.GsError):
            bare.decode_records(recs, features=True)
        an.close()
    finally:
        bare.close()


def test_the_script_s_failures_win_over_a_row_that_is_too_long(small):
    """about 141,000 groups with names of 236 bytes over one base: the row of an off-target there would pass 32 MB, which
    the decoder refuses (GS_ERR_UNSUPPORTED).  With a record behind it that the script fails on, the answer is that
    record's GS_ERR_FORMAT, word for word what it is without the flag"""
    n_groups = (1 << 25) // 237 + 200
    bed = "".join(f"cD\t25\t26\t{i:06d}{'y' * 230}\n" for i in range(n_groups))
    wide = decode.Record("wide", "ACGTTGCAAGCTTGCATGCAAGG", False, "cD", 7, dac.hex_list([(0, [dac.word("cD", 25, "+")])]))
    ok = decode.Record("ok", "ACGTTGCAAGCTTGCATGCAAGG", False, "cA", 7, dac.hex_list([(1, [dac.word("cA", 40, "-")])]))
    bad = decode.Record("far", "ACGTTGCAAGCTTGCATGCAAGG", False, "cA", 7, dac.hex_list([(1, [sum(ln for _, ln in dac.SQ) + 5])]))
    dec = api.Decoder(dac.SQ, small["fasta"], device=0)
    an = annotation(bed)
    try:
        dec.set_annotation(an)
        assert an.info()["entries"] == n_groups
        with pytest.raises(api.GsError) as e:
            dec.decode_records([ok, wide], complete=True, features=True)
        assert e.value.status == 3 and "32 MB" in str(e.value)
        plain = dec.decode_records([ok, wide], complete=False).splitlines()        # succinct rows do not grow with the names
        assert dec.decode_records([ok, wide], complete=False, features=True).splitlines() == [plain[0] + ",0,0,0,0", plain[1] + ",1,0,0,0"]
        with pytest.raises(api.GsError) as plain:
            dec.decode_records([ok, wide, bad], complete=True, first_record=10)
        with pytest.raises(api.GsError) as flagged:
            dec.decode_records([ok, wide, bad], complete=True, first_record=10, features=True)
        assert flagged.value.status == 6 and str(flagged.value) == str(plain.value) and "record 12 (far)" in str(flagged.value)
    finally:
        dec.close()
        an.close()


# ---- `enumerate --annotate` and `decode --annotate` give a site the same features ---------------------------------------
def run(args):
    env = dict(os.environ)
    env.pop("GS_ENCODER", None)
    return subprocess.run([str(CLI)] + [str(a) for a in args], capture_output=True, text=True, timeout=300, env=env)


def planted_genome(tmp_path):
    """three chromosomes (3,000, 2,000 and 1,500 bases) with planted near-copies of ten guides on both strands, sites at both
    ends of k2, and a BED file over k1 and k2 -> (FASTA path, BED path)"""
    rng = np.random.default_rng(77)
    lens = {"k1": 3000, "k2": 2000, "k3": 1500}
    chrom = {n: list(rng.choice(list("ACGT"), ln)) for n, ln in lens.items()}
    comp = {"A": "T", "C": "G", "G": "C", "T": "A"}
    at = {n: 40 for n in lens}
    for t in range(10):
        template = list(rng.choice(list("ACGT"), 20)) + list("TGG")
        for copy in range(6):
            name = list(lens)[int(rng.integers(0, 3))]
            site = list(template)
            for i in rng.choice(20, int(rng.integers(0, 4)), replace=False):
                site[i] = str(rng.choice([b for b in "ACGT" if b != site[i]]))
            if copy & 1:
                site = [comp[b] for b in reversed(site)]
            if at[name] + 23 > lens[name] - 5:
                continue
            chrom[name][at[name]:at[name] + 23] = site
            at[name] += 23 + int(rng.integers(0, 40))
    # sites at both ends of a chromosome: rows whose footprint begins at base 0 or ends at the last base
    chrom["k2"][0:23] = list("ACGTTGCATGCATTGCAAGCTGG")
    chrom["k2"][-23:] = [comp[b] for b in reversed("ACGTTGCATGCATTGCAAGCAGG")]
    fa = tmp_path / "g.fa"
    fa.write_text("".join(f">{n}\n{''.join(s)}\n" for n, s in chrom.items()))
    bed_rows = []
    for n, ln in lens.items():
        if n == "k3":
            continue
        bed_rows += [f"{n}\t0\t1\tfirst_{n}", f"{n}\t{ln - 1}\t{ln}\tlast_{n}", f"{n}\t{ln // 4}\t{ln // 2}\tgene_{n}"]
        bed_rows += [f"{n}\t{p}\t{p + 9}\texon_{'ab'[i & 1]}" for i, p in enumerate(range(30, ln - 20, 31))]
    bed = tmp_path / "f.bed"
    bed.write_text("\n".join(bed_rows) + "\n")
    return fa, bed


def test_enumerate_annotate_and_decode_annotate_agree(tmp_path):
    """On a genome of three chromosomes (3,000, 2,000 and 1,500 bases) with planted near-copies of ten guides, the same
    guides through `enumerate --format csv --mode complete --annotate BED` and through `enumerate --format sam --mode
    complete` followed by `decode --mode complete --annotate BED`: for every guide the multiset of (distance, strand,
    chromosome, features) over its rows is equal.  Both rules describe the same L + P bases of a site."""
    fa, bed = planted_genome(tmp_path)
    prefix = tmp_path / "g"
    assert run(["index", "--index", prefix, fa]).returncode == 0
    kmers = tmp_path / "kmers.csv"
    assert run(["kmers", prefix, "-o", kmers]).returncode == 0
    out_csv, out_sam, decoded = tmp_path / "db.csv", tmp_path / "db.sam", tmp_path / "decoded.csv"
    r = run(["enumerate", prefix, "-f", kmers, "-m", 3, "--format", "csv", "--mode", "complete", "--annotate", bed, "-o", out_csv])
    assert r.returncode == 0, r.stderr
    r = run(["enumerate", prefix, "-f", kmers, "-m", 3, "--format", "sam", "--mode", "complete", "-o", out_sam])
    assert r.returncode == 0, r.stderr
    r = run(["decode", "--mode", "complete", "--annotate", bed, "-o", decoded, out_sam, fa])
    assert r.returncode == 0, r.stderr
    by_enumerate, records = {}, []
    with open(out_csv) as f:
        for row in csv.DictReader(f):
            if row["match_chrm"] != "NA":
                by_enumerate.setdefault(row["id"], Counter())[row["match_distance"], row["match_strand"], row["match_chrm"],
                                                               row["match_features"]] += 1
    # the SAM database has one record for every perfect site of a guide (a guide planted twice has two, each with the
    # guide's whole list): the decoded rows are taken record by record, a record's rows beginning at match_number 0
    with open(decoded) as f:
        for row in csv.DictReader(f):
            if row["match_number"] == "0":
                records.append((row["id"], Counter()))
            assert records[-1][0] == row["id"]
            records[-1][1][row["distance"], row["sense"], row["chromosome"], row["match_features"]] += 1
    ids = {i for i, _ in records}
    assert len(ids) > 50 and len(records) > len(ids) and sum(len(c) for _, c in records) > len(records)
    assert any(";" in k[3] for _, c in records for k in c)
    assert any(k[3].startswith("first_") for _, c in records for k in c) and any("last_" in k[3] for _, c in records for k in c)
    for i, c in records:
        assert c == by_enumerate[i], i


def test_a_tile_at_the_border_of_the_lds_slice(small):
    """A tile is composed in the wave's slice while a0 + total <= 12288 (a0: the tile's offset in the text mod 16) and
    straight in HBM beyond.  Three records of 62 off-targets each are three tiles of 64 words; one off-target of the second
    lies under 46 groups with names of 200 bytes and one more whose name grows byte by byte over 48 values, so that its
    tile's total passes from 12288 - 24 to 12288 + 23 and crosses the border whatever a0 is.  The rows without the option are
    the Python model's, the column is annot_model's."""
    rng = np.random.default_rng(21)
    guide = "ACGTTGCAAGCTTGCATGCAAGG"

    def rec(name, d, first):
        ws = [first] + [dac.word("cA", int(x), "+-"[int(s)]) for x, s in zip(rng.integers(30, 90, 61), rng.integers(0, 2, 61))]
        r = decode.Record(name, guide, False, "cA", 3, dac.hex_list([(d, ws)]))
        assert len(r.hex) == 64 * 16
        return r

    recs = [rec("before", 0, dac.word("cA", 40, "+")), rec("wide", 1, dac.word("cD", 25, "+")), rec("behind", 2, dac.word("cB", 5, "-"))]
    model = decode.Decoder(dac.SQ, small["fasta"], dg.TABLES)
    plain = (HEADER["complete"] + "".join(r + "\n" for r in model.rows(recs, complete=True))).encode("latin-1")
    assert plain.count(b"\n") == 1 + 3 * 62
    fixed = "".join(f"cD\t25\t26\tf{i:02d}_" + "x" * 196 + "\n" for i in range(46)) + "cA\t35\t37\tshort\n"

    def expected(length):
        bed = fixed + "cD\t25\t26\t" + "s" * length + "\n"
        want, feats = dac.expected_complete(plain, dac.SQ, recs, bed)
        rows = want.split(b"\n")[1:-1]
        assert len(feats[62]) == 47 and {len(f) for f in feats[63:124]} == {0, 1}   # one wide row; `short` touches some others
        return bed, want, sum(len(r) + 1 for r in rows[62:124])

    start = 1 + DC_LDS - 24 - expected(1)[2]
    assert 1 <= start and start + 47 <= 230   # the parser admits names of 238 bytes here
    dec = api.Decoder(dac.SQ, small["fasta"], device=0)
    totals = []
    try:
        for length in range(start, start + 48):
            bed, want, total = expected(length)
            totals.append(total)
            an = annotation(bed)
            dec.set_annotation(an)
            got = dec.decode_records(recs, complete=True, features=True)
            dec.set_annotation(None)
            an.close()
            assert got == body(want), f"a name of {length} bytes"
    finally:
        dec.close()
    assert totals == list(range(DC_LDS - 24, DC_LDS + 24))
