"""`--annotate` on the host (no GPU): gs_debug_annotate_host - the kernels' shared header gs_annot_scan.h run on the CPU - and
the host encoders' twins against tests/annot_model.py, exactly, on the planted genome of tests/design_cases.py; the
annotation object's refusals."""
from importlib import import_module

import numpy as np
import pytest

import annot_cases as ac
import annot_model as am
import design_cases as dc
import oracle_lib as ol

api = import_module("guidescan-cli_amd.api")


def host_annotation(bed):
    rg = api.Regions.parse(bed.encode(), ac.structure())
    an = api.Annotation.build(rg, device=None)
    rg.close()   # the annotation stands alone
    return an


@pytest.fixture(scope="module")
def annotation():
    an = host_annotation(ac.case_bed())
    yield an
    an.close()


def assert_equal(got, want):
    for name, g, w in zip(("feat_offsets", "feats", "guide_counts"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape and np.array_equal(g, w), name


def test_every_position_of_every_chromosome_on_both_strands(annotation):
    offsets, hits, want = ac.every_position()
    names, lengths = ac.structure()
    gs = api.make_genome_structure(names, lengths)
    assert_equal(api.annotate_host_model(annotation, gs, offsets, hits, ac.L, ac.P, ac.M), want)


def test_the_cases_the_bed_file_is_made_of(annotation):
    """what the big comparison rests on, looked at row by row through the model: one base at either end, abutting, the
    gene once, a group in two pieces once, the stacks, the clipped s == 0 row, the empty chromosome"""
    names, lengths = ac.structure()
    groups, lines = am.bed_lines(ac.case_bed())
    feats = lambda c, s: [groups[g] for g in am.row_features(names[c], s, ac.W, lengths[c], lines)]
    assert feats(0, 501 - ac.W + 1) == ["one_base"] and feats(0, 501 - ac.W) == [] and feats(0, 501) == ["one_base"] and feats(0, 502) == []
    assert feats(0, 601) == ["one_footprint"] and feats(0, 624) == ["abuts_it"] and feats(0, 623) == ["one_footprint", "abuts_it"]
    assert feats(0, 1031) == ["gene", "exon0"] and feats(0, 1041) == ["gene"]          # spans the exon's edge: the gene once
    assert feats(0, 1991) == ["pieces", "between"]                                       # both pieces, the group once
    assert len(feats(1, 690)) == 70 and len(feats(1, 1490)) == 300
    assert feats(0, 0) == ["first_base"] and feats(1, 0) == ["head"] and feats(1, ac.W) == []
    assert all(not feats(2, s) for s in range(0, lengths[2], 97))
    assert "two_chromosomes" in feats(0, 3001) and "two_chromosomes" in feats(1, 101)
    assert annotation.info()["groups"] == len(groups) == len(annotation.names) and annotation.names == groups
    assert annotation.info()["entries"] >= 370 and annotation.info()["segments"] > 30


@pytest.mark.parametrize("n_hits", ac.SIZES)
def test_lists_that_begin_past_zero_with_empty_guides(annotation, n_hits):
    offsets, hits = ac.sized(n_hits)
    names, lengths = ac.structure()
    gs = api.make_genome_structure(names, lengths)
    want = am.annotate(offsets, hits, names, lengths, ac.L, ac.P, ac.M, ac.case_bed())
    assert int(offsets[0]) == 5 and want[0].shape[0] == n_hits + 1 and want[2].sum() > 0
    assert_equal(api.annotate_host_model(annotation, gs, offsets, hits, ac.L, ac.P, ac.M), want)


def test_a_distance_beyond_the_budget_is_refused(annotation):
    offsets, hits = ac.sized(64)
    names, lengths = ac.structure()
    with pytest.raises(api.GsError) as e:
        api.annotate_host_model(annotation, api.make_genome_structure(names, lengths), offsets, hits, ac.L, ac.P, 1)
    assert e.value.status == 1


@pytest.mark.parametrize("cfg", ac.TEXT_CFGS, ids=lambda c: f"complete{c['complete']}-max{c['max_off_targets']}")
def test_the_fast_path_twin_adds_one_column(annotation, cfg):
    b = ac.text_batch(np.random.default_rng(3))
    plain = api.format_guides(*b, ac.M, **cfg)
    twin = api.format_guides(*b, ac.M, features=annotation, **cfg)
    col = ac.check_text(twin, plain, ac.case_bed())
    assert plain.count(b",NA,NA,NA,0") == 1 and b"g5," not in plain
    if cfg["max_off_targets"] != 0:
        assert any(";" in c for c in col) and "NA" in col and any(c.count(";") >= 69 for c in col)
    # guide by guide, the per-guide twin writes the same bytes
    gs, ids, seqs, pams, senses, offsets, hits, spec = b
    one = "".join(api.format_guide(gs, ids[g], seqs[g], pams[g], senses[g], hits[int(offsets[g]):int(offsets[g + 1])], ac.M,
                                   specificity=spec[g], features=annotation, **cfg) for g in range(len(ids)))
    assert one.encode() == twin


def test_the_general_path_twin_adds_one_column(annotation):
    """hits with bulges: the row's width is still the guide's own L + P"""
    names, lengths = ac.structure()
    gs = api.make_genome_structure(names, lengths)
    hits = np.zeros(5, dtype=api.HIT_EX_DTYPE)
    hits["pos"] = [499 + ac.W - 1, -700, 1031 + ac.W - 2, lengths[0] + 3, lengths[0] + 700 + 5]
    hits["mismatches"] = [0, 0, 1, 1, 2]
    for i, s in enumerate((b"ACGTACGTACGTACGTACGTAGG", b"ACGTACGTAC.TACGTACGTAGG", b"ACGTACGTACGgTACGTACGTAGG", b"ACGTACGTACGTACGTACGTCGG",
                           b"AAGTACGTACGTACGTACGTTGG")):
        hits["seq"][i], hits["seq_len"][i] = s, len(s)
    hits["rna_bulges"][1] = hits["dna_bulges"][2] = 1
    for complete in (True, False):
        plain = api.format_guide_ex(gs, "b0", "ACGTACGTACGTACGTACGT", "NGG", True, hits, ac.M, complete=complete).encode()
        twin = api.format_guide_ex(gs, "b0", "ACGTACGTACGTACGTACGT", "NGG", True, hits, ac.M, complete=complete, features=annotation).encode()
        col = ac.check_text(twin, plain, ac.case_bed())
        assert len(col) == 4 and col[0] == "one_base" and col[1] == "NA" and col[3].count(";") >= 69


def test_the_header_and_the_flag_s_refusals(annotation):
    names, lengths = ac.structure()
    gs = api.make_genome_structure(names, lengths)
    for complete in (True, False):
        assert api.format_header(gs, complete=complete, features=True) == \
            api.format_header(gs, complete=complete)[:-1] + ",match_features\n"
    with pytest.raises(api.GsError) as e:
        api.format_header(gs, sam=True, features=True)
    assert e.value.status == 1
    b = ac.text_batch(np.random.default_rng(3), 4)
    with pytest.raises(api.GsError) as e:
        api.format_guides(*b, ac.M, sam=True, features=annotation)
    assert e.value.status == 1
    other = api.make_genome_structure(names, [n + 1 for n in lengths])   # not the structure the BED file was read against
    with pytest.raises(api.GsError) as e:
        api.format_guides(other, *b[1:], ac.M, features=annotation)
    assert e.value.status == 1


def test_a_semicolon_in_a_group_name_is_refused():
    names, lengths = ac.structure()
    rg = api.Regions.parse(f"{names[0]}\t5\t9\tfine\n{names[0]}\t50\t90\tgene;exon\n".encode(), (names, lengths))
    with pytest.raises(api.GsError) as e:
        api.Annotation.build(rg, device=None)
    assert e.value.status == 6 and "gene;exon" in str(e.value)
    rg.close()


def test_a_table_past_the_entry_cap_is_refused():
    names, lengths = ac.structure()
    bed = "".join(f"{names[0]}\t0\t1000\tg{i}\n" for i in range(100))
    before = api.annot_entry_cap()
    assert before == 1 << 31
    try:
        assert api.annot_entry_cap(99) == 99
        with pytest.raises(api.GsError) as e:
            host_annotation(bed)
        assert e.value.status == 1
        assert api.annot_entry_cap(100) == 100
        an = host_annotation(bed)
        assert an.info() == {"groups": 100, "segments": 1, "entries": 100}
        an.close()
    finally:
        api.annot_entry_cap(before)


# ---- the selection rule's model, shared with tests/test_gpu_annotate.py -------------------------------------------------

def dup_bed():
    """the chr2 copy of the planted duplicate only"""
    _, names, _, _ = dc.genome()
    s, e, c, at = dc.DUP
    return f"{names[c]}\t{at}\t{at + (e - s)}\tcopy\n"


def feature_hits_model(recs, oidx, distance, mismatches=dc.MISMATCHES):
    """adds feature_hits to every record: its off-target hits within `distance` whose row touches dup_bed(), the record's
    own site - the distance-0 hit that resolves to the record's chromosome, position and sense - left out"""
    _, names, lengths, _ = dc.genome()
    _, lines = am.bed_lines(dup_bed())
    opts = ol.make_opts(mismatches=mismatches)
    for r in recs:
        hits, _, raw = oidx.enumerate(r["seq"], "NGG", opts)
        ol.lib().gso_free(raw[0])
        n = 0
        for h in hits:
            loc = am.resolve(int(h[0]), lengths, 20, 3)
            if loc is None or h[1] > distance:
                continue
            if h[1] == 0 and loc == (r["chr"], r["pos"], r["sense"]):
                continue
            n += bool(am.row_features(names[loc[0]], loc[1], 23, lengths[loc[0]], lines))
        r["feature_hits"] = n
    return recs


def test_the_rule_s_model_decides_the_planted_duplicate():
    """max_hits = 0: the chr1 records of the `dup` group that lie in the copied segment have the chr2 copy as an off-target
    in a feature; the chr2 records' own site is the one in the feature and does not count"""
    text, names, lengths, _ = dc.genome()
    groups, recs = dc.model_records(dc.selection_bed())
    oidx = ol.OracleIndex(text)
    feature_hits_model(recs, oidx, dc.MISMATCHES)
    oidx.close()
    s, e, c, at = dc.DUP
    dup = [r for r in recs if groups[r["group"]] == "dup"]
    inside1 = [r for r in dup if r["chr"] == 0 and s <= r["pos"] - 1 and r["pos"] - 1 + 23 <= e]
    inside2 = [r for r in dup if r["chr"] == c and at <= r["pos"] - 1 and r["pos"] - 1 + 23 <= at + (e - s)]
    assert inside1 and len(inside1) == len(inside2)
    assert all(r["feature_hits"] >= 1 for r in inside1) and all(r["feature_hits"] == 0 for r in inside2)
    assert all(r["feature_hits"] == 0 for r in recs if groups[r["group"]] == "small")
