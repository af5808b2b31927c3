"""`--annotate` on the GPU (csrc/gs_annot.hip, the feature column of csrc/gs_textdev.hip, the feature rule of
csrc/gs_design.hip) against tests/annot_model.py: feature offsets, features and per-guide counts for equality, the text
byte for byte against the host encoders' twins.  The cases are those of tests/test_annot_model.py."""
import ctypes as C
from importlib import import_module

import numpy as np
import pytest

import annot_cases as ac
import annot_model as am
import design_cases as dc
import design_model as dm
import oracle_lib as ol
from test_annot_model import assert_equal, dup_bed, feature_hits_model
from test_gpu_design import device_design, selected
from test_design_model import assert_same
from test_gpu_text_device import device_text

api = import_module("guidescan-cli_amd.api")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    """the planted genome's index, the case BED's annotation on the device, the structure"""
    text, names, lengths, _ = dc.genome()
    gidx = api.GenomeIndex.build(text, device=0)
    rg = api.Regions.parse(ac.case_bed().encode(), (names, lengths))
    an = api.Annotation.build(rg, device=0)
    rg.close()
    yield gidx, an, api.make_genome_structure(names, lengths)
    gidx.set_annotation(None)
    an.close()
    gidx.close()


def test_every_position_of_every_chromosome_on_both_strands(gpu):
    gidx, an, gs = gpu
    offsets, hits, want = ac.every_position()
    assert_equal(gidx.annotate(an, gs, offsets, hits, ac.L, ac.P, ac.M), want)


@pytest.mark.parametrize("n_hits", ac.SIZES)
def test_lists_that_begin_past_zero_with_empty_guides(gpu, n_hits):
    gidx, an, gs = gpu
    offsets, hits = ac.sized(n_hits)
    names, lengths = ac.structure()
    want = am.annotate(offsets, hits, names, lengths, ac.L, ac.P, ac.M, ac.case_bed())
    assert_equal(gidx.annotate(an, gs, offsets, hits, ac.L, ac.P, ac.M), want)


def test_device_pointers_with_offsets_that_begin_past_zero(gpu):
    """gs_annotate_device itself on a list whose d_offsets[0] is 5: the results are indexed from the list's first hit"""
    import torch
    gidx, an, gs = gpu
    offsets, hits = ac.sized(257)
    names, lengths = ac.structure()
    want = am.annotate(offsets, hits, names, lengths, ac.L, ac.P, ac.M, ac.case_bed())
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
    d_o, d_h = up(offsets), up(hits)
    torch.cuda.synchronize()
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    n = len(offsets) - 1
    with gidx.locked():
        fo, ft, gc = gidx.annotate_device(an, gs, n, ac.L, ac.P, ac.M, d_o.data_ptr(), d_h.data_ptr())
        foff = np.empty(258, np.uint64)
        gcnt = np.empty((n, ac.M + 1), np.uint32)
        assert hip.hipMemcpy(foff.ctypes.data, fo, foff.nbytes, 2) == 0 and hip.hipMemcpy(gcnt.ctypes.data, gc, gcnt.nbytes, 2) == 0
        feats = np.empty(int(foff[-1]), np.uint32)
        assert hip.hipMemcpy(feats.ctypes.data, ft, feats.nbytes, 2) == 0
    assert_equal((foff, feats, gcnt), want)


def test_a_distance_beyond_the_budget_is_refused(gpu):
    gidx, an, gs = gpu
    offsets, hits = ac.sized(64)
    with pytest.raises(api.GsError) as e:
        gidx.annotate(an, gs, offsets, hits, ac.L, ac.P, 1)
    assert e.value.status == 1


@pytest.mark.parametrize("cfg", ac.TEXT_CFGS, ids=lambda c: f"complete{c['complete']}-max{c['max_off_targets']}")
def test_device_text_equals_the_host_twin(gpu, cfg):
    gidx, an, gs = gpu
    b = ac.text_batch(np.random.default_rng(3))
    host_an = api.Annotation.build(api.Regions.parse(ac.case_bed().encode(), ac.structure()), device=None)
    want = api.format_guides(*b, ac.M, features=host_an, **cfg)
    ac.check_text(want, api.format_guides(*b, ac.M, **cfg), ac.case_bed())
    gidx.set_annotation(an)
    got = device_text(gidx, *b, ac.M, features=True, **cfg)
    assert got == want
    # the offsets cut the text at the guides
    cuts = gidx.last_text_offsets(len(b[1]))
    assert int(cuts[-1]) == len(got)
    gs_, ids, seqs, pams, senses, offsets, hits, spec = b
    for g in range(len(ids)):
        piece = got[int(cuts[g]):int(cuts[g + 1])]
        one = api.format_guide(gs_, ids[g], seqs[g], pams[g], senses[g], hits[int(offsets[g]):int(offsets[g + 1])], ac.M,
                               specificity=spec[g], features=host_an, **cfg).encode()
        assert piece == one, g
    # without the flag the attached annotation changes nothing
    assert device_text(gidx, *b, ac.M, **cfg) == api.format_guides(*b, ac.M, **cfg)
    host_an.close()


def test_enumerate_text_with_the_column(gpu):
    """search, scoring, annotation and encoding in one call on real guides of the planted genome"""
    gidx, an, gs = gpu
    names, lengths = ac.structure()
    cand = [c for c in dc.candidates()[0] if 980 <= c[1] <= 1250][:48] + [c for c in dc.candidates()[1] if 160 <= c[1] <= 400][:16]
    assert len(cand) > 20
    seqs = np.frombuffer("".join(s for s, _, _ in cand).encode(), np.uint8).reshape(len(cand), 20)
    pams = np.tile(np.frombuffer(b"NGG", np.uint8), (len(cand), 1))
    ids = [f"c{i}" for i in range(len(cand))]
    gidx.set_annotation(an)
    plain = gidx.enumerate_text(seqs, pams, ids, None, gs, mismatches=ac.M)
    with_col = gidx.enumerate_text(seqs, pams, ids, None, gs, mismatches=ac.M, features=True)
    col = ac.check_text(with_col, plain, ac.case_bed())
    assert any(c.startswith("gene") for c in col) and "NA" in col


def test_the_flag_s_refusals(gpu):
    gidx, an, gs = gpu
    b = ac.text_batch(np.random.default_rng(3), 4)
    gidx.set_annotation(an)
    for kind in (dict(sam=True), dict(bam=True)):
        with pytest.raises(api.GsError) as e:
            device_text(gidx, *b, ac.M, features=True, **kind)
        assert e.value.status == 1
    gidx.set_annotation(None)
    with pytest.raises(api.GsError) as e:
        device_text(gidx, *b, ac.M, features=True)
    assert e.value.status == 1
    seqs = np.frombuffer("".join(b[2]).encode(), np.uint8).reshape(4, 20)
    pams = np.tile(np.frombuffer(b"NGG", np.uint8), (4, 1))
    with pytest.raises(api.GsError) as e:
        gidx.enumerate_text(seqs, pams, b[1], None, gs, mismatches=ac.M, features=True)
    assert e.value.status == 1
    rg = api.Regions.parse(ac.case_bed().encode(), ac.structure())
    host_only = api.Annotation.build(rg, device=None)
    rg.close()
    with pytest.raises(api.GsError) as e:
        gidx.set_annotation(host_only)
    assert e.value.status == 1
    host_only.close()


def test_a_semicolon_and_the_entry_cap_are_refused_on_the_device_too():
    names, lengths = ac.structure()
    rg = api.Regions.parse(f"{names[0]}\t50\t90\tgene;exon\n".encode(), (names, lengths))
    with pytest.raises(api.GsError) as e:
        api.Annotation.build(rg, device=0)
    assert e.value.status == 6 and "gene;exon" in str(e.value)
    rg.close()
    rg = api.Regions.parse("".join(f"{names[0]}\t0\t1000\tg{i}\n" for i in range(100)).encode(), (names, lengths))
    before = api.annot_entry_cap()
    try:
        api.annot_entry_cap(99)
        with pytest.raises(api.GsError) as e:
            api.Annotation.build(rg, device=0)
        assert e.value.status == 1
    finally:
        api.annot_entry_cap(before)
    rg.close()


def test_the_feature_rule_drops_the_records_whose_copy_lies_in_a_feature(gpu):
    """design_cases.DUP: chr1[300:360) is planted again on chr2; the chr2 copy alone is annotated.  max_hits = 0"""
    gidx, _, _ = gpu
    text, names, lengths, _ = dc.genome()
    groups, recs = dc.model_records(dc.selection_bed())
    oidx = ol.OracleIndex(text)
    dm.score(recs, oidx, lengths, "NGG", mismatches=dc.MISMATCHES)
    feature_hits_model(recs, oidx, dc.MISMATCHES)
    oidx.close()
    rg_an = api.Regions.parse(dup_bed().encode(), (names, lengths))
    an = api.Annotation.build(rg_an, device=0)
    rg_an.close()
    d, rg = device_design(dc.selection_bed(), prefix="f:")
    d.set_feature_rule(an, dc.MISMATCHES, 0)
    d.score(gidx, mismatches=dc.MISMATCHES, batch=100)   # several batches, the last one short
    host = d.to_host()
    want = {(r["group"], r["chr"], r["pos"], r["sense"]): r for r in recs}
    assert host["n"] == len(want)
    s, e, c, at = dc.DUP
    dropped1 = kept2 = 0
    for i in range(host["n"]):
        r = want[(int(host["group"][i]), int(host["chr"][i]), int(host["pos"][i]), chr(host["sense"][i]))]
        assert int(host["feature_hits"][i]) == r["feature_hits"], r
        assert bool(host["eligible"][i]) == (r["feature_hits"] == 0), r
        inside = lambda lo: lo <= r["pos"] - 1 and r["pos"] - 1 + 23 <= lo + (e - s)
        if groups[r["group"]] == "dup" and r["chr"] == 0 and inside(s):
            assert not host["eligible"][i]
            dropped1 += 1
        if groups[r["group"]] == "dup" and r["chr"] == c and inside(at):
            assert host["eligible"][i]
            kept2 += 1
    assert dropped1 and dropped1 == kept2
    model = [dict(r, eligible=r["feature_hits"] == 0) for r in recs]
    for n, sp in ((None, None), (2, None), (3, 0.5)):
        km = d.select("f:", per_region=n, min_specificity=sp)
        assert_same(selected(km), dm.arrays(dm.select(model, per_region=n, min_specificity=sp), groups, names, "NGG", "f:"))
        km.close()
    # a larger allowance, and the rule taken off again: every record eligible
    d.set_feature_rule(an, dc.MISMATCHES, 1000)
    assert d.score(gidx, mismatches=dc.MISMATCHES).to_host()["eligible"].all()
    d.set_feature_rule(None, 0, 0)
    assert "feature_hits" not in d.score(gidx, mismatches=dc.MISMATCHES).to_host()
    d.close()
    rg.close()
    an.close()
