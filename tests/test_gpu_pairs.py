"""Guide pairs for regions on the GPU (csrc/gs_pairs.hip) against tests/pairs_model.py on every case of
tests/pairs_cases.py: the pairs' arrays with the specificities bit for bit, the guides object and the table byte for byte,
the tallies; chunks of whole groups; and the selection of the same design before and after, unchanged."""
import os
from importlib import import_module

import numpy as np
import pytest

import design_cases as dc
import design_model as dm
import pairs_cases as pc
import pairs_model as pm
from test_design_model import assert_same
from test_gpu_design import device_design, selected
from test_pairs_model import assert_same_pairs

api = import_module("guidescan-cli_amd.api")

pytestmark = pytest.mark.gpu

PREFIX = "p:"


@pytest.fixture(scope="module")
def designs():
    """(record set, with -t 1) -> the design scored on the device, made when first asked for.  23-mers with a four-symbol
    PAM have a 58-bit key, which the search carries only with the table-seeded kernels: at the depth a 13 kb genome gets
    by default they are GS_ERR_UNSUPPORTED, so that shape is scored on a handle built with GS_PREFIX_K = 11 (a handle
    reads the environment once, when it is made)."""
    text = dc.genome()[0]
    indexes, made = {}, {}

    def index(deep):
        if deep not in indexes:
            saved = os.environ.get("GS_PREFIX_K")
            if deep:
                os.environ["GS_PREFIX_K"] = "11"
            try:
                indexes[deep] = api.GenomeIndex.build(text, device=0)
            finally:
                if saved is None:
                    os.environ.pop("GS_PREFIX_K", None)
                else:
                    os.environ["GS_PREFIX_K"] = saved
        return indexes[deep]

    def get(name, thr):
        if (name, thr) not in made:
            bed, pam, k, start, mismatches = pc.RECORD_SETS[name]
            d, rg = device_design(bed(), pam, k, start, prefix=PREFIX)
            d.score(index(2 * k + 3 * len(pam) > 52), mismatches=mismatches, start=start, threshold=1 if thr else -1)
            made[(name, thr)] = (d, rg)
        return made[(name, thr)][0]

    yield get
    for d, rg in made.values():
        d.close()
        rg.close()
    for gidx in indexes.values():
        gidx.close()


def run_case(d, case):
    """-> what the device gives and what the model wants: (pairs, guides, table, last) each"""
    groups, recs, kept, rule = pc.expected(case)
    _, _, pam, k, start, _ = pc.shape(case)
    names = dc.genome()[1]
    C = rule.get("cut_offset", 3)
    sel, place = pm.guides(recs, kept)
    want = (pm.arrays(recs, kept, k, len(pam), C, start, place), dm.arrays(sel, groups, names, pam, PREFIX),
            pm.table(recs, kept, groups, names, k, len(pam), C, start, PREFIX).encode(),
            pm.last(recs, kept, k, len(pam), n_groups=len(groups), **rule))
    km, pr = d.pairs(PREFIX, **rule)
    try:
        got = (pr.to_host(), selected(km), pr.rows(km), pr.last())
    finally:
        km.close()
        pr.close()
    return got, want


def assert_case(got, want, chunks=None):
    assert_same_pairs(got[0], want[0])
    assert_same(got[1], want[1])
    assert got[1]["n"] == len(want[1]["pos"])
    assert got[2] == want[2]
    assert got[3] == (want[3] if chunks is None else dict(want[3], chunks=chunks))


@pytest.mark.parametrize("case", pc.CASE_IDS)
def test_pairs_against_the_model(designs, case):
    name, thr, _, _, _, _ = pc.shape(case)
    got, want = run_case(designs(name, thr), case)
    assert_case(got, want)


def test_the_cases_decide_something():
    pc.assert_cases_decide()


@pytest.mark.parametrize("case", pc.CHUNK_CASES)
def test_chunks_of_whole_groups(designs, case):
    name, thr, _, _, _, _ = pc.shape(case)
    d = designs(name, thr)
    exact, below, group, count, n_chunks = pc.chunk_sizes(case)
    default = api.pairs_chunk()
    try:
        api.pairs_chunk(exact)
        got, want = run_case(d, case)
        assert_case(got, want, chunks=n_chunks)
        api.pairs_chunk(below)
        with pytest.raises(api.GsError) as e:
            d.pairs(PREFIX, **pc.expected(case)[3])
        assert e.value.status == 3 and f"'{group}'" in str(e.value) and str(count) in str(e.value)
    finally:
        api.pairs_chunk(default)
    got, want = run_case(d, case)
    assert_case(got, want)


def test_the_selection_of_the_design_is_what_it_was(designs):
    """select() and rows() go through the passes that pairs() shares with them: before and after, the model's"""
    d = designs("sel", True)
    groups, recs = pc.records("sel", True)
    names = dc.genome()[1]

    def check():
        for n, s in ((None, None), (3, 0.75), (7, None)):
            sel = dm.select(recs, per_region=n, min_specificity=s)
            km = d.select(PREFIX, per_region=n, min_specificity=s)
            assert_same(selected(km), dm.arrays(sel, groups, names, "NGG", PREFIX))
            km.close()
            assert d.rows(PREFIX, per_region=n, min_specificity=s).decode() == dm.rows(sel, groups, names, "NGG", PREFIX)
            assert d.last_select()["kept"] == len(sel)

    check()
    before = d.last_select()
    for case in ("n7", "t1_all"):
        km, pr = d.pairs(PREFIX, **pc.expected(case)[3])
        km.close()
        pr.close()
    assert d.last_select() == before
    host = d.to_host()
    assert int(host["eligible"].sum()) == sum(1 for r in recs if r["eligible"])
    check()


def test_an_unscored_design_and_a_bad_rule_are_bad_arguments(designs):
    bed, pam, k, start, _ = pc.RECORD_SETS["sel"]
    d, rg = device_design(bed(), pam, k, start)
    with pytest.raises(api.GsError) as e:
        d.pairs("", 40)
    assert e.value.status == 1
    d.close()
    rg.close()
    scored = designs("sel", False)
    for bad in (dict(max_span=3, min_span=4), dict(max_span=40, cut_offset=21)):
        with pytest.raises(api.GsError) as e:
            scored.pairs("", **bad)
        assert e.value.status == 1


def test_a_design_with_no_pair_gives_two_empty_objects(designs):
    d = designs("sel", False)
    km, pr = d.pairs(PREFIX, 0, min_span=0, cut_offset=3)   # no equal cuts at this offset
    assert pm.pairs(pc.records("sel", False)[1], 20, 3, 0, min_span=0) == []
    assert km.n == 0 and pr.to_host()["n"] == 0 and pr.rows(km).decode() == pm.HEADER
    assert pr.last()["counted"] == 0 and pr.last()["chunks"] == 0
    km.close()
    pr.close()
