"""Guide pairs for regions without a GPU: the host run of the device passes (gs_debug_pairs_host, through
csrc/gs_pairs_scan.h) against tests/pairs_model.py on every case of tests/pairs_cases.py - arrays equal, floats bit for
bit - the argument refusals, and the header's stand-alone check under the sanitizers."""
import ctypes as C
import shutil
import subprocess
from importlib import import_module

import numpy as np
import pytest

import oracle_lib as ol
import pairs_cases as pc
import pairs_model as pm

api = import_module("guidescan-cli_amd.api")


def columns(recs):
    return ([r["group"] for r in recs], [r["chr"] for r in recs], [r["pos"] for r in recs], [ord(r["sense"]) for r in recs],
            [r["spec"] for r in recs], [r["eligible"] for r in recs])


def assert_same_pairs(got, want):
    assert got["n"] == want["n"]
    for name in ("group", "chr", "a", "b", "cut_a", "cut_b", "spec_a", "spec_b"):
        assert got[name].dtype == want[name].dtype, name
        assert np.array_equal(got[name].view(np.uint32), want[name].view(np.uint32)), name


def test_the_cases_decide_something():
    pc.assert_cases_decide()
    for case in pc.CHUNK_CASES:
        pc.chunk_sizes(case)


@pytest.mark.parametrize("case", pc.CASE_IDS)
def test_host_passes_against_the_model(case):
    groups, recs, kept, rule = pc.expected(case)
    _, _, pam, k, _, _ = pc.shape(case)
    got, last = api.pairs_host(*columns(recs), k, len(pam), len(groups), **rule)
    assert_same_pairs(got, pm.arrays(recs, kept, k, len(pam), rule.get("cut_offset", 3), rule.get("start", False)))
    assert last == pm.last(recs, kept, k, len(pam), n_groups=len(groups), **rule)


@pytest.mark.parametrize("case", pc.CHUNK_CASES)
def test_chunks_of_whole_groups_on_the_host(case):
    groups, recs, kept, rule = pc.expected(case)
    _, _, pam, k, _, _ = pc.shape(case)
    exact, below, _, _, n_chunks = pc.chunk_sizes(case)
    one, _ = api.pairs_host(*columns(recs), k, len(pam), len(groups), **rule)
    default = api.pairs_chunk()
    try:
        assert api.pairs_chunk(exact) == exact
        got, last = api.pairs_host(*columns(recs), k, len(pam), len(groups), **rule)
        assert_same_pairs(got, one)
        assert last["chunks"] == n_chunks >= 3
        api.pairs_chunk(below)
        with pytest.raises(api.GsError) as e:
            api.pairs_host(*columns(recs), k, len(pam), len(groups), **rule)
        assert e.value.status == 3
    finally:
        api.pairs_chunk(default)
    assert api.pairs_chunk() == default == 1 << 26


def test_no_records_and_no_pairs_are_not_errors():
    got, last = api.pairs_host([], [], [], [], [], [], 20, 3, 4, max_span=40)
    assert got["n"] == 0 and last == dict(eligible=0, counted=0, kept=0, chunks=0, groups_without=4, groups_short=0)
    got, last = api.pairs_host([0, 1], [0, 0], [10, 12], [43, 45], [1.0, 1.0], [1, 1], 20, 3, 2, max_span=40)
    assert got["n"] == 0 and last["eligible"] == 2 and last["groups_without"] == 2


def test_argument_refusals():
    L = api.lib()
    cols = [np.array(x, dtype=dt) for x, dt in (([0, 0], np.uint32), ([0, 0], np.uint32), ([10, 30], np.uint32), ([43, 45], np.uint8),
                                                ([1.0, 0.5], np.float32), ([1, 1], np.uint8))]

    def status(k=20, **kw):
        rule = api.GsPairRule(kw.get("min_span", 1), kw.get("max_span", 40), kw.get("cut_offset", 3), kw.get("orientation", 0), 0, 0,
                              kw.get("min_specificity", -1.0), 0)
        h = C.c_void_p()
        rc = L.gs_debug_pairs_host(2, *[c.ctypes.data for c in cols], k, 3, 1, C.byref(rule), C.byref(h))
        if rc == 0:
            L.gs_pairs_free(h)
        return rc

    assert status() == 0
    assert status(min_span=41) == 1
    assert status(cut_offset=21) == 1 and status(cut_offset=20) == 0 and status(k=23, cut_offset=23) == 0
    assert status(orientation=3) == 1 and status(orientation=2) == 0
    assert status(min_specificity=float("nan")) == 1 and status(min_specificity=1.5) == 1 and status(min_specificity=1.0) == 0
    h = C.c_void_p()
    assert L.gs_debug_pairs_host(2, *[c.ctypes.data for c in cols], 20, 3, 1, None, C.byref(h)) == 1
    assert L.gs_design_pairs(None, b"", None, None, None, None) == 1
    assert L.gs_pairs_get(None, None, None, None, None, None, None, None, None, None) == 1
    assert L.gs_pairs_last(None, None) == 1 and L.gs_pairs_rows(None, None, None, None) == 1
    with pytest.raises(ValueError):
        api.pairs_host(*[c.tolist() for c in cols], 20, 3, 1, max_span=40, orientation="sideways")


def test_pairs_check_is_clean_under_the_sanitizers():
    if shutil.which("g++") is None or shutil.which("make") is None:
        pytest.skip("no host compiler")
    r = subprocess.run(["make", "-C", str(ol.ROOT / "guidescan-cli_amd" / "csrc"), "pairs-check"], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "pairs under" in r.stdout
