"""Guides for regions without a GPU: the BED parser (gs_regions_parse) against tests/design_model.py on hand-written
files, the host run of the device stages (gs_debug_design_host, through csrc/gs_regions_scan.h) against the model for
membership, order, selection and id bytes, and the header's stand-alone check under the sanitizers."""
import shutil
import subprocess
from importlib import import_module

import numpy as np
import pytest

import design_cases as dc
import design_model as dm
import oracle_lib as ol

api = import_module("guidescan-cli_amd.api")

NAMES, LENS = ["chr1", "chrII", "a_rather_long_chromosome_name"], [1000, 500, 2000]
LONGEST = len(NAMES[2])
CAP = 254 - (1 + LONGEST + 1 + 10 + 2)   # the longest group name an id still fits with, no prefix

ACCEPTED = {
    "tabs": "chr1\t0\t100\tg1\nchrII\t10\t20\tg2\n",
    "blanks": "chr1 0 100 g1\nchrII   10  20   g2\n",
    "mixed": "chr1 \t0\t 100 g1\n",
    "three_columns": "chr1\t0\t100\nchr1\t200\t300\n",
    "crlf": "chr1\t0\t100\tg1\r\nchrII\t10\t20\r\n",
    "no_final_newline": "chr1\t0\t100\tg1",
    "comments": "# a comment\ntrack name=x\nbrowser position chr1:1-10\n\nchr1\t5\t50\tg\n\n",
    "extra_columns": "chr1\t0\t100\tg1\t0\t+\t0\t100\n",
    "first_appearance": "chrII\t0\t10\tzeta\nchr1\t0\t10\talpha\nchr1\t50\t60\tzeta\n",
    "several_chromosomes": "chr1\t0\t10\tg\nchrII\t0\t10\tg\na_rather_long_chromosome_name\t5\t9\tg\n",
    "overlap_merged": "chr1\t0\t100\tg\nchr1\t50\t150\tg\nchr1\t400\t500\tg\n",
    "abut_merged": "chr1\t0\t100\tg\nchr1\t100\t150\tg\n",
    "abut_other_group": "chr1\t0\t100\tg\nchr1\t100\t150\th\n",
    "nested": "chr1\t0\t900\ta\nchr1\t100\t800\tb\nchr1\t200\t700\tc\nchr1\t300\t600\ta\n",
    "unsorted": "chr1\t500\t600\tg\nchr1\t0\t100\tg\nchr1\t90\t510\tg\n",
    "end_at_length": "chr1\t999\t1000\tg\nchrII\t0\t500\th\n",
    "leading_zeros": "chr1\t007\t0100\tg\n",
    "name_at_cap": "chr1\t0\t10\t" + "n" * CAP + "\n",
    "same_name_as_default": "chr1\t0\t10\nchr1\t5\t20\tchr1:0-10\n",
    "skipped_track_prefix": "tracker\t0\t10\nchr1\t0\t10\n",
}
REFUSED = {
    "two_fields": ("chr1\t0\t100\nchr1\t5\n", "few", 2),
    "blank_only_line": ("chr1\t0\t100\n \t \nchr1\t5\t9\n", "few", 2),
    "negative_start": ("chr1\t-1\t100\n", "integer", 1),
    "float_end": ("# c\nchr1\t1\t1e2\n", "integer", 2),
    "plus_sign": ("chr1\t+1\t100\n", "integer", 1),
    "nineteen_digits": ("chr1\t1\t1000000000000000000\n", "integer", 1),
    "start_equals_end": ("chr1\t0\t100\n\nchr1\t7\t7\n", "order", 3),
    "start_after_end": ("chr1\t9\t7\n", "order", 1),
    "beyond_length": ("chr1\t0\t1000\nchrII\t0\t501\n", "beyond", 2),
    "unknown_chromosome": ("chr1\t0\t1000\r\nchr3\t0\t10\r\n", "chromosome", 2),
    "comma_in_name": ("chr1\t0\t10\tgene,1\n", "comma", 1),
    "name_beyond_cap": ("chr1\t0\t10\tok\nchr1\t0\t10\t" + "n" * (CAP + 1) + "\n", "long", 2),
    "no_interval": ("# nothing\n\ntrack x\n", "empty", 0),
    "empty_file": ("", "empty", 0),
    "first_error_wins": ("chr1\t5\t5\nchr9\t0\t1\n", "order", 1),
}


@pytest.mark.parametrize("name", sorted(ACCEPTED))
def test_parser_accepts_what_the_model_accepts(name):
    raw = ACCEPTED[name].encode()
    groups, merged = dm.parse_bed(raw, NAMES, LENS)
    rg = api.Regions.parse(raw, (NAMES, LENS))
    assert rg.n_groups == len(groups)
    assert rg.n_intervals == sum(len(v) for v in merged.values())
    # membership of a one-base footprint (k = 1, P = 1 makes two) at every position, through the shared header
    parts = []
    for c, ln in enumerate(LENS):
        pos = np.arange(1, ln, dtype=np.uint32)
        parts.append((c, np.full((pos.size, 1), ord("A"), np.uint8), pos, np.full(pos.size, ord("+"), np.uint8), None, None))
    got = api.design_host_model(rg, parts, "N", 1)
    want = []
    for g in range(len(groups)):
        for c in range(len(LENS)):
            for p in range(1, LENS[c]):
                if any(s <= p - 1 and p + 1 <= e for s, e in merged.get((g, c), ())):
                    want.append(f"{groups[g]}:{NAMES[c]}:{p}:+")
    assert got["ids"] == "".join(want).encode()
    assert got["n"] == len(want)
    rg.close()


@pytest.mark.parametrize("name", sorted(REFUSED))
def test_parser_refuses_with_the_line_and_the_reason(name):
    text, kind, line = REFUSED[name]
    with pytest.raises(dm.BedError) as me:
        dm.parse_bed(text.encode(), NAMES, LENS)
    assert (me.value.kind, me.value.line) == (kind, line)
    with pytest.raises(api.RegionsFileError) as e:
        api.Regions.parse(text.encode(), (NAMES, LENS))
    assert e.value.status == 6
    assert (e.value.kind, e.value.line) == (dm.KINDS[kind], line)
    assert e.value.message == me.value.message


def test_the_cap_counts_the_prefix():
    raw = ("chr1\t0\t10\t" + "n" * CAP + "\n").encode()
    api.Regions.parse(raw, (NAMES, LENS)).close()
    with pytest.raises(api.RegionsFileError) as e:
        api.Regions.parse(raw, (NAMES, LENS), prefix="p")
    assert e.value.kind == dm.KINDS["long"] and e.value.line == 1
    with pytest.raises(dm.BedError):
        dm.parse_bed(raw, NAMES, LENS, prefix="p")


def test_a_regions_file_is_read_by_name(tmp_path):
    p = tmp_path / "r.bed"
    p.write_text(ACCEPTED["nested"])
    rg = api.Regions.parse(p, (NAMES, LENS))
    assert (rg.n_groups, rg.n_intervals) == (3, 3)
    with pytest.raises(api.GsError) as e:
        api.Regions.parse(tmp_path / "missing.bed", (NAMES, LENS))
    assert e.value.status == 5


# ---- the stages on the host against the model --------------------------------------------------------------------

def host_run(bed, pam="NGG", k=20, start=False, scores=None, prefix="", per_region=None, min_specificity=None, rows=False):
    """gs_debug_design_host on the toy genome's candidates; scores: {seq: (spec, eligible)} of the model"""
    _, names, lengths, _ = dc.genome()
    rg = api.Regions.parse(bed.encode(), (names, lengths), prefix=prefix)
    parts = []
    for c, cand in enumerate(dc.candidates(pam, k, start)):
        seqs = np.frombuffer("".join(s for s, _, _ in cand).encode(), dtype=np.uint8).reshape(len(cand), k)
        pos = np.array([p for _, p, _ in cand], dtype=np.uint32)
        sense = np.frombuffer("".join(s for _, _, s in cand).encode(), dtype=np.uint8)
        spec = elig = None
        if scores is not None:
            spec = np.array([scores.get(s, (0.0, True))[0] for s, _, _ in cand], dtype=np.float32)
            elig = np.array([scores.get(s, (0.0, True))[1] for s, _, _ in cand], dtype=np.uint8)
        parts.append((c, seqs, pos, sense, spec, elig))
    return api.design_host_model(rg, parts, pam, k, prefix, per_region, min_specificity, rows=rows)


def assert_same(got, want):
    assert got["ids"] == want["ids"]
    assert np.array_equal(got["id_off"], want["id_off"])
    assert got["seqs"] == want["seqs"] and got["pams"] == want["pams"]
    assert np.array_equal(got["pos"], want["pos"])
    assert np.array_equal(got["sense"], want["sense"]) and np.array_equal(got["sense_chars"], want["sense_chars"])


SHAPES = [("NGG", 20, False), ("NGG", 20, True), ("TTTN", 23, True), ("TTTN", 20, False), ("NGG", 23, False)]


@pytest.mark.parametrize("pam,k,start", SHAPES, ids=lambda v: str(v))
def test_membership_and_order_on_the_host(pam, k, start):
    _, names, lengths, _ = dc.genome()
    for name, bed in dc.membership_beds(pam, k, start).items():
        groups, recs = dc.model_records(bed, pam, k, start)
        sel = dm.select(recs)
        assert_same(host_run(bed, pam, k, start, prefix="x_"), dm.arrays(sel, groups, names, pam, "x_"))
        by_group = {g: sum(1 for r in sel if groups[r["group"]] == g) for g in groups}
        if name == "exact":
            assert by_group["exact_plus"] >= 1 and by_group["exact_minus"] >= 1
            assert by_group["short_plus"] == 0 and by_group["short_minus"] == 0
            assert {r["sense"] for r in sel} == {"+", "-"}
        if name == "whole":
            assert len(sel) == len(dc.candidates(pam, k, start)[1])
        if name == "abut_one_group":
            one = len(sel)
        if name == "abut_two_groups":
            assert len(sel) < one   # the sites across the seam are in neither group
        if name == "nested":
            assert max(sum(1 for r in recs if (r["chr"], r["pos"], r["sense"]) == key) for key in
                       {(r["chr"], r["pos"], r["sense"]) for r in recs}) == 3
        if name.startswith("count"):
            assert len(sel) == int(name[5:])
        if name == "none":
            assert len(sel) == 0


@pytest.fixture(scope="module")
def scored():
    """the selection BED's records with the model's specificity and eligibility under -t 1"""
    text, names, lengths, _ = dc.genome()
    oidx = ol.OracleIndex(text)
    groups, recs = dc.model_records(dc.selection_bed())
    dm.score(recs, oidx, lengths, "NGG", mismatches=dc.MISMATCHES, threshold=1)
    oidx.close()
    return groups, recs


def tie_across(groups, recs):
    """(N, group) such that the model's order of the group has equal specificities at places N and N + 1"""
    for g in range(len(groups)):
        order = dm.select([dict(r, eligible=True) for r in recs if r["group"] == g], per_region=10 ** 9)
        for n in range(1, len(order)):
            if order[n - 1]["spec"] == order[n]["spec"]:
                return n, g
    return None


def closing_up(recs):
    """N at which -t 1 changes the first N of some group: a record made ineligible, ranks closing up behind it"""
    for n in range(1, 40):
        # the first N of every group as if all were eligible, with the true eligibility kept on the records
        first_n = dm.select([dict(r, eligible=True, dropped=not r["eligible"]) for r in recs], per_region=n)
        kept = dm.select(recs, per_region=n)
        if any(r["dropped"] for r in first_n) and len(kept) == len(first_n):
            return n   # a dropped record stood among the first N, and its group still fills N: another moved up
    return None


def selection_cases(groups, recs):
    """(name, records as the case sees them, per_region, min_specificity)"""
    open_recs = [dict(r, eligible=True) for r in recs]
    n_tie, _ = tie_across(groups, recs)
    small = sum(1 for r in recs if groups[r["group"]] == "small")
    return [("all", open_recs, None, None), ("one", open_recs, 1, None), ("tie", open_recs, n_tie, None),
            ("more_than_the_small_group_has", open_recs, small + 3, None), ("split", open_recs, None, 0.75),
            ("split_and_cut", open_recs, 3, 0.75), ("threshold", recs, closing_up(recs), None), ("threshold_all", recs, None, None)]


def test_the_selection_cases_decide_something(scored):
    groups, recs = scored
    assert tie_across(groups, recs) is not None
    dup = [r for r in recs if groups[r["group"]] == "dup"]
    assert any(r["spec"] >= np.float32(0.75) for r in dup) and any(r["spec"] < np.float32(0.75) for r in dup)
    assert any(not r["eligible"] for r in dup) and any(r["eligible"] for r in dup)
    # ranks close up behind a record made ineligible: the N-th kept record differs with and without -t
    assert closing_up(recs) is not None
    small = sum(1 for r in recs if groups[r["group"]] == "small")
    assert 0 < small


def assert_cases_decide(groups, recs):
    """what the selection cases lean on, asserted next to every run of them: S = 0.75 and S = 0.6 split the group of
    the planted copies, -t 1 drops some of it, a tie stands across an N-th place, and ranks close up behind a drop"""
    dup = [r for r in recs if groups[r["group"]] == "dup"]
    for s in (0.75, 0.6):
        assert any(r["spec"] >= np.float32(s) for r in dup) and any(r["spec"] < np.float32(s) for r in dup)
    assert any(not r["eligible"] for r in dup) and any(r["eligible"] for r in dup)
    assert tie_across(groups, recs) is not None and closing_up(recs) is not None


def test_selection_on_the_host(scored):
    groups, recs = scored
    _, names, _, _ = dc.genome()
    assert_cases_decide(groups, recs)
    for name, rs, n, s in selection_cases(groups, recs):
        scores = {r["seq"]: (r["spec"], r["eligible"]) for r in rs}
        sel = dm.select(rs, per_region=n, min_specificity=s)
        got = host_run(dc.selection_bed(), scores=scores, prefix="d:", per_region=n, min_specificity=s, rows=True)
        assert_same(got, dm.arrays(sel, groups, names, "NGG", "d:"))
        assert got["rows"].decode() == dm.rows(sel, groups, names, "NGG", "d:"), name


def test_group_boundaries_on_workgroup_edges_on_the_host():
    _, names, _, _ = dc.genome()
    for name, bed in dc.edge_beds().items():
        groups, recs = dc.model_records(bed)
        sel = dm.select(recs)
        firsts = [next(i for i, r in enumerate(sel) if r["group"] == g) for g in range(len(groups))]
        assert firsts[1] == (256 if name == "begins_at_256" else 250)
        if name == "spans_250_520":
            assert firsts[2] == 521
        assert_same(host_run(bed), dm.arrays(sel, groups, names, "NGG"))


def test_ranks_across_workgroup_edges_on_the_host():
    """the edge BEDs ranked and cut: a group that begins at record 256 and one that spans records 250-520, with N smaller
    than the groups, a specificity bound and records made ineligible, so that a group's ranks start from its head's"""
    text, names, _, _ = dc.genome()
    oidx = ol.OracleIndex(text)
    scored_edges = dc.edge_scored(oidx)
    oidx.close()
    for name, (groups, recs) in scored_edges.items():
        for n, s, thr in dc.EDGE_SELECTIONS:
            rs = recs if thr else [dict(r, eligible=True) for r in recs]
            scores = {r["seq"]: (r["spec"], r["eligible"]) for r in rs}
            sel = dm.select(rs, per_region=n, min_specificity=s)
            got = host_run(dc.edge_beds()[name], scores=scores, per_region=n, min_specificity=s)
            assert_same(got, dm.arrays(sel, groups, names, "NGG"))


def test_a_selection_needs_scores_and_sane_arguments():
    _, names, lengths, _ = dc.genome()
    with pytest.raises(api.GsError) as e:
        host_run(dc.selection_bed(), per_region=2)
    assert e.value.status == 1
    with pytest.raises(ValueError):
        host_run(dc.selection_bed(), min_specificity=1.5)
    L = api.lib()
    assert L.gs_design_select(None, b"", 0, -1.0, None, None) == 1
    assert L.gs_design_score(None, None, None, 0, 3, 0, -1, 0, None) == 1
    assert L.gs_design_restrict(None, 0, None, None, None) == 1
    assert L.gs_design_concat(None, 0, None) == 1


def test_regions_check_is_clean_under_the_sanitizers():
    if shutil.which("g++") is None or shutil.which("make") is None:
        pytest.skip("no host compiler")
    r = subprocess.run(["make", "-C", str(ol.ROOT / "guidescan-cli_amd" / "csrc"), "regions-check"], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "membership queries" in r.stdout
