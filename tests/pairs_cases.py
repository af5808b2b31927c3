"""The record sets and rules that tests/test_pairs_model.py (host, no GPU), tests/test_gpu_pairs.py and
tests/test_cli_pairs_gpu.py run against tests/pairs_model.py, on the toy genome of tests/design_cases.py.  Everything is
derived from the model's own candidate list, and every case asserts that it decides something."""
from functools import lru_cache

import numpy as np

import design_cases as dc
import design_model as dm
import oracle_lib as ol
import pairs_model as pm


def pairs_bed():
    """the selection BED, a group that holds one candidate, and a group inside the family planted with one mismatch in
    every 20-mer: every record of it is dropped by -t 1"""
    _, names, _, _ = dc.genome()
    s, e = dc.NEAR[0][0], dc.NEAR[0][1]
    return dc.selection_bed() + f"{names[1]}\t{dc.trimmed(1, 1)}\tsingle\n{names[0]}\t{s}\t{e}\tdropped\n"


# name -> (BED, pam, k, start, mismatches of the score phase)
RECORD_SETS = {
    "sel": (pairs_bed, "NGG", 20, False, dc.MISMATCHES),
    "tttn": (dc.selection_bed, "TTTN", 23, True, dc.MISMATCHES),
    "begins_at_256": (lambda: dc.edge_beds()["begins_at_256"], "NGG", 20, False, dc.EDGE_MISMATCHES),
    "spans_250_520": (lambda: dc.edge_beds()["spans_250_520"], "NGG", 20, False, dc.EDGE_MISMATCHES),
}


@lru_cache(maxsize=None)
def scored(name):
    """-> (groups, records with the model's spec and eligibility under -t 1) of a record set"""
    bed, pam, k, start, mismatches = RECORD_SETS[name]
    text, _, lengths, _ = dc.genome()
    groups, recs = dc.model_records(bed(), pam, k, start)
    oidx = ol.OracleIndex(text)
    try:
        dm.score(recs, oidx, lengths, pam, mismatches=mismatches, start=start, threshold=1)
    finally:
        oidx.close()
    return groups, recs


def records(name, thr):
    """the set as a case sees it: with the eligibility of -t 1, or every record eligible"""
    groups, recs = scored(name)
    return groups, (recs if thr else [dict(r, eligible=True) for r in recs])


# (case, record set, with the eligibility of -t 1, the rule)
CASES = [
    ("any_1_40", "sel", False, dict(max_span=40)),
    ("out_1_40", "sel", False, dict(max_span=40, orientation="pam-out")),
    ("in_1_40", "sel", False, dict(max_span=40, orientation="pam-in")),
    ("equal_cuts", "sel", False, dict(max_span=0, min_span=0, cut_offset=0)),
    ("mid", "sel", False, dict(max_span=400, min_span=100)),
    ("wide", "sel", False, dict(max_span=10 ** 7)),
    ("near_2_63", "sel", False, dict(max_span=2 ** 63 - 1, min_span=0, orientation="pam-out")),
    ("offset_0", "sel", False, dict(max_span=40, cut_offset=0)),
    ("offset_k", "sel", False, dict(max_span=40, cut_offset=20)),
    ("n1", "sel", False, dict(max_span=400, per_region=1)),
    ("n7", "sel", False, dict(max_span=40, per_region=7)),
    ("n_beyond", "sel", False, dict(max_span=40, per_region=10 ** 6)),
    ("out_mid_n7", "sel", False, dict(max_span=400, min_span=100, orientation="pam-out", per_region=7)),
    ("s75", "sel", False, dict(max_span=400, per_region=7, min_specificity=0.75)),
    ("s75_t1", "sel", True, dict(max_span=400, per_region=100, min_specificity=0.5)),
    ("t1_all", "sel", True, dict(max_span=40)),
    ("tttn_any", "tttn", False, dict(max_span=40, start=True)),
    ("tttn_out", "tttn", False, dict(max_span=40, start=True, orientation="pam-out")),
    ("tttn_in", "tttn", False, dict(max_span=40, start=True, orientation="pam-in", per_region=7)),
    ("tttn_offset_k", "tttn", True, dict(max_span=40, start=True, cut_offset=23, min_specificity=0.5)),
    ("edge_a_wide", "begins_at_256", False, dict(max_span=10 ** 7)),
    ("edge_a_equal_cuts", "begins_at_256", False, dict(max_span=0, min_span=0)),
    ("edge_a_n7", "begins_at_256", False, dict(max_span=400, per_region=7)),
    ("edge_a_s75_t1", "begins_at_256", True, dict(max_span=400, per_region=100, min_specificity=0.75)),
    ("edge_b_wide", "spans_250_520", False, dict(max_span=10 ** 7)),
    ("edge_b_wide_out", "spans_250_520", False, dict(max_span=10 ** 7, orientation="pam-out", per_region=7)),
    ("edge_b_n1_s75", "spans_250_520", False, dict(max_span=400, per_region=1, min_specificity=0.75)),
    ("edge_b_t1", "spans_250_520", True, dict(max_span=40, min_span=0, orientation="pam-in")),
]
CASE_IDS = [c[0] for c in CASES]


@lru_cache(maxsize=None)
def expected(case):
    """-> (groups, records, kept pairs as indices into the records, the rule) of a case, by the model"""
    _, name, thr, rule = next(c for c in CASES if c[0] == case)
    _, pam, k, _, _ = RECORD_SETS[name]
    groups, recs = records(name, thr)
    return groups, recs, pm.pairs(recs, k, len(pam), **rule), rule


def shape(case):
    """-> (record set, with -t 1, pam, k, start, mismatches)"""
    _, name, thr, _ = next(c for c in CASES if c[0] == case)
    _, pam, k, start, mismatches = RECORD_SETS[name]
    return name, thr, pam, k, start, mismatches


def pair_set(case):
    groups, recs, kept, _ = expected(case)
    return set(kept)


def partners(case):
    """per record index: how many kept pairs it leads as a"""
    _, recs, kept, _ = expected(case)
    led = [0] * len(recs)
    for a, _ in kept:
        led[a] += 1
    return led


def assert_cases_decide():
    """what the cases lean on, asserted next to every run of them"""
    groups, recs = scored("sel")
    by_name = {g: [r for r in recs if groups[r["group"]] == g] for g in groups}
    assert len(by_name["single"]) == 1
    assert by_name["dropped"] and not any(r["eligible"] for r in by_name["dropped"])
    assert len({r["chr"] for r in by_name["dup"]}) == 2
    # no pair across the two chromosomes of `dup`, though the rule's span would take any two records of it
    g, rs, kept, _ = expected("wide")
    assert kept and all(rs[a]["chr"] == rs[b]["chr"] for a, b in kept)
    assert not any(groups[rs[a]["group"]] == "single" for a, _ in kept)
    # the three orientations differ, and the oriented ones together are a proper part of `any`
    any_, out, in_ = pair_set("any_1_40"), pair_set("out_1_40"), pair_set("in_1_40")
    assert out and in_ and out != in_ and not (out & in_) and (out | in_) < any_
    # equal cuts: pairs exist, each once
    for case in ("equal_cuts", "edge_a_equal_cuts"):
        zero = expected(case)[2]
        assert zero and len(set(zero)) == len(zero) and not {(b, a) for a, b in zero} & set(zero), case
    assert expected("mid")[2] and pair_set("offset_0") != any_ and pair_set("offset_k") != any_ and pair_set("offset_0") != pair_set("offset_k")
    assert expected("near_2_63")[2]
    # ties in the smaller specificity are broken by the larger one, then by place: both occur among the ranked pairs
    ranked = expected("any_1_40")
    words = [(ranked[1][a]["group"], min(ranked[1][a]["spec"], ranked[1][b]["spec"]), max(ranked[1][a]["spec"], ranked[1][b]["spec"]))
             for a, b in ranked[2]]
    assert any(x[:2] == y[:2] and x[2] != y[2] for x, y in zip(words, words[1:]))
    assert any(x == y for x, y in zip(words, words[1:]))
    # every N cuts a group that has more; N beyond the largest group cuts nothing
    for case in ("n1", "n7", "out_mid_n7", "s75", "s75_t1", "tttn_in", "edge_a_n7", "edge_a_s75_t1", "edge_b_wide_out", "edge_b_n1_s75"):
        _, rs, kept, rule = expected(case)
        _, pam, k, _, _ = RECORD_SETS[shape(case)[0]]
        by = pm.counted(rs, k, len(pam), **rule)
        assert kept and any(c > rule["per_region"] for c in by.values()), case
    _, rs, kept, rule = expected("n_beyond")
    assert set(kept) == any_ and max(pm.counted(rs, 20, 3, **rule).values()) < rule["per_region"]
    # the bound and -t 1 each change the result
    assert pm.pairs(records("sel", False)[1], 20, 3, **expected("s75_t1")[3]) != expected("s75_t1")[2] and pair_set("t1_all") < any_
    base = dict(expected("s75")[3], min_specificity=None)
    assert pm.pairs(records("sel", False)[1], 20, 3, **base) != expected("s75")[2]
    # the other shape: both PAM sides pair up under --start
    assert pair_set("tttn_out") and pair_set("tttn_any") > pair_set("tttn_out") and expected("tttn_in")[2] and expected("tttn_offset_k")[2]
    # a record with more than 256 partners and, in its group, an eligible record with none; runs of one (group,
    # chromosome) that begin at record 256 and span records 250-520
    for case in ("edge_b_wide",):
        _, rs, kept, _ = expected(case)
        led = partners(case)
        a = int(np.argmax(led))
        assert led[a] > 256 and any(led[i] == 0 and r["group"] == rs[a]["group"] for i, r in enumerate(rs)), case
    assert expected("edge_a_wide")[2] and expected("edge_b_wide_out")[2] and expected("edge_b_t1")[2] and expected("edge_a_s75_t1")[2] and expected("edge_b_n1_s75")[2]


def chunk_plan(counts, chunk):
    """the groups dealt greedily into chunks of whole groups of at most `chunk` pairs -> the pairs of each chunk"""
    out, acc = [], 0
    for c in counts:
        if acc + c > chunk:
            out.append(acc)
            acc = 0
        acc += c
    if acc:
        out.append(acc)
    return out


CHUNK_CASES = ("any_1_40", "n7", "out_1_40")


def chunk_sizes(case):
    """-> (a chunk the largest group fills exactly, a chunk below it, the largest group's name and pair count); asserts
    at least three chunks, one of them full and followed by another"""
    groups, recs, _, rule = expected(case)
    _, pam, k, _, _ = RECORD_SETS[shape(case)[0]]
    by = pm.counted(recs, k, len(pam), **rule)
    counts = [by.get(g, 0) for g in range(len(groups))]
    most = max(counts)
    plan = chunk_plan(counts, most)
    assert len(plan) >= 3 and most in plan[:-1], (case, counts, plan)
    return most, most - 1, groups[counts.index(most)], most, len(plan)
