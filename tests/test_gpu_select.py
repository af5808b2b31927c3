"""Library selection on the GPU: gs_kmers_filter (k_km_rule, the 64-bit scan, k_km_keep of csrc/gs_kmers.hip) byte for byte
against tests/select_model.py, and the spaced selection (k_ds_bounds, k_ds_space of csrc/gs_design.hip) driven through
Design.set_scores against the model and the host twin: ids, order, last_select and last_spacing.  The cases are those of
tests/test_select_model.py plus the ones that lie on the edges of the kernels' steps."""
from importlib import import_module

import numpy as np
import pytest

import design_cases as dc
import design_model as dm
import oracle_lib as ol
import pairs_model as pm
import select_model as sl
from test_design_model import assert_same
from test_gpu_design import device_design, selected
from test_select_model import K, P, RULES, api_rule, candidate_parts, chain_of, scores_of, spread_scores

api = import_module("guidescan-cli_amd.api")
kmers = import_module("guidescan-cli_amd.kmers")

pytestmark = pytest.mark.gpu


# ---- the sequence rules ----------------------------------------------------------------------------------------------

def check_filter(chrm, kw, pam="NGG", k=K, start=False):
    """one scan through the rule on the device against the model -> the filtered DeviceKmers"""
    cands = kmers.find_all_kmers(chrm, pam, k, start)
    kept, counts, _ = sl.filter_candidates(cands, **kw)
    km = api.generate_kmers(chrm, pam, k, start)
    assert km.n == len(cands)
    f = km.filter(api_rule(**kw))
    km.close()
    assert f.n == len(kept) and f.filter_counts == counts
    seqs, pams, pos, sense = f.to_host()
    assert seqs.tobytes() == "".join(c[0] for c in kept).encode() and pams.tobytes() == (pam * len(kept)).encode()
    assert pos.tolist() == [c[1] for c in kept] and sense.tobytes() == "".join(c[2] for c in kept).encode()
    return f, kept


@pytest.mark.parametrize("name", sorted(RULES))
def test_filter_on_whole_chromosomes(name):
    kw, passing = RULES[name]
    total = 0
    for _, chrm in dc.genome()[3]:
        f, kept = check_filter(chrm, kw)
        total += len(kept)
        f.close()
    if passing is not None:
        assert total == passing


def prefix_with(n, pam="NGG", k=K):
    """a prefix of a chromosome whose scan gives exactly n candidates"""
    for c, chrm in dc.genome()[3]:
        ends = sorted(pos - 1 + k + len(pam) for _, pos, _ in dc.candidates(pam, k)[c])
        if len(ends) > n and ends[n] > ends[n - 1]:
            piece = chrm[:ends[n - 1]]
            if len(kmers.find_all_kmers(piece, pam, k, False)) == n:
                return piece
    raise AssertionError(f"no prefix with {n} candidates")


@pytest.mark.parametrize("n", [63, 64, 65, 255, 256, 257])
def test_filter_on_workgroup_edges(n):
    piece = prefix_with(n)
    for name in ("all", "gc", "tttt"):
        f, kept = check_filter(piece, RULES[name][0])
        assert 0 < len(kept) < n
        f.close()
    # the last candidate decides too: kept by one rule and dropped by another
    last = kmers.find_all_kmers(piece, "NGG", K, False)[-1][0]
    for kw in (dict(exclude_motifs=(last,)), dict(exclude_motifs=(last[:-1] + ("A" if last[-1] != "A" else "C"),))):
        check_filter(piece, kw)[0].close()


def test_nothing_kept_everything_kept_and_the_ids_behind_the_filter():
    _, names, _, chromosomes = dc.genome()
    chrm = chromosomes[1][1]
    none, kept = check_filter(chrm, RULES["n"][0])
    assert none.n == 0 and none.csv("p_", names[1]) == b""
    none.encode_ids("p_", names[1])
    assert none.ids_to_host()[0] == b""
    none.close()
    everything, kept = check_filter(chrm, RULES["gc_open"][0])
    assert everything.n == len(dc.candidates()[1])
    everything.close()
    some, kept = check_filter(chrm, RULES["all"][0])
    rows = "".join(f"p_{names[1]}:{p}:{s},{q},NGG,{names[1]},{p},{s}\n" for q, p, s in kept)
    assert some.csv("p_", names[1]).decode() == rows
    some.encode_ids("p_", names[1])
    ids, off, sp = some.ids_to_host()
    assert ids.decode() == "".join(f"p_{names[1]}:{p}:{s}" for _, p, s in kept) and len(off) == len(kept) + 1
    assert sp.tolist() == [int(s == "+") for _, _, s in kept]
    with pytest.raises(api.GsError) as e:
        some.filter(api_rule(max_run=3))   # the object has ids now
    assert e.value.status == 1
    again = api.generate_kmers(chrm, "NGG", K)
    twice = again.filter(api_rule(gc=(40, 70))).filter(api_rule(max_run=3))   # a filtered object is a scan's: it filters again
    assert twice.n == len(sl.filter_candidates(dc.candidates()[1], gc=(40, 70), max_run=3)[0])
    for x in (some, again, twice):
        x.close()


@pytest.mark.parametrize("pam,k,start", [("NGG", 20, True), ("TTTN", 23, True), ("TTTN", 20, False)], ids=lambda v: str(v))
def test_filter_sees_the_guide_orientation(pam, k, start):
    for _, chrm in dc.genome()[3][:2]:
        check_filter(chrm, RULES["all"][0], pam, k, start)[0].close()


# ---- spacing -----------------------------------------------------------------------------------------------------------

def check_gpu_spaced(bed, recs, groups, n, d, cut_offset=3, start=False, min_specificity=None, decides=True):
    """k_ds_space through Design.set_scores against the model and the host twin -> the model's selection"""
    _, names, lengths, _ = dc.genome()
    sel, spacing = sl.select_spaced(recs, n, d, K, P, cut_offset, start, min_specificity)
    design, rg = device_design(bed, start=start)
    host = design.to_host()
    assert host["n"] == len(recs)
    by = scores_of(recs)
    sc = [by[(int(c), int(p), chr(s))] for c, p, s in zip(host["chr"], host["pos"], host["sense"])]
    design.set_scores(np.array([x[0] for x in sc], np.float32), np.array([x[1] for x in sc], np.uint8))
    assert design.info() == (len(recs), True)
    design.set_spacing(d, cut_offset, start)
    km = design.select("", n, min_specificity)
    want = dm.arrays(sel, groups, names, "NGG")
    assert_same(selected(km), want)
    km.close()
    assert design.last_select() == sl.last_select(recs, sel, len(groups), n)
    assert design.last_spacing() == spacing
    assert design.rows("", n, min_specificity).decode() == dm.rows(sel, groups, names, "NGG")
    twin = api.design_host_model(rg, candidate_parts("NGG", K, start, by), "NGG", K, "", n, min_specificity, min_spacing=d,
                                 cut_offset=cut_offset, start=start)
    assert twin["ids"] == want["ids"] and twin["last_spacing"] == spacing
    # the rule taken off again: the selection as it was
    design.set_spacing(0)
    km = design.select("", n, min_specificity)
    unspaced = dm.select(recs, n, min_specificity)
    assert_same(selected(km), dm.arrays(unspaced, groups, names, "NGG"))
    km.close()
    if decides:
        assert dm.ids(sel, groups, names) != dm.ids(unspaced, groups, names)
    design.close()
    rg.close()
    return sel, spacing


@pytest.fixture(scope="module")
def selection():
    groups, recs = dc.model_records(dc.selection_bed())
    return groups, spread_scores(recs)


def test_spacing_on_the_selection_groups(selection):
    groups, recs = selection
    bed = dc.selection_bed()
    for n, d in ((3, 25), (5, 10), (40, 7)):
        check_gpu_spaced(bed, recs, groups, n, d)
    sel, spacing = check_gpu_spaced(bed, recs, groups, 5, 10000)          # one pick per chromosome
    assert [sum(1 for r in sel if r["group"] == g) for g in range(len(groups))] == [2, 1, 1, 1]
    check_gpu_spaced(bed, recs, groups, 3, 25, min_specificity=0.75)       # below S: neither counts nor blocks
    check_gpu_spaced(bed, recs, groups, 3, 15, cut_offset=0)


def test_chain_ties_and_ineligible_records(selection):
    groups, recs = selection
    bed = dc.selection_bed()
    g, d = groups.index("big"), 25
    a, b, c = chain_of(recs, g, d)
    rs = [dict(r, spec=np.float32(0.1), eligible=True) for r in recs]
    for r in rs:
        for x, s in ((a, 1.0), (b, 0.9), (c, 0.8)):
            if (r["group"], r["chr"], r["pos"], r["sense"]) == (x["group"], x["chr"], x["pos"], x["sense"]):
                r["spec"] = np.float32(s)
    sel, _ = check_gpu_spaced(bed, rs, groups, 2, d)
    assert [(r["pos"], r["sense"]) for r in sel if r["group"] == g] == [(a["pos"], a["sense"]), (c["pos"], c["sense"])]
    flat_recs = [dict(r, spec=np.float32(0.5), eligible=True) for r in recs]
    check_gpu_spaced(bed, flat_recs, groups, 4, 12)                         # ties: position, then sense
    best = {g: dm.select([r for r in flat_recs if r["group"] == g], 1)[0] for g in range(len(groups))}
    check_gpu_spaced(bed, [dict(r, eligible=r is not best[r["group"]]) for r in flat_recs], groups, 4, 12)
    # N reached exactly on the last record of a group, and one more than the group can give
    found = None
    for d in range(2, 40):
        walk = sl.select_spaced(flat_recs, 1024, d, K, P)[0]
        for g in range(len(groups)):
            order = dm.select([r for r in flat_recs if r["group"] == g], 1024)
            picks = [r for r in walk if r["group"] == g]
            if picks[-1] is order[-1] and len(picks) < len(order) and found is None:
                found = (d, len(picks))
    assert found is not None
    check_gpu_spaced(bed, flat_recs, groups, found[1], found[0])
    _, more = check_gpu_spaced(bed, flat_recs, groups, found[1] + 1, found[0])
    assert more["groups_short_for_spacing"] >= 1


def test_a_plus_and_a_minus_record_with_one_cut(selection):
    """at the default cut offset the fixture has no such records (the host test makes them up); with the cut at the PAM's
    edge it has, and at D = 1 only an equal cut on the same chromosome conflicts"""
    groups, recs = selection
    twins = [(a, b) for a in recs for b in recs if (a["group"], a["chr"], a["sense"], b["sense"]) == (b["group"], b["chr"], "+", "-") and
             pm.cut(a, K, P, 0, False) == pm.cut(b, K, P, 0, False)]
    assert twins and not any(pm.cut(a, K, P, 3, False) == pm.cut(b, K, P, 3, False) for a in recs for b in recs
                             if a is not b and (a["group"], a["chr"]) == (b["group"], b["chr"]))
    sel, spacing = check_gpu_spaced(dc.selection_bed(), recs, groups, 40, 1, cut_offset=0)
    assert 0 < spacing["passed_over"] <= len(twins)
    assert not any(a in sel and b in sel for a, b in twins if a["eligible"] and b["eligible"])


def test_start_moves_the_cut(selection):
    groups, recs = dc.model_records(dc.selection_bed(), "NGG", K, True)
    spread_scores(recs, seed=11)
    deciding = [d for d in range(5, 40) if dm.ids(sl.select_spaced(recs, 3, d, K, P, 3, True)[0], groups, ["a", "b", "c"]) !=
                dm.ids(sl.select_spaced(recs, 3, d, K, P, 3, False)[0], groups, ["a", "b", "c"])]
    check_gpu_spaced(dc.selection_bed(), recs, groups, 3, deciding[0], start=True)


def blockers(recs, g, sel, d):
    """for every passed-over record of group g: (its place in the group's order, the place of the first kept record that
    blocks it)"""
    order = dm.select([dict(r, eligible=True) for r in recs if r["group"] == g], 10 ** 9)
    place = {(r["chr"], r["pos"], r["sense"]): i for i, r in enumerate(order)}
    kept = [r for r in sel if r["group"] == g]
    last = place[(kept[-1]["chr"], kept[-1]["pos"], kept[-1]["sense"])]
    out = []
    for r in order[:last]:
        me = (r["chr"], r["pos"], r["sense"])
        if any((q["chr"], q["pos"], q["sense"]) == me for q in kept) or not r["eligible"]:
            continue
        by = [place[(q["chr"], q["pos"], q["sense"])] for q in kept if q["chr"] == r["chr"] and
              abs(pm.cut(q, K, P, 3, False) - pm.cut(r, K, P, 3, False)) < d and place[(q["chr"], q["pos"], q["sense"])] < place[me]]
        out.append((place[me], min(by)))
    return out, place, kept


def test_spacing_across_the_steps_of_64():
    bed = dc.edge_beds()["spans_250_520"]
    groups, recs = dc.model_records(bed)
    assert [sum(1 for r in recs if r["group"] == g) for g in (0, 1)] == [250, 271]
    flat_recs = [dict(r, spec=np.float32(0.5), eligible=True) for r in recs]
    d = 9
    walk = sl.select_spaced(flat_recs, 1024, d, K, P)[0]
    full, place, kept = blockers(flat_recs, 1, walk, d)
    # a conflict between a pick of one step and a record of the next (the LDS list), and one inside a step (the ballots)
    assert any(j // 64 != i // 64 for j, i in full) and any(j // 64 == i // 64 for j, i in full)
    places = [place[(q["chr"], q["pos"], q["sense"])] for q in kept]
    second = next(n for n, at in enumerate(places, 1) if 64 <= at < 128)
    fifth = next(n for n, at in enumerate(places, 1) if 256 <= at < 320)
    for n in (second, fifth):                                              # the N-th pick in the second step, in the fifth
        check_gpu_spaced(bed, flat_recs, groups, n, d)
    spread = spread_scores([dict(r) for r in recs], seed=3)
    check_gpu_spaced(bed, spread, groups, 20, d)
    sel, _ = check_gpu_spaced(bed, spread, groups, 100, 2)                 # the kept list passes 64 entries
    assert max(sum(1 for r in sel if r["group"] == g) for g in (0, 1)) > 64
    check_gpu_spaced(bed, spread, groups, 1024, 5)
    check_gpu_spaced(bed, spread, groups, 1024, 1, decides=False)          # D = 1 on distinct cuts keeps every marked record but equal cuts


def test_a_group_at_record_256_and_a_group_with_no_record():
    _, names, _, _ = dc.genome()
    bed = dc.edge_beds()["begins_at_256"] + f"{names[0]}\t0\t5\tnothing\n{names[0]}\t2000\t2100\tsmall\n"
    groups, recs = dc.model_records(bed)
    assert groups[2] == "nothing" and not any(r["group"] == 2 for r in recs) and any(r["group"] == 3 for r in recs)
    spread_scores(recs, seed=5)
    for n, d in ((3, 25), (70, 4)):
        sel, _ = check_gpu_spaced(bed, recs, groups, n, d)
        assert sl.last_select(recs, sel, len(groups), n)["groups_empty"] == 1


def test_refusals_on_the_device(selection):
    groups, recs = selection
    design, rg = device_design(dc.selection_bed())
    design.set_scores(np.full(len(recs), 0.5, np.float32))
    design.set_spacing(10)
    for n in (None, 1025):
        with pytest.raises(api.GsError) as e:
            design.select("", n)
        assert e.value.status == 1
        with pytest.raises(api.GsError):
            design.rows("", n)
    with pytest.raises(api.GsError) as e:
        design.pairs("", 60)
    assert e.value.status == 1
    with pytest.raises(api.GsError):
        design.set_spacing(10, cut_offset=21)
    design.select("", 1024).close()
    design.set_spacing(0)
    km, pr = design.pairs("", 60)          # with the rule off the pairs are back
    km.close()
    pr.close()
    design.close()
    rg.close()


def test_the_real_score_then_the_spaced_selection():
    """api.design from the scan to the selection: sequence rules before the restriction, the search's own specificities,
    the picks spaced"""
    text, names, lengths, chromosomes = dc.genome()
    kw = dict(gc=(30, 80), max_run=4, exclude_sites=("CGTCTC",))
    groups, recs = dc.model_records(dc.selection_bed())
    recs = [r for r in recs if sl.charge(r["seq"], kw["gc"], kw["max_run"], sl.motif_list((), kw["exclude_sites"])) == sl.PASS]
    oidx = ol.OracleIndex(text)
    dm.score(recs, oidx, lengths, "NGG", mismatches=dc.MISMATCHES)
    oidx.close()
    sel, spacing = sl.select_spaced(recs, 3, 25, K, P)
    assert spacing["passed_over"] > 0 and len(recs) < 88
    gidx = api.GenomeIndex.build(text, device=0)
    rg = api.Regions.parse(dc.selection_bed().encode(), (names, lengths))
    km = api.design(gidx, rg, "NGG", K, per_region=3, chromosomes=chromosomes, mismatches=dc.MISMATCHES, seq_rule=api_rule(**kw),
                    min_spacing=25)
    assert_same(selected(km), dm.arrays(sel, groups, names, "NGG"))
    km.close()
    rg.close()
    gidx.close()
