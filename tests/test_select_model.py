"""Library selection without a GPU: the host twins of the sequence rules (gs_debug_kmers_filter_host) and of the spaced
selection (gs_debug_design_host_spaced), both through csrc/gs_select_scan.h, against tests/select_model.py on the toy
genome of tests/design_cases.py; the refusals; and the header's stand-alone check under the sanitizers.  Every case
asserts that it decides something, with the counts the model gave when the case was written."""
import shutil
import subprocess
from importlib import import_module

import numpy as np
import pytest

import design_cases as dc
import design_model as dm
import oracle_lib as ol
import pairs_model as pm
import select_model as sl
from test_design_model import SHAPES, assert_same

api = import_module("guidescan-cli_amd.api")

# name -> (the model's keywords, candidates passing of the 1,185 at NGG, k = 20)
RULES = {
    "gc": (dict(gc=(40, 70)), 792),
    "run": (dict(max_run=3), 917),
    "tttt": (dict(exclude_motifs=("TTTT",)), 1083),
    "site": (dict(exclude_sites=("CGTCTC",)), 1180),
    "iupac": (dict(exclude_motifs=("GGNCC",)), 1158),
    "gc_open": (dict(gc=(0, 100)), 1185),
    "n": (dict(exclude_motifs=("N",)), 0),
    "all": (dict(gc=(40, 70), max_run=3, exclude_motifs=("TTTT", "GGNCC"), exclude_sites=("CGTCTC",)), None),
}


def flat(pam="NGG", k=20, start=False):
    return [c for chrm in dc.candidates(pam, k, start) for c in chrm]


def api_rule(gc=None, max_run=None, exclude_motifs=(), exclude_sites=()):
    return api.SeqRule(gc=gc, max_run=max_run, exclude_motifs=exclude_motifs, exclude_sites=exclude_sites)


def host_charges(cands, k, **kw):
    seqs = np.frombuffer("".join(c[0] for c in cands).encode(), dtype=np.uint8).reshape(len(cands), k)
    return api.seq_rule_host(seqs, k, api_rule(**kw))


@pytest.mark.parametrize("pam,k,start", SHAPES, ids=lambda v: str(v))
@pytest.mark.parametrize("name", sorted(RULES))
def test_sequence_rules_on_the_host(name, pam, k, start):
    kw, passing = RULES[name]
    cands = flat(pam, k, start)
    kept, counts, charges = sl.filter_candidates(cands, **kw)
    got, got_counts = host_charges(cands, k, **kw)
    assert got.tolist() == charges
    assert got_counts == counts
    if (pam, k, start) == ("NGG", 20, False):
        assert [len(c) for c in dc.candidates()] == [564, 222, 399]
        if passing is not None:
            assert len(kept) == passing
        else:
            assert 0 < len(kept) < 792 and min(counts["gc"], counts["run"], counts["motif"]) > 0
    else:
        assert counts["scanned"] == len(cands) > 0


def test_the_sequence_cases_decide_at_their_edges():
    cands = flat()
    gcs = [sl.gc_count(c[0]) for c in cands]
    assert [gcs.count(g) for g in (8, 14, 7, 15)] == [223, 10, 160, 4]          # 40% and 70% of 20, and one beyond each
    runs = [sl.longest_run(c[0]) for c in cands]
    assert (runs.count(3), runs.count(4), sum(1 for r in runs if r >= 5)) == (514, 191, 77)
    tttt = [sl.motif_offsets(c[0], "TTTT") for c in cands]
    assert sum(1 for o in tttt if o) == 102
    assert sum(1 for o in tttt if o and o[0] == 0) == 10 and sum(1 for o in tttt if o and o[-1] == 16) == 7
    as_written = [bool(sl.motif_offsets(c[0], "CGTCTC")) for c in cands]
    reverse = [bool(sl.motif_offsets(c[0], "GAGACG")) for c in cands]
    assert sl.reverse_complement("CGTCTC") == "GAGACG"
    assert sum(as_written) == 2 and sum(r and not w for r, w in zip(reverse, as_written)) == 3
    assert sum(1 for c in cands if sl.motif_offsets(c[0], "GGNCC")) == 27
    # runs that end on the last base, and lower case, through the twin
    assert any(sl.longest_run(c[0]) > 3 and sl.longest_run(c[0][:-1]) <= 3 for c in cands)
    lower = [(c[0].lower(), c[1], c[2]) for c in cands]
    kw = RULES["all"][0]
    assert host_charges(lower, 20, **kw)[0].tolist() == sl.filter_candidates(cands, **kw)[2]


def test_a_motif_longer_than_k_and_the_charge_order():
    cands = flat()
    long_motif = "N" * 21
    got, counts = host_charges(cands, 20, exclude_motifs=(long_motif,))
    assert not got.any() and counts == sl.filter_candidates(cands, exclude_motifs=(long_motif,))[1]
    assert host_charges(cands, 20, exclude_motifs=("N" * 20,))[0].tolist() == [sl.MOTIF] * len(cands)
    # a candidate that fails two rules is charged to the first: GC before run before motif
    both = [c for c in cands if sl.gc_count(c[0]) < 8 and sl.longest_run(c[0]) > 3 and sl.motif_offsets(c[0], "TTTT")]
    assert both
    for kw, want in ((dict(gc=(40, 70), max_run=3, exclude_motifs=("TTTT",)), sl.GC), (dict(max_run=3, exclude_motifs=("TTTT",)), sl.RUN),
                     (dict(exclude_motifs=("TTTT",)), sl.MOTIF)):
        got, _ = host_charges(both, 20, **kw)
        assert got.tolist() == [want] * len(both) == [sl.charge(c[0], kw.get("gc"), kw.get("max_run"), kw.get("exclude_motifs", ())) for c in both]


REFUSED_MOTIFS = [(("ACXT",), ()), (("",), ()), ((), ("ACGU",)), (("A" * 33,), ()), (tuple("ACGTACGTACGTACGTA"), ()),
                  ((), tuple(["ACG"] * 9)), (("A",) * 15, ("AC",))]


@pytest.mark.parametrize("motifs,sites", REFUSED_MOTIFS)
def test_refused_rules_name_the_motif(motifs, sites):
    with pytest.raises(sl.RuleError) as me:
        sl.motif_list(motifs, sites)
    with pytest.raises(ValueError) as e:
        api.SeqRule(exclude_motifs=motifs, exclude_sites=sites)
    assert "\n" not in str(e.value) and f"'{me.value.motif}'" in str(e.value)


def test_rules_at_their_limits_are_taken():
    assert sl.motif_list(("A",) * 16) == ["A"] * 16 and api.SeqRule(exclude_motifs=("A",) * 16).n_motifs == 16
    assert len(sl.motif_list((), ("ACG",) * 8)) == 16 and api.SeqRule(exclude_sites=("ACG",) * 8).n_motifs == 16
    assert sl.motif_list((), ("GAATTC",)) == ["GAATTC"] and api.SeqRule(exclude_sites=("GAATTC", "gaattc")).n_motifs == 2   # a palindrome once
    assert api.SeqRule(exclude_motifs=("N" * 32,)).n_motifs == 1
    for gc in ((70, 40), (0, 101), (-1, 50)):
        with pytest.raises(sl.RuleError):
            sl.check_gc(gc)
        with pytest.raises(ValueError):
            api.SeqRule(gc=gc)
    with pytest.raises(ValueError):
        api.SeqRule(max_run=0)
    L, rule = api.lib(), api.GsSeqRule()
    L.gs_seq_rule_init(rule)
    rule.gc_min, rule.gc_max = 70, 40
    seqs, out = np.frombuffer(b"ACGT" * 5, dtype=np.uint8), np.zeros(1, np.uint8)
    assert L.gs_debug_kmers_filter_host(seqs.ctypes.data, 1, 20, rule, out.ctypes.data, None) == 1
    assert L.gs_kmers_filter(None, rule, None, None, None) == 1 and L.gs_seq_rule_add_motif(None, b"A", 0) == 1


# ---- spacing --------------------------------------------------------------------------------------------------------

K, P = 20, 3


def candidate_parts(pam="NGG", k=K, start=False, scores=None):
    """the toy genome's candidates as gs_debug_design_host takes them; scores: {(chr, pos, sense): (spec, eligible)}"""
    parts = []
    for c, cand in enumerate(dc.candidates(pam, k, start)):
        seqs = np.frombuffer("".join(s for s, _, _ in cand).encode(), dtype=np.uint8).reshape(len(cand), k)
        pos = np.array([p for _, p, _ in cand], dtype=np.uint32)
        sense = np.frombuffer("".join(s for _, _, s in cand).encode(), dtype=np.uint8)
        spec = np.array([scores.get((c, p, s), (0.0, True))[0] for _, p, s in cand], dtype=np.float32)
        elig = np.array([scores.get((c, p, s), (0.0, True))[1] for _, p, s in cand], dtype=np.uint8)
        parts.append((c, seqs, pos, sense, spec, elig))
    return parts


def spread_scores(recs, seed=7, levels=(1.0, 0.9, 0.75, 0.5, 0.5, 0.25), drop=5):
    """chosen ranks with ties: a level per record from a seeded generator, every `drop`-th draw not eligible"""
    rng = np.random.default_rng(seed)
    for r in recs:
        r["spec"] = np.float32(levels[int(rng.integers(len(levels)))])
        r["eligible"] = bool(rng.integers(drop) != 0)
    return recs


def scores_of(recs):
    return {(r["chr"], r["pos"], r["sense"]): (r["spec"], r["eligible"]) for r in recs}


def check_spaced(bed, recs, groups, n, d, cut_offset=3, start=False, min_specificity=None, pam="NGG", k=K, decides=True):
    """the host twin against the model: ids, order, last_select, last_spacing; -> the model's selection"""
    _, names, lengths, _ = dc.genome()
    sel, spacing = sl.select_spaced(recs, n, d, k, len(pam), cut_offset, start, min_specificity)
    rg = api.Regions.parse(bed.encode(), (names, lengths))
    got = api.design_host_model(rg, candidate_parts(pam, k, start, scores_of(recs)), pam, k, "", n, min_specificity, rows=True,
                                min_spacing=d, cut_offset=cut_offset, start=start)
    rg.close()
    assert_same(got, dm.arrays(sel, groups, names, pam))
    assert got["rows"].decode() == dm.rows(sel, groups, names, pam)
    assert got["last_spacing"] == spacing
    assert got["last_select"] == sl.last_select(recs, sel, len(groups), n)
    if decides:
        unspaced = dm.select(recs, n, min_specificity)
        assert dm.ids(sel, groups, names) != dm.ids(unspaced, groups, names) and spacing["passed_over"] > 0
    return sel, spacing


@pytest.fixture(scope="module")
def selection():
    groups, recs = dc.model_records(dc.selection_bed())
    assert [sum(1 for r in recs if r["group"] == g) for g in range(len(groups))] == [29, 7, 15, 37]
    return groups, spread_scores(recs)


def test_neighbouring_cuts_lie_close(selection):
    """what the rule is for: of the neighbouring cuts within a group most lie fewer than 10 bases apart"""
    groups, recs = selection
    near = total = 0
    for g in range(len(groups)):
        cuts = sorted((r["chr"], pm.cut(r, K, P, 3, False)) for r in recs if r["group"] == g)
        total += len(cuts) - 1
        near += sum(1 for a, b in zip(cuts, cuts[1:]) if a[0] == b[0] and b[1] - a[1] < 10)
    assert (near, total) == (52, 84)


def test_spacing_on_the_selection_groups(selection):
    groups, recs = selection
    bed = dc.selection_bed()
    for n, d in ((3, 25), (5, 10), (2, 1), (40, 7)):
        check_spaced(bed, recs, groups, n, d, decides=d > 1)
    # D beyond every group's span: one pick per chromosome, and the group of the planted copies lies on two
    sel, spacing = check_spaced(bed, recs, groups, 5, 10000)
    per_group = [sum(1 for r in sel if r["group"] == g) for g in range(len(groups))]
    assert per_group == [2, 1, 1, 1] and groups[0] == "dup" and spacing["groups_short_for_spacing"] == 4
    assert len({r["chr"] for r in sel if r["group"] == 0}) == 2
    # a bound on the specificity: records below S neither count nor block
    sel_s, _ = check_spaced(bed, recs, groups, 3, 25, min_specificity=0.75)
    assert all(r["spec"] >= np.float32(0.75) and r["eligible"] for r in sel_s)
    assert dm.ids(sel_s, groups, ["a", "b", "c"]) != dm.ids(check_spaced(bed, recs, groups, 3, 25)[0], groups, ["a", "b", "c"])


def chain_of(recs, g, d):
    """a, b, c of group g on one chromosome, in cut order: b within d of a and of c, c not within d of a"""
    members = sorted((r for r in recs if r["group"] == g), key=lambda r: (r["chr"], pm.cut(r, K, P, 3, False)))
    for i, a in enumerate(members):
        for j in range(i + 1, len(members)):
            for m in range(j + 1, len(members)):
                b, c = members[j], members[m]
                xa, xb, xc = (pm.cut(r, K, P, 3, False) for r in (a, b, c))
                if a["chr"] == b["chr"] == c["chr"] and 0 < xb - xa < d and 0 < xc - xb < d and xc - xa >= d:
                    return a, b, c
    return None


def test_the_chain_is_judged_against_the_kept_records_only(selection):
    groups, recs = selection
    g, d = groups.index("big"), 25
    a, b, c = chain_of(recs, g, d)
    rs = [dict(r, spec=np.float32(0.1), eligible=True) for r in recs]
    for r in rs:
        for x, s in ((a, 1.0), (b, 0.9), (c, 0.8)):
            if (r["group"], r["chr"], r["pos"], r["sense"]) == (x["group"], x["chr"], x["pos"], x["sense"]):
                r["spec"] = np.float32(s)
    sel, _ = check_spaced(dc.selection_bed(), rs, groups, 2, d)
    picked = [(r["pos"], r["sense"]) for r in sel if r["group"] == g]
    assert picked == [(a["pos"], a["sense"]), (c["pos"], c["sense"])]   # a rule against all better records would drop c


def test_ties_ineligible_records_and_the_last_record(selection):
    groups, recs = selection
    bed = dc.selection_bed()
    # all specificities equal: the order within a group is chromosome, position, sense
    flat_recs = [dict(r, spec=np.float32(0.5), eligible=True) for r in recs]
    sel, _ = check_spaced(bed, flat_recs, groups, 4, 12)
    for g in range(len(groups)):
        own = [(r["chr"], r["pos"], r["sense"] == "-") for r in sel if r["group"] == g]
        assert own == sorted(own) and own[0] == min((r["chr"], r["pos"], r["sense"] == "-") for r in recs if r["group"] == g)
    # records that are not eligible do not block: with the best record of every group dropped, its neighbour is picked
    best = {g: dm.select([r for r in flat_recs if r["group"] == g], 1)[0] for g in range(len(groups))}
    dropped = [dict(r, eligible=r is not best[r["group"]]) for r in flat_recs]
    sel_d, _ = check_spaced(bed, dropped, groups, 4, 12)
    firsts = {g: next(r for r in sel_d if r["group"] == g) for g in range(len(groups))}
    assert any(abs(pm.cut(firsts[g], K, P, 3, False) - pm.cut(best[g], K, P, 3, False)) < 12 and firsts[g]["chr"] == best[g]["chr"]
               for g in firsts)   # eligible, the dropped record would have blocked the one picked first
    # N reached exactly on the last record of a group, and an N the group cannot give
    found = None
    for d in range(2, 40):
        walk = sl.select_spaced(flat_recs, 1024, d, K, P)[0]
        for g in range(len(groups)):
            order = dm.select([r for r in flat_recs if r["group"] == g], 1024)
            picks = [r for r in walk if r["group"] == g]
            if picks[-1] is order[-1] and len(picks) < len(order) and found is None:
                found = (g, d, len(picks), order[-1])
    assert found is not None
    g, d, n, last_record = found
    sel_n, _ = check_spaced(bed, flat_recs, groups, n, d)
    assert [r for r in sel_n if r["group"] == g][-1] is last_record
    sel_more, more = check_spaced(bed, flat_recs, groups, n + 1, d)
    assert sum(1 for r in sel_more if r["group"] == g) == n and more["groups_short_for_spacing"] >= 1


def test_start_moves_the_cut_and_the_offset_counts():
    groups, recs = dc.model_records(dc.selection_bed(), "NGG", K, True)
    spread_scores(recs, seed=11)
    # the same records judged by the cut of the other side give another selection at some D: the first such D is run
    deciding = [d for d in range(5, 40) if dm.ids(sl.select_spaced(recs, 3, d, K, P, 3, True)[0], groups, ["a", "b", "c"]) !=
                dm.ids(sl.select_spaced(recs, 3, d, K, P, 3, False)[0], groups, ["a", "b", "c"])]
    assert deciding
    check_spaced(dc.selection_bed(), recs, groups, 3, deciding[0], start=True)
    groups, recs = dc.model_records(dc.selection_bed())
    spread_scores(recs, seed=11)
    by_offset = [dm.ids(check_spaced(dc.selection_bed(), recs, groups, 3, 15, cut_offset=c)[0], groups, ["a", "b", "c"]) for c in (0, 3, 20)]
    assert len({tuple(x) for x in by_offset}) > 1


def test_a_plus_and_a_minus_record_with_one_cut():
    """synthetic candidates, since the scan of the toy genome gives none: '+' at position p cuts at p - 1 + 17, '-' at
    p + 11 cuts at p + 10 + 6; at D = 1 the two conflict and the better one stays"""
    _, names, lengths, _ = dc.genome()
    bed = f"{names[0]}\t0\t400\tone\n"
    cands = [(100, "+", 0.5), (111, "-", 0.9), (140, "+", 0.7), (151, "-", 0.7), (200, "+", 0.2), (201, "+", 0.3)]
    recs = [{"group": 0, "chr": 0, "pos": p, "sense": s, "seq": "ACGT" * 5, "spec": np.float32(x), "eligible": True} for p, s, x in cands]
    assert pm.cut(recs[0], K, P, 3, False) == pm.cut(recs[1], K, P, 3, False) and pm.cut(recs[2], K, P, 3, False) == pm.cut(recs[3], K, P, 3, False)
    sel, spacing = sl.select_spaced(recs, 6, 1, K, P)
    assert [(r["pos"], r["sense"]) for r in sel] == [(111, "-"), (140, "+"), (201, "+"), (200, "+")] and spacing["passed_over"] == 2
    rg = api.Regions.parse(bed.encode(), (names, lengths))
    part = (0, np.frombuffer(("ACGT" * 5 * len(cands)).encode(), dtype=np.uint8).reshape(len(cands), K),
            np.array([c[0] for c in cands], dtype=np.uint32), np.frombuffer("".join(c[1] for c in cands).encode(), dtype=np.uint8),
            np.array([c[2] for c in cands], dtype=np.float32), np.ones(len(cands), np.uint8))
    got = api.design_host_model(rg, [part], "NGG", K, "", 6, None, min_spacing=1)
    rg.close()
    assert got["ids"] == "".join(dm.ids(sel, ["one"], names)).encode() and got["last_spacing"] == spacing


def test_spacing_across_steps_of_64_on_the_host():
    for name, bed in dc.edge_beds().items():
        groups, recs = dc.model_records(bed)
        spread_scores(recs, seed=3)
        for n, d in ((20, 9), (100, 2), (1024, 5), (1, 1)):
            check_spaced(bed, recs, groups, n, d, decides=(n, d) != (1, 1))


def test_refusals_of_the_spaced_selection():
    groups, recs = dc.model_records(dc.selection_bed())
    spread_scores(recs)
    _, names, lengths, _ = dc.genome()
    rg = api.Regions.parse(dc.selection_bed().encode(), (names, lengths))
    parts = candidate_parts(scores=scores_of(recs))
    for n in (None, 1025):
        with pytest.raises(sl.RuleError):
            sl.select_spaced(recs, n, 10, K, P)
        with pytest.raises(api.GsError) as e:
            api.design_host_model(rg, parts, "NGG", K, "", n, None, min_spacing=10)
        assert e.value.status == 1
    with pytest.raises(sl.RuleError):
        sl.select_spaced(recs, 3, 10, K, P, with_pairs=True)
    with pytest.raises(sl.RuleError):
        sl.select_spaced(recs, 3, 10, K, P, cut_offset=21)
    with pytest.raises(api.GsError):
        api.design_host_model(rg, parts, "NGG", K, "", 3, None, min_spacing=10, cut_offset=21)
    # D = 0 through the spaced twin is the selection as it was
    plain = api.design_host_model(rg, parts, "NGG", K, "", 3, None)
    zero = api.design_host_model(rg, parts, "NGG", K, "", 3, None, min_spacing=0)
    assert plain["ids"] == zero["ids"] and zero["last_spacing"] == {"passed_over": 0, "groups_short_for_spacing": 0}
    rg.close()
    L = api.lib()
    assert L.gs_design_set_spacing(None, 5, 3, 0) == 1 and L.gs_design_last_spacing(None, None) == 1
    assert L.gs_debug_design_set_scores(None, None, None) == 1


def test_select_check_is_clean_under_the_sanitizers():
    if shutil.which("g++") is None or shutil.which("make") is None:
        pytest.skip("no host compiler")
    r = subprocess.run(["make", "-C", str(ol.ROOT / "guidescan-cli_amd" / "csrc"), "select-check"], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all as restated" in r.stdout
