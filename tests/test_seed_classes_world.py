"""What tests/test_gpu_seed_classes.py leans on, asserted without a GPU: the planted world of tests/seed_classes_world.py
holds, in the ORACLE's lists, every site class on both strands and for both PAM pairs, class hits (the spaced lookup's
share) for every anchor at every budget, and the fat key and the fat entries - so that a GPU run equal to these lists has met
them.  Prints, per depth and budget, the oracle's hit and class counts."""
from collections import Counter

import pytest

import seed_classes_world as W

DEPTHS = [(14, 8), (13, 9)]


@pytest.fixture(scope="module", params=[(k, x, s) for k, x in DEPTHS for s in (False, True)],
                ids=[f"k{k}{'-start' if s else ''}" for k, x in DEPTHS for s in (False, True)])
def world(request):
    return W.world(*request.param)


def main_list(w):
    return "ttn" if w["start"] else "ngg-nag"


def test_counts_are_printed_and_class_hits_exist_for_every_anchor_and_budget(world):
    w = world
    for (m, name), per in sorted(w["expected"].items(), key=lambda kv: (kv[0][1], kv[0][0])):
        cls = w["class_hits"][(m, name)]
        print(f"k={w['k']} |X|={w['x_len']} start={w['start']} {name} m={m}: {sum(map(len, per))} hits, class hits "
              f"{cls[:W.N_ANCHORS]} on the anchors, {sum(cls)} in the batch")
        if m <= 4:
            assert all(c > 0 for c in cls[:W.N_ANCHORS]), (m, name, cls)
        else:
            assert sum(cls) == 0   # (no class at a budget the seeding launches do not serve)
    name = main_list(w)
    totals = [sum(map(len, w["expected"][(m, name)])) for m in (1, 2, 3, 4)]
    assert totals == sorted(totals) and totals[0] >= 100 and totals[3] >= 600, totals


def test_every_class_on_both_strands_and_for_both_pairs(world):
    """every planted site is in its anchor's list at budget 4 at the place, with the distance and the substituted positions
    it was planted with; together they are every triple x strand x pair of the list's tables"""
    w = world
    name = main_list(w)
    pairs = W.PAM_LISTS[w["start"]][name][2]
    want = Counter()
    for ai in range(W.N_ANCHORS):
        by_pos = {(r[0], r[2]): r for r in w["expected"][(4, name)][ai]}
        for s in w["sites"]:
            pair = s["pam"][:2] if w["start"] else s["pam"][1:]
            if s["anchor"] != ai or pair not in pairs:
                continue
            r = by_pos.get(W.reported(s, w["start"]))
            assert r is not None, s
            site = W.site_of(r[3], w["start"])
            guide = site[W.P:] if w["start"] else site[:W.L]
            assert r[1] == sum(s["triple"]) and [q for q, ch in enumerate(guide) if ch.islower()] == s["where"], (s, r)
            assert W.class_of(r[3], w["k"], w["x_len"], w["start"]) == s["triple"], (s, r)
            if s["kind"] == "class":
                want[(ai, s["triple"], s["strand"], pair)] += 1
    triples = W.triples(w["k"], w["x_len"])
    assert len(triples) == 35
    assert set(want) == {(ai, t, st, p) for ai in range(W.N_ANCHORS) for t in triples for st in (0, 1) for p in pairs}


def test_fat_key_fat_entries_and_literal_n(world):
    w = world
    kinds = Counter((s["kind"], s["strand"]) for s in w["sites"])
    # one (X, R) key of one strand's own-pair table: anchor 0's, with the family's sites and the class sites that leave X, R alone
    assert kinds[("fat-key", 0)] > 64 and kinds[("fat-key", 0)] + kinds[("fat-key", 1)] == W.FAT_KEY
    # one k-mer (X and O exact) with one PAM on one strand; one deep-table entry (O, R and the PAM exact) on the other
    assert kinds[("fat-kmer", 0)] >= 63 and kinds[("fat-deep", 1)] >= 63 and kinds[("fat-kmer", 1)] == kinds[("fat-deep", 0)] == 0
    assert len({s["pam"] for s in w["sites"] if s["kind"] == "fat-kmer"}) == 1
    assert len({s["pam"] for s in w["sites"] if s["kind"] == "fat-deep"}) == 1
    for m in (1, 2, 3, 4):
        recs = [r for e in w["expected"][(m, main_list(w))] for r in e]
        assert sum("N" in W.pam_of(r[3], w["start"]) for r in recs) >= 1, m
    # the N runs are there, one of them within a site's reach of the text's end
    assert (w["text"] == ord("N")).sum() > 12 and (w["text"][-1_100:] == ord("N")).any()
