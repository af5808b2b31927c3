"""The toy genome and the BED files that tests/test_design_model.py (host, no GPU) and tests/test_gpu_design.py run against
tests/design_model.py.  Everything is derived from the model's own candidate list, so a case says what it holds."""
from functools import lru_cache
from importlib import import_module

import numpy as np

import design_model as dm

synth = import_module("guidescan-cli_amd.synth")
kmers = import_module("guidescan-cli_amd.kmers")

LENGTHS = [6000, 2500, 4500]
DUP = (300, 360, 1, 1200)   # chr1[300:360) planted again at chr2[1200:1260)
# chr1[3000:3120) planted on chr3 with every 20th base substituted (one mismatch in every 20-mer: dropped by -t 1), and
# chr1[4000:4120) with every 10th (two mismatches: kept by -t 1, scored lower or higher as the CFD weights fall)
NEAR = ((3000, 3120, 2, 2000, 20), (4000, 4120, 2, 3000, 10))
MISMATCHES = 2   # of the selection cases: the planted families lie within it


@lru_cache(maxsize=None)
def genome():
    text, names, lengths = synth.make_genome(LENGTHS, seed=41, n_blocks=False)
    text = np.array(text, dtype=np.uint8)
    begin = np.concatenate([[0], np.cumsum(lengths)]).astype(int)
    s, e, c, at = DUP
    text[begin[c] + at:begin[c] + at + (e - s)] = text[s:e]
    for s, e, c, at, step in NEAR:
        cp = text[s:e].copy()
        cp[3::step] = np.frombuffer(b"CATG", dtype=np.uint8)[np.searchsorted(np.frombuffer(b"ACGT", dtype=np.uint8), cp[3::step])]
        text[begin[c] + at:begin[c] + at + (e - s)] = cp
    chromosomes = [(i, text[begin[i]:begin[i + 1]].tobytes()) for i in range(len(lengths))]
    return text, list(names), [int(x) for x in lengths], chromosomes


@lru_cache(maxsize=None)
def candidates(pam="NGG", k=20, start=False):
    """per chromosome: [(seq, pos, sense)] in the scan's order"""
    return [kmers.find_all_kmers(chrm, pam, k, start) for _, chrm in genome()[3]]


def trimmed(c, target, pam="NGG", k=20, start=False):
    """"A\tX": an interval [A, X) of chromosome c that holds exactly `target` candidates, A as small as there is one"""
    w = k + len(pam)
    begins = np.array(sorted(pos - 1 for _, pos, _ in candidates(pam, k, start)[c]))
    for a in range(0, 500):
        inside = begins[begins >= a]
        if inside.size < target:
            break
        x = int(inside[target - 1]) + w
        if int((inside + w <= x).sum()) == target:
            return f"{a}\t{x}"
    raise AssertionError(f"no interval of chromosome {c} holds exactly {target} candidates")


def membership_beds(pam="NGG", k=20, start=False):
    """name -> BED text"""
    _, names, lengths, _ = genome()
    w = k + len(pam)
    cand = candidates(pam, k, start)
    plus = next(p for _, p, s in cand[0] if s == "+" and p > 200)
    minus = next(p for _, p, s in cand[0] if s == "-" and p > 200)
    mid = next(p for _, p, s in cand[0] if p > 1000)
    seam = mid - 1 + 10
    a, b = mid - 1 - 50, mid - 1 + w + 50
    c1, c2, c3 = names
    beds = {
        "exact": f"{c1}\t{plus - 1}\t{plus - 1 + w}\texact_plus\n{c1}\t{minus - 1}\t{minus - 1 + w}\texact_minus\n"
                 f"{c1}\t{plus - 1}\t{plus - 2 + w}\tshort_plus\n{c1}\t{minus}\t{minus - 1 + w}\tshort_minus\n",
        "edges": f"{c1}\t0\t300\thead\n{c1}\t{lengths[0] - 300}\t{lengths[0]}\ttail\n",
        "whole": f"{c2} 0 {lengths[1]}\n",
        "abut_one_group": f"{c1}\t{a}\t{seam}\tgene\n{c1}\t{seam}\t{b}\tgene\n",
        "abut_two_groups": f"{c1}\t{a}\t{seam}\tleft\n{c1}\t{seam}\t{b}\tright\n",
        "nested": f"{c3}\t100\t900\tn1\n{c3}\t200\t800\tn2\n{c3}\t300\t700\tn3\n{c3}\t1500\t1700\tlater\n"
                  f"{c1}\t50\t400\tn2\n",
        "none": f"{c1}\t0\t5\tnothing\n",
    }
    for n in (63, 64, 65, 255, 256, 257):
        beds[f"count{n}"] = f"{c1}\t{trimmed(0, n, pam, k, start)}\tprefix\n"
    return beds


def selection_bed():
    """a group over both copies of the planted segment and what surrounds them, a small group, and one of every
    candidate of the third chromosome"""
    _, names, lengths, _ = genome()
    s, e, c, at = DUP
    return (f"# groups for the selection cases\n{names[0]}\t{s - 60}\t{e + 60}\tdup\n{names[c]}\t{at - 60}\t{at + (e - s) + 60}\tdup\n"
            f"{names[0]}\t2000\t2100\tsmall\n{names[0]}\t{NEAR[0][0]}\t{NEAR[0][1]}\tmix\n"
            f"{names[0]}\t{NEAR[1][0]}\t{NEAR[1][1]}\tmix\n{names[2]}\t0\t500\tbig\n")


def edge_beds():
    """group boundaries on a workgroup edge of the passes: a group that begins at record 256, and one that spans
    records 250-520"""
    _, names, lengths, _ = genome()
    return {
        "begins_at_256": f"{names[2]}\t{trimmed(2, 256)}\tfirst\n{names[1]}\t0\t{lengths[1]}\tsecond\n",
        "spans_250_520": f"{names[2]}\t{trimmed(2, 250)}\tfirst\n{names[0]}\t{trimmed(0, 271)}\tsecond\n"
                         f"{names[1]}\t0\t400\tthird\n",
    }


def model_records(bed, pam="NGG", k=20, start=False):
    _, names, lengths, chromosomes = genome()
    groups, merged = dm.parse_bed(bed.encode(), names, lengths)
    return groups, dm.records(groups, merged, chromosomes, pam, k, start)


# ---- the edge BEDs ranked: the rank, head and cut passes of the selection across workgroup edges ---------------------
EDGE_MISMATCHES = 1   # both planted families with one mismatch or none lie within it; the search of ~1,300 records stays short
# (per_region, min_specificity, with the eligibility of -t 1): N smaller than the groups; N beyond one workgroup of kept records
EDGE_SELECTIONS = ((7, None, False), (100, 0.75, True), (200, None, True), (1, 0.75, False))


def edge_scored(oidx):
    """name -> (groups, records with the model's spec and eligibility under -t 1) of edge_beds(); asserts that the cases
    decide something: in a group that does not begin at record 0 some record is not eligible and some falls below 0.75, so
    its ranks are not its places, and every N cuts a group that has more"""
    lengths = genome()[2]
    out = {}
    for name, bed in edge_beds().items():
        groups, recs = model_records(bed)
        dm.score(recs, oidx, lengths, "NGG", mismatches=EDGE_MISMATCHES, threshold=1)
        later = [r for r in recs if r["group"] >= 1]
        assert any(not r["eligible"] for r in later) and any(r["spec"] < np.float32(0.75) for r in later), name
        for n, s, thr in EDGE_SELECTIONS:
            rs = recs if thr else [dict(r, eligible=True) for r in recs]
            uncut, cut = dm.select(rs, None, s), dm.select(rs, n, s)
            assert len(cut) < len(uncut) and any(sum(1 for r in cut if r["group"] == g) == n for g in range(len(groups))), (name, n)
        out[name] = (groups, recs)
    return out
