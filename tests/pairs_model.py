"""Guide pairs for regions, restated in plain Python: the cut of a record, the pair test as a double loop over the
records of a group, the rank with sorted() on tuples, the cut to N, the guides and the table text.  Shares no code with
the library (csrc/gs_pairs_scan.h, csrc/gs_pairs.hip); records are the dicts of tests/design_model.py."""
import numpy as np

import design_model as dm

HEADER = "group,id_a,id_b,chromosome,cut_a,cut_b,span,specificity_a,specificity_b,pair_specificity\n"


def pam_right(r, start):
    """the protospacer lies in front of the PAM on the forward strand"""
    return (r["sense"] == "+") != start


def cut(r, k, P, C, start):
    """the forward-strand boundary x: the cut falls between bases x - 1 and x, C protospacer bases from the PAM"""
    q = r["pos"] - 1
    return q + k - C if pam_right(r, start) else q + P + C


def eligible(r, min_specificity):
    return bool(r.get("eligible", True)) and (min_specificity is None or np.float32(r["spec"]) >= np.float32(min_specificity))


def pairs(recs, k, P, max_span, min_span=1, cut_offset=3, orientation="any", per_region=None, min_specificity=None, start=False):
    """-> list of (a, b): indices into recs, group by group in ranked order, cut to per_region"""
    def place(i):
        r = recs[i]
        return (r["chr"], cut(r, k, P, cut_offset, start), r["sense"] == "-")

    out = []
    for g in sorted({r["group"] for r in recs}):
        members = sorted((i for i, r in enumerate(recs) if r["group"] == g and eligible(r, min_specificity)), key=place)
        found = []
        what = [(recs[i]["chr"], cut(recs[i], k, P, cut_offset, start), pam_right(recs[i], start)) for i in members]
        for x, a in enumerate(members):
            chr_a, cut_a, right_a = what[x]
            for y in range(x + 1, len(members)):
                chr_b, cut_b, right_b = what[y]
                if chr_a != chr_b:
                    continue
                if not min_span <= cut_b - cut_a <= max_span:
                    continue
                if orientation == "pam-out" and not (not right_a and right_b):
                    continue
                if orientation == "pam-in" and not (right_a and not right_b):
                    continue
                found.append((a, members[y]))
        # found is in enumeration order; sorted() is stable
        found.sort(key=lambda p: (-min(float(recs[p[0]]["spec"]), float(recs[p[1]]["spec"])),
                                  -max(float(recs[p[0]]["spec"]), float(recs[p[1]]["spec"]))))
        out += found if per_region is None else found[:per_region]
    return out


def counted(recs, k, P, max_span, **kw):
    """pairs per group before the cut to N: {group: count}"""
    kw = dict(kw, per_region=None)
    by = {}
    for a, _ in pairs(recs, k, P, max_span, **kw):
        by[recs[a]["group"]] = by.get(recs[a]["group"], 0) + 1
    return by


def guides(recs, kept):
    """the records that are a member of a kept pair, in the order of a selection without a cut -> (records, index in
    recs -> place)"""
    members = {i for p in kept for i in p}
    marked = [dict(r, eligible=(i in members), _i=i) for i, r in enumerate(recs)]
    sel = dm.select(marked)
    return sel, {r["_i"]: j for j, r in enumerate(sel)}


def arrays(recs, kept, k, P, cut_offset=3, start=False, place=None):
    """what Pairs.to_host gives; place: index in recs -> a / b (None: the index itself)"""
    def at(i):
        return i if place is None else place[i]

    ra, rb = [recs[a] for a, _ in kept], [recs[b] for _, b in kept]
    return {"n": len(kept),
            "group": np.array([r["group"] for r in ra], dtype=np.uint32),
            "chr": np.array([r["chr"] for r in ra], dtype=np.uint32),
            "a": np.array([at(a) for a, _ in kept], dtype=np.uint32),
            "b": np.array([at(b) for _, b in kept], dtype=np.uint32),
            "cut_a": np.array([cut(r, k, P, cut_offset, start) for r in ra], dtype=np.uint32),
            "cut_b": np.array([cut(r, k, P, cut_offset, start) for r in rb], dtype=np.uint32),
            "spec_a": np.array([r["spec"] for r in ra], dtype=np.float32),
            "spec_b": np.array([r["spec"] for r in rb], dtype=np.float32)}


def _f(x):
    return f"{float(np.float32(x)):.6f}"


def table(recs, kept, groups, names, k, P, cut_offset=3, start=False, prefix=""):
    out = [HEADER]
    for a, b in kept:
        ra, rb = recs[a], recs[b]
        ia, ib = dm.ids([ra, rb], groups, names, prefix)
        xa, xb = cut(ra, k, P, cut_offset, start), cut(rb, k, P, cut_offset, start)
        out.append(f"{groups[ra['group']]},{ia},{ib},{names[ra['chr']]},{xa},{xb},{xb - xa},{_f(ra['spec'])},{_f(rb['spec'])},"
                   f"{_f(min(np.float32(ra['spec']), np.float32(rb['spec'])))}\n")
    return "".join(out)


def last(recs, kept, k, P, max_span, n_groups, chunks=1, **kw):
    """what Pairs.last gives, chunks as told"""
    by = counted(recs, k, P, max_span, **kw)
    n = kw.get("per_region")
    total = sum(by.values())
    return {"eligible": sum(1 for r in recs if eligible(r, kw.get("min_specificity"))), "counted": total, "kept": len(kept),
            "chunks": chunks if total else 0, "groups_without": n_groups - len(by),
            "groups_short": sum(1 for c in by.values() if n is not None and c < n)}
