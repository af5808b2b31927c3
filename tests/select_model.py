"""Library selection restated in plain Python: the sequence rules on a candidate's protospacer with str methods and sets,
and the spacing between the picks of a group as a loop over sorted() tuples.  Shares no code with the library
(csrc/gs_select_scan.h, csrc/gs_kmers.hip, csrc/gs_design.hip); records are the dicts of tests/design_model.py."""
import numpy as np

import pairs_model as pm

IUPAC = {"A": "A", "C": "C", "G": "G", "T": "T", "R": "AG", "Y": "CT", "S": "CG", "W": "AT", "K": "GT", "M": "AC",
         "B": "CGT", "D": "AGT", "H": "ACT", "V": "ACG", "N": "ACGT"}
COMPLEMENT = {"A": "T", "C": "G", "G": "C", "T": "A", "R": "Y", "Y": "R", "S": "S", "W": "W", "K": "M", "M": "K",
              "B": "V", "V": "B", "D": "H", "H": "D", "N": "N"}
MAX_MOTIFS, MAX_LETTERS, MAX_PER_REGION = 16, 32, 1024
PASS, GC, RUN, MOTIF = 0, 1, 2, 3


class RuleError(Exception):
    """a rule the commands refuse; .motif names the motif where one is at fault"""

    def __init__(self, message, motif=None):
        super().__init__(message)
        self.motif = motif


def reverse_complement(motif):
    return "".join(COMPLEMENT[c] for c in reversed(motif.upper()))


def motif_list(exclude_motifs=(), exclude_sites=()):
    """the motifs after the expansion of the sites, upper case; RuleError for what is refused"""
    out = []
    for motifs, both in ((exclude_motifs, False), (exclude_sites, True)):
        for m in motifs:
            if m == "":
                raise RuleError("an empty motif", m)
            if len(m) > MAX_LETTERS:
                raise RuleError("a motif of more than 32 letters", m)
            if any(c.upper() not in IUPAC for c in m):
                raise RuleError("a letter outside ACGTRYSWKMBDHVN", m)
            new = [m.upper()]
            if both and reverse_complement(m) != m.upper():
                new.append(reverse_complement(m))
            if len(out) + len(new) > MAX_MOTIFS:
                raise RuleError("more than 16 motifs", m)
            out += new
    return out


def check_gc(gc):
    lo, hi = gc
    if not (isinstance(lo, int) and isinstance(hi, int) and 0 <= lo <= hi <= 100):
        raise RuleError("gc: 0 <= MIN <= MAX <= 100")


def gc_count(seq):
    return sum(1 for c in seq.upper() if c in "GC")


def longest_run(seq):
    s, best, i = seq.upper(), 0, 0
    while i < len(s):
        j = i
        while j < len(s) and s[j] == s[i]:
            j += 1
        best, i = max(best, j - i), j
    return best


def motif_offsets(seq, motif):
    """the offsets of the protospacer at which the motif matches"""
    s = seq.upper()
    return [o for o in range(len(s) - len(motif) + 1) if all(s[o + p] in IUPAC[motif[p]] for p in range(len(motif)))]


def charge(seq, gc=None, max_run=None, motifs=()):
    """PASS, or the first rule the protospacer fails in the order GC, RUN, MOTIF"""
    k = len(seq)
    if gc is not None and not gc[0] * k <= 100 * gc_count(seq) <= gc[1] * k:
        return GC
    if max_run is not None and longest_run(seq) > max_run:
        return RUN
    if any(motif_offsets(seq, m) for m in motifs):
        return MOTIF
    return PASS


def filter_candidates(cands, gc=None, max_run=None, exclude_motifs=(), exclude_sites=()):
    """cands: [(seq, pos, sense)] in the scan's order -> (those that pass, in that order; dict(scanned, gc, run, motif);
    the charge of every candidate)"""
    if gc is not None:
        check_gc(gc)
    if max_run is not None and max_run < 1:
        raise RuleError("max_run >= 1")
    motifs = motif_list(exclude_motifs, exclude_sites)
    charges = [charge(c[0], gc, max_run, motifs) for c in cands]
    counts = {"scanned": len(cands), "gc": charges.count(GC), "run": charges.count(RUN), "motif": charges.count(MOTIF)}
    return [c for c, ch in zip(cands, charges) if ch == PASS], counts, charges


def select_spaced(recs, per_region, min_spacing, k, P, cut_offset=3, start=False, min_specificity=None, with_pairs=False):
    """the records in output order under the spacing rule -> (kept records, dict(passed_over, groups_short_for_spacing)).
    Best first within a group - specificity descending, then chromosome, position, '+' before '-' - a marked record is
    kept iff every record already kept for the group on its chromosome has its cut min_spacing or more away, until
    per_region are kept."""
    if with_pairs:
        raise RuleError("a minimum spacing with pairs: pairs have their own span rule")
    if per_region is None or not 1 <= per_region <= MAX_PER_REGION:
        raise RuleError("a minimum spacing needs per_region from 1 to 1024")
    if cut_offset > k:
        raise RuleError("the cut offset lies beyond the k-mer length")

    def key(r):
        return (r["group"], -float(np.float32(r.get("spec", 0.0))), r["chr"], r["pos"], r["sense"] == "-")

    out, passed, short = [], 0, 0
    for g in sorted({r["group"] for r in recs}):
        marked = [r for r in sorted((r for r in recs if r["group"] == g), key=key) if pm.eligible(r, min_specificity)]
        kept = []
        for r in marked:
            if len(kept) == per_region:
                break
            x = pm.cut(r, k, P, cut_offset, start)
            if all(q["chr"] != r["chr"] or abs(pm.cut(q, k, P, cut_offset, start) - x) >= min_spacing for q in kept):
                kept.append(r)
            else:
                passed += 1
        if len(kept) < per_region <= len(marked):
            short += 1
        out += kept
    return out, {"passed_over": passed, "groups_short_for_spacing": short}


def last_select(recs, sel, n_groups, per_region):
    """what Design.last_select gives for a selection"""
    kept = [sum(1 for r in sel if r["group"] == g) for g in range(n_groups)]
    return {"records": len(recs), "kept": len(sel), "groups_empty": kept.count(0),
            "groups_short": sum(1 for c in kept if 0 < c < per_region)}
