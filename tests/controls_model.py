"""`guidescan controls` restated in plain Python: the counter-based generator with Python integers, the charges (the
sequence rules are tests/select_model.py's), and the walk as one loop with a character-by-character Hamming distance
(numpy compares a candidate's letters with those of every kept control at once: the loop over them in Python takes minutes).
Shares no code with the library (csrc/gs_controls_scan.h, csrc/gs_controls.hip).  Whether a candidate is targeting is an
input: the tests take it from the oracle."""
import numpy as np

import select_model as sl

M64 = (1 << 64) - 1
KEPT, GC, RUN, MOTIF, TARGETING, CLOSE = range(6)
COUNTS = ("kept", "gc", "run", "motif", "targeting", "close")


def mix(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def sequence(seed, i, L):
    """the protospacer of candidate i of the seed, as the sequence column prints it"""
    w = mix(mix(seed) ^ i)
    return "".join("ACGT"[(w >> (2 * j)) & 3] for j in range(L))


def sequences(seed, first, n, L):
    return [sequence(seed, first + j, L) for j in range(n)]


def hamming(a, b):
    return sum(1 for x, y in zip(a, b) if x != y)


def walk(targeting, n, L, pam="NGG", seed=0, first=0, gc=None, max_run=None, exclude_motifs=(), exclude_sites=(), min_distance=1,
         max_candidates=1 << 32, prefix="control_"):
    """targeting[j]: candidate first + j has a hit.  -> (kept counters, rows bytes, report dict, the charge of every
    candidate looked at)"""
    motifs = sl.motif_list(exclude_motifs, exclude_sites)
    kept, kept_seq, charges = [], [], []
    letters = np.zeros((min(n, len(targeting)) + 1, L), dtype=np.uint8)        # row t: the letters of kept control t
    limit = min(len(targeting), max_candidates)
    for j in range(limit):
        if len(kept) >= n:
            break
        s = sequence(seed, first + j, L)
        ch = sl.charge(s, gc, max_run, motifs)
        if ch == sl.PASS and targeting[j]:
            ch = TARGETING
        if ch == sl.PASS and kept:
            mine = np.frombuffer(s.encode(), dtype=np.uint8)
            if int((letters[:len(kept)] != mine).sum(axis=1).min()) < min_distance:
                ch = CLOSE
        if ch == KEPT:
            letters[len(kept)] = np.frombuffer(s.encode(), dtype=np.uint8)
            kept.append(first + j)
            kept_seq.append(s)
        charges.append(ch)
    report = {name: charges.count(c) for c, name in enumerate(COUNTS)}
    report["looked_at"] = len(charges)
    report["last_counter"] = first + len(charges) - 1 if charges else first
    rows = "".join(f"{prefix}{i},{s},{pam},NA,0,+\n" for i, s in zip(kept, kept_seq)).encode()
    return kept, rows, report, charges
