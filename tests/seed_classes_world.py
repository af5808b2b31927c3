"""A planted world for the seeding launches (gs_seed.hip: k_seed_a, k_seed_b, the spaced lookup), with the CPU oracle's
answer to every batch the GPU tests run on it.  TEST INFRASTRUCTURE: no GPU, no library but the oracle.

The seeding launches split a 20-mer's site by where its substitutions lie, in guide coordinates: X = [0, x_len) (the symbols
beyond the other strand's deep table), O = [x_len, k) (the rest of this strand's k-mer) and R = [k, 20) (the context behind the
k-mer) - the split `site_key` of tests/test_gpu_spaced.py uses.  Which launch, which table and which recipe finds a site
depends on the triple (substitutions in X, in O, in R), on the strand and on the PAM pair; the class (0, m, 0) at budget m
comes from the spaced lookup when that is on.  A genome sampled at random holds most of these classes for no guide in a
small batch, so here every one is planted, with the families that make single keys and entries heavy:

* every class: for each of four anchors absent from the text and every triple with sum <= 4 one site per strand (2), per
  PAM of the own pair (AGG-like) and of the second pair (TAG-like), the substituted positions drawn inside their region;
* a fat spaced key: 150 copies of anchor 0 with X and R exact and 1 .. min(4, |O|) substitutions in O, xGG with all four
  x, two thirds on one strand: more than 64 rows under one key of one strand's table (several rounds of the lookup);
* a fat k-mer entry: 80 copies of anchor 0 with X and O exact and 1 .. 4 substitutions in R, one strand, one PAM: a
  pair-table entry of 63 rows and more (GS_PT_BIG: the count sits in a header slot);
* a fat deep-table entry: 80 copies with O, R and the PAM exact and 1 .. 4 substitutions in X, on the other strand;
* sites with a literal N under the PAM's N (they belong to the window list, not to any table) and a few runs of N.

`start=True` is the mirror image behind TTN: the PAM in front of the guide, the regions counted from the guide's other end.
Sites lie 61 symbols apart (a prime: they take every offset within the Occ blocks and the table's sampling)."""
import functools

import numpy as np

import oracle_lib as ol

L, P = 20, 3
TEXT_LEN = 400_000
STEP = 61
ACGT = np.frombuffer(b"ACGT", np.uint8)
COMP = np.zeros(256, np.uint8)
for _a, _b in zip(b"ACGTN", b"TGCAN"):
    COMP[_a] = _b
N_ANCHORS = 4
N_SAMPLED = 12
FAT_KEY, FAT_KMER, FAT_DEEP = 150, 80, 80

# name -> (own pattern, alternatives, pairs that have a table, lookups per item: one per table and appending pass)
PAM_LISTS = {
    False: {"ngg": ("NGG", (), ("GG",), 1),
            "ngg-nag": ("NGG", ("NAG",), ("GG", "AG"), 2),
            "six": ("NGG", ("NAG", "CGG", "AGG", "TGG", "GGG"), ("GG", "AG"), 3)},
    True: {"ttn": ("TTN", (), ("TT",), 1)},
}
# the (budget, list) pairs the oracle answers: what tests/test_gpu_seed_classes.py runs
BATCHES = {
    False: [(m, "ngg-nag") for m in (1, 2, 3, 4, 5)] + [(m, "ngg") for m in (1, 2, 3, 4)] + [(3, "six")],
    True: [(m, "ttn") for m in (1, 2, 3, 4)],
}


def rc(b):
    return COMP[np.asarray(b, dtype=np.uint8)[::-1]]


def regions(k, x_len, start):
    """guide positions of X, O, R"""
    x, o, r = range(0, x_len), range(x_len, k), range(k, L)
    if start:
        x, o, r = (range(L - q.stop, L - q.start) for q in (x, o, r))
    return dict(X=list(x), O=list(o), R=list(r))


def triples(k, x_len, budget=4):
    return [(a, b, c) for a in range(min(budget, x_len) + 1) for b in range(min(budget, k - x_len) + 1)
            for c in range(min(budget, L - k) + 1) if a + b + c <= budget]


def _substituted(rng, anchor, reg, triple):
    site = anchor.copy()
    where = []
    for name, cnt in zip("XOR", triple):
        where += [int(q) for q in rng.choice(reg[name], size=cnt, replace=False)]
    for q in where:
        site[q] = rng.choice([b for b in ACGT if b != anchor[q]])
    return site, sorted(where)


def _pams(start):
    """(own pair's, second pair's) three-symbol PAMs with each first base, as the forward site spells them, and the own
    pair's with a literal N"""
    if start:
        return [b"TT" + bytes([x]) for x in b"ACGT"], [b"TC" + bytes([x]) for x in b"ACGT"], b"TTN"
    return [bytes([x]) + b"GG" for x in b"ACGT"], [bytes([x]) + b"AG" for x in b"ACGT"], b"NGG"


def site_of(seq, start):
    """a reported sequence as the forward site reads, guide + PAM (start: PAM + guide), the lower case of the substituted
    symbols kept.  The reference reports the complement of the site (search order reproduced: index.hpp:182-248), behind
    --start the site read backwards; what is compared with the library is the reported string itself, this is only for
    sorting the oracle's hits into classes"""
    if start:
        return seq[::-1]
    comp = dict(zip("ACGTNacgtn", "TGCANtgcan"))
    return "".join(comp[ch] for ch in seq)


def class_of(seq, k, x_len, start):
    """(substitutions in X, in O, in R) of a reported sequence: the oracle writes a substituted symbol in lower case"""
    s = site_of(seq, start)
    guide = s[P:P + L] if start else s[:L]
    low = {q for q, ch in enumerate(guide) if ch.islower()}
    reg = regions(k, x_len, start)
    return tuple(len(low & set(reg[n])) for n in "XOR")


def pam_of(seq, start):
    s = site_of(seq, start)
    return s[:P] if start else s[L:L + P]


def pair_of(seq, start):
    """the two concrete symbols of a reported PAM that name its table"""
    p = pam_of(seq, start)
    return p[:2] if start else p[1:]


def reported(site, start):
    """(position, strand flag) the oracle reports for a planted site: a site read off the forward text (behind --start: off the
    reverse strand) is reported at its last symbol, the other at minus its first"""
    if (site["strand"] == 0) != start:
        return site["at"] + L + P - 1, 1
    return -site["at"], 0


def is_class_hit(rec, m, k, x_len, start, pairs):
    """a hit the spaced lookup is there to find: distance exactly m, every substitution in O, a table's pair, no literal N"""
    pos, dist, index, seq = rec
    return (dist == m and class_of(seq, k, x_len, start) == (0, m, 0) and "N" not in pam_of(seq, start)
            and pair_of(seq, start) in pairs)


@functools.lru_cache(maxsize=None)
def planted(k, x_len, start=False):
    """-> dict(text, anchors, guides, seqs, sites): the text and what was written into it, without the oracle"""
    rng = np.random.default_rng(1000 * k + 10 * x_len + int(start))
    text = ACGT[rng.integers(0, 4, TEXT_LEN)].copy()
    reg = regions(k, x_len, start)
    own, second, lit = _pams(start)
    anchors = []
    while len(anchors) < N_ANCHORS:
        a = ACGT[rng.integers(0, 4, L)].copy()
        if all(bytes(t).find(bytes(s)) < 0 for t in (text,) for s in (a, rc(a))):
            anchors.append(a)
    sites = []
    at = [1_000]

    def put(kind, ai, triple, strand, pam, where, site):
        w = np.concatenate([np.frombuffer(pam, np.uint8), site] if start else [site, np.frombuffer(pam, np.uint8)])
        text[at[0]:at[0] + L + P] = w if strand == 0 else rc(w)
        sites.append(dict(kind=kind, anchor=ai, triple=triple, strand=strand, pam=pam.decode(), at=at[0], where=where,
                          seq=site.tobytes().decode()))
        at[0] += STEP

    for ai, a in enumerate(anchors):
        for tr in triples(k, x_len):
            for strand in (0, 1):
                for pams in (own, second):
                    site, where = _substituted(rng, a, reg, tr)
                    put("class", ai, tr, strand, pams[int(rng.integers(0, 4))], where, site)
    a0 = anchors[0]
    for c in range(FAT_KEY):
        tr = (0, 1 + c % min(4, k - x_len), 0)
        site, where = _substituted(rng, a0, reg, tr)
        put("fat-key", 0, tr, 0 if c % 3 else 1, own[c % 4], where, site)
    for c in range(FAT_KMER):
        tr = (0, 0, 1 + c % 4)
        site, where = _substituted(rng, a0, reg, tr)
        put("fat-kmer", 0, tr, 0, own[0], where, site)
    for c in range(FAT_DEEP):
        tr = (1 + c % 4, 0, 0)
        site, where = _substituted(rng, a0, reg, tr)
        put("fat-deep", 0, tr, 1, own[1], where, site)
    for c in range(12):   # a literal N under the PAM's N, both strands, up to two substitutions anywhere
        tr = [(0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (0, 1, 1)][c % 6]
        site, where = _substituted(rng, anchors[1], reg, tr)
        put("literal-n", 1, tr, c % 2, lit, where, site)
    assert at[0] < 100_000
    for s in (150_000, 222_222, 399_000):   # runs of N, one of them near the text's end
        text[s:s + int(rng.integers(1, 60))] = ord("N")
    # a dozen guides off the text's plain stretch, either strand, each in front of (behind) a PAM of the own pattern
    sampled = []
    t2 = (text, rc(text))
    p = 110_000
    while len(sampled) < N_SAMPLED:
        t = t2[len(sampled) % 2]
        w = bytes(t[p:p + L + P])
        ok = (w[:2] == b"TT") if start else (w[-2:] == b"GG")
        if ok and all(ch in b"ACGT" for ch in w):
            sampled.append(np.frombuffer(w[P:] if start else w[:L], np.uint8).copy())
            p += 3_001
        p += 1
    guides = [a.tobytes().decode() for a in anchors] + [rc(a).tobytes().decode() for a in anchors]
    guides += [s.tobytes().decode() for s in sampled]
    seqs = np.array([list(g.encode()) for g in guides], dtype=np.uint8)
    text.setflags(write=False)
    return dict(k=k, x_len=x_len, r_len=L - k, start=start, text=text, anchors=[a.tobytes().decode() for a in anchors], guides=guides,
                seqs=seqs, sites=sites, regions=reg)


@functools.lru_cache(maxsize=None)
def world(k, x_len, start=False):
    """planted(...) plus, per (budget, PAM list) of BATCHES: expected[(m, name)][i] = the oracle's records (position,
    distance, index, sequence) of guide i, class_hits[(m, name)][i] = how many of them the spaced lookup is there to find"""
    w = dict(planted(k, x_len, start))
    oidx = ol.OracleIndex(w["text"])
    expected, class_hits = {}, {}
    try:
        for m, name in BATCHES[start]:
            own, alt, pairs, _ = PAM_LISTS[start][name]
            opts = ol.make_opts(mismatches=m, alt_pams=alt, start=start)
            per = []
            for g in w["guides"]:
                hits, _, raw = oidx.enumerate(g, own, opts)
                ol.lib().gso_free(raw[0])
                per.append([(h[0], h[1], h[2], h[3]) for h in hits])
            expected[(m, name)] = per
            class_hits[(m, name)] = [sum(is_class_hit(r, m, k, x_len, start, pairs) for r in e) for e in per]
    finally:
        oidx.close()
    w.update(expected=expected, class_hits=class_hits)
    return w
