"""A plain model of the reference's scoring and the builders of synthesized hit lists (no test in here).

The model restates include/genomics/printer.hpp:98-170, 251-297 and src/genomics/structures.cxx:7-52 of the
reference on hit lists given as (guide, key, pos): the key layout is the one include/guidescan_amd.h documents,
the CFD of a hit is the oracle's gso_calculate_cfd, and the aggregation is written twice - guide by guide the
way the reference loops (specificity_csv / specificity_sam), and once over a whole batch in numpy
(specificity_batch) so that batches of 10^5 guides stay a matter of seconds.  tests/test_score_model.py holds
the two forms to each other and both to the oracle's text lines, the golden files and the host formatter.

The builders return small, seeded batches (seqs, offsets, hits, chromosome lengths) whose shapes sit on the
edges of the device kernels: hit counts either side of 64 / 512 / 4,096, distance classes cut by
--max-off-targets, chromosome structures of 0 .. 3,000 chromosomes, sequence shapes other than 20 + 3."""
from importlib import import_module

import numpy as np

import oracle_lib as ol

api = import_module("guidescan-cli_amd.api")

BASES = "ACGT"
PAM_SYMBOLS = "ACGNT"   # codes 0..4 of a PAM position
_COMP = str.maketrans("ACGTacgt", "TGCAtgca")


def complement(s: str) -> str:
    """sequences.cxx: base by base, case kept, anything else (N) unchanged"""
    return s.translate(_COMP)


def query_chars(guide: str, start: bool) -> str:
    """the character the search consumes at step t (process.hpp:63): the reverse complement read from its
    end, i.e. the guide's complement read forward; under --start the guide itself read from its end"""
    return guide[::-1] if start else complement(guide)


# ---- key <-> match.sequence ---------------------------------------------------------------------------

def encode_hit(guide: str, subs: dict, pam: str, distance: int, index: int, start: bool = False):
    """-> (key, match.sequence).  subs: {step t: base found there, one of ACGT other than the query character};
    pam: the PAM symbols as they stand in match.sequence (ACGNT).  Layout: bits 63..61 distance, bit 60 index,
    two bits per guide position from bit 59 down (0 = the query character, 1..3 = rank of the base found among
    the three others in A<C<G<T order), three bits per PAM position (A,C,G,N,T = 0..4), bit 0 zero."""
    L, q = len(guide), query_chars(guide, start)
    assert 2 * L + 3 * len(pam) <= 59 and 0 <= distance < 8 and index in (0, 1)
    key = (distance << 61) | (index << 60)
    ms, bit = [], 60
    for t in range(L):
        bit -= 2
        b = subs.get(t)
        if b is None:
            ms.append(q[t])
        else:
            others = [x for x in BASES if x != q[t]]
            key |= (others.index(b) + 1) << bit
            ms.append(b.lower())   # index.hpp:243: a substituted position is lower case
    for s in pam:
        bit -= 3
        key |= PAM_SYMBOLS.index(s) << bit
        ms.append(s)
    assert bit >= 1 and key & 1 == 0
    if start:   # the string a --start key stands for is the host decoder's
        return key, api.decode_sequence(guide, len(pam), key, api.GS_FLAG_PAM_AT_START)
    return key, "".join(ms)


def match_sequence(guide: str, P: int, key: int, start: bool = False) -> str:
    """match.sequence of (guide, key): the layout above read back"""
    if start:
        return api.decode_sequence(guide, P, key, api.GS_FLAG_PAM_AT_START)
    L, q = len(guide), query_chars(guide, False)
    ms, bit = [], 60
    for t in range(L):
        bit -= 2
        code = (key >> bit) & 3
        ms.append(q[t] if code == 0 else [x for x in BASES if x != q[t]][code - 1].lower())
    for _ in range(P):
        bit -= 3
        ms.append(PAM_SYMBOLS[(key >> bit) & 7])
    return "".join(ms)


def subs_of(sequence: str, L: int) -> dict:
    """the substitutions a match.sequence string shows: its lower-case positions"""
    return {t: c.upper() for t, c in enumerate(sequence[:L]) if c.islower()}


# ---- one hit ------------------------------------------------------------------------------------------

def hit_facts(guide: str, P: int, key: int, start: bool = False):
    """-> (CFD as float32, perfect-hit flag) of one hit: printer.hpp:133-146 / :264-277"""
    ms = complement(match_sequence(guide, P, key, start))
    pam = ms[20:23] if len(ms) >= 20 else ""
    cfd = np.float32(ol.lib().gso_calculate_cfd(guide.encode(), ms.encode(), pam.encode()))
    perfect = (key >> 61) == 0 and len(pam) == 3 and pam[1:3] == "GG"
    return cfd, perfect


def resolve_absolute(lengths, pos: int, L: int, P: int):
    """src/genomics/structures.cxx:7-52 as written -> (chromosome, start, strand) or None for the sentinel"""
    strand = "+"
    if pos < 0:
        pos, strand = -pos, "-"
    c, c_len = None, 0
    for i, ln in enumerate(lengths):
        if pos <= int(ln) - 1:   # (int64_t)(chr.length - 1): -1 for an empty chromosome, which nothing fits
            c, c_len = i, int(ln)
            break
        pos -= int(ln)
    # (the assert on an unnamed chromosome is compiled out of a release build: {"", 0} goes on)
    if strand == "+":
        end = pos + 1
        begin = end - L - P + 1
    else:
        begin = pos + 1
        end = begin + L + P - 1
    if begin < 0 or end > c_len:
        return None
    return c, begin, strand


def dropped_batch(lengths, pos: np.ndarray, L: int, P: int) -> np.ndarray:
    """resolve_absolute's sentinel for an array of positions: the first-fit loop subtracts whole chromosomes
    until the rest fits, which is the first chromosome whose END (prefix sum) exceeds |pos|; an empty
    chromosome's end equals the one before it and is never first"""
    pos = np.asarray(pos, dtype=np.int64)
    if len(lengths) == 0:
        return np.ones(pos.shape, dtype=bool)
    ends = np.cumsum(np.asarray(lengths, dtype=np.int64))
    ab = np.abs(pos)
    c = np.searchsorted(ends, ab, side="right")
    beyond = c >= len(ends)
    c = np.minimum(c, len(ends) - 1)
    off = ab - (ends[c] - np.asarray(lengths, dtype=np.int64)[c])
    plus = pos >= 0
    begin = np.where(plus, off + 1 - L - P + 1, off + 1)
    end = np.where(plus, off + 1, off + 1 + L + P - 1)
    return beyond | (begin < 0) | (end > np.asarray(lengths, dtype=np.int64)[c])


# ---- one guide: the reference's loops ---------------------------------------------------------------

def _classes(d):
    """the guide's hits split by distance, in order (off_targets[d])"""
    out = {}
    for h, dv in enumerate(d):
        out.setdefault(int(dv), []).append(h)
    return [out[k] for k in sorted(out)]


def _finish(terms, perfect_match):
    cfd_sum = np.cumsum(np.asarray(terms, dtype=np.float32), dtype=np.float32)[-1] if terms else np.float32(0.0)
    if not perfect_match:
        cfd_sum = np.float32(cfd_sum + np.float32(1.0))
    return np.float32(1.0) / cfd_sum if cfd_sum > 0 else np.float32(0.0)


def specificity_csv(d, cfd, dropped, perfect, max_off=-1):
    """get_csv_lines, printer.hpp:251-297: a distance class is cut at its raw index"""
    terms, perfect_match = [], False
    for cls in _classes(d):
        for i, h in enumerate(cls):
            if max_off != -1 and i >= max_off:
                break
            if perfect[h]:
                perfect_match = True
            if not dropped[h]:
                terms.append(cfd[h])
    return _finish(terms, perfect_match)


def specificity_sam(d, cfd, dropped, perfect, max_off=-1):
    """off_target_fields, printer.hpp:115-170: only hits that resolved count towards the cut"""
    terms, perfect_match = [], False
    for cls in _classes(d):
        n_off_targets = 0
        for h in cls:
            if max_off != -1 and n_off_targets >= max_off:
                break
            if perfect[h]:
                perfect_match = True
            if dropped[h]:
                continue
            terms.append(cfd[h])
            n_off_targets += 1
    return _finish(terms, perfect_match)


# ---- a whole batch ------------------------------------------------------------------------------------

def batch_facts(seqs, P, offsets, hits, lengths, start=False):
    """-> (distance, cfd float32, dropped, perfect) per hit; the CFD computed once per distinct (guide, key)"""
    seqs = np.ascontiguousarray(seqs, dtype=np.uint8)
    n, L = seqs.shape
    counts = np.diff(np.asarray(offsets).astype(np.int64))
    gid = np.repeat(np.arange(n), counts)
    keys = np.asarray(hits["key"], dtype=np.uint64)
    d = (keys >> np.uint64(61)).astype(np.int64)
    dropped = dropped_batch(lengths, hits["pos"], L, P)
    if keys.shape[0] == 0:
        return d, np.empty(0, np.float32), dropped, np.empty(0, bool)
    ug, ginv = np.unique(seqs.view(np.dtype((np.void, L))).ravel(), return_inverse=True)
    uk, kinv = np.unique(keys, return_inverse=True)
    up, pinv = np.unique(ginv.ravel()[gid].astype(np.int64) * len(uk) + kinv.ravel(), return_inverse=True)
    cfd_u, perfect_u = np.empty(len(up), np.float32), np.empty(len(up), bool)
    for j, p in enumerate(up):
        cfd_u[j], perfect_u[j] = hit_facts(ug[p // len(uk)].tobytes().decode(), P, int(uk[p % len(uk)]), start)
    return d, cfd_u[pinv.ravel()], dropped, perfect_u[pinv.ravel()]


def specificity_batch(offsets, d, cfd, dropped, perfect, max_off=-1, sam=False):
    """both aggregations over a whole batch.  A hit that does not count enters as +0: the partial sums start at
    +0 and no CFD is negative, and x + (+0) == x for every such x, so the sum over all hits in order equals the
    reference's sum over the hits that count (tests/test_score_model.py holds this to the loops above)."""
    off = np.asarray(offsets).astype(np.int64)
    n, nh = off.shape[0] - 1, int(off[-1])
    counts = np.diff(off)
    gid = np.repeat(np.arange(n), counts)
    if max_off == -1:
        inc = np.ones(nh, dtype=bool)
    else:
        idx = np.arange(nh)
        new = np.ones(nh, dtype=bool)   # first hit of its (guide, distance) class
        new[1:] = (gid[1:] != gid[:-1]) | (d[1:] != d[:-1])
        first = np.maximum.accumulate(np.where(new, idx, 0))
        if sam:
            ok = (~dropped).astype(np.int64)
            before = np.cumsum(ok) - ok   # resolved hits ahead of this one
            rank = before - before[first] if nh else before
        else:
            rank = idx - first
        inc = rank < max_off
    has_perfect = np.bincount(gid[inc & perfect], minlength=n) > 0
    term = np.where(inc & ~dropped, cfd, np.float32(0.0)).astype(np.float32)
    sums = np.zeros(n, dtype=np.float32)
    light = counts <= 4
    for j in range(4):   # the guides with a handful of hits: their j-th hit, all guides at once
        m = light & (counts > j)
        sums[m] = sums[m] + term[off[:-1][m] + j]
    for g in np.flatnonzero(~light):
        sums[g] = np.cumsum(term[off[g]:off[g + 1]], dtype=np.float32)[-1]
    sums = sums + np.where(has_perfect, np.float32(0.0), np.float32(1.0)).astype(np.float32)
    spec = np.zeros(n, dtype=np.float32)
    np.divide(np.float32(1.0), sums, out=spec, where=sums > 0)
    return spec


def specificity_loops(offsets, d, cfd, dropped, perfect, max_off=-1, sam=False):
    """the batch through the per-guide loops"""
    off = np.asarray(offsets).astype(np.int64)
    fn = specificity_sam if sam else specificity_csv
    return np.array([fn(d[a:b], cfd[a:b], dropped[a:b], perfect[a:b], max_off) for a, b in zip(off[:-1], off[1:])],
                    dtype=np.float32).reshape(-1)


# ---- builders -----------------------------------------------------------------------------------------

GENOME = [5000, 23, 3000, 61, 40000]   # the chromosome structure of the batches that are not about geometry
NGG_TAILS = ["GG"] * 8 + ["AG"] * 3 + ["NG", "GN", "CG", "GA", "TG", "GT", "TT"]
LADDER_COUNTS = [0, 1, 2, 7, 8, 9, 31, 32, 33, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1023, 1024, 1025, 1535, 1536,
                 1537, 4095, 4096, 4097, 8191, 8192, 8193, 12289, 70000]
MAXOFF_VALUES = [0, 1, 2, 63, 64, 65, 100, 1000]
SHAPES = [(20, 3, True), (20, 4, True), (20, 0, False), (17, 3, False), (18, 3, False), (19, 3, False),
          (19, 4, False), (21, 2, False), (22, 1, False), (23, 0, False), (23, 4, False), (28, 1, False)]


def _guide(rng, L=20):
    return "".join(rng.choice(list(BASES), L))


def _ngg_pam(rng, tail=None):
    """the PAM of an NGG-style hit as it stands in match.sequence: the complement of what the text reads"""
    tail = NGG_TAILS[rng.integers(len(NGG_TAILS))] if tail is None else tail
    return complement(BASES[rng.integers(4)] + tail)


def _free_pam(rng, P):
    """P symbols, G-rich on the text side so that `GG` at positions 21 and 22 happens and fails to"""
    return complement("".join(rng.choice(list("ACGTN"), P, p=[.15, .1, .55, .15, .05])))


def _template(rng, guide, nsub, pam, index, start=False):
    q = query_chars(guide, start)
    subs = {}
    for t in rng.choice(len(guide), nsub, replace=False):
        others = [b for b in BASES if b != q[t]]
        subs[int(t)] = others[rng.integers(3)]
    return encode_hit(guide, subs, pam, nsub, index, start)[0]


def _pool(rng, guide, n, P=3, start=False, dists=(0, 1, 2, 3, 4), ngg=True):
    """up to n distinct keys of the guide at the given distances (there are few distinct ones at distance 0)"""
    keys = set()
    for _ in range(8 * n):
        if len(keys) >= n:
            break
        pam = (_ngg_pam(rng) if ngg else _free_pam(rng, P)) if P else ""
        keys.add(_template(rng, guide, int(dists[rng.integers(len(dists))]), pam, int(rng.integers(2)), start))
    return np.array(sorted(keys), dtype=np.uint64)


def _positions(rng, lengths, L, P, n, near=0.06):
    """n signed positions below the genome length: inside the longest chromosome where the window fits, and a
    share `near` within a window's length of a chromosome join, where resolve_absolute drops most of them"""
    lengths = np.asarray(lengths, dtype=np.int64)
    cum = np.concatenate([[0], np.cumsum(lengths)])
    W, big = L + P, int(np.argmax(lengths))
    ab = cum[big] + rng.integers(W, lengths[big] - W, n)
    at_join = cum[rng.integers(0, cum.shape[0], n)] + rng.integers(-W, W, n)
    ab = np.where(rng.random(n) < near, np.clip(at_join, 0, cum[-1] - 1), ab)
    return ab * np.where(rng.random(n) < 0.5, -1, 1)


def _dropped_position(lengths, c, plus=True):
    """a position three bases inside chromosome c's start (+ strand) or end (- strand): the window leaves it"""
    cum = np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64))])
    return int(cum[c] + 3) if plus else -int(cum[c + 1] - 3)


def _assemble(guides, per_guide, lengths, P, start=False, **extra):
    """guides: strings; per_guide: (keys, positions) in canonical order"""
    L = len(guides[0])
    counts = [len(k) for k, _ in per_guide]
    offsets = np.zeros(len(guides) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(counts, dtype=np.uint64)
    hits = np.empty(int(offsets[-1]), dtype=api.HIT_DTYPE)
    if hits.shape[0]:
        hits["key"] = np.concatenate([np.asarray(k, dtype=np.uint64) for k, _ in per_guide])
        hits["pos"] = np.concatenate([np.asarray(p, dtype=np.int64) for _, p in per_guide])
    seqs = np.frombuffer("".join(guides).encode(), dtype=np.uint8).reshape(len(guides), L).copy()
    return dict(seqs=seqs, offsets=offsets, hits=hits, lengths=list(lengths), L=L, P=P, start=start, **extra)


def _random_guide_hits(rng, guide, count, lengths, P=3, start=False, dists=(0, 1, 2, 3, 4), ngg=True, near=0.06):
    if count == 0:
        return np.empty(0, np.uint64), np.empty(0, np.int64)
    pool = _pool(rng, guide, min(count, 400), P, start, dists, ngg)
    keys = np.sort(pool[rng.integers(0, pool.shape[0], count)])
    return keys, _positions(rng, lengths, len(guide), P, count, near)


def build_ladder(seed=5):
    """The length ladder with the perfect-hit guides in it.  Order: empty first and last, runs of empty guides,
    the 4,096-hit guide second so that a prefix sum of exactly 4,096 is followed by empty guides and then a
    one-hit guide, the long guides early so that many straddle multiples of 4,096, a short guide as the last
    one with hits.  `named` maps the perfect-hit guides to their index."""
    rng = np.random.default_rng(seed)
    plan = [0, 4096, 0, 0, 0, 1, 8192, 7, 0, 0, 4095, 2, 4097, 8, 12289, 9, 0, 8191, 31, 8193, 32, 70000, 33, 63, 1537,
            64, 1536, 65, 1535, 127, 1025, 128, 1024, 129, 1023, 511, 513, 512]
    assert sorted(plan[:2] + [c for c in plan[2:] if c]) == LADDER_COUNTS
    guides, per_guide, named = [], [], {}
    for c in plan:
        g = _guide(rng)
        guides.append(g)
        # every other guide without a distance-0 hit: the +1 of a guide that has no perfect hit
        dists = (0, 1, 2, 3, 4) if len(guides) % 2 else (1, 2, 3, 4)
        per_guide.append(_random_guide_hits(rng, g, c, GENOME, dists=dists))

    def special(name, d0, n_rest=20, d0_pos=None):
        """d0: (PAM tail on the text side, index) of the distance-0 hits; then n_rest hits at distances 1..4"""
        g = _guide(rng)
        k0 = [_template(rng, g, 0, _ngg_pam(rng, tail), index) for tail, index in d0]
        rest, rest_pos = _random_guide_hits(rng, g, n_rest, GENOME, dists=(1, 2, 3, 4), near=0.0)
        pos0 = _positions(rng, GENOME, 20, 3, len(k0), near=0.0)
        if d0_pos is not None:
            pos0[:] = d0_pos
        order = np.argsort(np.array(k0, dtype=np.uint64), kind="stable")
        named[name] = len(guides)
        guides.append(g)
        per_guide.append((np.concatenate([np.array(k0, dtype=np.uint64)[order], rest]),
                          np.concatenate([pos0[order], rest_pos])))

    special("perfect_forward", [("GG", 0)])
    special("perfect_reverse_only", [("AG", 0), ("GG", 1)])
    special("only_xAG", [("AG", 0), ("AG", 1)])
    special("perfect_dropped", [("GG", 1)], d0_pos=_dropped_position(GENOME, 2))
    # a guide without a perfect hit up to place 4,094 of a chunk; then the guide whose distance-0 hit is the
    # chunk's last place and whose other hits are the next chunk's first; then one without a perfect hit again
    so_far = sum(len(k) for k, _ in per_guide)
    g = _guide(rng)
    guides.append(g)
    per_guide.append(_random_guide_hits(rng, g, (4095 - so_far) % 4096, GENOME, dists=(1, 2, 3, 4)))
    special("perfect_at_chunk_end", [("GG", 0)], n_rest=40)
    assert int(sum(len(k) for k, _ in per_guide[:named["perfect_at_chunk_end"]])) % 4096 == 4095
    for c, dists in ((11, (1, 2, 3)), (0, ()), (0, ()), (5, (0, 1, 2)), (0, ())):
        g = _guide(rng)
        guides.append(g)
        per_guide.append(_random_guide_hits(rng, g, c, GENOME, dists=dists or (0,)))
    return _assemble(guides, per_guide, GENOME, 3, named=named, heaviest=plan.index(70000))


def build_maxoff(seed=7):
    """Guides whose distance classes are cut by --max-off-targets: class sizes (1, 70, 130, 5,000), boundaries at
    places 63/64 and 127/128, lists of exactly 64 and 128 hits, dropped hits at the first and last place of the
    64-hit blocks and sprinkled through every class, and a distance-0 class AAG (forward index), TGG, AGG
    (reverse index: later in key order) whose perfect hits a cut at 1 leaves out."""
    rng = np.random.default_rng(seed)
    guides, per_guide, named = [], [], {}

    def classes(name, sizes, forced=(), near=0.08):
        g = _guide(rng)
        keys = []
        for dist, size in enumerate(sizes):
            if size:
                pool = _pool(rng, g, min(size, 300), dists=(dist,))
                keys.append(np.sort(pool[rng.integers(0, pool.shape[0], size)]))
        keys = np.concatenate(keys) if keys else np.empty(0, np.uint64)
        pos = _positions(rng, GENOME, 20, 3, keys.shape[0], near) if keys.shape[0] else np.empty(0, np.int64)
        for j, at in enumerate(forced):
            pos[at] = _dropped_position(GENOME, 2 + 2 * (j % 2), plus=j % 3 != 0)
        named[name] = len(guides)
        guides.append(g)
        per_guide.append((keys, pos))

    classes("empty_first", ())
    classes("ladder_1_70_130_5000", (1, 70, 130, 5000), forced=(63, 64, 70, 71, 127, 128, 191, 192, 200, 201, 5200))
    classes("blocks_64_64_200", (64, 64, 200), forced=(0, 63, 64, 127, 128))
    classes("list_of_64", (10, 54), forced=(5, 63))
    classes("list_of_128", (64, 64), forced=(0, 64, 127))
    classes("no_distance_0", (0, 64, 64), forced=(0, 1, 63))
    # (in the second guide the SAM rule passes over the dropped AAG hit and takes CAG, 0.259, where CSV takes nothing)
    for name, second, drop_first in (("aag_tgg_agg", "TGG", False), ("aag_dropped_cag_agg", "CAG", True)):
        g = _guide(rng)
        d0 = [_template(rng, g, 0, complement("AAG"), 0), _template(rng, g, 0, complement(second), 1),
              _template(rng, g, 0, complement("AGG"), 1)]
        assert d0 == sorted(d0)
        rest, rest_pos = _random_guide_hits(rng, g, 5, GENOME, dists=(1,), near=0.0)
        pos0 = _positions(rng, GENOME, 20, 3, 3, near=0.0)
        if drop_first:
            pos0[0] = _dropped_position(GENOME, 4, plus=False)
        named[name] = len(guides)
        guides.append(g)
        per_guide.append((np.concatenate([np.array(d0, dtype=np.uint64), rest]), np.concatenate([pos0, rest_pos])))
    classes("cut_at_1000", (3, 1000, 2000), near=0.1)
    classes("one_class_of_1001", (0, 0, 1001), near=0.1)
    for _ in range(10):
        g = _guide(rng)
        guides.append(g)
        per_guide.append(_random_guide_hits(rng, g, int(rng.integers(0, 21)), GENOME, near=0.2))
    classes("empty_last", ())
    return _assemble(guides, per_guide, GENOME, 3, named=named)


def build_tickets(n, seed=9, n_heavy=40):
    """n guides of 0..3 hits with n_heavy guides of 1,000..3,000 hits scattered among them, from 48 distinct
    guide sequences with 24 keys each (so that the model scores 1,152 templates, not 10^6 hits)"""
    rng = np.random.default_rng(seed)
    pool_guides = [_guide(rng) for _ in range(48)]
    pools = np.stack([_pool(rng, g, 24) for g in pool_guides])   # [48, 24], every row ascending
    which = rng.integers(0, 48, n)
    counts = rng.integers(0, 4, n)
    heavy = rng.choice(n, min(n_heavy, n), replace=False)
    counts[heavy] = rng.integers(1000, 3001, heavy.shape[0])
    offsets = np.zeros(n + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum(counts, dtype=np.uint64)
    gid = np.repeat(np.arange(n), counts)
    nh = gid.shape[0]
    t = rng.integers(0, 24, nh)
    # ascending template index inside a guide == ascending key: sort (guide, template) pairs
    t = np.sort(gid * 24 + t) - gid * 24
    hits = np.empty(nh, dtype=api.HIT_DTYPE)
    hits["key"] = pools[which[gid], t]
    hits["pos"] = _positions(rng, GENOME, 20, 3, nh, near=0.05)
    seqs = np.frombuffer("".join(pool_guides).encode(), dtype=np.uint8).reshape(48, 20)[which].copy()
    return dict(seqs=seqs, offsets=offsets, hits=hits, lengths=list(GENOME), L=20, P=3, start=False, heavy=np.sort(heavy))


def geometry_structures(seed=13):
    """-> [(name, chromosome lengths, indices of the joins to visit)]; join j is the prefix sum of the first j
    chromosomes (0 = the genome's first base, n_chr = its end)"""
    rng = np.random.default_rng(seed)
    many = [int(x) for x in rng.integers(23, 201, 3000)]

    def some(n_chr):
        fixed = [0, 1, 2, 3, n_chr // 2, n_chr - 1, n_chr] + [j for j in (2047, 2048, 2049) if j <= n_chr]
        return sorted(set(fixed) | {int(j) for j in rng.integers(1, n_chr, 8)})

    return [
        ("3000_chromosomes", many, some(3000)),
        ("2048_chromosomes", many[:2048], some(2048)),
        ("2049_chromosomes", many[:2049], some(2049)),
        ("one_chromosome_of_3000", [3000], [0, 1]),
        ("short_ones_between_long", [5_000_000, 23, 22, 1, 61, 3_000_000], list(range(7))),
        ("empty_chromosome_inside", [400, 0, 300, 0, 0, 50, 500], list(range(8))),
        ("beyond_2_to_32", [2 ** 31 + 5] * 3, list(range(4))),
        ("no_chromosome", [], []),
    ]


def build_geometry(lengths, joins, seed=17):
    """one hit per guide: every offset -24..24 around each join, both signs, position 0 and the genome's last.
    The hits alternate between a perfect distance-0 one (kept: 1, dropped: 0) and distance-1..2 ones (kept:
    1 / (1 + CFD), dropped: 1), so each hit's fate shows in its guide's specificity."""
    rng = np.random.default_rng(seed)
    cum = np.concatenate([[0], np.cumsum(np.asarray(lengths, dtype=np.int64))])
    G = int(cum[-1])
    if G:
        ab = {0, G - 1} | {int(cum[j]) + o for j in joins for o in range(-24, 25)}
        ab = sorted(a for a in ab if 0 <= a < G)
        pos = [a for a in ab] + [-a for a in ab if a]
    else:
        pos = [0, 5, -5, 1000, -1000]   # nothing to resolve against: every hit is dropped
    pool_guides = [_guide(rng) for _ in range(8)]
    templates = []
    for g in pool_guides:
        templates.append([_template(rng, g, 0, _ngg_pam(rng, "GG"), 1), _template(rng, g, 1, _ngg_pam(rng, "GG"), 0),
                          _template(rng, g, 2, _ngg_pam(rng, "AG"), 1)])
    guides, per_guide = [], []
    for i, p in enumerate(pos):
        guides.append(pool_guides[i % 8])
        per_guide.append((np.array([templates[i % 8][(i // 8) % 3]], dtype=np.uint64), np.array([p], dtype=np.int64)))
    return _assemble(guides, per_guide, lengths, 3)


def build_shape(L, P, start, seed=19, n_guides=6, per=50):
    """a few hundred hits at distances 0..3 for one (L, P, --start); where position 21 or 22 of the match sequence
    is a guide position, every other guide reads G there"""
    rng = np.random.default_rng(seed + 100 * L + 10 * P + int(start))
    lengths = [20000, 700]
    guides, per_guide = [], []
    for i in range(n_guides):
        g = list(_guide(rng, L))
        if i % 2 == 0 and not start:
            for at in (21, 22):
                if at < L:
                    g[at] = "G"
        g = "".join(g)
        guides.append(g)
        per_guide.append(_random_guide_hits(rng, g, per + i, lengths, P, start, dists=(0, 0, 1, 2, 3), ngg=False))
    return _assemble(guides, per_guide, lengths, P, start)
