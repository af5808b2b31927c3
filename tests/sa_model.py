"""The suffix-array verifier's rules (gs_index_verify_sa: k_v_permutation, k_v_full, k_v_order in gs_verify.hip) restated in
numpy, from the header's and the kernels' statement of them.  TEST INFRASTRUCTURE: no GPU, no library; what the GPU reports
are compared with, field by field (tests/test_gpu_verify_sa.py), and itself checked against sorted() and exhaustively on
small texts (tests/test_sa_model.py).

A report is the dict GenomeIndex.verify_sa returns: rows, not_permutation, sampled, out_of_order, undecided, bwt_mismatch.

 * text: the FORWARD genome text (uint8, no sentinel) the array is checked against; strand 1 means its reverse complement
   (A<->T, C<->G, a<->t, c<->g, every other byte as it is: k_v_revcomp, as the index's k_revcomp), and `sa` is then that strand's array.
 * built_text: the forward text the index was BUILT from, where that is another one (same length).  The index keeps two
   things of it that the verifier reads: the BWT symbol class of every row (built_text[sa[r] - 1]: A, C, G, T, or "extra"
   for every other byte and for the sentinel), and the list of its runs of 'N', by which sampled mode skips.
"""
import numpy as np

N = ord("N")
MAX_STEPS = 1 << 16      # k_v_order: pairs still equal after this many comparison steps are `undecided`
_MASK = (1 << 64) - 1


def as_text(s):
    return np.frombuffer(s.encode() if isinstance(s, str) else bytes(s), dtype=np.uint8).copy()


_COMPLEMENT = np.arange(256, dtype=np.uint8)
for _a, _b in ("AT", "TA", "CG", "GC", "at", "ta", "cg", "gc"):
    _COMPLEMENT[ord(_a)] = ord(_b)
_CLASS = np.full(256, 4, dtype=np.int64)      # A, C, G, T -> 0..3; every other byte, the sentinel included -> 4 ("extra")
for _i, _b in enumerate(b"ACGT"):
    _CLASS[_b] = _i


def base_text(seed=7, n=40_000):
    """the text the verifier's tests share: random ACGT with a run of 300 N, a tandem repeat (period 5 x 2,000 copies), a
    dozen R / Y bytes and 5 N at the very end"""
    rng = np.random.default_rng(seed)
    t = as_text("ACGT")[rng.integers(0, 4, n)]
    t[5_000:5_300] = N
    t[12_000:22_000] = np.tile(as_text("ACGTT"), 2_000)
    for i, p in enumerate(rng.choice(np.arange(23_000, 39_000), 12, replace=False)):
        t[p] = ord("RY"[i & 1])
    t[-5:] = N
    return t


def reverse_complement(text):
    """k_v_revcomp: the text backwards, A<->T and C<->G in either case, the rest unchanged"""
    return _COMPLEMENT[np.asarray(text, dtype=np.uint8)[::-1]]


def strand_text(text, strand):
    """the strand's text with the 0 sentinel after it (n = len + 1 bytes)"""
    t = np.asarray(text, dtype=np.uint8)
    if strand:
        t = reverse_complement(t)
    return np.concatenate([t, np.zeros(1, np.uint8)])


def suffix_array(text):
    """suffix array of text + 0 sentinel (int64[n]) by prefix doubling: rows ordered by (rank of the first k symbols, rank
    of the next k), k = 1, 2, 4, ... until every rank is its own.  The sentinel is unique and smallest; a suffix that has
    no symbol k further on gets -1 there (never reached once the sentinel has told it apart, kept for plainness)."""
    t = np.concatenate([np.asarray(text, dtype=np.uint8), np.zeros(1, np.uint8)]).astype(np.int64)
    n = t.shape[0]
    rank = t
    k = 1
    while True:
        nxt = np.full(n, -1, dtype=np.int64)
        nxt[:n - k] = rank[k:]
        sa = np.lexsort((nxt, rank))                    # by rank, ties by nxt
        differs = (rank[sa][1:] != rank[sa][:-1]) | (nxt[sa][1:] != nxt[sa][:-1])
        new = np.empty(n, dtype=np.int64)
        new[sa] = np.concatenate([[0], np.cumsum(differs)])
        rank = new
        if rank.max() == n - 1:
            return np.argsort(rank).astype(np.int64)
        k *= 2


def bitmap_count(sa, n):
    """k_v_permutation: rows whose value is out of range or was seen before (which of two equal rows is 'before' depends
    on the order the threads arrive in; the count does not)"""
    sa = np.asarray(sa).astype(np.int64)
    ok = sa[(sa >= 0) & (sa < n)]
    return int(sa.shape[0] - ok.shape[0]) + int(ok.shape[0] - np.unique(ok).shape[0])


def _bwt_mismatch(t, b, sa, rows):
    """rows (all with sa[r] in range) whose block symbol - the class of b[sa[r] - 1], the sentinel for sa[r] = 0 - is not
    the class of t[sa[r] - 1]"""
    p = sa[rows]
    n = t.shape[0]
    prev = np.where(p > 0, p - 1, n - 1)
    return int((_CLASS[b[prev]] != _CLASS[t[prev]]).sum())


def every_row_report(text, sa, built_text=None, strand=0):
    """gs_index_verify_sa(n_samples = GS_VERIFY_ALL_ROWS): k_v_permutation + k_v_full.

    not_permutation: the bitmap count + rows r with isa[sa[r]] != r, isa the inverse of the given sa (what the index holds).
    out_of_order: pairs (r, r+1) that fail  text[sa[r]] < text[sa[r+1]], or equal symbols (not the sentinel) and
        isa[sa[r]+1] < isa[sa[r+1]+1];  a value out of range, or the same value twice in a pair, counts as well.
    bwt_mismatch: over ALL rows, row n-1 included."""
    t = strand_text(text, strand)
    b = t if built_text is None else strand_text(built_text, strand)
    n = t.shape[0]
    sa = np.asarray(sa).astype(np.int64)
    assert sa.shape == (n,) and b.shape == (n,)
    rows = np.arange(n)
    inr = (sa >= 0) & (sa < n)
    isa = np.full(n + 1, -1, dtype=np.int64)
    isa[sa[inr]] = rows[inr]
    not_inverse = int((isa[sa[inr]] != rows[inr]).sum())
    pa, pb = sa[:-1], sa[1:]
    ooo = int((~inr).sum())                              # (a row out of range is counted and nothing of it is read)
    both = inr[:-1] & inr[1:] & (pa != pb)
    ooo += int((inr[:-1] & ~both).sum())
    pa, pb = pa[both], pb[both]
    ca, cb = t[pa], t[pb]
    # (equal and not the sentinel: neither is the last suffix, so pa + 1 and pb + 1 are positions)
    tie_bad = (ca == 0) | (pa + 1 >= n) | (pb + 1 >= n) | ~(isa[np.minimum(pa + 1, n)] < isa[np.minimum(pb + 1, n)])
    ooo += int(((ca > cb) | ((ca == cb) & tie_bad)).sum())
    return dict(rows=n, not_permutation=bitmap_count(sa, n) + not_inverse, sampled=n - 1, out_of_order=ooo, undecided=0,
                bwt_mismatch=_bwt_mismatch(t, b, sa, rows[inr]))


def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & _MASK
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & _MASK
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & _MASK
    return x ^ (x >> 31)


def sampled_rows(n, samples, seed):
    """k_v_order's rows: sample i looks at pair (r, r+1), r = i*stride + splitmix64(i ^ seed) % stride clamped to n-2,
    stride = (n-1) // samples (at least 1).  With samples < n-1 the last (n-1) mod samples pairs are beyond every sample's
    stride and never looked at; with samples = n-1 the rows are 0 .. n-2, every pair once."""
    samples = min(samples, n - 1)
    stride = max((n - 1) // samples, 1) if samples else 1
    return [min(i * stride + splitmix64(i ^ seed) % stride, n - 2) for i in range(samples)]


def run_left(b):
    """left[p]: symbols of the run of 'N' of b that holds p, at or after p (0: b[p] is not 'N') - v_run_left over the
    index's run list"""
    left = np.zeros(b.shape[0] + 1, dtype=np.int64)
    for p in np.flatnonzero(b == N)[::-1]:
        left[p] = left[p + 1] + 1
    return left[:-1]


def walk_pair(t, left, x, y, step, limit):
    """k_v_order's loop over the suffixes at x and y from comparison step `step` up to `limit` steps: ('ok' | 'bad', ...)
    once a step decides (x's suffix is the smaller one: ok), else (None, x, y, limit) - where the walk stands.  Inside
    runs of 'N' both advance by min(left[x], left[y]) in ONE step when that exceeds 1.  t: the strand's bytes + sentinel."""
    while step < limit:
        cx, cy = t[x], t[y]
        if cx != cy:                      # (the sentinel is the smallest byte: reaching it first is being smaller)
            return ("bad" if cx > cy else "ok"), x, y, step
        if cx == 0:                       # both at the sentinel: the same suffix twice
            return "bad", x, y, step
        adv = 1
        if cx == N:
            m = min(left[x], left[y])
            if m > 1:
                adv = m
        x += adv
        y += adv
        step += 1
    return None, x, y, step


def compare_pair(t, left, x, y, max_steps=MAX_STEPS):
    """'ok', 'bad', or 'undecided' after max_steps steps"""
    return walk_pair(t, left, x, y, 0, max_steps)[0] or "undecided"


def next_special(tn):
    """nxt[p]: the first position at or after p that holds 'N' or the sentinel"""
    special = np.flatnonzero((tn == N) | (tn == 0))
    return special[np.searchsorted(special, np.arange(tn.shape[0]))]


def compare_pair_long(t, tn, nxt, left, x, y, max_steps=MAX_STEPS):
    """compare_pair for pairs thousands of symbols alike, the same answer (tests/test_sa_model.py holds the two against each
    other): the first 32 steps by walk_pair; after them, stretches of equal symbols that are neither 'N' nor the sentinel -
    one step per symbol - are taken a slice at a time, and every other position is one step of walk_pair.
    tn: t as a uint8 array, nxt: next_special(tn)."""
    how, x, y, step = walk_pair(t, left, x, y, 0, min(32, max_steps))
    chunk = 256
    while how is None and step < max_steps:
        k = int(min(chunk, max_steps - step, nxt[x] - x, nxt[y] - y))
        stop = np.flatnonzero(tn[x:x + k] != tn[y:y + k])
        j = int(stop[0]) if stop.size else k
        x, y, step = x + j, y + j, step + j
        if j == k and k == chunk:
            chunk = min(chunk * 4, 1 << 16)
        elif step < max_steps:            # a difference, an 'N' or the sentinel: one step of the loop itself
            how, x, y, step = walk_pair(t, left, x, y, step, step + 1)
    return how or "undecided"


def direct_report(text, sa, samples, seed, built_text=None, strand=0, max_steps=MAX_STEPS, plain=False):
    """gs_index_verify_sa(n_samples = samples): k_v_permutation + k_v_order.

    Per sample: a pair with a value out of range or the same value twice is out of order; else the BWT symbol of row r (r
    only: row n-1 is never a sample's r, so its symbol is never looked at in this mode) and the walk of compare_pair.
    The run list is the BUILT text's.  plain=True: every walk by compare_pair itself."""
    t = strand_text(text, strand)
    b = t if built_text is None else strand_text(built_text, strand)
    n = t.shape[0]
    sa = np.asarray(sa).astype(np.int64)
    assert sa.shape == (n,) and b.shape == (n,)
    samples = min(samples, n - 1)
    left = run_left(b).tolist()
    tb, nxt = t.tobytes(), next_special(t)
    rep = dict(rows=n, not_permutation=bitmap_count(sa, n), sampled=samples, out_of_order=0, undecided=0, bwt_mismatch=0)
    prev = np.where(sa > 0, sa - 1, n - 1) % n            # (rows out of range are never looked up below)
    differs = _CLASS[b[prev]] != _CLASS[t[prev]]
    for r in sampled_rows(n, samples, seed):
        assert r != n - 1
        pa, pb = int(sa[r]), int(sa[r + 1])
        if not (0 <= pa < n and 0 <= pb < n) or pa == pb:
            rep["out_of_order"] += 1
            continue
        rep["bwt_mismatch"] += int(differs[r])
        how = compare_pair(tb, left, pa, pb, max_steps) if plain else compare_pair_long(tb, t, nxt, left, pa, pb, max_steps)
        rep["out_of_order"] += how == "bad"
        rep["undecided"] += how == "undecided"
    return rep
