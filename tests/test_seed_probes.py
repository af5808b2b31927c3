"""The probe lists of the two seeding launches (gs_seed.hip) against the recipes they are made from.  A recipe's digit d at a
step whose guide symbol is qc used to mean "the d-th other base counted cyclically from qc" (k_search_body still reads it so);
the seeding launches read it as "the base qc ^ (d + 1)", under which a recipe's effect on the table index is one constant
for every guide (gs_kernels.h: gs_recipe_delta, gs_probe_a, gs_probe_b).  The lists enumerate all three digits at every
substituted step, so both rules must name the SAME probes per item - checked here as multisets, per guide, against a plain
Python reading of the recipe words under the old rule - and a hit's path (gs_seed_path, the new rule) must spell exactly
the substitutions of the k-mer its probe read (index.hpp:230-247: a substitution is recorded as the text base's place among
the three other bases).  Host only: the entry points run the functions the kernels run."""
import random
from importlib import import_module

import numpy as np
import pytest

api = import_module("guidescan-cli_amd.api")

P = 3
PSG, PSP = 57, 56   # path bits: guide symbol t's code at PSG - 2 t, PAM symbol u's at PSP - 2 L - 3 u
SHAPES = [(20, 14, 8), (20, 13, 9), (23, 14, 11)]   # (L, k, |X|)
BUDGETS = [1, 2, 3, 4]
N_GUIDES = 50


def thresholds(L, k, nx, m):
    """a*(o) as a batch with PAM-pair and deep tables plans them (gs_enumerate.hip: plan_thresholds)"""
    return [int(x) for x in api.choose_thresholds(m, nx, k - nx, L - k, 1.0, 0.4, 1.6)]


def guides(L, seed):
    rng = random.Random(seed)
    return [[rng.randrange(4) for _ in range(L)] for _ in range(N_GUIDES)]


def fields(words):
    """(step, digit) of the seven fields of every recipe word, as two (n, 7) arrays"""
    f = np.stack([(words >> np.uint64(12 + 7 * i)) & np.uint64(127) for i in range(7)], axis=1).astype(np.int64)
    return f >> 2, f & 3


def old_rule_index(words, own, q_at_step, nst):
    """the table index a recipe probes for one guide under the cyclic digit rule: own index ^ one xor per field, the field's
    digit d standing for the base (qc + 1 + d) & 3 (3: an unused field, nothing); step s lies at bits 2 (nst - 1 - s)"""
    s, d = fields(words)
    qc = np.asarray(q_at_step, dtype=np.int64)[np.minimum(s, nst - 1)]
    x = np.where(d == 3, 0, (qc ^ ((qc + 1 + d) & 3)) << (2 * (nst - 1 - np.minimum(s, nst - 1))))
    return own ^ np.bitwise_xor.reduce(x, axis=1)


def rot_py(idx, k, rs):
    """the copy rotated at step rs: that step's symbol and everything after it swap places (numpy arrays or ints)"""
    sh = 2 * (k - 1 - rs)
    return ((idx >> (sh + 2)) << (sh + 2)) | ((idx & ((1 << sh) - 1)) << 2) | ((idx >> sh) & 3)


def unrot_py(ridx, k, rs):
    sh = 2 * (k - 1 - rs)
    return ((ridx >> (sh + 2)) << (sh + 2)) | ((ridx & 3) << sh) | ((ridx >> 2) & ((1 << sh) - 1))


def pack(copy, idx, cnt, lo):
    return np.sort((copy.astype(np.uint64) << np.uint64(40)) | (idx.astype(np.uint64) << np.uint64(6)) |
                   (cnt.astype(np.uint64) << np.uint64(3)) | lo.astype(np.uint64))


def rot_firsts(words):
    """31 (a table without rotated copies), the lowest step the list names, and one in between (a table that dropped some)"""
    named = (words[(words & np.uint64(64)) != 0] >> np.uint64(7)) & np.uint64(31)
    if named.size == 0:
        return [31]
    lo, hi = int(named.min()), int(named.max())
    return sorted({31, lo, (lo + hi + 1) // 2})


def a_probe_indices(pr, q, k, rf):
    """(copy, index in that copy) of every probe of this strand's list for guide q"""
    pidx0 = sum(q[t] << (2 * (k - 1 - t)) for t in range(k))
    copy = ((pr[:, 1] >> 4) & 15).astype(np.int64)
    own = np.full(copy.shape, pidx0, dtype=np.int64)
    for c in np.unique(copy):
        if c:
            own[copy == c] = rot_py(pidx0, k, rf + int(c) - 1)
    return copy, own ^ pr[:, 0].astype(np.int64)


@pytest.mark.parametrize("m", BUDGETS)
@pytest.mark.parametrize("L,k,nx", SHAPES)
def test_same_probes_this_strand(L, k, nx, m):
    astar = thresholds(L, k, nx, m)
    for trimmed in (False, True):
        words = api.seed_recipes_a8(k, m, nx, astar, trimmed=trimmed)
        cnt, lo = (words & np.uint64(7)).astype(np.int64), ((words >> np.uint64(3)) & np.uint64(7)).astype(np.int64)
        rs = ((words >> np.uint64(7)) & np.uint64(31)).astype(np.int64)
        for rf in rot_firsts(words):
            pr = api.seed_probes(k, L, P, m, nx, astar, 2 if trimmed else 1, rot_first=rf)
            assert pr.shape[0] == words.shape[0]
            assert np.array_equal((pr[:, 1] >> 14) & 7, pr[:, 1] & 7) and not (pr[:, 1] & ~np.uint32(0x1C0F7)).any()
            rot = ((words & np.uint64(64)) != 0) & (rs >= rf)
            assert rf == 31 or rot.any()
            for q in guides(L, 1000 * L + 10 * k + m):
                pidx0 = sum(q[t] << (2 * (k - 1 - t)) for t in range(k))
                idx = old_rule_index(words, pidx0, q[:k], k)
                idx = np.where(rot, rot_py(idx, k, np.where(rot, rs, k - 1)), idx)   # rotation applied afterwards
                want = pack(np.where(rot, rs - rf + 1, 0), idx, cnt, lo)
                copy, pidx = a_probe_indices(pr, q, k, rf)
                got = pack(copy, pidx, (pr[:, 1] & 7).astype(np.int64), np.zeros_like(copy))
                assert np.array_equal(want, got), (trimmed, rf)


@pytest.mark.parametrize("m", BUDGETS)
@pytest.mark.parametrize("L,k,nx", SHAPES)
def test_same_probes_other_strand(L, k, nx, m):
    astar = thresholds(L, k, nx, m)
    words = api.seed_recipes(k, L, P, m, nx, astar, deep=True)[2]
    pr = api.seed_probes(k, L, P, m, nx, astar, 0)
    assert pr.shape[0] == words.shape[0]
    nst = L - nx
    cnt, lo = (words & np.uint64(7)).astype(np.int64), ((words >> np.uint64(3)) & np.uint64(7)).astype(np.int64)
    assert not (pr[:, 1] & ~np.uint32((7 << 27) | (7 << 14) | 7)).any() and np.array_equal((pr[:, 1] >> 14) & 7, pr[:, 1] & 7)
    for q in guides(L, 2000 * L + 10 * k + m):
        # step y consumes guide symbol L-1-y; the deep table holds the complements, the xor of two bases stays what it was
        pidxg = sum((3 - q[L - 1 - y]) << (2 * (nst - 1 - y)) for y in range(nst))
        want = pack(np.zeros_like(cnt), old_rule_index(words, pidxg, [q[L - 1 - y] for y in range(nst)], nst), cnt, lo)
        got = pack(np.zeros_like(cnt), pidxg ^ pr[:, 0].astype(np.int64), (pr[:, 1] & 7).astype(np.int64),
                   ((pr[:, 1] >> 27) & 7).astype(np.int64))
        assert np.array_equal(want, got)


def code(text_sym, q_sym):
    """index.hpp:230-247: nothing where the text shows the guide's base, else the text base's place among the other three"""
    return 0 if text_sym == q_sym else 1 + text_sym - (1 if text_sym > q_sym else 0)


@pytest.mark.parametrize("m", BUDGETS)
@pytest.mark.parametrize("L,k,nx", SHAPES)
def test_path_agrees_with_index_this_strand(L, k, nx, m):
    astar = thresholds(L, k, nx, m)
    words = api.seed_recipes_a8(k, m, nx, astar)
    rf = rot_firsts(words)[0]
    pr = api.seed_probes(k, L, P, m, nx, astar, 1, rot_first=rf)
    rng = random.Random(7 * L + k + m)
    for q in guides(L, 3000 * L + 10 * k + m):
        qw = sum(s << (2 * t) for t, s in enumerate(q))
        copy, pidx = a_probe_indices(pr, q, k, rf)
        for i in rng.sample(range(len(words)), min(200, len(words))):
            plain = int(pidx[i]) if copy[i] == 0 else unrot_py(int(pidx[i]), k, rf + int(copy[i]) - 1)
            kmer = [(plain >> (2 * (k - 1 - t))) & 3 for t in range(k)]
            want = sum(code(kmer[t], q[t]) << (PSG - 2 * t) for t in range(k))   # nothing beyond the k-mer, no PAM field
            path, delta = api.seed_path(qw, int(words[i]), L, P, k, sid=i)
            assert path == want, (i, hex(path), hex(want))
            assert sum(1 for t in range(k) if kmer[t] != q[t]) == int(words[i]) & 7
            assert delta == plain ^ sum(q[t] << (2 * (k - 1 - t)) for t in range(k))


@pytest.mark.parametrize("m", BUDGETS)
@pytest.mark.parametrize("L,k,nx", SHAPES)
def test_path_agrees_with_index_other_strand(L, k, nx, m):
    astar = thresholds(L, k, nx, m)
    words = api.seed_recipes(k, L, P, m, nx, astar, deep=True)[2]
    pr = api.seed_probes(k, L, P, m, nx, astar, 0)
    nst = L - nx
    rng = random.Random(11 * L + k + m)
    for q in guides(L, 4000 * L + 10 * k + m):
        qw = sum(s << (2 * t) for t, s in enumerate(q))
        pidxg = sum((3 - q[L - 1 - y]) << (2 * (nst - 1 - y)) for y in range(nst))
        pams = [[rng.choice([0, 1, 2, 3, 4])] + [rng.randrange(4) for _ in range(P - 1)] for _ in range(4)]
        pam_words = [sum(c << (3 * u) for u, c in enumerate(pw)) for pw in pams]
        for i in rng.sample(range(len(words)), min(200, len(words))):
            idx = pidxg ^ int(pr[i, 0])
            # the entry's symbol for step y is the complement of the text base at guide position L-1-y
            text = {L - 1 - y: 3 - ((idx >> (2 * (nst - 1 - y))) & 3) for y in range(nst)}
            want = sum(code(text[t], q[t]) << (PSG - 2 * t) for t in text)   # nothing in X (guide positions below |X|)
            bx, pj = rng.randrange(4), rng.randrange(4)
            tb = 3 - bx   # entry bx of a deep-table line: the (complemented) base under the pattern's N
            want |= (tb if tb < 3 else 4) << (PSP - 2 * L)
            for u in range(1, P):
                want |= (pams[pj][u] if pams[pj][u] < 3 else 4) << (PSP - 2 * L - 3 * u)
            path, delta = api.seed_path(qw, int(words[i]), L, P, nst, side_b=True, sid=i | (bx << 24) | (pj << 26), pams=pam_words)
            assert path == want, (i, hex(path), hex(want))
            assert sum(1 for t in text if text[t] != q[t]) == int(words[i]) & 7
            assert delta == int(pr[i, 0])


@pytest.mark.parametrize("k", [13, 14, 16])
def test_rotation_is_linear(k):
    rng = random.Random(k)
    for rs in range(k - 1):
        for _ in range(200):
            a, b = rng.randrange(1 << (2 * k)), rng.randrange(1 << (2 * k))
            ra, rb = api.rot_index(a, k, rs), api.rot_index(b, k, rs)
            assert api.rot_index(a ^ b, k, rs) == ra ^ rb
            assert ra == rot_py(a, k, rs) & 0xFFFFFFFF and unrot_py(ra, k, rs) == a
