"""The seeded form of the bulge-aware search on the CPU: gs_debug_bulge_seeds and gs_debug_bulge_verify run gb_child
(gs_bulge_step.h), the transition function k_search_bulge runs, and are held here against a Python restatement of the
reference's recursion (include/genomics/index.hpp:250-375 with the PAM stage :125-170), written from that text and
sharing nothing with the library.

Seeds: the restatement walks an index in which every base is present and stops where a path has consumed k genome
symbols; entries (table index, state word, match.sequence so far) are compared as sorted lists, duplicates included.
Two shapes have too many paths for one list: at (L, k) = (20, 14) the budgets (3, 1, 1) and (0, 3, 3) give 6.3 and 11.0
million seeds per guide (the largest of the other 18 lists has 129,780).  There the tree is compared sub-tree by
sub-tree - the paths whose first 10 consumed genome symbols are a given prefix, entry by entry as sorted lists - for the
guide's own prefix, prefixes with one and two substitutions, the prefixes a DNA bulge and an RNA bulge shift, and random
ones (most of which must be empty on both sides); and the library's count of the whole tree is compared with the
restatement's (the same recursion, memoised on its arguments - with every base present the subtree's size depends on
nothing else).  So at these four cases most entries are covered by the count only: 50,000 to 295,000 of the 6 and 11
million are compared entry by entry (walking all of them through the restatement takes a minute per case).  k = 14 puts
the index bits at their widest, and every bit of them is inside some compared entry.

Verification: the restatement runs from the root over a short text through a naive suffix array; the library's side is
every seed of the guide, at every place of the text its k-mer occurs, verified against the 16 symbols before that
place.  Both give (match.sequence, where the match begins, mismatches, dna bulges, rna bulges) per path; compared as
sorted lists, duplicates included."""
import functools
import random
import sys
from importlib import import_module

import pytest

api = import_module("guidescan-cli_amd.api")

sys.setrecursionlimit(10_000)
COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "N": "N"}
CODE = {"A": 0, "C": 1, "G": 2, "T": 3}
ALPHABET = "ATCG"                                   # search_alphabet, index.hpp:31
NONE, DNA, RNA = 0, 1, 2                            # bulge_state


def revcomp(s):
    return "".join(COMP[c] for c in reversed(s))


# ---- the restatement ------------------------------------------------------------------------------------------------
def pam_search(ix, pam, end, node, match, callback):
    """index.hpp:125-170 as process.hpp calls it: no mismatches; 'N' is a literal N, then A,T,C,G at no cost"""
    if end == 0:
        callback(node, match)
        return
    c = pam[end - 1]
    ch = ix.extend(node, c)
    if ch is not None:
        pam_search(ix, pam, end - 1, ch, match + c, callback)
    if c != "N":
        return
    for a in ALPHABET:
        ch = ix.extend(node, a)
        if ch is not None:
            pam_search(ix, pam, end - 1, ch, match + a, callback)


def bulge_search(ix, query, pams, mismatches, max_rna, max_dna, on_match, stop=None):
    """index.hpp:250-375 with max_bulge_size = 1.  aff = (mismatches, dna_bulges, rna_bulges, state, curr_bulge_size);
    stop(node, position, sequence, aff) -> True ends a path before anything else is tried (the seeds' depth)"""
    last = len(query) - 1

    def rec(position, node, sequence, aff):
        if stop is not None and stop(node, position, sequence, aff):
            return
        mm, dna, rna, state, curr = aff
        d = aff
        if max_dna > dna and (state != DNA or curr == 1):
            d = (mm, dna + 1, rna, DNA, 0)
        if d[3] == DNA and d[4] < 1 and position != last:
            d = (d[0], d[1], d[2], DNA, d[4] + 1)
            for a in ALPHABET:
                ch = ix.extend(node, a)
                if ch is not None:
                    rec(position, ch, sequence + a.lower(), d)
        if position < 0:
            for pam in pams:
                pam_search(ix, pam, len(pam), node, sequence, lambda nd, sq: on_match(nd, sq, aff))
            return
        c = query[position]
        ch = ix.extend(node, c)
        if ch is not None:
            rec(position - 1, ch, sequence + c, (mm, dna, rna, NONE, curr))
        if mismatches > mm:
            for a in ALPHABET:
                if a == c:
                    continue
                ch = ix.extend(node, a)
                if ch is not None:
                    rec(position - 1, ch, sequence + a.lower(), (mm + 1, dna, rna, NONE, curr))
        r = aff
        if max_rna > rna and (state != RNA or curr == 1):
            r = (mm, dna, rna + 1, RNA, 0)
        if r[3] == RNA and r[4] < 1 and position != last:
            rec(position - 1, node, sequence + ".", (r[0], r[1], r[2], RNA, r[4] + 1))

    rec(last, ix.root(), "", (0, 0, 0, NONE, 0))


class EveryBase:
    """an index in which every base extends every pattern: a node is the symbols consumed so far, first to last"""

    def root(self):
        return ""

    def extend(self, node, c):
        return node + c if c in CODE else None


class PrefixOnly(EveryBase):
    """the same, restricted to the paths whose first consumed genome symbols are `prefix`"""

    def __init__(self, prefix):
        self.prefix = prefix

    def extend(self, node, c):
        if len(node) < len(self.prefix) and c != self.prefix[len(node)]:
            return None
        return node + c if c in CODE else None


class NaiveIndex:
    """a text behind a sorted list of its suffixes; a node is the pattern matched so far, in text order"""

    def __init__(self, text):
        self.text = text
        self.order = sorted(range(len(text) + 1), key=lambda p: text[p:])     # the empty suffix first, as the sentinel

    def root(self):
        return ""

    def extend(self, node, c):
        pat = c + node
        return pat if pat in self.text else None

    def rows(self, node):
        """where the pattern occurs, in suffix order: the reference's sp..ep loop"""
        return [p for p in self.order if self.text.startswith(node, p)]


def state_word(position, L, aff, seq_len):
    mm, dna, rna, state, curr = aff
    return (L - 1 - position) | mm << 6 | dna << 9 | rna << 12 | state << 15 | curr << 17 | seq_len << 18


def table_index(consumed, k):
    return sum(CODE[c] << (2 * (k - 1 - t)) for t, c in enumerate(consumed))


def the_query(guide, start):
    return guide if start else revcomp(guide)         # process.hpp:63 / 84-87


def restated_seeds(guide, k, m, rna, dna, start, prefix=None):
    out = []

    def stop(node, position, sequence, aff):
        if len(node) < k:
            return False
        out.append((table_index(node, k), state_word(position, len(guide), aff, len(sequence)), sequence.encode()))
        return True

    bulge_search(EveryBase() if prefix is None else PrefixOnly(prefix), the_query(guide, start), [], m, rna, dna, None, stop)
    return out


def restated_seed_count(L, k, m, max_rna, max_dna):
    """the number of paths of the same recursion that consume k genome symbols, every base present"""
    @functools.lru_cache(maxsize=None)
    def rec(position, consumed, mm, dna, rna, state, curr):
        if consumed == k:
            return 1
        total = 0
        d = (dna, state, curr)
        if max_dna > dna and (state != DNA or curr == 1):
            d = (dna + 1, DNA, 0)
        if d[1] == DNA and d[2] < 1 and position != L - 1:
            total += 4 * rec(position, consumed + 1, mm, d[0], rna, DNA, 1)
        if position < 0:
            return total
        total += rec(position - 1, consumed + 1, mm, dna, rna, NONE, curr)
        if m > mm:
            total += 3 * rec(position - 1, consumed + 1, mm + 1, dna, rna, NONE, curr)
        r = (rna, state, curr)
        if max_rna > rna and (state != RNA or curr == 1):
            r = (rna + 1, RNA, 0)
        if r[1] == RNA and r[2] < 1 and position != L - 1:
            total += rec(position - 1, consumed, mm, dna, r[0], RNA, 1)
        return total

    return rec(L - 1, 0, 0, 0, 0, NONE, 0)


def random_guide(L, seed):
    rng = random.Random(seed)
    return "".join(rng.choice("ACGT") for _ in range(L))


PREFIX_LEN = 10


def sub_tree_prefixes(guide, start):
    """the first 10 consumed genome symbols of the sub-trees that are compared entry by entry at k = 14"""
    c = the_query(guide, start)[::-1]                    # the query in consumption order
    other = {"A": "C", "C": "G", "G": "T", "T": "A"}
    own = c[:PREFIX_LEN]
    out = [own]
    out += [own[:i] + other[own[i]] + own[i + 1:] for i in (0, 3, 7)]                     # one substitution
    out += [own[:2] + other[own[2]] + own[3:5] + other[other[own[5]]] + own[6:]]          # two
    out += [c[:i] + x + c[i:PREFIX_LEN - 1] for i, x in ((1, "A"), (4, "G"), (7, "T"))]   # a DNA bulge before step i
    out += [c[:i] + c[i + 1:PREFIX_LEN + 1] for i in (1, 5)]                              # an RNA bulge at step i
    rng = random.Random(5)
    out += ["".join(rng.choice("ACGT") for _ in range(PREFIX_LEN)) for _ in range(4)]
    return list(dict.fromkeys(out))


SHAPES = [(20, 4), (20, 7), (20, 14), (10, 7)]
BUDGETS = [(1, 1, 1), (3, 1, 1), (0, 3, 3), (2, 0, 1), (2, 1, 0)]
LIST_LIMIT = 1_000_000          # entries a list comparison may have


@pytest.mark.parametrize("start", [False, True], ids=["end", "start"])
@pytest.mark.parametrize("budget", BUDGETS, ids=lambda b: "m%d-rna%d-dna%d" % b)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "L%d-k%d" % s)
def test_seeds_against_the_restatement(shape, budget, start):
    (L, k), (m, rna, dna) = shape, budget
    guide = random_guide(L, 100 * L + k)
    want_n = restated_seed_count(L, k, m, rna, dna)
    if want_n > LIST_LIMIT:
        assert (shape, budget) in (((20, 14), (3, 1, 1)), ((20, 14), (0, 3, 3))), want_n      # the two named above
        assert api.bulge_seeds(guide, k, m, rna, dna, start=start, count_only=True) == want_n
        entries = 0
        for prefix in sub_tree_prefixes(guide, start):
            value = table_index(prefix, len(prefix))
            got = api.bulge_seeds(guide, k, m, rna, dna, start=start, prefix_len=len(prefix), prefix=value)
            want = restated_seeds(guide, k, m, rna, dna, start, prefix=prefix)
            assert sorted(zip(got["index"].tolist(), got["state"].tolist(), got["seq"].tolist())) == sorted(want), prefix
            assert all(i >> (2 * (k - len(prefix))) == value for i in got["index"].tolist())
            entries += len(want)
        print("entries compared", entries)
        assert entries > 20_000, entries
        return
    got = api.bulge_seeds(guide, k, m, rna, dna, start=start)
    want = restated_seeds(guide, k, m, rna, dna, start)
    assert len(want) == want_n
    assert sorted(zip(got["index"].tolist(), got["state"].tolist(), got["seq"].tolist())) == sorted(want)


def test_seed_arguments_are_checked():
    import ctypes as C
    n = C.c_uint64(0)
    L_ = api.lib()
    assert L_.gs_debug_bulge_seeds(b"ACGTNACGTA", 10, 4, 1, 0, 0, 0, 0, 0, None, 0, C.byref(n)) == 1      # a guide with an N
    assert L_.gs_debug_bulge_seeds(b"ACGTAACGTA", 10, 8, 1, 3, 0, 0, 0, 0, None, 0, C.byref(n)) == 1      # L - rna < k
    assert L_.gs_debug_bulge_seeds(b"ACGTAACGTA", 10, 7, 1, 3, 0, 0, 0, 0, None, 0, C.byref(n)) == 0      # L - rna == k
    assert L_.gs_debug_bulge_seeds(b"ACGTAACGTA", 10, 7, 1, 0, 0, 0, 8, 0, None, 0, C.byref(n)) == 1      # a prefix longer than k
    assert L_.gs_debug_bulge_seeds(b"ACGTAACGTA", 10, 7, 1, 0, 0, 0, 2, 16, None, 0, C.byref(n)) == 1     # a prefix beyond its length


# ---- verification ---------------------------------------------------------------------------------------------------
def nibble(c):
    return CODE[c] if c in CODE else 4 if c == "N" else 5


def context_nibbles(text, p):
    """the 16 symbols before text[p], nearest first; 6 before the text start"""
    return sum((nibble(text[p - j]) if p >= j else 6) << (4 * (j - 1)) for j in range(1, 17))


def restated_matches(text, guide, pam, alts, m, rna, dna, start):
    ix = NaiveIndex(text)
    pams = [the_query(a, start) for a in alts] + [the_query(pam, start)]      # process.hpp:51-56: alt PAMs first
    out = []
    bulge_search(ix, the_query(guide, start), pams, m, rna, dna,
                 lambda node, seq, aff: out.extend((seq.encode(), p, aff[0], aff[1], aff[2]) for p in ix.rows(node)))
    return out


def seeded_matches(text, guide, pam, alts, k, m, rna, dna, start):
    out = []
    memo = {}
    for s in api.bulge_seeds(guide, k, m, rna, dna, start=start):
        idx = int(s["index"])
        # consumption step t at bits 2(k-1-t); the text holds the consumed symbols last to first
        kmer = "".join("ACGT"[(idx >> (2 * t)) & 3] for t in range(k))
        p = text.find(kmer)
        while p >= 0:
            key = (int(s["state"]), bytes(s["seq"]), p)
            if key not in memo:
                memo[key] = api.bulge_verify(s["state"], s["seq"], context_nibbles(text, p), guide, pam, k, alt_pams=alts,
                                             mismatches=m, rna_bulges=rna, dna_bulges=dna, start=start)
            for r in memo[key]:
                st = api.bulge_state(r["state"])
                out.append((bytes(r["seq"]), p - int(r["consumed"]), st["mismatches"], st["dna_bulges"], st["rna_bulges"]))
            p = text.find(kmer, p + 1)
    return out


GUIDE = "GATTACAGGCTTAACGTCCA"                       # consumed as its reverse complement TGGACGTTAAGCCTGTAATC, right to left
SITE = revcomp(GUIDE)


def site(pam_text, body=SITE):
    """a site as the searched text shows it: the pattern's symbols, then the query"""
    return pam_text + body


def check(text, k, m, rna, dna, pam="NGG", alts=(), guide=GUIDE, start=False, least=1):
    L = len(guide)
    p_max = max(len(p) for p in (pam,) + tuple(alts))
    assert L - rna >= k and L + dna + p_max - k <= 16, "the shape is not eligible for the seeded form"
    want = restated_matches(text, guide, pam, alts, m, rna, dna, start)
    got = seeded_matches(text, guide, pam, alts, k, m, rna, dna, start)
    assert len(want) >= least, (len(want), least)
    assert sorted(got) == sorted(want)
    return want


def test_contexts_of_bases_only():
    """an exact site, one with a substitution near the PAM, one with a genome base too many and one with a base missing,
    in one text: each kind of step is verified from the context"""
    sub = SITE[:3] + "A" + SITE[4:]
    extra = SITE[:5] + "T" + SITE[5:]
    missing = SITE[:6] + SITE[7:]
    text = "ACGT" + site("CCA") + "TT" + site("CCT", sub) + "GA" + site("CCG", extra) + "AC" + site("CCC", missing) + "G"
    want = check(text, 8, 1, 1, 1, least=4)             # (with a DNA bulge and P = 3, 20-mers need k >= 8)
    assert any(r[3] for r in want) and any(r[4] for r in want) and any(r[2] for r in want)
    check(text, 7, 2, 1, 0, least=3)
    check(text, 8, 3, 1, 1, least=4)


def test_sixteen_symbols_needed_exactly():
    """L + dna + p_max - k == 16: the match's last symbol is the context's sixteenth"""
    text = "T" + site("CCA") + "ACGTAC" + site("CCG", SITE[:2] + "G" + SITE[3:])
    want = check(text, 7, 2, 1, 0, least=2)
    assert max(len(r[0]) - r[0].count(b".") for r in want) == 23
    check(text, 8, 2, 1, 1, least=2)                    # 20 + 1 + 3 - 8
    check(text, 7, 1, 0, 0, pam="NGG", alts=("NAG",), least=1)


def test_a_literal_n_under_the_patterns_n_and_under_a_fixed_symbol():
    """index.hpp:139-149: the pattern's N meets a literal N of the text (upper case N in match.sequence); under a
    fixed PAM symbol or a guide symbol an N matches nothing"""
    text = "AC" + site("CCN") + "GT" + site("CNA") + "TG" + site("NCA") + "CA" + site("CCA", SITE[:1] + "N" + SITE[2:]) + "A"
    want = check(text, 8, 1, 1, 1, least=1)
    assert any(r[0].endswith(b"NCC") for r in want)     # match.sequence is written in consumption order
    assert not any(b"N" in r[0][:-3] or b"N" in r[0][-2:] for r in want)
    want = check(text, 8, 1, 0, 1, pam="NNN", least=3)
    assert any(r[0].endswith(b"NCC") or r[0].endswith(b"ANC") or r[0].endswith(b"ACN") for r in want)


@pytest.mark.parametrize("other", ["X", None], ids=["another-symbol", "the-text-start"])
def test_other_symbols_and_the_text_start_inside_and_just_beyond(other):
    """a symbol outside A,C,G,T,N, or the text's start, just beyond the symbols a match reads (the match stands) and one
    symbol nearer (it does not)"""
    lead = other or ""
    beyond = lead + site("CCA")                         # the match reads up to the symbol after `lead`
    want = check(beyond + "GATC", 8, 1, 1, 1, least=1)
    assert any(r[1] == len(lead) for r in want)
    inside = lead + site("CA")                          # its PAM's last symbol would be `lead`
    text = inside + "GATC" + ("X" + site("CCA") if other is None else "")
    want = check(text, 7, 1, 0, 0, least=0)
    assert not any(r[1] <= len(lead) for r in want)
    # a DNA bulge needs one symbol more: the site that stood without bulges still stands, its bulged variants do not
    want = check(beyond + "GATC", 8, 0, 0, 1, least=1)
    assert all(r[3] == 0 for r in want if r[1] <= len(lead))


@pytest.mark.parametrize("pam,alts,k", [("NGG", (), 7), ("NNN", (), 7), ("N", (), 7), ("NNGAA", (), 10),
                                        ("NGG", ("NAG", "N", "NNGAA", "GG", "TNGA"), 10)],
                         ids=["NGG", "NNN", "N", "NNGAA", "mixed-lengths"])
def test_patterns(pam, alts, k):
    """own patterns of 1, 3 and 5 symbols, and alt PAMs of 1 to 5 symbols next to NGG: every pattern's PAM stage ends
    after its own symbols"""
    text = ("A" + site("TTCAG") + "C" + site("GTCCA") + "G" + site("ACTCC", SITE[:4] + "C" + SITE[5:]) + "T" +
            site("TCAT") + "A")
    want = check(text, k, 1, 1, 1 if k == 10 else 0, pam=pam, alts=alts, least=1)
    if alts:
        assert len({len(r[0]) for r in want}) >= 3


def test_pam_at_the_start():
    """--start: the query is the guide itself and the patterns are read as written (process.hpp:84-87)"""
    text = "AC" + "TGG" + GUIDE + "GT" + "AAG" + GUIDE[:9] + "T" + GUIDE[10:] + "CC"
    want = check(text, 8, 1, 1, 1, pam="NGG", alts=("NAG",), start=True, least=2)
    assert any(r[0].endswith(b"GGT") for r in want)     # consumption order: the guide from its end, then the PAM from its end
