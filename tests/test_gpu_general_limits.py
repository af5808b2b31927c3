"""The general search path (gs_general.hip) at its limits against the CPU oracle: a wave that takes a second item, the
record pool's second pass, the stack's room rule, the widths of the packed fields, alt PAMs of their own lengths and
raw hit counts, literal symbols next to bulges on a genome with many BWT runs of N, R and Y, the refusals and the
iteration bound.

Every comparison is, per guide, the full ordered list of (pos, mismatches, index, match.sequence, dna_bulges,
rna_bulges) against oracle_lib; every batch also pins that no item's stack outgrew its 1,024 nodes of LDS
(gs_debug_general_last).  One 60,000-base genome, one handle, one OracleIndex for the whole file."""
import ctypes as C
from importlib import import_module

import numpy as np
import pytest

import oracle_lib as ol
from test_gpu_parity import general_hits_as_records, oracle_general_records

api = import_module("guidescan-cli_amd.api")
synth = import_module("guidescan-cli_amd.synth")

pytestmark = pytest.mark.gpu

GSTACK = 1024                      # nodes of LDS one wave's stack has (gs_general.hip)
ACGT = np.frombuffer(b"ACGT", np.uint8)
FAMILY_AT, FAMILY_EVERY, FAMILY_LEN, FAMILY_COPIES = 1000, 1400, 300, 40
STRETCH_AT, STRETCH_BASES = 58_500, 200
SPARSE_AT, SPARSE_END, SPARSE_EVERY = 56_000, 58_400, 6
PAMS_1_TO_8 = ("N", "NG", "NAG", "NGAN", "NNGRR", "NNNNGA", "NNAGAAW", "NNNNGATT")
ALT31_MIXED = tuple((PAMS_1_TO_8 * 4)[:31])
# 31 three-symbol patterns: with the guides' own PAM the 32 patterns one batch may have (the own one is pamid 31)
ALT31_EQUAL = tuple([f"N{a}{b}" for a in "ACGT" for b in "ACGT"] + [f"{a}NG" for a in "ACGT"] +
                    [f"NN{a}" for a in "ACGT"] + [f"{a}GG" for a in "ACGT"] + ["RGG", "NGR", "NNN"])
assert len(ALT31_MIXED) == 31 and len(ALT31_EQUAL) == 31


def make_world_text():
    """60,000 random bases; a 300-base family planted 40 times (3 % divergence, strands alternating); a literal N every
    977 bases and a literal R every 1,931; one stretch of 200 bases with a single N / R / Y between each two of them;
    behind the stretch a few PAM sites (AGG TGG CGG AGG, then YGG and RGG) so that guides read across its end have
    hits, and a G behind three of its Rs for the pattern NRG.
    In that stretch the suffixes behind the Ys all begin base-N-base-R and sort next to each other, so its 67 Ys make
    only 18 runs of the BWT (N: 76, R: 38 with the periodic ones).  The many runs come from a second, sparse stretch:
    an N / R / Y every sixth symbol over 2,400 bases, each between random bases on both sides."""
    rng = np.random.default_rng(11)
    text = ACGT[rng.integers(0, 4, 60_000)]
    fam = ACGT[rng.integers(0, 4, FAMILY_LEN)]
    for i in range(FAMILY_COPIES):
        c = fam.copy()
        at = rng.choice(FAMILY_LEN, FAMILY_LEN * 3 // 100, replace=False)
        c[at] = ACGT[(np.searchsorted(ACGT, c[at]) + rng.integers(1, 4, at.size)) % 4]
        if i & 1:
            c = synth.reverse_complement_bytes(c)
        text[FAMILY_AT + FAMILY_EVERY * i:FAMILY_AT + FAMILY_EVERY * i + FAMILY_LEN] = c
    text[500::977] = ord("N")
    text[700::1931] = ord("R")
    at = np.arange(SPARSE_AT, SPARSE_END, SPARSE_EVERY)
    text[at] = np.frombuffer(b"NRY", np.uint8)[np.arange(at.size) % 3]
    s = text[STRETCH_AT:STRETCH_AT + 2 * STRETCH_BASES]
    s[0::2] = ACGT[rng.integers(0, 4, STRETCH_BASES)]
    s[1::2] = np.frombuffer(b"NRY", np.uint8)[np.arange(STRETCH_BASES) % 3]
    for k in (10, 40, 70):                     # symbol k of the stretch is an R: base, R, G is a site of NRG
        assert s[2 * k + 1] == ord("R")
        s[2 * k + 2] = ord("G")
    end = STRETCH_AT + 2 * STRETCH_BASES
    text[end:end + 18] = np.frombuffer(b"AGGTGGCGGAGGYGGRGG", np.uint8)
    return np.ascontiguousarray(text)


def bwt_runs(oidx, which, sym):
    """runs of `sym` in the BWT of one strand's text"""
    sa = oidx.sa(which).astype(np.int64)
    t = oidx.text if which == "fwd" else oidx.rtext
    bwt = np.where(sa > 0, t[np.maximum(sa, 1) - 1], 0)
    is_s = bwt == ord(sym)
    return int(is_s[0]) + int(np.count_nonzero(is_s[1:] & ~is_s[:-1]))


class World:
    def __init__(self):
        self.text = make_world_text()
        self.oidx = ol.OracleIndex(self.text)
        self.gidx = api.GenomeIndex.build(self.text, device=0)
        self.is_base = np.isin(self.text, ACGT)
        self._expected = {}

    def close(self):
        self.gidx.close()
        self.oidx.close()

    def planted(self, n, L, P, nwild=0, start=False, pam_tail=b"", first=2000, step=29):
        """n windows of the text whose L + P symbols are all bases -> (guides, pams) as lists of str.  The guide's PAM is
        the text's own with its first nwild symbols made N (with start: the PAM precedes the guide and its last nwild
        symbols become N); pam_tail: only windows whose PAM ends in these symbols"""
        guides, pams, p = [], [], first
        while len(guides) < n:
            assert p + L + P <= self.text.size, "the text has too few such windows"
            w = self.text[p:p + L + P]
            pam = (w[:P] if start else w[L:]).tobytes()
            if self.is_base[p:p + L + P].all() and pam.endswith(pam_tail):
                g = (w[P:] if start else w[:L]).tobytes().decode()
                pam = pam.decode()
                pam = pam[:P - nwild] + "N" * nwild if start else "N" * nwild + pam[nwild:]
                guides.append(g)
                pams.append(pam)
                p += step
            else:
                p += 1
        return guides, pams

    def family(self, n, first=0):
        """consecutive 20-mers of the family's first copy, each followed by that copy's own PAM (first symbol N)"""
        a = FAMILY_AT + first
        return ([self.text[a + j:a + j + 20].tobytes().decode() for j in range(n)],
                ["N" + self.text[a + j + 21:a + j + 23].tobytes().decode() for j in range(n)])

    def expected(self, guides, pams, m=0, rna=0, dna=0, alt=(), start=False):
        """the oracle's records per guide; computed once per batch and configuration, shared among the tests"""
        key = (tuple(guides), tuple(pams), m, rna, dna, tuple(alt), start)
        if key not in self._expected:
            opts = ol.make_opts(mismatches=m, alt_pams=alt, start=start, rna_bulges=rna, dna_bulges=dna)
            self._expected[key] = [oracle_general_records(self.oidx, g, p, opts) for g, p in zip(guides, pams)]
        return self._expected[key]

    def run(self, guides, pams, m=0, rna=0, dna=0, alt=(), start=False, **kw):
        """one general-path call -> what enumerate_general returns; the stack's high-water mark is pinned on the way"""
        seqs = np.array([list(g.encode()) for g in guides], dtype=np.uint8).reshape(len(guides), len(guides[0]))
        P = len(pams[0])
        pam_a = np.array([list(p.encode()) for p in pams], dtype=np.uint8).reshape(len(guides), P)
        res = self.gidx.enumerate_general(seqs, pam_a, mismatches=m, rna_bulges=rna, dna_bulges=dna, alt_pams=alt,
                                          start=start, **kw)
        last = self.gidx.general_last()
        print(f"general_last {len(guides)} guides L={len(guides[0])} P={P} m={m} rna={rna} dna={dna} alts={len(alt)} "
              f"start={start}: items={last[0]} workgroups={last[1]} pool={last[2]} T={last[3]} passes={last[4]} "
              f"stack={last[5]} cut={last[6]} tight={last[7]} hits={int(res[0][-1])}")
        assert last[0] == 2 * len(guides) and 1 <= last[5] <= GSTACK, last
        return res

    def check(self, guides, pams, oracle_alt=None, force_pams=False, **cfg):
        """run the batch and hold every guide's records against the oracle's -> (offsets, hits, expected, general_last)"""
        res = self.run(guides, pams, force_pams=force_pams, **cfg)
        last = self.gidx.general_last()
        exp = self.expected(guides, pams, **(cfg if oracle_alt is None else dict(cfg, alt=oracle_alt)))
        for i in range(len(guides)):
            assert general_hits_as_records(res[0], res[1], i) == exp[i], (i, guides[i], pams[i], cfg)
        return res[0], res[1], exp, last


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.close()


def same(a, b):
    return np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes()


def test_the_world_has_many_runs_of_each_symbol(world):
    """occ_sym's binary search needs lists to search: N, R and Y each head well over 64 runs of the BWT on both strands
    (a workgroup of the run lists' builder is 64 lanes wide, and so is a wave of the search)"""
    for which in ("fwd", "rev"):
        for sym in "NRY":
            assert bwt_runs(world.oidx, which, sym) > 64, (which, sym)


@pytest.mark.parametrize("cfg", [dict(m=1, rna=1), dict(m=2)], ids=["m1-rna1", "m2"])
def test_more_items_than_waves(world, cfg):
    """1,024 planted 20-mers + NGG are 2,048 items for at most 3 workgroups per CU: every wave takes further items, so
    the per-item reset of the stack, of the match count and of the counters decides the result.  The same batch
    reversed gives every guide the same list (another wave, another predecessor on it).
    Oracle: m=1 rna=1 14,807 hits in 0.24 s, m=2 7,098 hits in 0.28 s (the windows inside the family's copies have
    up to 270)."""
    guides, pams = world.planted(1024, 20, 3, nwild=1, pam_tail=b"GG")
    assert set(pams) == {"NGG"}
    off, hits, exp, last = world.check(guides, pams, **cfg)
    assert last[0] == 2048 and last[0] > last[1], last           # items > workgroups
    assert sum(len(e) for e in exp) > 500
    roff, rhits = world.run(guides[::-1], pams[::-1], **cfg)
    n = len(guides)
    for i in range(n):
        a = hits[off[i]:off[i + 1]]
        b = rhits[roff[n - 1 - i]:roff[n - i]]
        assert a.tobytes() == b.tobytes(), i


POOL_CFG = dict(m=3, rna=1, dna=1)


def test_the_pools_second_pass(world):
    """a pool smaller than the batch's records T: the pass counts what did not fit, is run again with room for T, and
    gives the bytes of the one-pass run - at a pool of 1 and of T - 1 records two passes, at T and T + 1 one.
    8 family guides at m=3 rna=1 dna=1: the oracle takes 1.6 s for 47,946 hits."""
    guides, pams = world.family(8)
    off, hits, exp, last = world.check(guides, pams, **POOL_CFG)
    T = last[3]
    assert T > 1000 and off[-1] > 1000 and last[4] == 1 and last[2] == 65536, last   # (T counts intervals, not rows)
    try:
        for pool, passes in ((1, 2), (T - 1, 2), (T, 1), (T + 1, 1)):
            world.gidx.set_option("GS_GENERAL_POOL", pool)
            got = world.run(guides, pams, **POOL_CFG)
            now = world.gidx.general_last()
            assert same(got, (off, hits)), pool
            assert now[2] == pool and now[3] == T and now[4] == passes, (pool, now)
            assert now[5:] == last[5:], (pool, now, last)      # the second pass walks the same tree
    finally:
        world.gidx.set_option("GS_GENERAL_POOL", None)


def test_the_stack_rule_changes_nothing(world):
    """limit = 1,024 - 11 x (L + p_max + max_dna + patterns + 4) nodes: beyond it a pop shrinks to the lanes whose
    children still fit, to one lane when none does.  GS_GENERAL_STACK lowers the limit: at 1 every step pops one node
    (no room at all: word 7), at 11 and 12 the first lane finds room only on an almost empty stack, at 64 pops are cut
    (word 6) - and every run gives the bytes of the run without the option, which equal the oracle.
    Measured on an MI355X, [largest stack, steps cut, steps without room]:
      31 alt PAMs m=4 (limit 320)  unset [237, 12671, 0]    1 and 11 [46, 250436, 250582]   12 [46, 250436, 250436]
                                   64 [72, 93312, 3020]
      m=3 rna=1 dna=1 (limit 705)  unset [653, 288187, 0]   1 and 11 [54, 9210160, 9210320] 12 [54, 9210160, 9210160]
                                   64 [87, 7298627, 2345855]
    A pop of 64 lanes needs 704 free nodes, so without the option the rule already cuts pops (word 6) on every batch of
    this file; what the option adds is the branch without room for one lane's children (word 7), which a natural input
    reaches only in test_31_alt_pams_and_three_dna_bulges_near_the_limit below."""
    fam, fpams = world.family(8)
    for guides, pams, cfg in ((fam, fpams, dict(m=4, alt=ALT31_MIXED)), (fam, fpams, POOL_CFG)):
        off, hits, exp, last = world.check(guides, pams, **cfg)
        try:
            for nodes in (1, 11, 12, 64):
                world.gidx.set_option("GS_GENERAL_STACK", nodes)
                got = world.run(guides, pams, **cfg)
                now = world.gidx.general_last()
                assert same(got, (off, hits)), (nodes, cfg)
                assert now[3] == last[3], (nodes, now, last)
                if nodes == 1:
                    assert now[7] > 0, now
                if nodes == 64:
                    assert now[6] > 0, now
        finally:
            world.gidx.set_option("GS_GENERAL_STACK", None)
        assert same(world.run(guides, pams, **cfg), (off, hits))


def test_31_alt_pams_and_three_dna_bulges_near_the_limit(world):
    """31 alt PAMs + the guides' own at equal length 3 with dna=3: the computed limit is 1,024 - 11 x 62 = 342 nodes,
    the lowest a batch of 20-mers can have; the own pattern is pamid 31, the last value of the 5-bit field.
    Measured on an MI355X (4 family guides, m=1 dna=3; 8 items, 2,161 hits from 4,561 records): largest stack 340 of
    the limit's 342, 54,304 steps whose pop the rule cut, 236 steps without room for one lane's children.  So this
    natural input reaches both branches of the rule without GS_GENERAL_STACK, and both are asserted; the counters are
    sums and a maximum over items, each item's walk is its own, so they do not depend on scheduling.
    The same patterns at m=2 without bulges (limit 375): stack 186, 460 steps cut, none without room."""
    guides, pams = world.family(4)
    off, hits, exp, last = world.check(guides, pams, m=1, dna=3, alt=ALT31_EQUAL)
    assert off[-1] > 0
    assert last[6] > 0 and last[7] > 0, last
    off2, hits2, _, _ = world.check(guides, pams, m=2, alt=ALT31_EQUAL)
    assert off2[-1] > 0


FIELD_CASES = [
    # id, planted(...) arguments, search configuration, least hits over the batch
    ("L21-P8-dna3-m1", dict(n=8, L=21, P=8, nwild=4), dict(m=1, dna=3), 8),
    ("L21-P8-dna3-m0", dict(n=8, L=21, P=8, nwild=4), dict(m=0, dna=3), 8),
    ("L24-P8-m2", dict(n=8, L=24, P=8, nwild=4), dict(m=2), 8),
    ("L28-P4-start-m3", dict(n=8, L=28, P=4, nwild=2, start=True), dict(m=3, start=True), 8),
    ("L31-P0-m3-rna2", dict(n=8, L=31, P=0), dict(m=3, rna=2, alt=("NGG", "NAG")), 8),
    ("L10-P2-m7", dict(n=8, L=10, P=2, nwild=1, pam_tail=b"G"), dict(m=7), 100_000),
]


@pytest.mark.parametrize("case", FIELD_CASES, ids=[c[0] for c in FIELD_CASES])
def test_field_widths_planted(world, case):
    """the packed fields at their last values, 8 planted guides each.  Oracle on this genome:
      L=21 P=8 (NNNN + 4 bases) dna=3 m=1: 95 hits, sequences of 29 to 32 symbols
      L=21 P=8 dna=3 m=0: 32 hits; some hit has seq_len 32 - the last byte of seq[7], no NUL in gs_hit_ex::seq
      L=24 P=8 (NNNN + 4 bases) m=2: 8 hits, every sequence has 32 symbols
      L=28 P=4 --start m=3: 8 hits of 32 symbols, the PAM first
      L=31 P=0 m=3 rna=2: 457 hits in 0.4 s; alt PAMs are passed and dropped (process.hpp:52-53), the oracle runs with
        an empty PAM.  (Found here: gs_enumerate_general_pams counted the dropped patterns' lengths into
        L + dna_bulges + p_max and refused this batch.)
      L=10 P=2 (NG) m=7: the 3-bit field's last value; 107,990 hits in 1.2 s"""
    name, plant, cfg, least = case
    guides, pams = world.planted(**plant)
    ocfg = dict(oracle_alt=()) if plant["P"] == 0 else {}
    off, hits, exp, last = world.check(guides, pams, **cfg, **ocfg)
    assert off[-1] >= least, (name, off[-1])
    longest = max(len(r[3]) for e in exp for r in e)
    if plant["L"] + plant["P"] + cfg.get("dna", 0) == 32:
        assert longest == 32 and int(hits["seq_len"].max()) == 32, (name, longest)
        full = hits[hits["seq_len"] == 32][0]
        assert len(bytes(full["seq"])) == 32 and len(api.decode_sequence_ex(full)) == 32
    if name == "L10-P2-m7":
        assert int(hits["mismatches"].max()) == 7
    if name == "L31-P0-m3-rna2":
        assert int(hits["rna_bulges"].max()) == 2 and longest == 31


@pytest.mark.parametrize("cfg", [dict(m=1, rna=3), dict(m=1, dna=3)], ids=["rna3", "dna3"])
def test_three_bulges_of_one_kind(world, cfg):
    """the 3-bit bulge counts at 3, 4 family guides (oracle: rna=3 1,183 hits, dna=3 688 hits)"""
    guides, pams = world.family(4)
    off, hits, exp, last = world.check(guides, pams, **cfg)
    kind = "rna_bulges" if "rna" in cfg else "dna_bulges"
    assert int(hits[kind].max()) == 3 and off[-1] > 100


# of the family's first 8 guides the one with the fewest hits at m=0 rna=3 dna=3.  Found by running the oracle on each
# of family(8)'s guides once (about 2 s each): 434,229  375,826  394,695  471,031  486,469  427,946  394,443  383,676
LEAST_GUIDE = 1


def test_the_largest_batch_of_records(world):
    """one family guide at m=0 rna=3 dna=3: 375,826 hits (oracle: 2.1 s) from two items - the largest T of this file,
    both bulge fields at 3 at once, duplicates of one sequence in their thousands for the (sequence, row) order and the
    flags to get right."""
    guides, pams = world.family(1, first=LEAST_GUIDE)
    off, hits, exp, last = world.check(guides, pams, m=0, rna=3, dna=3)
    assert off[-1] > 100_000 and last[3] > 10_000, last
    assert int(hits["rna_bulges"].max()) == 3 and int(hits["dna_bulges"].max()) == 3


@pytest.mark.parametrize("start", [False, True], ids=["end", "start"])
@pytest.mark.parametrize("alt", [ALT31_MIXED, ("NG", "NNGRRT", "NAG", "N")], ids=["31-patterns", "4-patterns"])
def test_alt_pams_of_their_own_lengths(world, alt, start):
    """gs_enumerate_general_pams: the PAM stage of pattern j ends after its own symbols (1 to 8 of them), so one guide's
    hits carry sequences of L + 1 ... L + 8 symbols; the oracle searches each alt PAM at its own length"""
    guides, pams = world.family(8)
    if start:
        a = FAMILY_AT + 40                                # the copy's own PAM before the guide, its last symbol N
        guides = [world.text[a + j:a + j + 20].tobytes().decode() for j in range(8)]
        pams = [world.text[a + j - 3:a + j - 1].tobytes().decode() + "N" for j in range(8)]
    off, hits, exp, last = world.check(guides, pams, m=4, alt=alt, start=start)
    lens = {len(r[3]) for e in exp for r in e}
    assert len(lens) >= 3 and off[-1] > 0, lens


def test_equal_lengths_through_the_pams_entry_point(world):
    """with equal lengths gs_enumerate_general_pams gives the bytes of gs_enumerate_general"""
    guides, pams = world.family(8)
    for cfg in (dict(m=3, alt=("NAG", "NGA", "NNG")), dict(m=1, rna=1, dna=1, alt=("NAG",)), dict(m=2)):
        a = world.check(guides, pams, **cfg)
        b = world.check(guides, pams, force_pams=True, **cfg)
        assert same(a, b), cfg


def test_raw_hits_count_what_the_sets_drop(world):
    """gs_result_ex_raw_hits without bulges: raw[g] is the sum, over the patterns of the list, of the oracle's hits for
    guide g with that pattern as its only PAM - one pattern yields no duplicate sequences, and duplicates across
    patterns (NGG next to NNG: every NGG site twice) are exactly what raw counts and the sets drop"""
    guides, pams = world.family(8)
    own = pams
    for alt, m in ((("NNG", "NAG"), 3), (("NG", "NNGRRT", "NAG", "N"), 2), ((), 3)):
        off, hits, raw = world.run(guides, own, m=m, alt=alt, raw=True)
        exp = world.expected(guides, own, m=m, alt=alt)
        for i in range(8):
            assert general_hits_as_records(off, hits, i) == exp[i], (i, alt)
        want = np.zeros(8, dtype=np.int64)
        for pat in alt:
            # as an only PAM a pattern is the guide's own: the oracle takes it per guide
            want += [len(e) for e in world.expected(guides, [pat] * 8, m=m)]
        want += [len(e) for e in world.expected(guides, own, m=m)]
        assert raw.dtype == np.uint32 and raw.tolist() == want.tolist(), (alt, raw, want)
        n_hits = np.diff(off).astype(np.int64)
        assert (raw >= n_hits).all()
        if alt:
            assert (raw > n_hits).any(), alt
        else:
            assert (raw == n_hits).all()


def test_literal_symbols_with_bulges(world):
    """a guide's N and R are charged a mismatch against bases and skipped or passed by a bulge like any other symbol:
    16 planted guides with N written at symbol 3 and R at symbol 11, m=2 rna=1 dna=1 (oracle: 8,327 hits in 0.35 s)"""
    guides, pams = world.planted(16, 20, 3, nwild=1, pam_tail=b"GG")
    guides = [g[:3] + "N" + g[4:11] + "R" + g[12:] for g in guides]
    off, hits, exp, last = world.check(guides, pams, m=2, rna=1, dna=1)
    assert off[-1] > 16
    assert any(r[4] for e in exp for r in e) and any(r[5] for e in exp for r in e)    # both kinds of bulge are there


def stretch_guides():
    end = STRETCH_AT + 2 * STRETCH_BASES
    ends = [end - 1 + 3 * j for j in range(6)]                         # guides read across the stretch's end
    ends += [STRETCH_AT + 2 * k - 1 for k in (10, 40, 70)]             # guides inside it, an NRG site behind them
    ends += [STRETCH_AT + 7, STRETCH_AT + 12]                          # and across its beginning
    return ends


@pytest.mark.parametrize("dna", [0, 1], ids=["no-bulge", "dna1"])
def test_many_runs_of_n_r_and_y(world, dna):
    """guides read across the stretch where every other symbol is an N, an R or a Y: each step of such a guide asks
    occ_sym for a symbol with more than 64 runs, at rows before the first run (lo == 0), inside runs (the d < len clamp)
    and behind the last; own PAM NRG, then NGG next to the alt PAMs RGG and YGG, at m=2"""
    guides = [world.text[e - 19:e + 1].tobytes().decode() for e in stretch_guides()]
    seen = ""
    for own, alt in (("NRG", ()), ("NGG", ("RGG", "YGG"))):
        off, hits, exp, last = world.check(guides, [own] * len(guides), m=2, dna=dna, alt=alt)
        assert off[-1] > 0, (own, alt)
        seen += "".join(r[3] for e in exp for r in e)
    for sym in "NRY":
        assert sym in seen, sym      # upper case in match.sequence: the symbol met itself in the genome


def test_refusals_leave_the_handle_usable(world):
    """what the general path does not hold is refused with GS_ERR_UNSUPPORTED (3) before anything is launched, a NULL
    alt_lens next to alt PAMs with GS_ERR_ARG (1), and the next call on the handle equals the oracle"""
    g20, p3 = world.planted(2, 20, 3, nwild=1, pam_tail=b"GG")

    def still_fine():
        world.check(g20, p3, m=1, rna=1)

    refused = [
        ("L=32", world.planted(2, 32, 0), dict(m=1)),
        ("P=9", world.planted(2, 20, 9, nwild=5), dict(m=1)),
        ("m=8", (g20, p3), dict(m=8)),
        ("32 alt PAMs", (g20, p3), dict(m=1, alt=ALT31_EQUAL + ("NGA",))),
        ("rna=4", (g20, p3), dict(m=1, rna=4)),
        ("dna=4", (g20, p3), dict(m=1, dna=4)),
        ("L+dna+p_max=33", world.planted(2, 24, 8, nwild=4), dict(m=1, dna=1)),
        ("L+dna+p_max=33 by an alt PAM", world.planted(2, 24, 3, nwild=1), dict(m=1, dna=1, alt=("NNNNNNGG",))),
        ("alt_lens holding 0", (g20, p3), dict(m=1, alt=("NG", ""))),
        ("alt_lens holding 9", (g20, p3), dict(m=1, alt=("NGGNGGNGG",))),
    ]
    for name, (guides, pams), cfg in refused:
        with pytest.raises(api.GsError) as e:
            world.run(guides, pams, **cfg)
        assert e.value.status == 3, (name, str(e.value))
        still_fine()
    # n_alt > 0 without alt_lens
    seqs = np.array([list(g.encode()) for g in g20], dtype=np.uint8)
    pam_a = np.array([list(p.encode()) for p in p3], dtype=np.uint8)
    r = C.c_void_p()
    rc = api.lib().gs_enumerate_general_pams(world.gidx._h, seqs.ctypes.data, 2, 20, pam_a.ctypes.data, 3, b"NAG", None, 1,
                                             1, 0, 0, 0, C.byref(r))
    assert rc == 1 and not r.value
    still_fine()


def test_an_empty_batch(world):
    for kw in (dict(), dict(force_pams=True, alt_pams=("NG",))):
        off, hits, raw = world.gidx.enumerate_general(np.empty((0, 20), np.uint8), np.empty((0, 3), np.uint8), mismatches=2,
                                                      rna_bulges=1, raw=True, **kw)
        assert off.tolist() == [0] and hits.size == 0 and raw.size == 0
        assert world.gidx.general_last()[0] == 0


def test_the_iteration_bound_returns_cleanly(world):
    """GS_BULGE_MAX_ITER=3: every item gives up at its fourth step, every wave drains the queue, the call returns
    GS_ERR_DEVICE (2) naming the bound; without the option the same batch equals the oracle again"""
    guides, pams = world.planted(1024, 20, 3, nwild=1, pam_tail=b"GG")
    try:
        world.gidx.set_option("GS_BULGE_MAX_ITER", 3)
        with pytest.raises(api.GsError) as e:
            world.run(guides, pams, m=1, rna=1)
        assert e.value.status == 2 and "exceeded its iteration bound" in str(e.value)
    finally:
        world.gidx.set_option("GS_BULGE_MAX_ITER", None)
    world.check(guides, pams, m=1, rna=1)
