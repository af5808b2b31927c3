"""The seeded form of the bulge-aware search (gs_bulge.hip, GS_BULGE_FORM=1) against the CPU oracle and against the
walk: seeds from the strand tables at three table depths, row nodes verified by context, interval nodes walked, the
exception rows (literal N, other symbols, both ends of the text), the eligibility rules and the routing of a mixed
batch, the iteration bound, and the command line's --bulge-form.

Every comparison is, per guide, the full ordered list of (pos, mismatches, index, match.sequence, dna_bulges,
rna_bulges) against oracle_lib, and whole-array equality of offsets, hits and raw counts with the same call under
GS_BULGE_FORM=0 on the same handle.  One 60,000-base genome (test_gpu_general_limits.make_world_text with a site
planted 5 symbols from each end of the text), handles at the default table depth (k = 7) and at GS_PREFIX_K = 4 and 10,
one OracleIndex for the whole file.

Shapes.  The seeded form needs L + dna_bulges + p_max - k <= 16 and L - rna_bulges >= k.  20-mers with a 3-symbol PAM
are eligible at k = 7 without DNA bulges and at k = 10 with up to 3; the family batches that run at all three depths
with 3 bulges of each kind use the family's 14-mers (14 + 3 + 3 - 4 = 16, 14 - 3 = 11 >= 10)."""
import ctypes as C
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor
from importlib import import_module

import numpy as np
import pytest

import oracle_lib as ol
from test_gpu_general_limits import ALT31_EQUAL, FAMILY_AT, GSTACK, make_world_text
from test_gpu_parity import general_hits_as_records

api = import_module("guidescan-cli_amd.api")

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", np.uint8)
CLI = ol.ROOT / "guidescan-cli_amd" / "bin" / "guidescan"
END_SITE = b"GCTTAGACCTGATTCAGGCATGG"          # a 20-mer and its PAM, planted 5 symbols from each end of the text
GSO_HIT_DTYPE = np.dtype([(n, np.dtype(t)) if not hasattr(t, "_length_") else (n, "S48") for n, t in ol.GsoHit._fields_])
assert GSO_HIT_DTYPE.itemsize == C.sizeof(ol.GsoHit)
ROWS_DEFAULT = 8                              # GS_BULGE_ROWS when it is not set (gs_bulge_step.h)


def make_text():
    text = make_world_text().copy()
    site = np.frombuffer(END_SITE, np.uint8)
    text[5:5 + site.size] = site
    text[text.size - 5 - site.size:text.size - 5] = site
    return np.ascontiguousarray(text)


def build_handle(text, k=None):
    """a handle reads the environment once, when it is made"""
    saved = os.environ.get("GS_PREFIX_K")
    if k is not None:
        os.environ["GS_PREFIX_K"] = str(k)
    try:
        return api.GenomeIndex.build(text, device=0)
    finally:
        if saved is None:
            os.environ.pop("GS_PREFIX_K", None)
        else:
            os.environ["GS_PREFIX_K"] = saved


class World:
    def __init__(self):
        self.text = make_text()
        self.oidx = ol.OracleIndex(self.text)
        self.h = {7: build_handle(self.text), 4: build_handle(self.text, 4), 10: build_handle(self.text, 10)}
        self.is_base = np.isin(self.text, ACGT)
        self._expected = {}
        self._walked = {}

    def close(self):
        for h in self.h.values():
            h.close()
        self.oidx.close()

    def planted(self, n, L, P, nwild=0, start=False, pam_tail=b"", first=2000, step=29):
        """n windows of the text whose L + P symbols are all bases -> (guides, pams); the guide's PAM is the text's own
        with its first nwild symbols made N (with start: the PAM precedes the guide, its last nwild symbols become N)"""
        guides, pams, p = [], [], first
        while len(guides) < n:
            assert p + L + P <= self.text.size, "the text has too few such windows"
            w = self.text[p:p + L + P]
            pam = (w[:P] if start else w[L:]).tobytes()
            if self.is_base[p:p + L + P].all() and pam.endswith(pam_tail):
                pam = pam.decode()
                guides.append((w[P:] if start else w[:L]).tobytes().decode())
                pams.append(pam[:P - nwild] + "N" * nwild if start else "N" * nwild + pam[nwild:])
                p += step
            else:
                p += 1
        return guides, pams

    def family(self, n, L=20):
        """consecutive L-mers of the family's first copy, each followed by that copy's own PAM (first symbol N)"""
        a = FAMILY_AT
        return ([self.text[a + j:a + j + L].tobytes().decode() for j in range(n)],
                ["N" + self.text[a + j + L + 1:a + j + L + 3].tobytes().decode() for j in range(n)])

    def expected(self, guides, pams, m=0, rna=0, dna=0, alt=(), start=False):
        """the oracle's records per guide as lists of tuples (oracle_general_records' form)"""
        off, arr = self.expected_arrays(guides, pams, m=m, rna=rna, dna=dna, alt=alt, start=start)
        return [general_hits_as_records(off, arr, i) for i in range(len(guides))]

    def expected_arrays(self, guides, pams, m=0, rna=0, dna=0, alt=(), start=False):
        """-> (offsets, the oracle's records of the whole batch in the hits' layout); computed once per batch and
        configuration and shared among the tests.  The records are oracle_general_records' (gso_enumerate's output,
        every row, in its order), taken over as arrays: the family's batches have 1.6 million of them, and every run is
        held against all of them, in order"""
        key = (tuple(guides), tuple(pams), m, rna, dna, tuple(alt), start)
        if key not in self._expected:
            opts = ol.make_opts(mismatches=m, alt_pams=alt, start=start, rna_bulges=rna, dna_bulges=dna)
            def one(gp):
                g, p = gp
                out, ctr = C.POINTER(ol.GsoHit)(), ol.GsoCounters()
                n = ol.lib().gso_enumerate(self.oidx.fwd, self.oidx.rev, self.oidx.length, g.encode(), p.encode(),
                                           C.byref(opts), C.byref(out), C.byref(ctr))
                assert n >= 0
                raw = np.frombuffer(C.string_at(out, n * C.sizeof(ol.GsoHit)), dtype=GSO_HIT_DTYPE) if n else \
                    np.zeros(0, dtype=GSO_HIT_DTYPE)
                ol.lib().gso_free(out)
                arr = np.zeros(n, dtype=api.HIT_EX_DTYPE)
                for f in ("pos", "mismatches", "index", "dna_bulges", "rna_bulges"):
                    arr[f] = raw[f]
                # the sequence is a C string: it ends at its first NUL, whatever the buffer holds behind it
                b = np.ascontiguousarray(raw["sequence"]).view(np.uint8).reshape(n, 48).copy()
                end = np.where((b == 0).any(axis=1), (b == 0).argmax(axis=1), 48)
                assert n == 0 or int(end.max()) <= 32
                b[np.arange(48)[None, :] >= end[:, None]] = 0
                arr["seq"] = np.ascontiguousarray(b[:, :32]).view("S32").reshape(n)
                arr["seq_len"] = end
                return arr

            # (the oracle's index is read-only and gso_enumerate keeps its state on its stack - gso_enumerate_batch runs it from
            # threads the same way; ctypes releases the interpreter lock for the call)
            with ThreadPoolExecutor(8) as pool:
                parts = list(pool.map(one, zip(guides, pams)))
            offsets = np.concatenate(([0], np.cumsum([len(a) for a in parts]))).astype(np.uint64)
            self._expected[key] = (offsets, np.concatenate(parts))
        return self._expected[key]

    def call(self, h, guides, pams, m=0, rna=0, dna=0, alt=(), start=False):
        seqs = np.array([list(g.encode()) for g in guides], dtype=np.uint8).reshape(len(guides), len(guides[0]))
        P = len(pams[0])
        pam_a = np.array([list(p.encode()) for p in pams], dtype=np.uint8).reshape(len(guides), P)
        return h.enumerate_general(seqs, pam_a, mismatches=m, rna_bulges=rna, dna_bulges=dna, alt_pams=alt, start=start,
                                   raw=True)

    def walked(self, k, guides, pams, pool=None, **cfg):
        """the same call under GS_BULGE_FORM=0 on the same handle; once per handle and batch"""
        key = (k, tuple(guides), tuple(pams), tuple(sorted(cfg.items())))
        if key not in self._walked:
            h = self.h[k] if not isinstance(k, tuple) else k[1]
            h.set_option("GS_BULGE_FORM", 0)
            h.set_option("GS_GENERAL_POOL", pool)
            try:
                self._walked[key] = self.call(h, guides, pams, **cfg)
                assert h.bulge_last()[:2] == [0, len(guides)]
            finally:
                h.set_option("GS_BULGE_FORM", None)
                h.set_option("GS_GENERAL_POOL", None)
        return self._walked[key]

    def check(self, k, guides, pams, rows=None, handle=None, pool=None, **cfg):
        """the batch under GS_BULGE_FORM=1 on the handle of depth k (rows: GS_BULGE_ROWS; pool: GS_GENERAL_POOL, the
        records the first pass's pool holds - a batch that outgrows the guess is searched twice) against the oracle and
        against the walk -> (offsets, hits, raw, bulge_last)"""
        h = handle or self.h[k]
        h.set_option("GS_BULGE_FORM", 1)
        h.set_option("GS_BULGE_ROWS", rows)
        h.set_option("GS_GENERAL_POOL", pool)
        try:
            off, hits, raw = self.call(h, guides, pams, **cfg)
            last = h.bulge_last()
            passes = h.general_last()[4]
        finally:
            h.set_option("GS_BULGE_FORM", None)
            h.set_option("GS_BULGE_ROWS", None)
            h.set_option("GS_GENERAL_POOL", None)
        self.passes = passes
        print(f"bulge_last k={k} rows={rows} {len(guides)} guides L={len(guides[0])} {cfg}: seeded={last[0]} walked={last[1]} "
              f"seeds={last[2]} empty={last[3]} row_nodes={last[4]} interval_nodes={last[5]} exc={last[6]} stack={last[7]} "
              f"hits={int(off[-1])}")
        assert last[0] + last[1] == len(guides) and last[7] <= GSTACK, last
        eoff, earr = self.expected_arrays(guides, pams, **cfg)
        assert np.array_equal(off, eoff), (cfg, off, eoff)
        for f in api.HIT_EX_DTYPE.names:                  # every record of every guide, in order, field by field
            assert np.array_equal(hits[f], earr[f]), (f, cfg)
        woff, whits, wraw = self.walked((k, h) if handle else k, guides, pams, pool=pool, **cfg)
        assert np.array_equal(off, woff) and hits.tobytes() == whits.tobytes() and np.array_equal(raw, wraw), (k, cfg)
        return off, hits, raw, last


@pytest.fixture(scope="module")
def world():
    w = World()
    yield w
    w.close()


def test_more_items_than_waves(world):
    """1,024 planted 20-mers + NGG, m=1 rna=1, at the default depth: 2,048 items for at most 3 workgroups per CU, so
    every wave takes further items and the per-item reset of the stack and of the counters decides the result"""
    guides, pams = world.planted(1024, 20, 3, nwild=1, pam_tail=b"GG")
    off, hits, raw, last = world.check(7, guides, pams, m=1, rna=1)
    assert last[0] == 1024 and last[1] == 0 and last[2] > 0, last
    assert off[-1] > 500


def kmer_rows(world, which, kmer):
    """rows of the strand's suffix array that begin with kmer"""
    t = (world.oidx.text if which == "fwd" else world.oidx.rtext).tobytes()
    n, at = 0, t.find(kmer)
    while at >= 0:
        n, at = n + 1, t.find(kmer, at + 1)
    return n


@pytest.mark.parametrize("cfg", [dict(m=3, rna=1, dna=1), dict(m=0, rna=3, dna=3)], ids=["m3-rna1-dna1", "m0-rna3-dna3"])
@pytest.mark.parametrize("k", [4, 7, 10])
def test_family_at_three_depths_and_three_thresholds(world, k, cfg):
    """8 family 14-mers: GS_BULGE_ROWS=0 makes every seed an interval node, 1,000,000 makes every seed a chain of row
    nodes, 1 sends only the single-row seeds to the context; the result is the oracle's and the walk's each time"""
    guides, pams = world.family(8, L=14)
    results, passes = {}, {}
    for rows in (0, 1, 1_000_000):
        # the batch outgrows the guessed pool of 65,536 records and would be searched twice each time: the run at
        # rows=1 does that (the seeded form's second pass), the others and the walk get room for every record at once
        off, hits, raw, last = world.check(k, guides, pams, rows=rows, pool=None if rows == 1 else 1 << 23, **cfg)
        passes[rows] = world.passes
        assert last[0] == 8 and last[1] == 0 and last[2] > last[3] and (k < 10 or last[3] > 0), last
        if rows == 0:
            assert last[4] == 0 and last[5] == last[2] - last[3], last
        if rows == 1_000_000:
            assert last[5] == 0 and last[4] >= last[2] - last[3], last
        if rows == 1:
            assert last[5] > 0 and (k == 4 or last[4] > 0), last
        results[rows] = last
    assert results[0][2] == results[1][2] == results[1_000_000][2]        # the seeds do not depend on the threshold
    assert off[-1] > 100 and passes[0] == passes[1_000_000] == 1 and passes[1] == (2 if off[-1] > 65536 else passes[1]), passes
    if k == 4:
        # the family's own 4-mers head intervals beyond the default threshold: at the default some seeds are walked
        comp = str.maketrans("ACGT", "TGCA")
        for g in guides:                 # the first four symbols a guide consumes, as either strand's text shows them
            for kmer in (g[:4], g[:4].translate(comp)[::-1], g[-4:], g[-4:].translate(comp)[::-1]):
                assert min(kmer_rows(world, which, kmer.encode()) for which in ("fwd", "rev")) > ROWS_DEFAULT
        if cfg["m"] == 3:                # (one batch is enough to see it; the other has 1.6 million hits)
            off, hits, raw, last = world.check(k, guides, pams, **cfg)
            assert last[5] > 0, last


def test_pam_at_the_start(world):
    guides, pams = world.planted(16, 20, 3, nwild=1, start=True, pam_tail=b"")
    off, hits, raw, last = world.check(7, guides, pams, m=1, rna=1, start=True)
    assert last[0] == 16 and off[-1] >= 16
    off, hits, raw, last = world.check(10, guides, pams, m=1, rna=1, dna=1, start=True)
    assert last[0] == 16 and int(hits["dna_bulges"].max()) == 1


ALT31_ACGTN = tuple(p for p in ALT31_EQUAL if set(p) <= set("ACGTN"))
ALT31_ACGTN = (ALT31_ACGTN + ("ANN", "CNN", "TNN", "GNN", "NAN", "NCN"))[:31]


def test_31_alt_pams_of_three_symbols(world):
    """31 alt PAMs over A,C,G,T,N next to the guides' own: the own pattern is pamid 31, the last value of the field"""
    assert len(ALT31_ACGTN) == 31 and len(set(ALT31_ACGTN)) == 31
    guides, pams = world.family(4)
    off, hits, raw, last = world.check(7, guides, pams, m=2, rna=1, alt=ALT31_ACGTN)
    assert last[0] == 4 and off[-1] > 100
    assert (raw > np.diff(off)).any()                  # patterns that overlap: raw counts what the sets drop


def test_alt_pams_of_lengths_one_to_five(world):
    """the PAM stage of a pattern ends after its own symbols; the longest decides the eligibility (20 + 1 + 5 - 10)"""
    guides, pams = world.family(8)
    alt = ("N", "NG", "NAG", "NGAN", "NNGAA", "TNGA", "GG")
    off, hits, raw, last = world.check(10, guides, pams, m=2, rna=1, dna=1, alt=alt)
    assert last[0] == 8
    exp = world.expected(guides, pams, m=2, rna=1, dna=1, alt=alt)
    assert len({len(r[3]) for e in exp for r in e}) >= 5


@pytest.mark.parametrize("own", ["NGG", "NNN"])
def test_guides_across_the_literal_n_sites(world, own):
    """guides whose PAM lies over a literal N of the text (one every 977 symbols), on both strands: the rows there are
    exception rows, an N under the pattern's N matches and an N under a fixed symbol or a guide symbol does not"""
    guides = []
    for at in range(500 + 977, 500 + 977 * 12, 977):
        assert world.text[at] == ord("N")
        for a in (at - 20, at - 21, at - 22, at + 3, at + 2, at + 1):        # the N at each place of the PAM, either strand
            w = world.text[a:a + 20]
            if world.is_base[a:a + 20].all():
                g = w.tobytes().decode()
                guides.append(g if a < at else g.translate(str.maketrans("ACGT", "TGCA"))[::-1])
    assert len(guides) >= 32
    off, hits, raw, last = world.check(7, guides, [own] * len(guides), m=1, rna=1)
    assert last[0] == len(guides) and last[6] > 0, last
    exp = world.expected(guides, [own] * len(guides), m=1, rna=1)
    if own == "NNN":
        assert any("N" in r[3] for e in exp for r in e)         # a literal N under the pattern's N


def test_the_sites_at_the_texts_ends(world):
    """the site 5 symbols from the text's start and the one 5 from its end: on one strand or the other the context of
    their rows runs off the text, with and without a DNA bulge that asks for one symbol more"""
    g = END_SITE[:20].decode()
    rc = g.translate(str.maketrans("ACGT", "TGCA"))[::-1]
    guides = [g, rc, g[1:] + "A", "T" + g[:-1]]
    for k, cfg in ((7, dict(m=2, rna=1)), (10, dict(m=2, rna=1, dna=1)), (10, dict(m=1, dna=3))):
        off, hits, raw, last = world.check(k, guides, ["NGG"] * 4, **cfg)
        assert last[0] == 4 and last[6] > 0, last
        exp = world.expected(guides, ["NGG"] * 4, **cfg)
        assert sum(1 for r in exp[0] if r[1] == 0 and r[4] == 0 and r[5] == 0) == 2        # the two planted sites


def test_eligibility_context(world):
    """L + dna + p_max - k: 16 is seeded, 17 walks - 21-mers with a 2-symbol PAM at k = 10 with dna=3, then with one
    3-symbol alt PAM next to it"""
    guides, pams = world.planted(8, 21, 2, nwild=1)
    off, hits, raw, last = world.check(10, guides, pams, m=1, dna=3)
    assert last[:2] == [8, 0], last
    off, hits, raw, last = world.check(10, guides, pams, m=1, dna=3, alt=("NAG",))
    assert last[:2] == [0, 8], last


def test_eligibility_seeds_in_the_guide_stage(world):
    """L - rna == k is seeded, k + 1 walks: 10-mers with rna=3 at k = 7 and on a handle of depth 8"""
    guides, pams = world.planted(8, 10, 3, nwild=1, pam_tail=b"GG")
    off, hits, raw, last = world.check(7, guides, pams, m=0, rna=3)
    assert last[:2] == [8, 0] and last[2] > 0, last
    h8 = build_handle(world.text, 8)
    try:
        off, hits, raw, last = world.check(8, guides, pams, handle=h8, m=0, rna=3)
        assert last[:2] == [0, 8], last
    finally:
        h8.close()


def test_eligibility_patterns_and_guides(world):
    """a pattern with an R makes the whole batch walk; a batch of 6 guides over A,C,G,T and 2 with an N is split 6 / 2
    and its result is the oracle's, guide by guide in the batch's order"""
    guides, pams = world.planted(8, 20, 3, nwild=1, pam_tail=b"GG")
    off, hits, raw, last = world.check(7, guides, pams, m=1, rna=1, alt=("RGG",))
    assert last[:2] == [0, 8], last
    off, hits, raw, last = world.check(7, guides, ["NRG"] * 8, m=1, rna=1)
    assert last[:2] == [0, 8], last
    mixed = list(guides)
    mixed[2] = mixed[2][:5] + "N" + mixed[2][6:]
    mixed[7] = "N" + mixed[7][1:]
    off, hits, raw, last = world.check(7, mixed, pams, m=1, rna=1)
    assert last[:2] == [6, 2] and last[2] > 0, last
    assert all(off[i + 1] > off[i] for i in range(8))


def test_the_iteration_bound_returns_cleanly(world):
    """GS_BULGE_MAX_ITER=1000 on the family batch: every item gives up, every wave drains the queue, the call returns
    GS_ERR_DEVICE (2) naming the bound; without the option the next call on the handle is correct"""
    guides, pams = world.family(8, L=14)
    h = world.h[7]
    h.set_option("GS_BULGE_MAX_ITER", 1000)
    try:
        with pytest.raises(api.GsError) as e:
            world.check(7, guides, pams, m=3, rna=1, dna=1)
        assert e.value.status == 2 and "exceeded its iteration bound" in str(e.value)
        assert h.bulge_last()[0] == 8
    finally:
        h.set_option("GS_BULGE_MAX_ITER", None)
    world.check(7, guides, pams, m=3, rna=1, dna=1)


CLI_RUNS = {
    "m1_csv_rna1": ["-m", "1", "--rna-bulges", "1"],
    "m1_csv_dna1": ["-m", "1", "--dna-bulges", "1"],
    "m1_csv_dna1_nag_start": ["-m", "1", "--dna-bulges", "1", "-a", "NAG", "--start"],
}


@pytest.fixture(scope="module")
def indexed(toy, tmp_path_factory):
    d = tmp_path_factory.mktemp("cli_bulge")
    subprocess.run([str(CLI), "index", "--index", str(d / "toy"), str(toy["dir"] / "toy.fa")], check=True, timeout=120)
    return d


@pytest.mark.parametrize("name", sorted(CLI_RUNS))
def test_cli_bulge_forms_write_the_references_bytes(toy, indexed, name):
    """`guidescan enumerate --bulge-form seeded` and `walk` write the reference's file byte for byte; GS_PREFIX_K=8 keeps
    20-mers with a 3-symbol PAM and one DNA bulge eligible (20 + 1 + 3 - 8 = 16), and the GS_DEBUG line names the form"""
    ref = (toy["dir"] / f"ref_{name}.csv").read_bytes()
    env = dict(os.environ, GS_PREFIX_K="8", GS_DEBUG="1")
    for form in ("seeded", "walk"):
        out = indexed / f"{name}.{form}.csv"
        r = subprocess.run([str(CLI), "enumerate", str(indexed / "toy"), "-f", str(toy["dir"] / "kmers.csv"), "-o", str(out),
                            "-n", "1", "--bulge-form", form] + CLI_RUNS[name], check=True, timeout=300, env=env,
                           stderr=subprocess.PIPE, text=True)
        assert out.read_bytes() == ref, form
        lines = [ln for ln in r.stderr.splitlines() if "bulge search: form" in ln]
        assert lines and (any("form seeded" in ln for ln in lines) if form == "seeded" else all("form walk" in ln for ln in lines)), lines
