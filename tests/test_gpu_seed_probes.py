"""The two seeding launches read their probes from guide-independent lists (gs_recipes.hip: gs_probes_attach; the digit of a
recipe stands for the base qc ^ (d + 1)), the one launch keeps the recipes' own rule: on guides that are KNOWN mutants of
sampled sites - every single substitution of 40 sites, 600 double and 600 triple ones: every step and every base on both
sides, the rotated copies of the PAM-pair tables included - the three forms return the same bytes, and every mutant finds
its source site at a distance equal to the substitutions made, spelled as the site's own sequence (index.hpp:182-248: the
recursion whose matches these are; 230-247: how a substitution is recorded).  Once more on a handle whose PAM-pair tables
were built without rotated copies (the list of this strand's probes depends on the copies a table holds).
chr1-sized genome: the smallest at which the seeding form runs (deep tables need a table depth of 13)."""
import re
from importlib import import_module

import numpy as np
import pytest

api = import_module("guidescan-cli_amd.api")
synth = import_module("guidescan-cli_amd.synth")

pytestmark = pytest.mark.gpu

L, P = 20, 3
N_SITES, N_DOUBLE, N_TRIPLE = 40, 600, 600
_form0 = {}   # the one launch's answer on the module's handle, computed by whichever test needs it first


@pytest.fixture(scope="module")
def chr1():
    text, names, lengths = synth.make_genome([synth.CHR1_LENGTH], seed=1)
    gidx = api.GenomeIndex.build(text, device=0)
    yield text, gidx
    gidx.close()


@pytest.fixture(scope="module")
def mutants(chr1):
    """(seqs, pams, source site of each guide, substitutions made): the 40 sites themselves, then their mutants"""
    text, _ = chr1
    sites, pams, _, _ = synth.sample_guides(text, N_SITES, seed=2024, L=L)
    rng = np.random.Generator(np.random.PCG64(5))
    bases = np.frombuffer(b"ACGT", np.uint8)
    seqs, src, nsub = [s.copy() for s in sites], list(range(N_SITES)), [0] * N_SITES
    for i in range(N_SITES):   # all 60 single substitutions of each site
        for t in range(L):
            for b in bases:
                if b != sites[i, t]:
                    g = sites[i].copy()
                    g[t] = b
                    seqs.append(g)
                    src.append(i)
                    nsub.append(1)
    for n, s in ((N_DOUBLE, 2), (N_TRIPLE, 3)):
        for _ in range(n):
            i = int(rng.integers(N_SITES))
            g = sites[i].copy()
            for t in rng.choice(L, size=s, replace=False):
                g[t] = rng.choice(bases[bases != sites[i, t]])
            seqs.append(g)
            src.append(i)
            nsub.append(s)
    seqs = np.stack(seqs)
    assert seqs.shape[0] == N_SITES * 61 + N_DOUBLE + N_TRIPLE
    return seqs, np.tile(pams[0], (seqs.shape[0], 1)), np.array(src), np.array(nsub)


def run(gidx, seqs, pams, form):
    gidx.set_option("GS_SEED_FORM", str(form))
    off, hits, _ = gidx.enumerate(seqs, pams, mismatches=3)
    return off, hits, gidx.last_sharing()["form"]


def form0(chr1, mutants):
    if not _form0:
        _, gidx = chr1
        try:
            off, hits, f = run(gidx, mutants[0], mutants[1], 0)
        finally:
            gidx.set_option("GS_SEED_FORM", None)
        assert f == 0
        _form0["off"], _form0["hits"] = off, hits
    return _form0["off"], _form0["hits"]


def copies_built(err):
    return [int(x) for x in re.findall(r"PAM-pair table: strand \d, pair \d+ at context depth \d+: .*?rows, (\d+) rotated copies", err)]


def assert_sources_found(seqs, src, nsub, off, hits):
    """every guide's hits hold its source site - the position and strand of the site's own exact hit - at the distance of the
    substitutions made, and the hit spells the site's sequence"""
    for g in range(seqs.shape[0]):
        i = int(src[g])
        own = [h for h in hits[off[i]:off[i + 1]] if int(h["key"]) >> 61 == 0]
        assert own, i
        guide, site = seqs[g].tobytes().decode(), seqs[i].tobytes().decode()
        mine = hits[off[g]:off[g + 1]]
        for o in own:
            same = [h for h in mine if h["pos"] == o["pos"] and (int(h["key"]) >> 60) & 1 == (int(o["key"]) >> 60) & 1]
            assert len(same) == 1, (g, i, len(same))
            assert int(same[0]["key"]) >> 61 == int(nsub[g]), (g, int(same[0]["key"]) >> 61, int(nsub[g]))
            # (match.sequence shows a substituted base in lower case: exactly the positions this guide was changed at)
            spelled, exact = api.decode_sequence(guide, P, int(same[0]["key"])), api.decode_sequence(site, P, int(o["key"]))
            assert spelled.upper() == exact, (g, spelled, exact)
            assert [c.islower() for c in spelled[:L]] == [a != b for a, b in zip(guide, site)], (g, spelled, guide, site)


def test_mutants_of_sampled_sites_through_all_three_forms(chr1, mutants, capfd):
    _, gidx = chr1
    seqs, pams, src, nsub = mutants
    gidx.set_options(GS_SEED_SORT_FROM="1", GS_DEBUG="1")
    try:
        capfd.readouterr()
        off0, hits0 = form0(chr1, mutants)
        built = copies_built(capfd.readouterr().err)
        assert built == [] or min(built) > 0, built   # (built by this batch if by no earlier one: then with rotated copies)
        assert_sources_found(seqs, src, nsub, off0, hits0)
        for form in (1, 2):
            off, hits, f = run(gidx, seqs, pams, form)
            assert f == 3, f   # the two seeding launches ran
            assert np.array_equal(off0, off) and hits0.tobytes() == hits.tobytes(), form
    finally:
        gidx.set_options(GS_SEED_SORT_FROM=None, GS_SEED_FORM=None, GS_DEBUG=None)


def test_pair_tables_without_rotated_copies(chr1, mutants, capfd):
    """a cap on the index's bytes that leaves room for the PAM-pair tables of GG but for none of their rotated copies
    (gs_pairtab_ensure's ladder), set ahead of the handle's first NGG batch and lifted after it: the tables stay as built"""
    text, gidx0 = chr1
    seqs, pams, src, nsub = mutants
    off0, hits0 = form0(chr1, mutants)
    k = L + 2 - gidx0.last_launch()["x_len"]   # (deep tables: |X| = L - (k - 2))
    n = int(text.shape[0]) + 1
    plain = 2 * 8 * 4 ** k + 10 * 1.5 * 2 * n / 16 + 8 * 4 ** k + 64e6   # both strands' tables, their row arrays, the build's scratch
    gidx = api.GenomeIndex.build(text, device=0)
    try:
        gidx.set_options(GS_DEBUG="1", GS_SEED_SORT_FROM="1", GS_PAIRTAB_RESERVE_GB="0",
                         GS_INDEX_BUDGET_GB=f"{(gidx.device_bytes + plain + 8 * 4 ** k) / 1e9:.9f}")   # half a copy's worth to spare
        capfd.readouterr()
        off, hits, f = run(gidx, seqs[:N_SITES], pams[:N_SITES], 2)
        err = capfd.readouterr().err
        assert copies_built(err) == [0, 0], err
        gidx.set_options(GS_INDEX_BUDGET_GB=None, GS_PAIRTAB_RESERVE_GB=None)
        for form in (1, 2):
            off, hits, f = run(gidx, seqs, pams, form)
            assert f == 3, f
            assert copies_built(capfd.readouterr().err) == []   # no table was built again
            assert np.array_equal(off0, off) and hits0.tobytes() == hits.tobytes(), form
        assert_sources_found(seqs, src, nsub, off, hits)
    finally:
        gidx.close()
