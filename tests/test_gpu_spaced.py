"""The spaced tables of the seeding launches (gs_pairtab.hip, gs_seed.hip): the sites without a substitution in X and with
the whole budget inside O come from ONE lookup per item keyed on (X, R) instead of from the class's recipes.  The bytes
must not depend on it: every case is compared with the same handle's seeding launches without the lookup
(GS_SEED_SPACED=0) and with k_search's one launch (GS_SEED_FORM=0), the in-library reference.

On a chr1-sized genome, the smallest at which deep tables - and with them the seeding launches - exist: table depth 13,
|X| = 9, |O| = 4, |R| = 7, so the key has 32 bits and the class 12 .. 108 recipes; GS_SPACED_FROM=1 takes the path for
every budget.  (Search order reproduced: index.hpp:182-248; PAM list: process.hpp:51-63.)"""
from importlib import import_module

import numpy as np
import pytest

api = import_module("guidescan-cli_amd.api")
synth = import_module("guidescan-cli_amd.synth")

pytestmark = pytest.mark.gpu

L, P = 20, 3
CODE = np.full(256, 255, np.uint8)
CODE[list(b"ACGT")] = [0, 1, 2, 3]


@pytest.fixture(scope="module")
def chr1_text():
    text, names, lengths = synth.make_genome([synth.CHR1_LENGTH], seed=1)
    return text


@pytest.fixture(scope="module")
def chr1(chr1_text):
    gidx = api.GenomeIndex.build(chr1_text, device=0)
    gidx.set_option("GS_SPACED_FROM", "1")
    yield chr1_text, gidx
    gidx.close()


def three_settings(gidx, seqs, pams, **kw):
    """-> the bytes (identical in all three), the counters with the lookup on, the forms of the two seeding-launch runs"""
    try:
        gidx.set_options(GS_SEED_SPACED="1", GS_SEED_FORM=None)
        off1, hits1, _ = gidx.enumerate(seqs, pams, **kw)
        ctr1, f1 = gidx.last_counters(), gidx.last_sharing()["form"]
        gidx.set_option("GS_SEED_SPACED", "0")
        off0, hits0, _ = gidx.enumerate(seqs, pams, **kw)
        ctr0, f0 = gidx.last_counters(), gidx.last_sharing()["form"]
        gidx.set_option("GS_SEED_FORM", "0")
        offr, hitsr, _ = gidx.enumerate(seqs, pams, **kw)
        fr = gidx.last_sharing()["form"]
    finally:
        gidx.set_options(GS_SEED_SPACED=None, GS_SEED_FORM=None)
    print({k: v for k, v in ctr1.items() if k.startswith("spaced")}, "forms", f1, f0, fr, "hits", int(offr[-1]))
    assert fr == 0 and ctr0["spaced_items"] == 0
    assert np.array_equal(offr, off0) and hitsr.tobytes() == hits0.tobytes()
    assert np.array_equal(offr, off1) and hitsr.tobytes() == hits1.tobytes()
    assert int(offr[-1]) >= seqs.shape[0]   # every sampled guide finds its own site
    return (offr, hitsr), ctr1, (f1, f0)


@pytest.mark.parametrize("m", [1, 2, 3, 4])
@pytest.mark.parametrize("n", [1, 64, 1000])
def test_equal_bytes(chr1, n, m):
    text, gidx = chr1
    seqs, pams, _, _ = synth.sample_guides(text, n, seed=500 + 10 * m + n % 7)
    _, ctr, forms = three_settings(gidx, seqs, pams, mismatches=m)
    assert forms == (3, 3)
    assert ctr["spaced_items"] >= 2 * n, ctr   # one lookup per (guide, strand) item and table (a redo of overflowing guides adds its own)


@pytest.mark.parametrize("alts,start,lookups", [(("NAG",), False, 2), (("NAG", "CGG", "AGG", "TGG", "GGG"), False, 3), ((), True, 1)])
def test_equal_bytes_pam_lists_and_start(chr1, alts, start, lookups):
    """two PAM-pair tables (NGG + NAG: two lookups per item); six patterns = two appending passes, the first (NAG, CGG, AGG,
    TGG) through both tables, the second (GGG, NGG) through one: three lookups per item; the PAM at the 5' end (TTN)"""
    text, gidx = chr1
    n = 300
    seqs, pams, _, _ = synth.sample_guides(text, n, seed=41)
    if start:
        pams = np.tile(np.frombuffer(b"TTN", np.uint8), (n, 1))
    _, ctr, forms = three_settings(gidx, seqs, pams, mismatches=3, alt_pams=alts, start=start)
    assert forms == (3, 3)
    assert ctr["spaced_items"] == 2 * n * lookups, ctr


def site_key(guide, k, x_len, r_len):
    """the key of a guide's own site: its first x_len and its symbols k .. k + r_len - 1 in consumption order, as the packed
    guide record holds them (k_prepare: the complement of guide symbol t at bits 2 t)"""
    s = 3 - CODE[np.frombuffer(guide, np.uint8)].astype(np.int64)
    x = sum(int(s[t]) << (2 * (x_len - 1 - t)) for t in range(x_len))
    r = sum(int(s[k + j]) << (2 * j) for j in range(r_len))
    return (x << (2 * r_len)) | r


def test_table_content(chr1):
    """for 200 guides the rows under the key of the guide's own site hold that site's row, and every row under the key
    spells the key's X and R in the strand's text"""
    text, gidx = chr1
    n = 200
    seqs, pams, pos, strands = synth.sample_guides(text, n, seed=77)
    gidx.set_option("GS_SEED_SPACED", "1")
    try:
        gidx.enumerate(seqs, pams, mismatches=3)   # builds the tables
    finally:
        gidx.set_option("GS_SEED_SPACED", None)
    slot, info = None, None
    for s in (0, 1):   # the slot that holds the guides' own pattern (NGG): the one whose rows are sites of theirs
        inf = gidx.spaced_rows(s, 0, 0)[2]
        if inf["built"] and slot is None:
            slot, info = s, inf
        elif inf["built"]:
            g0, minus0 = seqs[0].tobytes(), strands[0] == ord("-")
            rows0 = gidx.spaced_rows(s, 0 if minus0 else 1, site_key(g0, inf["k"], inf["x_len"], inf["r_len"]))[0]
            own0 = (int(pos[0]) if minus0 else int(text.shape[0]) - (int(pos[0]) + L + P)) + P + L - inf["k"]
            if rows0.shape[0] and own0 in set(gidx.resolve(rows0[:, 2].astype(np.uint64), strand=0 if minus0 else 1).tolist()):
                slot, info = s, inf
    assert slot is not None and info["rows"] > 0, info
    k, x_len, r_len = info["k"], info["x_len"], info["r_len"]
    assert (k, x_len, r_len) == (13, 9, 7) and 2 * (x_len + r_len) - info["key_bits_in_row"] >= 8, info
    total = int(text.shape[0])
    rc = synth.reverse_complement_bytes(text)
    texts = (text, rc)
    seen_rows = 0
    for i in range(n):
        g = seqs[i].tobytes()
        key = site_key(g, k, x_len, r_len)
        # the site as the strand's text spells it, left to right: the PAM's complement reversed, then the guide's; the
        # forward-strand site of a "+" guide lies in the reverse strand's text and the other way round
        minus = strands[i] == ord("-")
        strand = 0 if minus else 1
        start = int(pos[i]) if minus else total - (int(pos[i]) + L + P)
        own = start + P + L - k   # where the suffix of the site's k-mer begins
        rows, n_rows, _ = gidx.spaced_rows(slot, strand, key)
        assert 1 <= n_rows == rows.shape[0], (i, n_rows)
        seen_rows += n_rows
        at = gidx.resolve(rows[:, 2].astype(np.uint64), strand=strand).astype(np.int64)
        assert own in set(at.tolist()), (i, own, at[:8])
        t = texts[strand]
        for p, o_sym, w in zip(at.tolist(), rows[:, 1].tolist(), rows[:, 3].tolist()):
            kmer = CODE[t[p:p + k]][::-1].astype(np.int64)         # consumption step j = text symbol p + k-1-j
            ctx = CODE[t[p - r_len:p]][::-1].astype(np.int64)      # step k + j = text symbol p - 1 - j
            x = sum(int(kmer[j]) << (2 * (x_len - 1 - j)) for j in range(x_len))
            r = sum(int(ctx[j]) << (2 * j) for j in range(r_len))
            assert (x << (2 * r_len)) | r == key, (i, p)
            assert o_sym == sum(int(kmer[j]) << (2 * (k - 1 - j)) for j in range(x_len, k)), (i, p)
            assert w & ((1 << (2 * r_len)) - 1) == r, (i, p)
    assert seen_rows >= n


def test_long_keys_on_a_repeat_rich_genome():
    """guides from inside the planted families: keys with more than 64 rows (several rounds of the lookup) and k-mer
    entries of 63 rows and more (a header slot in the row arrays, which is not a row); the seeding launches forced"""
    text, names, lengths = synth.make_repeat_genome([synth.CHR1_LENGTH], seed=1)
    gidx = api.GenomeIndex.build(text, device=0)
    try:
        gidx.set_options(GS_SPACED_FROM="1", GS_HEAVY="0", GS_SPLIT_SHARE="0")
        seqs, pams, pos, strands = synth.sample_guides(text, 1500, seed=5)
        gidx.set_option("GS_SEED_FORM", "0")
        off, hits, _ = gidx.enumerate(seqs, pams, mismatches=3)
        per = np.diff(off)
        pick = np.sort(np.concatenate([np.argsort(-per, kind="stable")[:150], np.arange(0, 1500, 15)]))
        pick = np.unique(pick)
        assert int(per[pick].max()) >= 1000, per[pick].max()   # the family's guides are there
        (offr, hitsr), ctr, forms = three_settings(gidx, seqs[pick], pams[pick], mismatches=3)
        assert forms == (3, 3)
        assert ctr["spaced_rows_max"] > 64, ctr
        assert ctr["spaced_matches"] > 0, ctr   # rows that passed the lookup's filter: what runs behind a match ran
        # a k-mer entry of 63 rows and more: under the key of the heaviest guide's own site that many rows share their O
        info = gidx.spaced_rows(0, 0, 0)[2]
        assert info["built"] == 1, info
        big = 0
        for i in np.argsort(-per, kind="stable")[:20]:
            key = site_key(seqs[i].tobytes(), info["k"], info["x_len"], info["r_len"])
            for strand in (0, 1):
                rows, n_rows, _ = gidx.spaced_rows(0, strand, key, cap=2048)
                if rows.shape[0]:
                    big = max(big, int(np.unique(rows[:, 1], return_counts=True)[1].max()))
            if big >= 63:
                break
        assert big >= 63, big
    finally:
        gidx.close()


def test_memory_ladder(chr1_text):
    """a handle whose cap leaves no room for the spaced tables runs the batch without them; a handle that has them gives
    them up first when a batch runs out of device memory (injected: GS_DBG_NOMEM) and redoes the batch: same bytes"""
    text = chr1_text
    seqs, pams, _, _ = synth.sample_guides(text, 400, seed=9)
    gidx = api.GenomeIndex.build(text, device=0)
    try:
        gidx.set_options(GS_SPACED_FROM="1", GS_SEED_SPACED="0")
        ref_off, ref_hits, _ = gidx.enumerate(seqs, pams, mismatches=3)   # PAM-pair + deep tables are in place
        assert gidx.last_sharing()["form"] == 3
        with_tables = gidx.device_bytes
        gidx.set_options(GS_SEED_SPACED="1", GS_INDEX_BUDGET_GB=f"{with_tables / 1e9 + 0.05:.3f}")
        off, hits, _ = gidx.enumerate(seqs, pams, mismatches=3)
        ctr = gidx.last_counters()
        assert gidx.last_sharing()["form"] == 3 and ctr["spaced_items"] == 0 and ctr["spaced_bytes"] == 0, ctr
        assert gidx.device_bytes == with_tables
        assert np.array_equal(off, ref_off) and hits.tobytes() == ref_hits.tobytes()
        gidx.set_option("GS_INDEX_BUDGET_GB", None)
        off, hits, _ = gidx.enumerate(seqs, pams, mismatches=3)
        ctr = gidx.last_counters()
        print({k: v for k, v in ctr.items() if k.startswith("spaced")})
        assert ctr["spaced_items"] == 2 * 400 and ctr["spaced_bytes"] > 0, ctr
        assert gidx.device_bytes == with_tables + ctr["spaced_bytes"]
        assert np.array_equal(off, ref_off) and hits.tobytes() == ref_hits.tobytes()
        gidx.set_option("GS_DBG_NOMEM", "1")   # the next pass ends as if out of memory: the first rung of the ladder
        off, hits, _ = gidx.enumerate(seqs, pams, mismatches=3)
        ctr = gidx.last_counters()
        assert ctr["spaced_items"] == 0 and ctr["spaced_bytes"] == 0, ctr
        assert gidx.device_bytes == with_tables   # nothing else went
        assert gidx.last_sharing()["form"] == 3 and ctr["items_pair_tables"] > 0
        assert np.array_equal(off, ref_off) and hits.tobytes() == ref_hits.tobytes()
    finally:
        gidx.close()
