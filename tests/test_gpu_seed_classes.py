"""The seeding launches (gs_seed.hip: k_seed_a, k_seed_b) and the spaced lookup inside k_seed_a against the CPU oracle, site
class by site class, at the table depths 13 and 14 and at both ends of the spaced tables' key split.

The world of tests/seed_classes_world.py plants, for four anchors, a site of every class (substitutions in X, in O, in R) on
both strands and for two PAM pairs, a key of the spaced table with more than 64 rows, a pair-table entry and a deep-table
entry of 63 rows and more, and sites with a literal N under the PAM; tests/test_seed_classes_world.py shows without a GPU
that the oracle's lists hold all of them.  Every case here compares the library's hit list with the oracle's guide by
guide (position, distance, strand flag, reported sequence), asserts that the two seeding launches ran (form 3) at the
geometry the world was planted for, and reads the lookup's counters: `spaced_matches` must reach the number of hits only
the lookup's class holds - a lookup that finds nothing, or the wrong rows, cannot hide behind a comparison of the library
with itself.  Depth 14 is the depth of every hg38-sized handle (|X| = 8, |O| = 6, |R| = 6, a class of 540 / 1,215 recipes at
budgets 3 / 4: the lookup on by default); GS_SPACED_BITS gives the 400-kb text the key split of that size (the whole key
in the offsets, no key bits with the row) and the smallest legal one.

Why `spaced_matches` EQUALS the oracle's class count where the PAM patterns leave the symbol beside the pair free (NGG, NAG,
TTN) and no guide was searched a second time (the lookups' count says so): a row is counted in k_seed_a where it passed the filter "the key's bits with
the row equal the item's, O differs in exactly m symbols"; the rows under a key have the item's X and R (the offsets give
the key's top bits, the filter the others), the table holds only rows of the pair table (the pattern's pair, no symbol
outside A,C,G,T within the site), and `resolve` then tests nothing but the pattern's concrete symbols against the row's
context - so every counted row is a reported hit of distance m with all substitutions in O, and every such hit is a row
under that key.  A list with concrete first symbols (CGG, AGG ...) drops counted rows in `resolve`: a lower bound there.

Run on the GPU box with `pytest -m gpu`."""
import ctypes as C
from importlib import import_module

import numpy as np
import pytest

import seed_classes_world as W
from test_gpu_low_memory import built
from test_gpu_parity import gpu_hits_as_records

api = import_module("guidescan-cli_amd.api")

pytestmark = pytest.mark.gpu

DEPTHS = {14: 8, 13: 9}                 # table depth -> |X|
PAIR_CODE = dict(GG=5, AG=7, TT=15)     # the pair as the strand's consumption sees it (gs_debug_spaced_rows: info["code"])
CODE = np.full(256, 255, np.uint8)
CODE[list(b"ACGT")] = [0, 1, 2, 3]
SWITCHES = ("GS_SPACED_FROM", "GS_SEED_SPACED", "GS_SEED_FORM", "GS_SEED_SORT_FROM", "GS_SPACED_BITS", "GS_SLOT_CAP", "GS_NO_ARENA")


def handle(w):
    """the `built()` pattern of test_gpu_low_memory.py at the world's depth; GS_HEAVY / GS_SPLIT_SHARE: the planted families must
    not move the batch to a sharing form (tests/test_gpu_spaced.py::test_long_keys_on_a_repeat_rich_genome)"""
    return built(w, GS_PREFIX_K=str(w["k"]), GS_HEAVY="0", GS_SPLIT_SHARE="0")


@pytest.fixture(scope="module", params=sorted(DEPTHS, reverse=True), ids=lambda k: f"k{k}")
def end(request):
    w = W.world(request.param, DEPTHS[request.param])
    with handle(w) as gidx:
        yield w, gidx


def lookup_default(w, m):
    """GS_SPACED_FROM's default: a class of 256 recipes or more, C(|O|, m) 3^m"""
    n_o, cls = w["k"] - w["x_len"], 1.0
    for i in range(m):
        cls = cls * (n_o - i) / (i + 1) * 3.0
    return m <= n_o and cls >= 256


def run(gidx, w, m, name, lookup, form=3, what="", **switches):
    """one batch under the given switches: the lists, the form, the geometry and the lookup's counters -> the counters.
    lookup: whether the spaced lookup must have run"""
    own, alt, pairs, lookups = W.PAM_LISTS[w["start"]][name]
    n = len(w["guides"])
    pams = np.tile(np.frombuffer(own.encode(), np.uint8), (n, 1))
    try:
        gidx.set_options(**switches)
        offsets, hits, _ = gidx.enumerate(w["seqs"], pams, mismatches=m, alt_pams=alt, start=w["start"])
        ctr, got_form, launch = gidx.last_counters(), gidx.last_sharing()["form"], gidx.last_launch()
        infos = [gidx.spaced_rows(s, 0, 0)[2] for s in (0, 1)]
    finally:
        gidx.set_options(**{k: None for k in SWITCHES})
    exp, cls = w["expected"][(m, name)], sum(w["class_hits"][(m, name)])
    sp = {k: v for k, v in ctr.items() if k.startswith("spaced") and k not in ("spaced_bytes", "spaced_build_us")}
    print(f"[seed classes] k={w['k']} {name} m={m} {what} {switches}: form {got_form}, {sp}, "
          f"sp_rem {[i['key_bits_in_row'] for i in infos if i['built']]}, redone {ctr['guides_redone']}, "
          f"hits {int(offsets[-1])}, oracle class hits {cls}")
    for i, g in enumerate(w["guides"]):
        assert gpu_hits_as_records(offsets, hits, i, g, W.P, w["start"]) == exp[i], (w["k"], name, m, what, i)
    assert got_form == form, (got_form, what)
    if form != 3:
        assert ctr["spaced_items"] == 0, ctr
        return ctr
    assert launch["x_len"] == w["x_len"] and launch["spec"] and launch["deep"], launch
    for inf in infos:
        if inf["built"]:
            assert (inf["k"], inf["x_len"], inf["r_len"]) == (w["k"], w["x_len"], w["r_len"]), inf
    if not lookup:
        assert ctr["spaced_items"] == 0 and ctr["spaced_matches"] == 0, ctr
        return ctr
    assert {PAIR_CODE[p] for p in pairs} <= {i["code"] for i in infos if i["built"]}, infos   # (a table of an earlier list may remain)
    if ctr["guides_redone"] == 0:
        assert ctr["spaced_items"] == 2 * n * lookups, ctr     # one lookup per (guide, strand) item, table and appending pass
    else:
        assert ctr["spaced_items"] >= 2 * n * lookups, ctr     # (a second search of the overflowing guides adds its own)
    assert ctr["spaced_matches"] > 0 and cls > 0
    # (no second search: no guide overflowed, or the arena held what did - the item count shows that no lookup ran twice)
    if name != "six" and ctr["spaced_items"] == 2 * n * lookups:
        assert ctr["spaced_matches"] == cls, (ctr, cls)         # (the module's head: every counted row is a class hit)
    else:
        assert ctr["spaced_matches"] >= cls, (ctr, cls)
    assert ctr["spaced_rows_max"] > 64, ctr                     # the fat key: several rounds of 64 rows
    return ctr


SETTINGS = {"from1": dict(GS_SPACED_FROM="1"), "default": dict(), "off": dict(GS_SEED_SPACED="0")}


@pytest.mark.parametrize("setting", list(SETTINGS))
@pytest.mark.parametrize("m", [1, 2, 3, 4])
def test_budgets_and_lookup_settings(end, m, setting):
    """NGG + NAG, two pair tables: the lookup at every budget, where the default takes it (depth 14: budgets 3 and 4; depth 13:
    never, its class has 108 recipes at the most), and the class from its recipes"""
    w, gidx = end
    lookup = dict(from1=True, default=lookup_default(w, m), off=False)[setting]
    assert setting != "default" or lookup == (w["k"] == 14 and m >= 3)
    run(gidx, w, m, "ngg-nag", lookup, what=setting, **SETTINGS[setting])


def test_budget_five_keeps_the_one_launch(end):
    w, gidx = end
    run(gidx, w, 5, "ngg-nag", False, form=0, GS_SPACED_FROM="1")


@pytest.mark.parametrize("form", [1, 2])
def test_seed_forms(end, form):
    """the launches in the order given, and scheduled (a 20-guide batch: seven of the eight XCD pieces nearly empty)"""
    w, gidx = end
    extra = dict(GS_SEED_SORT_FROM="1") if form == 2 else {}
    run(gidx, w, 3, "ngg-nag", True, what=f"GS_SEED_FORM={form}", GS_SPACED_FROM="1", GS_SEED_FORM=str(form), **extra)


@pytest.mark.parametrize("name", ["ngg", "six"])
def test_pam_lists(end, name):
    """one pair table; six patterns in two appending passes through two tables (three lookups per item)"""
    w, gidx = end
    run(gidx, w, 3, name, True, GS_SPACED_FROM="1")


@pytest.mark.parametrize("k", sorted(DEPTHS, reverse=True))
def test_start_ttn_on_the_mirrored_world(k):
    w = W.world(k, DEPTHS[k], True)
    with handle(w) as gidx:
        for m in (3, 1):
            run(gidx, w, m, "ttn", True, GS_SPACED_FROM="1")


def test_overflow_redo_with_the_lookup_on(end):
    """64 slots per item and no arena: anchor 0's items overflow and their guide is searched once more, lookup included"""
    w, gidx = end
    ctr = run(gidx, w, 4, "ngg-nag", True, what="redo", GS_SPACED_FROM="1", GS_SLOT_CAP="64", GS_NO_ARENA="1")
    assert ctr["guides_redone"] >= 1 and ctr["spaced_items"] > 2 * len(w["guides"]) * 2, ctr   # (the second search's lookups)


def device_words(gidx, slot, strand, which, index, words_per_entry):
    """one entry of a slot's device array (gs_debug_index_array with an offset: the depth-14 arrays are gigabytes)"""
    L_ = api.lib()
    L_.gs_debug_index_array.restype = C.c_int
    L_.gs_debug_index_array.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_char_p, C.c_uint64, C.c_void_p, C.c_uint64, C.c_void_p]
    out = np.zeros(words_per_entry, dtype=np.uint32)
    total = C.c_uint64()
    rc = L_.gs_debug_index_array(gidx._h, slot, strand, which.encode(), 4 * words_per_entry * index, out.ctypes.data, out.nbytes,
                                 C.byref(total))
    assert rc == 0 and total.value >= 4 * words_per_entry * (index + 1), (rc, total.value, index)
    return out


def test_the_heavy_entries_are_there(end):
    """what says that the fat k-mer entry and the fat deep-table entry were met: the handle's own tables.  The pair-table
    entry of anchor 0's k-mer carries GS_PT_BIG (63) as its count - the entry the recipe without a substitution in X and O
    reads for anchor 0, whose rows' count then comes from the header slot - and the deep-table entry of anchor 0's O, R and
    PAM heads 80 rows and more; the lists of anchor 0 equal the oracle's in every case of this file, and they hold those
    sites.  (No counter of the kernels says which entries an item read, and none is added for this.)"""
    w, gidx = end
    k, x_len = w["k"], w["x_len"]
    run(gidx, w, 3, "ngg-nag", True, GS_SPACED_FROM="1")   # (the tables exist whatever ran before)
    slot = [s for s in (0, 1) if gidx.spaced_rows(s, 0, 0)[2]["code"] == PAIR_CODE["GG"]][0]
    a0 = CODE[np.frombuffer(w["anchors"][0].encode(), np.uint8)].astype(np.int64)
    # the pair table's index: the k-mer as the strand consumes it, the complement of guide symbol t at bits 2 (k-1-t)
    # (tests/test_gpu_spaced.py::site_key); a site planted on the forward text lies in the reverse strand's table
    entry = sum(int(3 - a0[t]) << (2 * (k - 1 - t)) for t in range(k))
    fat = [s for s in w["sites"] if s["kind"] == "fat-kmer"]
    assert len(fat) >= 63 and {s["strand"] for s in fat} == {0}
    tab = device_words(gidx, slot, 1, "tab", entry, 2)
    first, cnt = int(tab[0]), int(tab[1]) & 63
    assert cnt == 63, (cnt, entry)
    rows = int(device_words(gidx, slot, 1, "rowid", first, 1)[0])   # the header slot: the entry's true count
    print(f"[seed classes] k={k}: pair-table entry of anchor 0's k-mer: count field {cnt}, {rows} rows behind the header slot")
    assert rows >= len(fat)
    # the deep table's index: guide symbol L-1-y at bits 2 (kb-1-y) of the kb = k - 2 symbols behind X, then the base under the
    # PAM's N (tests/index_tables_model.py::deep_table); a site planted reverse-complemented is spelled by the reverse strand's text
    fat = [s for s in w["sites"] if s["kind"] == "fat-deep"]
    kb = W.L - x_len
    assert len(fat) >= 63 and {s["strand"] for s in fat} == {1} and len({s["pam"] for s in fat}) == 1
    i = sum(int(a0[W.L - 1 - y]) << (2 * (kb - 1 - y)) for y in range(kb))
    deep = device_words(gidx, slot, 1, "deep", 4 * i + int(CODE[ord(fat[0]["pam"][0])]), 4)
    print(f"[seed classes] k={k}: deep-table entry of anchor 0's O, R and {fat[0]['pam']}: {int(deep[1]) & 0x7FFFFFFF} rows")
    assert int(deep[1]) & 0x7FFFFFFF >= len(fat)


# (last in the file: the tables are built anew under each value, and once more by whatever runs behind)
@pytest.mark.parametrize("bits", ["full", "smallest"])
def test_key_split(end, bits):
    """GS_SPACED_BITS at the key's full width - at depth 14 the whole 28-bit key in the offsets, 2^28 of them, no key bits with
    the row: the hg38-sized form; at depth 13 the 32-bit key leaves 4 bits with the row, the offsets' limit being 28 - and at
    the smallest d the 32-bit payload word allows"""
    w, gidx = end
    k, x_len, r_len = w["k"], w["x_len"], w["r_len"]
    key_bits, obits = 2 * (x_len + r_len), 2 * (k - x_len)
    want_rem = key_bits - min(28, key_bits) if bits == "full" else min(key_bits - 1, 32 - obits)
    assert k != 14 or want_rem == (0 if bits == "full" else 20)
    for m in ((3, 4) if k == 14 else (2,)):
        run(gidx, w, m, "ngg", True, what=f"GS_SPACED_BITS {bits}", GS_SPACED_FROM="1", GS_SPACED_BITS="32" if bits == "full" else "1")
        slot = [s for s in (0, 1) if gidx.spaced_rows(s, 0, 0)[2]["code"] == PAIR_CODE["GG"]][0]
        for strand in (0, 1):
            info = gidx.spaced_rows(slot, strand, 0)[2]
            assert info["built"] and info["key_bits_in_row"] == want_rem, (info, want_rem)
