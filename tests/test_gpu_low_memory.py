"""The low-memory table ladder and the out-of-memory recoveries, against the CPU oracle.

A handle that has stepped down (no context arrays, no inverse suffix array, no rotated table copies, no PAM-pair or
deep tables) serves every later batch of a job from the slower paths.  Every rung is forced by a switch here - never by
how much device memory happens to be free -, every batch is compared with the oracle guide by guide, and every run
shows from what the library reports (counters, the search's form, device_bytes, GS_DEBUG lines) that the rung it names
is the one that ran.  The recoveries of gs_enumerate_device are reached by injection (GS_DBG_NOMEM: the next n passes
of a batch end as if out of device memory after the main pass) - no device memory is exhausted.

Run on the GPU box with `pytest -m gpu`."""
import contextlib
import ctypes as C
import os
import re
from importlib import import_module

import numpy as np
import pytest

import oracle_lib as ol
from test_gpu_parity import gpu_hits_as_records, oracle_hits_as_records, two_sided_genome

api = import_module("guidescan-cli_amd.api")
synth = import_module("guidescan-cli_amd.synth")

pytestmark = pytest.mark.gpu

K, L = 12, 20   # the hg38-size code path at a table of 256 MiB: eight rotated copies are 2 GiB per strand
GS_ERR_NOMEM = 4

CASES = {
    "m3": dict(m=3),
    "m2": dict(m=2),
    "m4-nag": dict(m=4, alt=("NAG",)),
    "m3-ngn": dict(m=3, alt=("NGN",)),        # a pattern without a PAM-pair table: strand tables and their rotated copies
    "m3-start-ttn": dict(m=3, start=True, pam="TTN"),
    "m5": dict(m=5),                          # past the two seeding launches
}
# (hits in total, hits whose PAM shows a literal N) the oracle must reach, so that a degenerate fixture cannot pass
FLOORS = {"m3": (101, 10)}


def rot_copies(k, rot_first=3):
    """rotated copies per strand table, as build_ptab plans them"""
    return k - 1 - rot_first if k >= 4 and rot_first + 1 < k else 0


def rot_bytes(k, rot_first=3):
    """... and their bytes, both strands"""
    return 2 * 16 * 4 ** k * rot_copies(k, rot_first)


@pytest.fixture(scope="module")
def world():
    text, fam = two_sided_genome(str(K), L)
    sampled, _, _, _ = synth.sample_guides(text, 40, seed=3, L=L)
    guides = [fam.tobytes().decode(), synth.reverse_complement_bytes(fam).tobytes().decode()]
    guides += [sampled[i].tobytes().decode() for i in range(sampled.shape[0])]
    seqs = np.array([list(g.encode()) for g in guides], dtype=np.uint8)
    oidx = ol.OracleIndex(text)
    expected, totals = {}, {}
    try:
        for name, c in CASES.items():
            own, start = c.get("pam", "NGG"), c.get("start", False)
            opts = ol.make_opts(mismatches=c["m"], alt_pams=c.get("alt", ()), start=start)
            expected[name] = [oracle_hits_as_records(oidx, g, own, opts, 3, start)[0] for g in guides]
            pam_of = (lambda s: s[:3]) if start else (lambda s: s[-3:])
            totals[name] = (sum(len(e) for e in expected[name]),
                            sum(1 for e in expected[name] for h in e if "N" in pam_of(h[3])))
    finally:
        oidx.close()
    print("oracle hits (total, literal N under the PAM):", totals)
    for name, (tot, with_n) in FLOORS.items():
        assert totals[name][0] >= tot and totals[name][1] >= with_n, (name, totals)
    return dict(text=text, n=int(text.shape[0]) + 1, guides=guides, seqs=seqs, expected=expected, totals=totals)


@contextlib.contextmanager
def built(w, **env):
    """a handle made under GS_PREFIX_K, GS_DEBUG and the given switches (a handle reads the environment once, when it
    is made); closed before the next one is built.  The free memory the derived tables leave to the batch is set to
    zero: whether a rung's tables are built does not depend on what other processes hold on the card, as long as the
    tables themselves (12 GB at most here) find room."""
    env = {**dict(GS_PREFIX_K=str(K), GS_DEBUG="1", GS_PAIRTAB_RESERVE_GB="0", GS_ROT_RESERVE_GB="0"), **env}
    saved = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        gidx = api.GenomeIndex.build(w["text"], device=0)
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    try:
        yield gidx
    finally:
        gidx.close()


def _hip():
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return hip


def enumerate_case(gidx, w, name, entry="host"):
    """one batch through the host-pointer entry point or through enumerate_device -> (offsets, hits)"""
    c = CASES[name]
    own, start, alt = c.get("pam", "NGG"), c.get("start", False), c.get("alt", ())
    n = len(w["guides"])
    pams = np.tile(np.frombuffer(own.encode(), np.uint8), (n, 1))
    if entry == "host":
        offsets, hits, _ = gidx.enumerate(w["seqs"], pams, mismatches=c["m"], alt_pams=alt, start=start)
        return offsets, hits
    import torch
    d_s, d_p = torch.from_numpy(w["seqs"]).cuda(), torch.from_numpy(pams).cuda()
    torch.cuda.synchronize()
    hip = _hip()
    with gidx.locked():   # the results stay in the handle's buffers until they are copied
        d_off, d_hits, st = gidx.enumerate_device(d_s.data_ptr(), n, L, d_p.data_ptr(), 3, mismatches=c["m"], alt_pams=alt,
                                                  start=start)
        offsets = np.empty(n + 1, dtype=np.uint64)
        assert hip.hipMemcpy(offsets.ctypes.data, d_off, 8 * (n + 1), 2) == 0
        hits = np.empty(st["n_hits"], dtype=api.HIT_DTYPE)
        if st["n_hits"]:
            assert hip.hipMemcpy(hits.ctypes.data, d_hits, 16 * st["n_hits"], 2) == 0
    assert int(offsets[-1]) == st["n_hits"]
    return offsets, hits


def run(gidx, w, name, capfd, entry="host", what=""):
    """one batch, compared with the oracle guide by guide -> what the library reported about it"""
    c = CASES[name]
    capfd.readouterr()
    offsets, hits = enumerate_case(gidx, w, name, entry)
    err = capfd.readouterr().err
    start = c.get("start", False)
    for i, g in enumerate(w["guides"]):
        assert gpu_hits_as_records(offsets, hits, i, g, 3, start) == w["expected"][name][i], (what, name, i)
    assert int(offsets[-1]) == w["totals"][name][0]
    cnt, sh = gidx.last_counters(), gidx.last_sharing()
    mt = re.findall(r"\|X\|=(\d+)", err)
    ev = dict(two_sided="two-sided seeding" in err, deep="with deep tables" in err, walk="k_search (walk)" in err,
              rot_built=[int(x) for x in re.findall(r"strand \d: (\d+) rotated table copies built", err)],
              x_len=int(mt[-1]) if mt else None, launch=gidx.last_launch(),
              form=sh["form"], items_two_sided=cnt["items_two_sided"], items_one_sided=cnt["items_one_sided"],
              items_pair_tables=cnt["items_pair_tables"], slots=cnt["slots_per_item"], max_item=cnt["matches_max_per_item"],
              redone=cnt["guides_redone"], device_wide=cnt["ordered_device_wide"], bytes=gidx.device_bytes,
              err=err, raw=(offsets.tobytes(), hits.tobytes()))
    with capfd.disabled():   # the evidence of every run, kept whatever the next run's capture drops
        print(f"[{what}] {name}/{entry}:", {k: v for k, v in ev.items() if k not in ("err", "raw")})
    return ev


def assert_top_rung(ev):
    """PAM-pair + deep tables, the two seeding launches"""
    assert ev["two_sided"] and ev["deep"] and ev["form"] == 3 and ev["items_pair_tables"] > 0, ev["err"]
    assert ev["items_two_sided"] > 0 and ev["items_one_sided"] == 0


@pytest.fixture(scope="module")
def fresh_bytes(world):
    """device_bytes of a default handle before its first batch: strands with context arrays, tables and the inverse
    suffix array - no rotated copy, no PAM-pair table yet"""
    with built(world) as gidx:
        return gidx.device_bytes


def expect(name, pair=True, deep=True, spec=True, kb=K - 2):
    """what a batch shows on a handle with context arrays and inverse suffix arrays: PAM-pair tables serve the items
    whose patterns all end in concrete pairs (not NGN); deep tables and the kernel without the strand tables' side go
    with them; the two seeding launches (form 3) up to four mismatches"""
    pairable = pair and name != "m3-ngn"
    d = pairable and deep
    s = d and spec
    return dict(pair=pairable, deep=d, spec=s, form=3 if s and CASES[name]["m"] <= 4 else 0, x_len=L - kb if d else L + 3 - K)


def assert_rung(ev, name, **kw):
    want = expect(name, **kw)
    got = dict(pair=ev["items_pair_tables"] > 0, deep=ev["launch"]["deep"], spec=ev["launch"]["spec"], form=ev["form"],
               x_len=ev["launch"]["x_len"])
    assert got == want and ev["deep"] == want["deep"], (name, kw, ev["err"])
    assert ev["two_sided"] and not ev["walk"] and not ev["launch"]["walk"] and ev["items_two_sided"] > 0
    assert ev["x_len"] in (None, want["x_len"])   # (the GS_DEBUG line says the same)


def under(extra):
    """GS_INDEX_BUDGET_GB 1 MB under a default handle's own bytes + extra (the strands differ by their exception rows,
    a few KB, and each gets half the cap)"""
    return lambda fresh: dict(GS_INDEX_BUDGET_GB=f"{(fresh + extra - 1_000_000) / 1e9:.9f}")


# the switches of each index-time step (from a default handle's bytes), and what it leaves: context arrays, inverse
# suffix array, rotated copies per table, PAM-pair tables
RUNGS = {
    "default": (lambda fresh: dict(), dict(ctx=True, isa=True, rot=rot_copies(K), pair=True)),
    "no-ctx": (lambda fresh: dict(GS_NO_CTX="1"), dict(ctx=False, isa=False, rot=0, pair=False)),
    "no-isa": (lambda fresh: dict(GS_NO_ISA="1"), dict(ctx=True, isa=False, rot=rot_copies(K), pair=False)),
    "no-rot": (lambda fresh: dict(GS_NO_ROT="1"), dict(ctx=True, isa=True, rot=0, pair=True)),
    "rot-first-one-copy": (lambda fresh: dict(GS_ROT_FIRST=str(K - 2)), dict(ctx=True, isa=True, rot=1, pair=True)),
    "rot-first-no-copy": (lambda fresh: dict(GS_ROT_FIRST=str(K - 1)), dict(ctx=True, isa=True, rot=0, pair=True)),
    "budget-copies-go": (under(rot_bytes(K)), dict(ctx=True, isa=True, rot=0, pair=True)),
    "budget-isa-goes": (under(0), dict(ctx=True, isa=False, rot=0, pair=False)),
}


@pytest.mark.parametrize("rung", list(RUNGS))
def test_every_index_time_step_against_the_oracle(world, fresh_bytes, rung, capfd):
    w = world
    env, want = RUNGS[rung]
    assert rot_copies(K, K - 2) == 1 and rot_copies(K, K - 1) == 0 and rot_copies(K) == 8
    with built(w, **env(fresh_bytes)) as gidx:
        # the handle as built: the inverse suffix array is 4 bytes per row and strand, the context arrays 6
        b0 = gidx.device_bytes
        if not want["ctx"]:
            assert b0 <= fresh_bytes - 2 * 10 * w["n"], (b0, fresh_bytes)
        elif not want["isa"]:
            assert b0 == fresh_bytes - 2 * 4 * w["n"], (b0, fresh_bytes)
        else:
            assert b0 == fresh_bytes, (b0, fresh_bytes)
        # the first batch that reads rotated copies builds them - without PAM-pair tables, so that device_bytes moves
        # by the copies alone
        gidx.set_option("GS_NO_PAIRTAB", "1")
        ev = run(gidx, w, "m3-ngn", capfd, what=rung + ", no pair tables")
        gidx.set_option("GS_NO_PAIRTAB", None)
        assert ev["rot_built"] == ([want["rot"]] * 2 if want["rot"] else []), ev["err"]
        rb = rot_bytes(K, K - 1 - want["rot"])
        assert ev["bytes"] - b0 == rb and ev["items_pair_tables"] == 0, (ev["bytes"], b0, rb)
        assert ev["two_sided"] == want["isa"] and ev["walk"] == (not want["ctx"])
        for name in CASES:
            ev = run(gidx, w, name, capfd, what=rung)
            assert ev["rot_built"] == [] and ev["launch"]["rot_copies"] == want["rot"], ev["err"]   # written once
            if want["isa"]:
                assert_rung(ev, name, pair=want["pair"])
                continue
            assert ev["walk"] == ev["launch"]["walk"] == (not want["ctx"])
            assert not ev["two_sided"] and ev["items_two_sided"] == 0 and ev["form"] == 0, ev["err"]
            assert ev["items_pair_tables"] == 0 and not ev["launch"]["deep"] and not ev["launch"]["spec"]
            assert ev["bytes"] == b0 + rb


def test_a_table_without_context_arrays_at_the_deepest_depth(world, capfd):
    """GS_NO_CTX at k = 14 (the depth of an hg38-size handle: 2^28 table entries, whose context masks are set in
    pieces of 2^24 rows)"""
    w = world
    with built(w, GS_NO_CTX="1", GS_PREFIX_K="14") as gidx:
        for name in CASES:
            ev = run(gidx, w, name, capfd, what="no-ctx, k = 14")
            assert ev["walk"] and ev["launch"]["walk"] and not ev["two_sided"] and ev["items_pair_tables"] == 0


def test_every_batch_time_step_against_the_oracle(world, capfd):
    w = world
    n_items = 2 * len(w["guides"])

    def all_cases(what, check):
        out = {}
        for name in CASES:
            out[name] = run(gidx, w, name, capfd, what=what)
            check(out[name], name)
        return out

    with built(w) as gidx:
        base = all_cases("default", assert_rung)
        assert_top_rung(base["m3"])
        assert all(ev["launch"]["take"] == 1 and ev["launch"]["seed_take"] == (1 if ev["form"] == 3 else 0) for ev in base.values())
        # the fixture's own sizes, which the sizing switches below are set either side of
        assert 64 < base["m4-nag"]["max_item"] < 1024 and base["m4-nag"]["slots"] == 128 and base["m5"]["slots"] == 128, base["m4-nag"]
        assert all(base[name]["slots"] == 64 for name in CASES if CASES[name]["m"] <= 3)
        assert base["m3-ngn"]["max_item"] > 64 and base["m3-ngn"]["redone"] > 0   # 64 slots overflow by themselves

        def same_bytes(ev, name):
            assert ev["raw"] == base[name]["raw"]

        gidx.set_option("GS_NO_DEEP", "1")   # PAM-pair tables, the strand tables on the other strand's side
        all_cases("GS_NO_DEEP", lambda ev, name: assert_rung(ev, name, deep=False))
        gidx.set_option("GS_NO_DEEP", None)

        gidx.set_option("GS_NO_SPEC", "1")   # pair + deep tables under the kernel that keeps the strand tables' side
        all_cases("GS_NO_SPEC", lambda ev, name: assert_rung(ev, name, spec=False))
        gidx.set_option("GS_NO_SPEC", None)

        # deep tables indexed by 11 guide symbols instead of k - 2 = 10 (legal: kb + 3 >= k, L - kb + 2 <= k, kb <= 14)
        gidx.set_option("GS_DEEP_SYMBOLS", str(K - 1))
        all_cases("GS_DEEP_SYMBOLS", lambda ev, name: assert_rung(ev, name, kb=K - 1))
        gidx.set_option("GS_DEEP_SYMBOLS", None)

        def back(ev, name):
            assert_rung(ev, name)
            same_bytes(ev, name)
        all_cases("GS_DEEP_SYMBOLS removed", back)

        # items a wave takes per visit to the work counter, either side of the batch's 84 items: in the two seeding
        # launches, and in the one launch
        for take in (3, n_items + 116):
            def seed_take(ev, name):
                assert_rung(ev, name)
                assert ev["launch"]["seed_take"] == (take if ev["form"] == 3 else 0) and ev["launch"]["take"] == 1
                same_bytes(ev, name)
            gidx.set_option("GS_SEED_TAKE", str(take))
            all_cases("GS_SEED_TAKE", seed_take)
            gidx.set_option("GS_SEED_TAKE", None)

            def search_take(ev, name):
                assert_rung(ev, name)
                assert ev["launch"]["take"] == take and ev["launch"]["seed_take"] == (1 if ev["form"] == 3 else 0)
                same_bytes(ev, name)
            gidx.set_option("GS_SEARCH_TAKE", str(take))
            all_cases("GS_SEARCH_TAKE", search_take)
            gidx.set_option("GS_SEARCH_TAKE", None)

        # slots per item either side of the largest item's records (budgets beyond three: up to three it is 64), and
        # GS_ORDER_WIDE_FROM, from which the device-wide ordering takes the whole batch, either side of the slots
        for cap, wide_from in ((1, None), (4 * 1024, None), (4 * 1024, 8 * 1024), (None, 64), (None, 65)):
            def sized(ev, name):
                assert_rung(ev, name)
                slots = base[name]["slots"] if cap is None or CASES[name]["m"] <= 3 else max(cap, 64)
                assert ev["slots"] == slots and ev["max_item"] == base[name]["max_item"], ev
                assert (ev["redone"] > 0) == (ev["max_item"] > slots), ev
                assert ev["device_wide"] == (slots >= (wide_from or 1024)), ev
                same_bytes(ev, name)
            gidx.set_options(GS_SLOT_CAP=cap, GS_ORDER_WIDE_FROM=wide_from)
            out = all_cases(f"GS_SLOT_CAP={cap} GS_ORDER_WIDE_FROM={wide_from}", sized)
            if cap == 1:
                assert out["m4-nag"]["redone"] > 0   # the overflow redo under a cap below the largest item
        gidx.set_options(GS_SLOT_CAP=None, GS_ORDER_WIDE_FROM=None)
        all_cases("switches removed", back)


def test_pair_tables_that_did_not_fit_are_not_tried_again_until_memory_comes_back(world, capfd):
    """GS_INDEX_BUDGET_GB set on a live handle ahead of its first NGG batch: no PAM-pair table fits.  A batch with two
    pairs (GG, AG) makes the handle remember both (pairtab_nofit): they are not tried again when the cap is gone -
    until a recovery gives memory back (the rotated copies dropped), which clears that memory.  A lone pair that did
    not fit (GG before that batch, TT) is not remembered: asking again costs nothing, what the memory spares is
    freeing and rebuilding the first pair's tables every batch."""
    w = world
    with built(w) as gidx:
        b0 = gidx.device_bytes
        gidx.set_option("GS_INDEX_BUDGET_GB", f"{b0 / 1e9:.9f}")
        for name in ("m3", "m4-nag", "m2", "m3-ngn", "m3-start-ttn", "m5"):
            ev = run(gidx, w, name, capfd, what="cap at the strands' own bytes")
            assert_rung(ev, name, pair=False)
            # (GG and AG are not asked for again once the two-pair batch has marked them)
            assert ("not enough free memory" in ev["err"]) == (name in ("m3", "m4-nag", "m3-start-ttn")), ev["err"]
            assert ev["bytes"] == b0 + rot_bytes(K)
        gidx.set_option("GS_INDEX_BUDGET_GB", None)
        for name in CASES:
            ev = run(gidx, w, name, capfd, what="cap removed")
            assert "not enough free memory" not in ev["err"]
            assert_rung(ev, name, pair=name == "m3-start-ttn")   # TT was never marked: built now
            assert ("deep table:" in ev["err"]) == (name == "m3-start-ttn"), ev["err"]
        gidx.set_option("GS_DBG_NOMEM", "1")
        ev = run(gidx, w, "m3", capfd, what="copies dropped")
        assert "rotated table copies dropped" in ev["err"]
        assert_top_rung(ev)   # the redo itself already places the pair's tables again
        for name in CASES:
            assert_rung(run(gidx, w, name, capfd, what="after the copies were dropped"), name)


ENTRIES = ["host", "device"]


def warm(gidx, w, capfd, entry):
    """the top rung's batch and the batch that reads rotated copies, both run normally and their bytes kept"""
    a = run(gidx, w, "m3", capfd, entry, what="before")
    assert_top_rung(a)
    b = run(gidx, w, "m3-ngn", capfd, entry, what="before")
    assert b["rot_built"] == [rot_copies(K)] * 2
    return a, b


@pytest.mark.parametrize("entry", ENTRIES)
def test_recovery_releases_the_workspace_and_redoes_the_batch(world, capfd, entry):
    w = world
    with built(w) as gidx:
        a, b = warm(gidx, w, capfd, entry)
        gidx.set_option("GS_DBG_RELEASE_MIN", "0")
        for name, before in (("m3", a), ("m3-ngn", b)):
            gidx.set_option("GS_DBG_NOMEM", "1")
            ev = run(gidx, w, name, capfd, entry, what="workspace released")
            assert "of workspace released, batch redone" in ev["err"] and "dropped" not in ev["err"], ev["err"]
            assert ev["raw"] == before["raw"] and ev["bytes"] == b["bytes"] and ev["rot_built"] == []
            assert ev["form"] == before["form"] and ev["items_pair_tables"] == before["items_pair_tables"]
        # the hook has run out: nothing is released, nothing redone
        ev = run(gidx, w, "m3", capfd, entry, what="hook exhausted")
        assert "out of device memory" not in ev["err"] and ev["raw"] == a["raw"]
        assert_top_rung(ev)


@pytest.mark.parametrize("entry", ENTRIES)
def test_recovery_drops_the_rotated_copies_for_good(world, capfd, entry):
    w = world
    with built(w) as gidx:
        a, b = warm(gidx, w, capfd, entry)
        gidx.set_option("GS_DBG_NOMEM", "1")
        ev = run(gidx, w, "m3-ngn", capfd, entry, what="copies dropped")
        # (less than RELEASE_REDO_MIN of workspace: released, but not worth a redo by itself)
        assert "workspace released" not in ev["err"] and "rotated table copies dropped" in ev["err"], ev["err"]
        assert "PAM-pair tables dropped" not in ev["err"]
        assert ev["bytes"] == b["bytes"] - rot_bytes(K) and ev["raw"] == b["raw"]
        # later batches that would read copies do not build them again
        ev = run(gidx, w, "m3-ngn", capfd, entry, what="after the copies were dropped")
        assert ev["rot_built"] == [] and ev["bytes"] == b["bytes"] - rot_bytes(K) and ev["raw"] == b["raw"], ev["err"]
        for name in ("m3-start-ttn", "m4-nag", "m5", "m3-ngn"):
            ev = run(gidx, w, name, capfd, entry, what="after the copies were dropped")
            assert ev["rot_built"] == [] and "out of device memory" not in ev["err"], ev["err"]
        # the PAM-pair tables are untouched
        ev = run(gidx, w, "m3", capfd, entry, what="after the copies were dropped")
        assert_top_rung(ev)
        assert ev["raw"] == a["raw"]


@pytest.mark.parametrize("entry", ENTRIES)
def test_recovery_drops_the_pair_tables_after_the_copies(world, fresh_bytes, capfd, entry):
    w = world
    with built(w) as gidx:
        a, b = warm(gidx, w, capfd, entry)
        gidx.set_option("GS_DBG_NOMEM", "2")
        ev = run(gidx, w, "m3-ngn", capfd, entry, what="copies and pair tables dropped")
        assert "rotated table copies dropped" in ev["err"] and "PAM-pair tables dropped" in ev["err"], ev["err"]
        assert ev["raw"] == b["raw"] and ev["bytes"] == fresh_bytes   # every derived table has gone: nothing leaks
        # the next batch, other budgets and patterns (shapes the handle has not seen), and a prepared handle
        for name in ("m3", "m2", "m4-nag", "m3-start-ttn", "m5", "m3-ngn"):
            ev = run(gidx, w, name, capfd, entry, what="after both were dropped")
            assert ev["items_pair_tables"] == 0 and ev["form"] != 3 and not ev["deep"] and ev["rot_built"] == [], ev["err"]
            assert ev["two_sided"] and ev["bytes"] == fresh_bytes
        gidx.prepare(4096, L=L, pam="NGG", mismatches=3)
        gidx.prepare(4096, L=L, pam="NGG", alt_pams=("NAG",), mismatches=4)
        for name in ("m3", "m4-nag"):
            ev = run(gidx, w, name, capfd, entry, what="prepared after both were dropped")
            assert ev["items_pair_tables"] == 0 and ev["form"] != 3 and not ev["deep"] and ev["bytes"] == fresh_bytes


@pytest.mark.parametrize("entry", ENTRIES)
def test_out_of_memory_past_the_last_recovery_fails_cleanly(world, fresh_bytes, capfd, entry):
    w = world
    with built(w) as gidx:
        a, b = warm(gidx, w, capfd, entry)
        gidx.set_option("GS_DBG_NOMEM", "3")   # the pass, the redo without copies, the redo without pair tables
        capfd.readouterr()
        with pytest.raises(api.GsError) as e:
            enumerate_case(gidx, w, "m3-ngn", entry)
        assert e.value.status == GS_ERR_NOMEM
        err = capfd.readouterr().err
        assert "rotated table copies dropped" in err and "PAM-pair tables dropped" in err, err
        assert gidx.device_bytes == fresh_bytes
        # the hook has run out: the handle answers again, from the lowest rung
        for name in ("m3-ngn", "m3", "m4-nag"):
            ev = run(gidx, w, name, capfd, entry, what="after the failed call")
            assert "out of device memory" not in ev["err"] and ev["items_pair_tables"] == 0 and ev["bytes"] == fresh_bytes
        assert run(gidx, w, "m3-ngn", capfd, entry, what="after the failed call")["raw"] == b["raw"]
