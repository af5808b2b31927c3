"""The workspace buffers (gs_buffer: what a handle or a decoder grows on demand and keeps from call to call) have an
owner: nothing outlives the handle, the decoder or the call that held it, and an out-of-memory recovery releases the
bulk buffers its groups name and nothing else.  What is counted are the process's live buffers and their bytes
(gs_debug_buffers_live) and the handle's workspace per group (gs_debug_workspace) - never the card's free memory.
The toy genome, the guides and the oracle comparison are those of test_gpu_low_memory.py.  GPU only."""
import re
from importlib import import_module

import numpy as np
import pytest

import bam_make as bm
import decode_golden as dg
from test_gpu_decode_bam_device import GOOD as BAM_GOOD, as_bam, through
from test_gpu_low_memory import CASES, built, run, world  # noqa: F401  (world is a fixture)
from test_gpu_text_device import device_text
from test_text_batch import random_batch

api = import_module("guidescan-cli_amd.api")

pytestmark = pytest.mark.gpu


def test_nothing_outlives_a_handle(world, capfd):
    w = world
    before = api.buffers_live()
    with built(w) as gidx:
        ws = gidx.workspace()
        assert set(ws) == set(api.WORKSPACE_GROUPS)
        run(gidx, w, "m3", capfd, what="m <= 3")
        assert gidx.workspace()["batch"]["buffers"] > 0
        # the same batch ordered device-wide: no tile ordering, the smallest slots, and the wide ordering from the 64
        # slots a budget of three has anyway - the family guide and every other guide go through it
        gidx.set_options(GS_NO_TILE_ORDER="1", GS_SLOT_CAP="1", GS_ORDER_WIDE_FROM="64")
        ev = run(gidx, w, "m3", capfd, what="device-wide ordering")
        assert ev["device_wide"] and gidx.workspace()["big"]["buffers"] > 0, ev
        # ... and a budget of five in tiles
        gidx.set_options(GS_NO_TILE_ORDER=None, GS_SLOT_CAP=None)
        run(gidx, w, "m5", capfd, what="tile ordering")
        assert gidx.last_counters()["ordered_in_tiles"] and gidx.workspace()["tile"]["buffers"] > 0
        gidx.set_option("GS_ORDER_WIDE_FROM", None)
        # score, then the text of a synthetic batch as CSV and as SAM, then BGZF members
        offsets, hits, _ = gidx.enumerate(w["seqs"], np.tile(np.frombuffer(b"NGG", np.uint8), (len(w["guides"]), 1)), mismatches=3)
        gs = api.make_genome_structure(["chr1"], [w["n"]])
        cfd, spec = gidx.score(gs, w["seqs"], 3, offsets, hits)
        assert cfd.shape[0] == hits.shape[0] and gidx.workspace()["score"]["buffers"] > 0
        b = random_batch(np.random.default_rng(11), 64)
        for cfg in (dict(), dict(sam=True)):
            assert device_text(gidx, *b, 3, **cfg) == api.format_guides(*b, 3, **cfg)
        assert gidx.workspace()["text"]["buffers"] > 0
        raw = np.frombuffer(b"".join(g.encode() for g in w["guides"]) * 50, dtype=np.uint8)
        assert api.inflate_bgzf(gidx.bgzf_compress(raw)) == raw.tobytes()
        assert gidx.workspace()["bgzf"]["buffers"] > 0
        # the general path with a bulge: device scratch of the call alone
        live = api.buffers_live()
        off, _ = gidx.enumerate_general(w["seqs"][:4], np.tile(np.frombuffer(b"NGG", np.uint8), (4, 1)), mismatches=1, rna_bulges=1)[:2]
        assert int(off[-1]) > 0 and api.buffers_live() == live
        ws = gidx.workspace()
        held = sum(g["buffers"] for g in ws.values())
        now = api.buffers_live()
        # (the handle's recipe sets hold buffers beside the groups)
        assert now[0] >= before[0] + held > before[0] and now[1] >= before[1] + sum(g["bytes"] for g in ws.values())
        assert all(g["releasable"] <= g["bytes"] for g in ws.values()) and ws["bgzf"]["releasable"] == 0
    assert api.buffers_live() == before


def test_nothing_outlives_a_decoder_or_a_call():
    before = api.buffers_live()
    name, mode = BAM_GOOD[0]
    sq, recs, fasta = dg.loaded(name)
    dec = api.Decoder(sq, fasta, device=0)
    try:
        opened = api.buffers_live()
        assert opened[0] > before[0] and opened[1] > before[1]   # the text and its tables
        want = dg.expected(name, mode).decode()
        rows = dec.decode_records(recs, complete=mode == "complete", on_device=True)
        assert rows == want[want.index("\n") + 1:]
        head, brecs = as_bam(name)
        assert through(dec, head, brecs, mode == "complete") == rows
        assert api.buffers_live()[0] > opened[0]
    finally:
        dec.close()
    assert api.buffers_live() == before
    # the handle-less inflate holds its three buffers for the call
    data = b"".join(bm.members(b"workspace " * 20_000)) + bm.EOF_BLOCK
    assert api.inflate_bgzf(data) == b"workspace " * 20_000
    assert api.buffers_live() == before


def test_the_recovery_releases_the_bulk_buffers_and_only_them(world, capfd):
    w = world
    with built(w) as gidx:
        run(gidx, w, "m3", capfd, what="first")
        a = run(gidx, w, "m3", capfd, what="steady")
        ws = gidx.workspace()
        gidx.set_option("GS_DBG_RELEASE_MIN", "0")
        gidx.set_option("GS_DBG_NOMEM", "1")
        ev = run(gidx, w, "m3", capfd, what="workspace released")
        m = re.search(r"\((\d+) bytes\) of workspace released, batch redone", ev["err"])
        assert m, ev["err"]
        assert int(m.group(1)) == sum(g["releasable"] for g in ws.values()) > 0, (m.group(0), ws)
        assert ev["raw"] == a["raw"]
        after = gidx.workspace()
        for g in api.WORKSPACE_GROUPS:   # what is not bulk was not touched
            assert after[g]["bytes"] - after[g]["releasable"] == ws[g]["bytes"] - ws[g]["releasable"], (g, ws, after)
            assert after[g]["buffers"] <= ws[g]["buffers"]
