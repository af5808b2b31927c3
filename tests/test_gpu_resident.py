"""The device arrays a handle keeps between calls have one owner each (gs_resident: a strand's arrays, a PAM-pair slot's
tables): what gs_debug_resident reports - arrays and the bytes they count for - follows every table that is built, rebuilt
or dropped, and is what gs_index_device_bytes sums.  The count of arrays is the leak check: nothing here looks at the free
device memory, which moves with other processes' work.

The genome is the low-memory tests' (table depth 12); the guides are 19-mers, so that the spaced tables' key (|X| = 9,
|R| = 7 behind deep tables over 10 guide symbols; |X| = 8 over 11) fits its 32 bits at that depth.

Run on the GPU box with `pytest -m gpu`."""
import re
from importlib import import_module

import numpy as np
import pytest

import oracle_lib as ol
from test_gpu_low_memory import K, built, rot_bytes, rot_copies
from test_gpu_parity import two_sided_genome

api = import_module("guidescan-cli_amd.api")
synth = import_module("guidescan-cli_amd.synth")

pytestmark = pytest.mark.gpu

L = 19
KB = (K - 2, K - 1)   # guide symbols the deep tables are indexed by: the default, and the second value legal at this depth


@pytest.fixture(scope="module")
def world():
    text, fam = two_sided_genome(str(K), 20)
    sampled, _, _, _ = synth.sample_guides(text, 40, seed=3, L=L)
    seqs = np.concatenate([fam[None, 1:], sampled]).astype(np.uint8)   # the family's 19-mer: the symbols next to its PAMs
    pams = np.tile(np.frombuffer(b"NGG", np.uint8), (seqs.shape[0], 1))
    return dict(text=text, n=int(text.shape[0]) + 1, seqs=seqs, pams=pams)


def batch(gidx, w, capfd, m=3):
    """one NGG batch -> what it returned and what the library said about it"""
    capfd.readouterr()
    offsets, hits, _ = gidx.enumerate(w["seqs"], w["pams"], mismatches=m)
    err = capfd.readouterr().err
    ev = dict(raw=(offsets.tobytes(), hits.tobytes()), n_hits=int(offsets[-1]), err=err, launch=gidx.last_launch(),
              spaced_items=gidx.last_counters()["spaced_items"], res=gidx.resident(), bytes=gidx.device_bytes)
    with capfd.disabled():
        print({k: v for k, v in ev.items() if k not in ("raw", "err")})
    return ev


class PairTables:
    """the bytes the PAM-pair slots must count for, from the GS_DEBUG lines of the builders (gs_pairtab.hip): 8 per entry
    of the table and of each rotated copy, 10 per row, 64 per deep entry, the spaced tables' rows and offsets"""

    def __init__(self):
        self.pair, self.deep, self.spaced = {}, {}, {}

    def read(self, err):
        for s, rows, nrot in re.findall(r"PAM-pair table: strand (\d), pair \d+ at context depth \d+: (\d+) of \d+ rows, (\d+) rotated", err):
            self.pair[s] = (8 * 4 ** K * (1 + int(nrot)) + 10 * int(rows), 4 + (int(nrot) > 0))
            self.deep.pop(s, None)     # a table built again starts without the tables derived from it
            self.spaced.pop(s, None)
        for s, lines in re.findall(r"deep table: strand (\d), pair \d+: (\d+) lines", err):
            self.deep[s] = 64 * int(lines)
        for s, rows, direct in re.findall(r"spaced table: strand (\d), pair \d+: (\d+) rows by \d+ key bits \(.*?\), (\d+) direct", err):
            self.spaced[s] = 8 * int(rows) + 16 + 4 * (2 ** int(direct) + 1)
        return self

    @property
    def bytes(self):
        return sum(b for b, _ in self.pair.values()) + sum(self.deep.values()) + sum(self.spaced.values())

    @property
    def arrays(self):
        return sum(a for _, a in self.pair.values()) + len(self.deep) + 2 * len(self.spaced)


STRAND_ARRAYS = 9   # Occ blocks, suffix array, table; the general path's four run arrays; the two 'N' run arrays


@pytest.fixture(scope="module")
def fresh(world):
    """a default handle before its first batch"""
    with built(world) as gidx:
        return dict(res=gidx.resident(), bytes=gidx.device_bytes)


def test_a_fresh_handle_counts_every_array_once(world, fresh):
    w, n = world, world["n"]
    res = fresh["res"]
    # per strand: ... + both context arrays and both exception-row arrays + the inverse suffix array
    assert res["strand_arrays"] == 2 * (STRAND_ARRAYS + 4 + 1) and res["pairtab_arrays"] == 0 and res["pairtab_bytes"] == 0
    assert res["strand_bytes"] == fresh["bytes"]
    blocks = 64 * ((n >> 7) + 1)
    exc = res["strand_bytes"] - 2 * (blocks + 4 * n + 16 * 4 ** K + 6 * n + 4 * n)   # 12 bytes per exception row
    assert exc > 0 and exc % 12 == 0, exc
    with built(w, GS_NO_ISA="1") as gidx:
        r = gidx.resident()
        assert r["strand_arrays"] == 2 * (STRAND_ARRAYS + 4) and r["pairtab_arrays"] == 0
        assert r["strand_bytes"] == gidx.device_bytes == fresh["bytes"] - 2 * 4 * n
    with built(w, GS_NO_CTX="1") as gidx:
        r = gidx.resident()
        assert r["strand_arrays"] == 2 * STRAND_ARRAYS and r["pairtab_arrays"] == 0
        assert r["strand_bytes"] == gidx.device_bytes == 2 * (blocks + 4 * n + 16 * 4 ** K)


def test_pair_deep_and_spaced_tables_built_rebuilt_and_dropped(world, fresh, capfd):
    w = world
    with built(w) as gidx:
        gidx.set_option("GS_NO_PAIRTAB", "1")
        plain = batch(gidx, w, capfd)
        assert plain["launch"]["pair_tables"] == 0 and not plain["launch"]["deep"] and plain["n_hits"] > 100
    # GS_INDEX_BUDGET_GB on the live handle leaves the pair tables room for no rotated copy (one more is 2 x 8 x 4^k bytes):
    # how many a table gets otherwise follows the recipes of the batch that builds it, and a later batch that asks for
    # more builds the whole slot again - then nothing of the first deep tables could be left behind anyway
    tight = f"{(fresh['bytes'] + 600_000_000) / 1e9:.9f}"

    def first_batches(gidx, kb):
        """pair tables under the cap, deep tables over kb guide symbols; the cap lifted, the spaced tables"""
        pt = PairTables()
        gidx.set_options(GS_SPACED_FROM="1", GS_DEEP_SYMBOLS=str(kb), GS_INDEX_BUDGET_GB=tight)
        ev = batch(gidx, w, capfd)
        pt.read(ev["err"])
        assert ev["launch"]["pair_tables"] == 1 and ev["launch"]["deep"] and ev["spaced_items"] == 0, ev["err"]
        assert [a for _, a in pt.pair.values()] == [4, 4] and ev["raw"] == plain["raw"], ev["err"]
        gidx.set_option("GS_INDEX_BUDGET_GB", None)
        ev = batch(gidx, w, capfd)
        pt.read(ev["err"])
        assert ev["launch"]["deep"] and ev["launch"]["x_len"] == L - kb, ev["err"]
        assert ev["spaced_items"] == 2 * w["seqs"].shape[0] and len(pt.pair) == len(pt.deep) == len(pt.spaced) == 2, ev["err"]
        assert pt.deep["0"] == pt.deep["1"] == 64 * 4 ** kb and "PAM-pair table:" not in ev["err"]
        assert ev["raw"] == plain["raw"]
        assert ev["res"] == dict(strand_arrays=fresh["res"]["strand_arrays"], strand_bytes=fresh["bytes"],
                                 pairtab_arrays=pt.arrays, pairtab_bytes=pt.bytes), (ev["res"], pt.__dict__)
        assert ev["bytes"] == fresh["bytes"] + pt.bytes and pt.arrays == 2 * (4 + 1 + 2)
        return ev, pt

    with built(w) as a:
        first, pt = first_batches(a, KB[1])
        first_spaced = sum(pt.spaced.values())
        first_info = a.spaced_rows(0, 0, 0)[2]
        assert (first_info["built"], first_info["x_len"]) == (1, L - KB[1]), first_info
        # deep tables over another number of guide symbols: rebuilt - they alone, the pair tables stay -, and the spaced
        # tables with them at the new |X|: the same arrays, and not a byte of the first ones still counted
        a.set_option("GS_DEEP_SYMBOLS", str(KB[0]))
        ev = batch(a, w, capfd)
        pt.read(ev["err"])
        assert ev["launch"]["deep"] and ev["launch"]["x_len"] == L - KB[0] and ev["spaced_items"] > 0, ev["err"]
        assert "PAM-pair table:" not in ev["err"] and "deep table: strand 1" in ev["err"] and "spaced table: strand 1" in ev["err"], ev["err"]
        assert pt.deep["0"] == pt.deep["1"] == 64 * 4 ** KB[0]
        # the spaced tables are other tables now (|X|, and the key bits kept with a row) of the same size - a table's rows are
        # the pair table's and its direct bits follow from their number -, so that they were rebuilt shows in the tables, not
        # in the bytes: the bytes move with them where they are dropped, below.  The pair tables proper were not touched
        info = a.spaced_rows(0, 0, 0)[2]
        assert (info["built"], info["x_len"], info["key_bits_in_row"]) == (1, L - KB[0], first_info["key_bits_in_row"] + 2), info
        assert sum(pt.spaced.values()) == first_spaced and first["res"]["pairtab_bytes"] - 2 * 64 * 4 ** KB[1] == \
            ev["res"]["pairtab_bytes"] - 2 * 64 * 4 ** KB[0]
        assert ev["raw"] == plain["raw"]
        assert ev["res"]["pairtab_arrays"] == pt.arrays == first["res"]["pairtab_arrays"]
        assert ev["res"]["pairtab_bytes"] == pt.bytes and ev["bytes"] == fresh["bytes"] + pt.bytes, (ev["res"], pt.__dict__)
        with built(w) as b:   # ... as on a handle that only ever ran with that value
            evb, ptb = first_batches(b, KB[0])
            assert pt.pair == ptb.pair, (pt.pair, ptb.pair)
            assert ev["bytes"] == evb["bytes"] and ev["res"] == evb["res"], (ev["res"], evb["res"])

        # the spaced tables dropped (the first rung when a batch runs out of memory): four arrays and their bytes go
        a.set_option("GS_DBG_NOMEM", "1")
        ev = batch(a, w, capfd)
        assert "spaced tables dropped" in ev["err"] and ev["spaced_items"] == 0 and ev["raw"] == plain["raw"], ev["err"]
        sp = sum(pt.spaced.values())
        pt.spaced.clear()
        assert ev["res"]["pairtab_arrays"] == pt.arrays == first["res"]["pairtab_arrays"] - 4
        assert ev["res"]["pairtab_bytes"] == pt.bytes and ev["bytes"] == fresh["bytes"] + pt.bytes and sp > 0


def test_rotated_copies_built_and_released(world, fresh, capfd):
    w = world
    with built(w) as gidx:
        gidx.set_option("GS_NO_PAIRTAB", "1")
        ev = batch(gidx, w, capfd)
        assert ev["launch"]["rot_copies"] == rot_copies(K) and ev["res"]["pairtab_arrays"] == 0
        assert ev["res"]["strand_arrays"] == fresh["res"]["strand_arrays"] + 2
        assert ev["res"]["strand_bytes"] == ev["bytes"] == fresh["bytes"] + rot_bytes(K)
        gidx.set_option("GS_DBG_NOMEM", "1")
        again = batch(gidx, w, capfd)
        assert "rotated table copies dropped" in again["err"] and again["raw"] == ev["raw"], again["err"]
        assert again["res"] == fresh["res"] and again["bytes"] == fresh["bytes"]


def test_rank_resolve_and_prepare_on_call_length_scratch(world, capfd):
    w, n = world, world["n"]
    oidx = ol.OracleIndex(w["text"])
    rng = np.random.default_rng(5)
    try:
        with built(w) as gidx:
            before = gidx.resident()
            for count in (1, 64, 1000):
                for s, h in ((0, oidx.fwd), (1, oidx.rev)):
                    rows = rng.integers(0, n + 1, count).astype(np.uint64)
                    rows[0] = n   # one past the last row: a legal argument of Occ
                    got = gidx.rank_bwt4(rows, strand=s)
                    assert got.tolist() == [[ol.lib().gso_rank_bwt(h, int(r), c) for c in b"ACGT"] for r in rows]
                    rows = rng.integers(0, n, count).astype(np.uint64)
                    rows[-1] = n - 1
                    assert gidx.resolve(rows, strand=s).tolist() == [ol.lib().gso_locate(h, int(r)) for r in rows]
            assert gidx.resident() == before
            # gs_index_prepare leaves what the handle learnt from its batches alone: gs_index::seen, the matches per item
            # seen at each budget, is not readable from outside - what it feeds is: the slots per item of the next batch
            # of that budget (beyond three mismatches), which a `seen` overwritten by the generated few-hit guides would shrink
            batch(gidx, w, capfd, m=4)
            learnt = batch(gidx, w, capfd, m=4)
            slots = gidx.last_counters()["slots_per_item"]
            res = gidx.resident()
            gidx.prepare(4096, L=L, pam="NGG", mismatches=4)
            assert gidx.resident() == res
            ev = batch(gidx, w, capfd, m=4)
            assert gidx.last_counters()["slots_per_item"] == slots and ev["raw"] == learnt["raw"]
    finally:
        oidx.close()
