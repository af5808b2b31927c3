"""gs_score.hip on synthesized hit lists, bit for bit against the model of tests/score_model.py (which
tests/test_score_model.py holds to the oracle, the golden files and the host formatter on the CPU).

The scoring entry point takes the hit list as an argument, so the edges of its kernels are driven directly:
guides of 0 .. 70,000 hits either side of the 64 / 512 / 4,096 steps, 3 x 10^5 guides through the ticket
scheme of k_score_sum, distance classes cut by --max-off-targets across 64-hit blocks, 0 .. 3,000
chromosomes and positions beyond 2^32, sequence shapes other than 20 + 3.  The outputs are prefilled with NaN
before every call (a guide or hit nobody wrote shows), every case runs with the CFD array given and without
it, and every comparison is for equality of bits.  Run on the GPU box with `pytest -m gpu`."""
from importlib import import_module

import numpy as np
import pytest

import score_model as sm

api = sm.api
synth = import_module("guidescan-cli_amd.synth")

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def handle():
    """a handle for its workspace only: the genome structure a case scores against is the case's own"""
    text, _, _ = synth.make_genome([3000], seed=2)
    g = api.GenomeIndex.build(text, device=0)
    yield g
    g.close()


class DeviceBatch:
    """a builder's batch in HBM with its model facts"""

    def __init__(self, batch):
        import torch
        self.torch = torch
        self.batch = batch
        self.n, self.L, self.P, self.start = batch["seqs"].shape[0], batch["L"], batch["P"], batch["start"]
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()
        self.d_g, self.d_o = up(batch["seqs"]), up(batch["offsets"])
        self.nh = batch["hits"].shape[0]
        self.d_h = up(batch["hits"]) if self.nh else None
        self.gs = api.make_genome_structure([f"c{i}" for i in range(len(batch["lengths"]))], batch["lengths"])
        self.facts = sm.batch_facts(batch["seqs"], self.P, batch["offsets"], batch["hits"], batch["lengths"], self.start)

    def run(self, handle, sam, max_off, want_cfd):
        torch = self.torch
        d_s = torch.full((self.n,), float("nan"), dtype=torch.float32, device="cuda")
        d_c = torch.full((max(self.nh, 1),), float("nan"), dtype=torch.float32, device="cuda") if want_cfd else None
        torch.cuda.synchronize()
        handle.score_device(self.gs, self.d_g.data_ptr(), self.n, self.L, self.P, self.d_o.data_ptr(),
                            self.d_h.data_ptr() if self.d_h is not None else None,
                            d_c.data_ptr() if want_cfd else None, d_s.data_ptr(), sam=sam, start=self.start,
                            max_off_targets=max_off)
        return (d_c.cpu().numpy()[:self.nh] if want_cfd else None), d_s.cpu().numpy()

    def check(self, handle, sam=False, max_off=-1):
        """both buffer layouts of this (sam, max_off) against the model; -> the model's specificities"""
        exp_cfd = self.facts[1]
        exp = sm.specificity_batch(self.batch["offsets"], *self.facts, max_off=max_off, sam=sam)
        for want_cfd in (True, False):
            cfd, spec = self.run(handle, sam, max_off, want_cfd)
            bad = np.flatnonzero(spec.view(np.uint32) != exp.view(np.uint32))
            assert bad.size == 0, (f"{bad.size} of {self.n} specificities differ (sam={sam}, max_off={max_off}, cfd array "
                                   f"{want_cfd}); first: " + str([(int(g), spec[g], exp[g]) for g in bad[:5]]))
            if want_cfd:
                bad = np.flatnonzero(cfd.view(np.uint32) != exp_cfd.view(np.uint32))
                assert bad.size == 0, (f"{bad.size} of {self.nh} CFDs differ (sam={sam}, max_off={max_off}); first: " +
                                       str([(int(h), cfd[h], exp_cfd[h]) for h in bad[:5]]))
        return exp


@pytest.fixture(scope="module")
def ladder():
    return DeviceBatch(sm.build_ladder())


@pytest.fixture(scope="module")
def maxoff():
    return DeviceBatch(sm.build_maxoff())


def test_length_ladder_and_perfect_hit_rules(handle, ladder):
    """k_score_sum's rounds of 512 and its chain's steps of 32 / 64, k_score_hits' chunks of 4,096: hit counts
    0 .. 70,000 either side of every step, empty guides at the chunk edges, the last guide's loads past the
    array's end; and where the perfect hit comes from (tests/test_score_model.py pins what the batch holds)"""
    exp = ladder.check(handle)
    named = ladder.batch["named"]
    one = np.float32(1.0)
    assert exp[named["only_xAG"]] < one / np.float32(1.4)       # 1 + two xAG scores of 0.259...
    assert exp[named["perfect_forward"]] <= one and exp[0] == one and exp[-1] == one
    ladder.check(handle, sam=True)   # the same sums through the SAM flag


@pytest.mark.parametrize("max_off", sm.MAXOFF_VALUES)
def test_max_off_targets_ladder(handle, maxoff, max_off):
    """k_score_sum_maxoff's carry (cur_d, raw, kept) across 64-hit blocks, the CSV rule (raw index) and the SAM
    rule (hits that resolved), cuts either side of a block and far beyond one"""
    csv = maxoff.check(handle, sam=False, max_off=max_off)
    sam = maxoff.check(handle, sam=True, max_off=max_off)
    if max_off >= 1:
        assert (csv.view(np.uint32) != sam.view(np.uint32)).any()


def test_max_off_ladder_uncut(handle, maxoff):
    maxoff.check(handle)
    maxoff.check(handle, sam=True)


def test_many_guides_take_the_ticket_path(handle):
    """n = 1,200 x CUs + 7 guides: by gs_score_device's launch arithmetic the first 128 x CUs tickets are one guide
    each, the others four, and the last ticket is cut at n; every guide must be written exactly once, in the
    order k_score_place gives.  Once more with max_off = 1: the grid-stride kernel."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    n = 1200 * cus + 7
    waves = min((n + 3) // 4, cus * 8) * 4
    p0 = min(n, 4 * waves)
    take = min(64, max(1, (n - p0) // (waves * 8)))
    assert take == 4 and (n - p0) % take != 0
    t = DeviceBatch(sm.build_tickets(n))
    assert t.nh < 10 ** 6
    exp = t.check(handle)
    assert len(set(exp.view(np.uint32).tolist())) > 1000
    t.check(handle, sam=False, max_off=1)
    t.check(handle, sam=True, max_off=1)


@pytest.mark.parametrize("structure", sm.geometry_structures(), ids=lambda s: s[0])
def test_chromosome_geometry(handle, structure):
    """the 4,096-bin table and its walk-on bit, bin_shift == 0, the memory path beyond 2,048 chromosomes, empty
    chromosomes, positions beyond 2^32, no chromosome at all: one hit per guide, every offset -24 .. 24 around
    the joins with both signs.  SAM with max_off = 5 reads the fact bytes where the plain run reads cfm."""
    name, lengths, joins = structure
    b = DeviceBatch(sm.build_geometry(lengths, joins))
    exp = b.check(handle)
    dropped = b.facts[2]
    assert dropped.all() if not lengths else (dropped.any() and not dropped.all())
    b.check(handle, sam=True, max_off=5)
    b.check(handle, sam=False, max_off=5)
    assert len(set(exp.tolist())) >= (1 if not lengths else 3)


@pytest.mark.parametrize("L,P,start", sm.SHAPES, ids=lambda v: str(int(v)))
def test_sequence_shapes(handle, L, P, start):
    """pam_len and `scored` away from 20 + 3, and the perfect-hit test reading positions 21 and 22 wherever they
    fall: the CFD is 1.0 wherever the reference says "not a 20-mer with a 3-symbol PAM" """
    b = DeviceBatch(sm.build_shape(L, P, start))
    if L != 20 or L + P < 23:
        assert (b.facts[1] == np.float32(1.0)).all()
    for sam, max_off in ((False, -1), (True, -1), (False, 3), (True, 3)):
        b.check(handle, sam=sam, max_off=max_off)
