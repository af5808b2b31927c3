"""The search pass's form as data (host only; gs_debug_search_form, gs_enumerate.hip: choose_form).  The table the comments
state: no heavy pass - plain (the two seeding launches when every item goes through PAM-pair + deep tables at m <= 4);
dense heavy passes, or any in a batch of at most 64 items per wave slot - heavy; few heavy items and a k-mer interval of
GS_SPLIT_FROM rows or more - split; GS_HEAVY / GS_SPLIT_SHARE override the choice but never where sharing is not allowed."""
from importlib import import_module

import pytest

api = import_module("guidescan-cli_amd.api")

CUS = 256
BIG = 2_000_000          # items of a 1 M guide batch: far beyond 64 per wave slot (256 CUs x 32 waves x 64)
SMALL = 64 * CUS * 32    # at most 64 items per wave slot


def form(**kw):
    base = dict(items=BIG, cus=CUS, share_min=512, backoff=0, main=1, walk=0, one_chunk=1, counting=0, spec=1, m=3)
    base.update(kw)
    return api.search_form(**base)


def test_no_heavy_pass_is_plain():
    f = form()
    assert f["estimate"] == 1 and f["thresh"] == 8 * 512
    assert (f["heavy"], f["split"], f["seed_form"], f["form"]) == (0, 0, 2, 3)   # spec, m <= 4: the two seeding launches
    for kw in (dict(spec=0), dict(m=5), dict(m=6, spec=1)):
        f = form(**kw)
        assert (f["heavy"], f["split"], f["seed_form"], f["form"]) == (0, 0, 0, 0), kw


def test_dense_or_small_batch_is_heavy():
    f = form(est_heavy=BIG // 32)                 # 2 x 62,500 heavy items: one per sixteen
    assert (f["heavy"], f["split"], f["seed_form"], f["form"]) == (1, 0, 0, 1)
    f = form(est_heavy=BIG // 32 - 1)             # just below: not dense
    assert f["heavy"] == 0
    f = form(items=SMALL, est_heavy=1)            # any heavy item in a batch of at most 64 items per wave slot
    assert (f["heavy"], f["form"]) == (1, 1)
    f = form(items=SMALL + 1, est_heavy=1)
    assert f["heavy"] == 0
    # the last batch of the same shape, scaled to this batch's size: 1 heavy pass per 16 items
    assert form(last_hpass=1000, last_items=16_000)["heavy"] == 1
    assert form(last_hpass=999, last_items=16_000)["heavy"] == 0


def test_few_heavy_items_with_a_large_interval_split():
    f = form(est_heavy=8, est_max=1 << 19)
    assert (f["heavy"], f["split"], f["seed_form"], f["form"]) == (0, 2, 0, 2)
    assert form(est_heavy=8, est_max=(1 << 19) - 1)["form"] == 3      # below GS_SPLIT_FROM: plain
    assert form(est_heavy=8, est_max=1000, split_from=1000)["split"] == 2
    assert form(est_heavy=0, est_max=1 << 20)["split"] == 0            # no heavy item seen


@pytest.mark.parametrize("blocked", [dict(backoff=2), dict(counting=1), dict(walk=1), dict(one_chunk=0), dict(main=0),
                                     dict(share_min=0)])
def test_switches_never_force_sharing_where_it_is_not_allowed(blocked):
    for sw in (dict(heavy=1), dict(split_share=1), dict(split_share=2), dict(split_share=3)):
        f = form(**blocked, **sw)
        assert (f["heavy"], f["split"], f["estimate"]) == (0, 0, 0), (blocked, sw)
        assert f["form"] in (0, 3)
    assert form(**blocked, est_heavy=BIG)["heavy"] == 0


def test_switches_override_the_choice():
    assert (form(heavy=1)["heavy"], form(heavy=1)["form"]) == (1, 1)
    f = form(est_heavy=BIG, heavy=0)
    assert (f["heavy"], f["split"], f["form"]) == (0, 0, 3)                 # dense, but GS_HEAVY=0: the unshared forms
    f = form(est_heavy=8, est_max=1 << 20, heavy=0)
    assert f["split"] == 0                                                   # GS_HEAVY drops the split too
    for s in (1, 2, 3):
        f = form(est_heavy=BIG, split_share=s)
        assert (f["heavy"], f["split"], f["form"]) == (0, s, 2)
    f = form(est_heavy=BIG, split_share=0)
    assert (f["heavy"], f["split"]) == (1, 0)                                # 0: no split, the choice stays
    assert form(seed_form=1)["seed_form"] == 1 and form(seed_form=0)["form"] == 0
    assert form(spec=0, seed_form=2)["seed_form"] == 0                       # never where the choice had none


def test_large_share_min_does_not_force_the_heavy_form():
    """8 x share_min saturates at 2^31 rows: GS_SHARE_MIN = 2^29 used to wrap the threshold to 0 (every guide heavy)"""
    for smin in (1 << 28, 1 << 29, (1 << 32) - 1):
        f = form(share_min=smin)
        assert f["thresh"] == 1 << 31
        assert (f["heavy"], f["form"]) == (0, 3)
    assert form(share_min=(1 << 28) - 1)["thresh"] == 8 * ((1 << 28) - 1)


def test_backoff_boundary():
    """the main pass counts the back-off down before it tests it: 1 at the batch's start still shares, 2 does not"""
    assert form(backoff=1)["estimate"] == 1
    assert form(backoff=1, heavy=1)["heavy"] == 1
    assert form(backoff=2)["estimate"] == 0
    assert form(backoff=2, heavy=1)["heavy"] == 0
    assert form(backoff=1, main=0)["estimate"] == 0        # a redo pass neither shares nor counts down
