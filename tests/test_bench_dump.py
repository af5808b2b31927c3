"""bench.py --dump-outputs: the arrays written from the last timed step's CSR result (host logic only: the copy back from HBM
is the library's own buffers, exercised on the GPU box by the bench itself).  Exact in float64, within the byte budget, the
same sample for the same result, whole guides only."""
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
import bench  # noqa: E402

HIT = [("pos", "<i8"), ("key", "<u8")]


def fake_result(n, seed=1, mean_hits=3.0):
    rng = np.random.default_rng(seed)
    counts = rng.poisson(mean_hits, n).astype(np.uint64)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    hits = np.empty(int(off[-1]), dtype=HIT)
    hits["pos"] = rng.integers(-3_100_000_000, 3_100_000_000, hits.shape[0])
    hits["key"] = rng.integers(0, 1 << 63, hits.shape[0], dtype=np.uint64) | (rng.integers(0, 2, hits.shape[0], dtype=np.uint64) << np.uint64(63))
    return off, hits


def nbytes(files):
    return sum(a.nbytes for a in files.values())


def test_everything_fits_and_is_exact():
    off, hits = fake_result(1000)
    f = bench.output_arrays(off, hits)
    assert set(f) == {"hit_counts", "hits"} and all(a.dtype == np.float64 for a in f.values())
    assert np.array_equal(f["hit_counts"], np.diff(off).astype(np.float64))
    t = f["hits"]
    assert t.shape == (hits.shape[0], 4)
    assert np.array_equal(t[:, 0], np.repeat(np.arange(1000), np.diff(off).astype(np.int64)))
    assert np.array_equal(t[:, 1].astype(np.int64), hits["pos"])
    key = (t[:, 2].astype(np.uint64) << np.uint64(32)) | t[:, 3].astype(np.uint64)
    assert np.array_equal(key, hits["key"])


def test_a_large_result_is_sampled_by_whole_guides_within_the_budget():
    off, hits = fake_result(5000, mean_hits=40.0)
    budget = 1 << 20
    f = bench.output_arrays(off, hits, budget=budget)
    assert nbytes(f) + 4096 <= budget
    t = f["hits"]
    assert 0 < t.shape[0] < hits.shape[0]
    g = np.unique(t[:, 0]).astype(np.int64)
    counts = np.diff(off).astype(np.int64)
    assert t.shape[0] == counts[g].sum()                   # every hit of each guide taken
    assert np.all(np.diff(t[:, 0]) >= 0)                   # in guide order
    rows = np.concatenate([np.arange(off[i], off[i + 1]) for i in g]).astype(np.int64)
    assert np.array_equal(t[:, 1].astype(np.int64), hits["pos"][rows])
    again = bench.output_arrays(off.copy(), hits.copy(), budget=budget)
    assert all(np.array_equal(f[k], again[k]) for k in f)   # the same result gives the same files


def test_many_guides_are_sampled_and_scores_follow_the_rows():
    off, hits = fake_result(20000, mean_hits=1.0)
    cfd = np.random.default_rng(3).random(hits.shape[0]).astype(np.float32)
    spec = np.random.default_rng(4).random(20000).astype(np.float32)
    budget = 1 << 18
    f = bench.output_arrays(off, hits, cfd, spec, budget=budget)
    assert set(f) == {"hit_counts", "hits", "cfd", "specificity", "guides"}
    assert nbytes(f) + 4096 <= budget
    g = f["guides"].astype(np.int64)
    assert g.size < 20000 and np.all(np.diff(g) > 0)
    assert np.array_equal(f["hit_counts"], np.diff(off).astype(np.float64)[g])
    assert np.array_equal(f["specificity"], spec[g]) and f["cfd"].dtype == np.float32
    t = f["hits"]
    assert f["cfd"].shape[0] == t.shape[0]
    for r in range(0, t.shape[0], 97):
        i = int(t[r, 0])
        j = int(np.searchsorted(t[:, 0], i))                # first row of guide i
        assert f["cfd"][r] == cfd[int(off[i]) + r - j]


def test_no_hits():
    off = np.zeros(11, dtype=np.uint64)
    f = bench.output_arrays(off, np.empty(0, dtype=HIT))
    assert f["hits"].shape == (0, 4) and np.array_equal(f["hit_counts"], np.zeros(10))
