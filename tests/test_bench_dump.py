"""bench.py --dump-outputs on the host side: what is written, in which precision, and within the 64 MB budget."""
import os

import numpy as np

import bench

NAMES = ("windspeed", "winddir", "thc", "sb_con")


def _fields(ny, nx, dtype, seed=0):
    rng = np.random.default_rng(seed)
    return {n: rng.standard_normal((ny, nx)).astype(dtype) for n in NAMES}


def _written(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in os.listdir(d)}


def test_small_grid_written_whole(tmp_path):
    for dt in (np.float64, np.float32):
        f = _fields(384, 512, dt)
        out = tmp_path / np.dtype(dt).name
        assert sorted(bench.dump_outputs(str(out), f)) == sorted(NAMES)
        got = _written(out)
        assert sorted(got) == sorted(NAMES)
        for n in NAMES:
            assert got[n].dtype == dt and np.array_equal(got[n], f[n])


def test_large_grid_sampled_within_budget(tmp_path):
    ny, nx = 1280, 2048                                   # 4 x 21 MB in fp64: over the budget
    f = _fields(ny, nx, np.float64)
    assert sum(a.nbytes for a in f.values()) > bench.DUMP_BUDGET
    bench.dump_outputs(str(tmp_path / "a"), f)
    bench.dump_outputs(str(tmp_path / "b"), _fields(ny, nx, np.float64))
    assert sum(os.path.getsize(tmp_path / "a" / n) for n in os.listdir(tmp_path / "a")) <= bench.DUMP_BUDGET
    got, again = _written(tmp_path / "a"), _written(tmp_path / "b")
    assert sorted(got) == sorted(NAMES + ("sample_index",))
    idx = got["sample_index"]
    assert idx.dtype == np.float64 and idx.size == bench.DUMP_SAMPLE
    k = idx.astype(np.int64)
    assert np.array_equal(k, idx) and np.all(np.diff(k) > 0) and k[0] >= 0 and k[-1] < ny * nx
    for n in NAMES:
        assert got[n].dtype == np.float64 and np.array_equal(got[n], f[n].reshape(-1)[k])
        assert np.array_equal(got[n], again[n])         # the same inputs give the same sample
    assert np.array_equal(idx, again["sample_index"])
