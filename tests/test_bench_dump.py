"""bench.py --dump-outputs without a GPU: what dump_outputs writes, how it keeps to its size limit, and that its sample
is the same from run to run."""
import os

import numpy as np

import bench


def _arrays(nprob, m, n):
    rng = np.random.default_rng(7)
    return {"x": rng.standard_normal((nprob, n)), "fvec": rng.standard_normal((nprob, m)).astype(np.float32),
            "status": np.zeros(nprob, dtype=np.int32)}


def _size(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_small_outputs_are_written_whole_in_float64(tmp_path):
    a = _arrays(5, 40, 3)
    shapes = bench.dump_outputs(str(tmp_path), a)
    assert shapes == {"x": [5, 3], "fvec": [5, 40], "status": [5]}
    assert sorted(os.listdir(tmp_path)) == ["fvec.npy", "status.npy", "x.npy"]
    for k, v in a.items():
        got = np.load(tmp_path / f"{k}.npy")
        assert got.dtype == np.float64 and np.array_equal(got, v.astype(np.float64))


def test_large_outputs_keep_to_the_limit_with_a_fixed_sample(tmp_path):
    nprob, m, n, limit = 300, 500, 20, 400_000
    a = _arrays(nprob, m, n)
    d1, d2 = tmp_path / "one", tmp_path / "two"
    s1 = bench.dump_outputs(str(d1), a, limit=limit)
    s2 = bench.dump_outputs(str(d2), a, limit=limit)
    assert s1 == s2 and s1["x"] == [nprob, n] and s1["status"] == [nprob]       # the largest array gives way, the others stay whole
    keep = s1["fvec"][0]
    assert 0 < keep < nprob and s1["fvec_index"] == [keep]
    payload = 8 * (nprob * n + nprob + keep * m + keep)
    assert payload <= limit and payload + 8 * (m + 1) > limit                  # as many problems as fit
    assert _size(d1) <= limit + 5 * 128                                        # payload + one .npy header per file
    idx = np.load(d1 / "fvec_index.npy")
    assert np.array_equal(idx, np.load(d2 / "fvec_index.npy")) and np.all(np.diff(idx) > 0)
    assert np.array_equal(np.load(d1 / "fvec.npy"), a["fvec"][idx.astype(int)].astype(np.float64))
