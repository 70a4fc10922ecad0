"""bench.py --dump-outputs: the writer on the host (no GPU needed); the end-to-end runs are in tests/test_gpu_multirank.py."""
import importlib.util
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench():
    spec = importlib.util.spec_from_file_location("bench_under_test", os.path.join(ROOT, "bench.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_small_outputs_are_written_whole(tmp_path):
    bench = _bench()
    g = torch.Generator().manual_seed(0)
    a = torch.randn(10, 3, 3, generator=g, dtype=torch.float64)
    b = torch.randn(10, generator=g, dtype=torch.float32)
    n = torch.arange(10)
    bench.dump_outputs({"a": (a, 0), "b": (b, 0), "n": (n, 0), "s": (torch.tensor([1.5]), None)}, 10, str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == ["a.npy", "b.npy", "n.npy", "s.npy"]
    ra, rb, rn = (np.load(tmp_path / f) for f in ("a.npy", "b.npy", "n.npy"))
    assert ra.dtype == np.float64 and np.array_equal(ra, a.numpy())
    assert rb.dtype == np.float32 and np.array_equal(rb, b.numpy())
    assert rn.dtype == np.float64 and np.array_equal(rn, np.arange(10.0))


def test_large_outputs_keep_one_seeded_sample_within_the_budget(tmp_path):
    bench = _bench()
    units, budget = 5000, 200_000
    g = torch.Generator().manual_seed(1)
    post = torch.randn(4, units, 6, generator=g, dtype=torch.float64)  # time first, units second
    res = torch.randn(units, generator=g, dtype=torch.float32)
    whole = torch.randn(7, generator=g, dtype=torch.float64)  # no unit axis: kept whole
    outs = {"post": (post, 1), "res": (res, 0), "whole": (whole, None)}
    for d in ("one", "two"):
        bench.dump_outputs(outs, units, str(tmp_path / d), budget=budget)
    files = sorted(os.listdir(tmp_path / "one"))
    assert files == ["post.npy", "res.npy", "sample_index.npy", "whole.npy"]
    assert sum(os.path.getsize(tmp_path / "one" / f) for f in files) <= budget
    idx = np.load(tmp_path / "one" / "sample_index.npy")
    assert idx.dtype == np.float64 and 0 < len(idx) < units and np.all(np.diff(idx) > 0)
    k = idx.astype(np.int64)
    assert np.array_equal(np.load(tmp_path / "one" / "post.npy"), post.numpy()[:, k])
    assert np.array_equal(np.load(tmp_path / "one" / "res.npy"), res.numpy()[k])
    assert np.array_equal(np.load(tmp_path / "one" / "whole.npy"), whole.numpy())
    for f in files:  # the same sample every time
        assert np.array_equal(np.load(tmp_path / "one" / f), np.load(tmp_path / "two" / f))
