"""bench.py's command line and its --dump-outputs writer, without a GPU (a stand-in engine with host tensors)."""
import os
import sys

import numpy as np
import torch

import bench


class _Eng(object):
    def __init__(self, n):
        self.flat_grads = torch.arange(n, dtype=torch.float32)
        self.flat_params = -self.flat_grads
        self.norm_out = torch.tensor([3.0, 0.5])


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_plain_call_runs_only_the_headline(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "3"])
    a = bench.parse()
    assert (a.gpus, a.steps, a.warmup) == (1, 7, 3)
    assert a.full is False and a.dump_outputs is None


def test_full_and_dump_outputs_options(monkeypatch, tmp_path):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--steps", "2", "--full", "--dump-outputs", str(tmp_path)])
    a = bench.parse()
    assert a.full is True and a.dump_outputs == str(tmp_path) and a.steps == 2


def test_dump_outputs_train_is_a_fixed_float32_sample(tmp_path):
    n = bench.DUMP_SAMPLE + 1000003              # larger than the sample: the parameter-sized buffers are sampled
    eng = _Eng(n)
    names = bench.dump_outputs(str(tmp_path / "a"), torch.tensor([1.25]), eng)
    assert names == ["grad_norm", "grads_sample", "loss", "params_sample"]
    a = _load(str(tmp_path / "a"))
    assert sorted(a) == names
    assert all(v.dtype == np.float32 for v in a.values())
    assert sum(os.path.getsize(str(tmp_path / "a" / (k + ".npy"))) for k in a) <= bench.DUMP_LIMIT
    assert a["loss"].tolist() == [1.25] and a["grad_norm"].tolist() == [3.0, 0.5]
    g = a["grads_sample"]
    assert g.shape == (bench.DUMP_SAMPLE,) and (np.diff(g) > 0).all() and g[0] >= 0 and g[-1] < n      # distinct indices, sorted
    np.testing.assert_array_equal(a["params_sample"], -g)                                              # the same indices in both buffers
    bench.dump_outputs(str(tmp_path / "b"), torch.tensor([1.25]), _Eng(n))
    b = _load(str(tmp_path / "b"))
    for k in names:                                                                                    # the same sample every run
        np.testing.assert_array_equal(a[k], b[k])


def test_dump_outputs_small_buffers_whole_and_infer_scores(tmp_path):
    bench.dump_outputs(str(tmp_path / "t"), torch.tensor([0.5]), _Eng(1000))
    t = _load(str(tmp_path / "t"))
    np.testing.assert_array_equal(t["grads_sample"], np.arange(1000, dtype=np.float32))
    scores = torch.randn(3, 400, dtype=torch.float64)
    assert bench.dump_outputs(str(tmp_path / "i"), scores, None) == ["scores"]
    s = _load(str(tmp_path / "i"))["scores"]
    assert s.dtype == np.float32 and s.shape == (3, 400)
    np.testing.assert_array_equal(s, scores.float().numpy())
