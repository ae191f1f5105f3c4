"""bench.py's plain call on the GPU: the headline line only, `steps` timed steps, and the outputs of the last one dumped the same way every run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
EXTRAS = ("roofline", "cpu_baseline", "other_configs", "replicas")


def _bench(*args):
    r = subprocess.run([sys.executable, os.path.join(REPO, "bench.py"), "--gpus", "1"] + list(args), capture_output=True, text=True, timeout=500, cwd=REPO)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0])


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


@pytest.mark.timeout(900)
def test_plain_train_run_is_the_headline_and_dumps_its_last_step(tmp_path):
    runs = []
    for tag in ("a", "b"):
        d = _bench("--steps", "3", "--warmup", "5", "--clips", "4", "--dump-outputs", str(tmp_path / tag))
        assert all(k in d for k in HEADLINE) and not any(k in d for k in EXTRAS)
        assert d["steps"] == 3 and d["dtype"] == "bf16" and d["higher_is_better"] is True and d["unit"] == "clips/s"
        assert abs(d["value"] - 4 * 1e3 / d["ms_per_step"]) < 1e-2 * d["value"]
        runs.append(_load(str(tmp_path / tag)))
    a, b = runs
    assert sorted(a) == ["grad_norm", "grads_sample", "loss", "params_sample"]
    assert all(v.dtype == np.float32 and np.isfinite(v).all() for v in a.values())
    assert a["loss"].shape == (1,) and a["loss"][0] > 0 and a["grad_norm"][0] > 0
    for k in a:                      # seeded inputs, the same dropout draws: two processes compute the same step
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)


@pytest.mark.timeout(600)
def test_plain_infer_run_dumps_the_scores(tmp_path):
    d = _bench("--mode", "infer", "--steps", "2", "--warmup", "1", "--clips", "2", "--dump-outputs", str(tmp_path))
    assert d["steps"] == 2 and d["dtype"] == "f32" and not any(k in d for k in EXTRAS)
    s = _load(str(tmp_path))
    assert sorted(s) == ["scores"] and s["scores"].shape == (2, 400) and s["scores"].dtype == np.float32 and np.isfinite(s["scores"]).all()
