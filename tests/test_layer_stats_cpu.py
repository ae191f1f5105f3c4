"""CPU: per-parameter training statistics and skipped-step diagnosis -- everything that needs no device: the configuration check, diagnostics.diagnose on
hand-made records, the argument failures of mvf_flat_segment_stats / mvf_bn_stats_nonfinite (from host addresses that are never read), the runner's log
suffix and error text over a stub engine, and a warning-free compile of csrc/layer_stats.hip under the project's flags."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import layer_stats_numpy as ln
from mvfnet_amd import diagnostics as D


# ------------------------------------------------------------------------------------------------ configuration
def test_check_layer_stats_accepts_and_refuses():
    chk = D.check_layer_stats
    assert chk(None) is None
    assert chk({}) == dict(interval=None, on_skip=True, top=1)
    assert chk(dict(interval=np.int64(50), on_skip=False, top=3)) == dict(interval=50, on_skip=False, top=3)
    assert chk(dict(top=2), guard_on=True) == dict(interval=None, on_skip=True, top=2)
    assert chk(dict(on_skip=False), guard_on=False) == dict(interval=None, on_skip=False, top=1)
    with pytest.raises(ValueError, match="unknown key 'every'"):
        chk(dict(every=5))
    with pytest.raises(ValueError, match="layer_stats must be"):
        chk(True)
    for bad in (0, -1, True, 2.0, "20"):
        with pytest.raises(ValueError, match="interval must be"):
            chk(dict(interval=bad))
        with pytest.raises(ValueError, match="top must be"):
            chk(dict(top=bad))
    for bad in (1, None, "yes"):
        with pytest.raises(ValueError, match="on_skip must be"):
            chk(dict(on_skip=bad))
    with pytest.raises(ValueError, match="nonfinite_guard"):
        chk({}, guard_on=False)


def test_runner_and_train_network_refuse_a_bad_config_before_anything_is_built():
    from mvfnet_amd.runner import Runner, train_network

    class Untouched(object):
        def __getattr__(self, name):
            raise AssertionError("the model was touched (%s)" % name)
    with pytest.raises(ValueError, match="unknown key"):
        Runner(Untouched(), layer_stats=dict(every=5), nonfinite_guard={})
    with pytest.raises(ValueError, match="nonfinite_guard"):
        Runner(Untouched(), layer_stats={})                                  # on_skip defaults to True: it needs the guard
    with pytest.raises(ValueError, match="top must be"):
        train_network(Untouched(), [], dict(layer_stats=dict(top=0), nonfinite_guard={}, optimizer=dict(type="SGD", lr=0.01)))
    with pytest.raises(ValueError, match="nonfinite_guard"):
        train_network(Untouched(), [], dict(layer_stats=dict(interval=5), optimizer=dict(type="SGD", lr=0.01)))


# ------------------------------------------------------------------------------------------------ diagnose
BN = ["backbone.bn1.running_mean", "backbone.bn1.running_var", "backbone.layer1.0.bn1.running_mean", "backbone.layer1.0.bn1.running_var"]
PARAMS = ["backbone.conv1.weight", "backbone.bn1.weight", "backbone.layer1.0.conv1.weight", "cls_head.fc_cls.weight", "cls_head.fc_cls.bias"]


def _grad(n_nan=(0,) * 5, n_inf=(0,) * 5, absmax=(1.0,) * 5):
    g = np.zeros(5, ln.FLAT_STATS_DTYPE)
    g["n_nan"], g["n_inf"], g["absmax"] = n_nan, n_inf, absmax
    g["sumsq"] = g["absmax"] ** 2
    return g


def test_diagnose_the_four_kinds():
    all_on = [True] * 5
    # forward: the first non-finite statistic in the table's order, whatever the gradients say
    r = D.diagnose(7, BN, [0, 0, 3, 64], PARAMS, all_on, _grad(n_nan=(9, 9, 9, 9, 9)))
    assert (r["step"], r["kind"], r["where"]) == (7, "forward", "backbone.layer1.0.bn1")
    assert r["detail"]["statistics"] == {BN[2]: 3, BN[3]: 64}
    r = D.diagnose(7, BN, [0, 2, 3, 64], PARAMS, all_on, _grad())
    assert (r["kind"], r["where"]) == ("forward", "backbone.bn1") and r["detail"]["batchnorms_hit"] == 2
    # backward: some but not all -- the LAST poisoned parameter in parameter order
    r = D.diagnose(8, BN, [0, 0, 0, 0], PARAMS, all_on, _grad(n_nan=(5, 1, 1, 0, 0)))
    assert (r["kind"], r["where"]) == ("backward", PARAMS[2]) and r["detail"]["n_nan"] == 1 and r["detail"]["parameters_hit"] == 3
    r = D.diagnose(8, BN, [0, 0, 0, 0], PARAMS, all_on, _grad(n_inf=(0, 0, 0, 2, 0)))
    assert (r["kind"], r["where"], r["detail"]["n_inf"]) == ("backward", PARAMS[3], 2)
    # loss: every trained parameter, the head's included
    r = D.diagnose(9, BN, [0, 0, 0, 0], PARAMS, all_on, _grad(n_nan=(1, 1, 1, 1, 1)))
    assert (r["kind"], r["where"]) == ("loss", PARAMS[4])
    # norm_overflow: nothing non-finite anywhere -- the largest absmax
    r = D.diagnose(10, BN, [0, 0, 0, 0], PARAMS, all_on, _grad(absmax=(1.0, 3e19, 2.0, 1e19, 0.5)))
    assert (r["kind"], r["where"]) == ("norm_overflow", PARAMS[1]) and r["detail"]["absmax"] == 3e19
    assert set(r) == {"step", "kind", "where", "detail"} and r["kind"] in D.KINDS


def test_diagnose_tie_rules_and_untrained_parameters():
    frozen_stem = [False, False, True, True, True]
    # a parameter that is not trained never enters the decision: its NaN does not make a 'backward', and 'every trained' is counted without it
    r = D.diagnose(1, BN, [0, 0, 0, 0], PARAMS, frozen_stem, _grad(n_nan=(4, 4, 0, 0, 0), absmax=(9.0, 9.0, 1.0, 2.0, 2.0)))
    assert (r["kind"], r["where"]) == ("norm_overflow", PARAMS[3])          # equal absmax: the first of equals, among trained ones
    r = D.diagnose(1, BN, [0, 0, 0, 0], PARAMS, frozen_stem, _grad(n_nan=(0, 0, 1, 1, 1)))
    assert (r["kind"], r["where"]) == ("loss", PARAMS[4])
    r = D.diagnose(1, BN, [0, 0, 0, 0], PARAMS, frozen_stem, _grad(n_nan=(0, 0, 1, 0, 1)))
    assert (r["kind"], r["where"]) == ("backward", PARAMS[4])
    # no BatchNorm in training mode (an empty table), nothing trained
    r = D.diagnose(2, [], [], PARAMS, [False] * 5, _grad(n_nan=(1, 1, 1, 1, 1)))
    assert (r["kind"], r["where"]) == ("norm_overflow", None)
    r = D.diagnose(2, [], [], PARAMS, [True] * 5, _grad(n_nan=(1, 1, 1, 1, 1)))
    assert r["kind"] == "loss"
    # records arrive as int64 words from the device: four per parameter
    words = _grad(n_inf=(0, 0, 7, 0, 0)).view(np.int64).reshape(5, 4)
    r = D.diagnose(3, BN, np.zeros(4, np.int64), PARAMS, [True] * 5, words)
    assert (r["kind"], r["where"], r["detail"]["n_inf"]) == ("backward", PARAMS[2], 7)
    with pytest.raises(ValueError, match="diagnose"):
        D.diagnose(3, BN, [0, 0], PARAMS, [True] * 5, _grad())


def test_rows_and_summary():
    g, w, u = _grad(absmax=(1.0, 2.0, 3.0, 4.0, 5.0)), _grad(absmax=(10.0, 0.0, 10.0, 10.0, 10.0)), _grad(absmax=(0.1, 0.0, 0.4, 0.2, 0.3))
    tab = D.rows(PARAMS, [False, True, True, True, True], g, w, u, 0.5)
    assert list(tab) == PARAMS
    assert tab[PARAMS[2]]["grad_norm"] == 1.5 and tab[PARAMS[2]]["grad_absmax"] == 1.5 and tab[PARAMS[2]]["weight_norm"] == 10.0
    assert abs(tab[PARAMS[2]]["update_ratio"] - 0.04) < 1e-15 and np.isnan(tab[PARAMS[1]]["update_ratio"]) and not tab[PARAMS[0]]["trained"]
    # the untrained stem (smallest ratio) and the zero-norm parameter (nan) are left out
    assert D.summary(tab, 1) == " upd/w min 0.02 %s max 0.04 %s gnorm max 2.5 %s" % (PARAMS[3], PARAMS[2], PARAMS[4])
    assert D.summary(tab, 2) == " upd/w min 0.02 %s, 0.03 %s max 0.04 %s, 0.03 %s gnorm max 2.5 %s, 2 %s" % (PARAMS[3], PARAMS[4], PARAMS[2], PARAMS[4], PARAMS[4],
                                                                                                   PARAMS[3])
    assert D.summary({}, 1) == ""


# ------------------------------------------------------------------------------------------------ the restatement itself
def test_restatement_on_a_hand_computed_table():
    x = np.array([3.0, -4.0, np.nan, 1e19, -np.inf, -0.0, 1e-30], np.float32)
    got = ln.flat_segment_stats(x, None, [0, 2, 3, 5])
    assert got["sumsq"].tolist() == [25.0, 0.0, float(np.float64(np.float32(1e19)) ** 2), float(np.float64(np.float32(1e-30)) ** 2)]
    assert got["absmax"].tolist() == [4.0, 0.0, float(np.float32(1e19)), float(np.float32(1e-30))]
    assert got["n_nan"].tolist() == [0, 1, 0, 0] and got["n_inf"].tolist() == [0, 0, 1, 0]
    y = np.array([1.0, -4.0, 0.0, 1e19, -np.inf, 0.0, 0.0], np.float32)
    got = ln.flat_segment_stats(x, y, [0, 2, 3, 5])
    assert got["sumsq"][0] == 4.0 and got["n_nan"].tolist() == [0, 1, 1, 0] and got["n_inf"].tolist() == [0, 0, 0, 0]          # -inf - -inf is a NaN
    assert ln.bn_stats_nonfinite([[1.0, np.nan], [np.inf], [0.0, -0.0, 1e-45]]).tolist() == [1, 1, 0]


# ------------------------------------------------------------------------------------------------ argument failures, no GPU
def test_argument_failures_return_before_any_launch():
    from mvfnet_amd import _lib
    lib = _lib.lib
    EINVAL, EWS = -1, -3
    host = (C.c_double * 4096)()
    base = C.cast(host, C.c_void_p).value
    assert base % 8 == 0
    x, y, first, out, guard, step, ws = base, base + 4096, base + 8192, base + 12288, base + 16384, base + 16400, base + 20480
    n, nseg = 1000, 4
    need = lib.mvf_flat_stats_workspace_bytes(n, nseg)
    assert need == (1 + nseg) * 32 and lib.mvf_flat_stats_workspace_bytes(4097, 1) == 3 * 32
    assert lib.mvf_flat_stats_workspace_bytes(0, 1) == 0 and lib.mvf_flat_stats_workspace_bytes(3, 4) == 0 and lib.mvf_flat_stats_workspace_bytes(3, 0) == 0
    call = lib.mvf_flat_segment_stats
    cases = [
        ((None, None, n, first, nseg, out, None, None, ws, need), EINVAL, b"NULL"),
        ((x, None, n, None, nseg, out, None, None, ws, need), EINVAL, b"NULL"),
        ((x, None, n, first, nseg, None, None, None, ws, need), EINVAL, b"NULL"),
        ((x, None, 0, first, nseg, out, None, None, ws, need), EINVAL, b"n=0"),
        ((x, None, n, first, 0, out, None, None, ws, need), EINVAL, b"nseg=0"),
        ((x, None, 3, first, 4, out, None, None, ws, need), EINVAL, b"nseg=4"),
        ((x + 2, None, n, first, nseg, out, None, None, ws, need), EINVAL, b"4-byte"),
        ((x, y + 1, n, first, nseg, out, None, None, ws, need), EINVAL, b"4-byte"),
        ((x, None, n, first, nseg, out, guard + 2, None, ws, need), EINVAL, b"4-byte"),
        ((x, None, n, first + 4, nseg, out, None, None, ws, need), EINVAL, b"8-byte"),
        ((x, None, n, first, nseg, out + 4, None, None, ws, need), EINVAL, b"8-byte"),
        ((x, None, n, first, nseg, out, guard, step + 4, ws, need), EINVAL, b"8-byte"),
        ((x, None, n, first, nseg, out, None, None, ws + 4, need), EINVAL, b"8-byte"),
        ((x, None, n, first, nseg, out, None, step, ws, need), EINVAL, b"needs the guard"),
        ((x, None, n, first, nseg, x + 3992, None, None, ws, need), EINVAL, b"out overlaps"),
        ((x, out - 3992, n, first, nseg, out, None, None, ws, need), EINVAL, b"out overlaps"),
        ((x, None, n, first, nseg, out, None, None, x + 8, need), EINVAL, b"workspace overlaps"),
        ((x, ws - 3992, n, first, nseg, out, None, None, ws, need), EINVAL, b"workspace overlaps"),
        ((x, None, n, first, nseg, out, None, None, None, need), EWS, b"workspace too small"),
        ((x, None, n, first, nseg, out, None, None, ws, need - 1), EWS, b"workspace too small"),
    ]
    for args, want, text in cases:
        assert call(*(args + (None,))) == want, (args, lib.mvf_last_error())
        assert b"flat_segment_stats" in lib.mvf_last_error() and text in lib.mvf_last_error(), (args, lib.mvf_last_error())
    call = lib.mvf_bn_stats_nonfinite
    cases = [
        ((None, 4, 100, out, None), b"segment table"),
        ((first + 4, 4, 100, out, None), b"segment table"),
        ((first, 0, 100, out, None), b"nseg=0"),
        ((first, 4, 0, out, None), b"n=0"),
        ((first, 4, 3, out, None), b"cannot share"),
        ((first, 4, 100, None, None), b"counts"),
        ((first, 4, 100, out + 4, None), b"counts"),
        ((first, 4, 100, out, guard + 1), b"guard"),
        ((first, 4, 100, first + 32, None), b"overlaps"),
        ((first, 4, 100, out, out + 16), b"guard overlaps"),
    ]
    for args, text in cases:
        assert call(*(args + (None,))) == EINVAL, (args, lib.mvf_last_error())
        assert b"bn_stats_nonfinite" in lib.mvf_last_error() and text in lib.mvf_last_error(), (args, lib.mvf_last_error())


# ------------------------------------------------------------------------------------------------ the runner over a stub engine
ROWS = D.rows(PARAMS, [False, True, True, True, True], _grad(absmax=(1.0, 2.0, 3.0, 4.0, 5.0)), _grad(absmax=(10.0, 0.0, 10.0, 10.0, 10.0)),
              _grad(absmax=(0.1, 0.0, 0.4, 0.2, 0.3)), 1.0)
SUFFIX = " upd/w min 0.02 %s max 0.04 %s gnorm max 5 %s" % (PARAMS[3], PARAMS[2], PARAMS[4])


class _Engine(object):
    flat_ema, max_norm, initial_lr = None, None, None
    norm_out = [1.5]
    accumulated_loss = 0.75

    def __init__(self, skips=()):
        self.calls, self.steps, self.skips, self.enabled, self.armed, self.measured = [], 0, set(skips), None, False, None

    def _step(self, what):
        self.steps += 1
        self.calls.append(what + ("*" if self.armed else ""))
        if self.armed:
            self.measured = self.steps
        self.armed = False

    def train_step(self, imgs, labels, lr=None):
        self._step("step")
        return 0.25

    def accumulate_step(self, imgs, labels):
        self.calls.append("micro")

    def apply_accumulated(self, lr=None):
        self._step("apply")

    def enable_step_guard(self):
        pass

    def guard_state(self):
        seen = [s for s in self.skips if s <= self.steps]
        run = 0
        while self.steps - run in self.skips:
            run += 1
        return dict(skipped_last=self.steps in self.skips, skipped=len(seen), consecutive=run, steps=self.steps)

    def enable_layer_stats(self, on_skip=True):
        self.enabled = on_skip

    def measure_layer_stats(self):
        self.armed = True

    def layer_stats(self):
        self.calls.append("read")
        return dict(step=self.measured, grad_scale=1.0, params=ROWS)

    def last_skip(self):
        seen = [s for s in self.skips if s <= self.steps]
        if not seen:
            return None
        return dict(step=max(seen), kind="backward", where=PARAMS[2], detail={})


class _Model(object):
    def __init__(self, eng):
        self.eng = eng

    def train_engine(self, **opt):
        return self.eng

    def train(self, mode=True):
        return self


BATCH = dict(img_group="x", label="y")
BASE = "Epoch [1] iter %d lr 0.01000 loss_cls 0.2500 grad_norm 1.500"


def test_runner_arms_the_step_before_each_log_point_and_appends_the_suffix():
    from mvfnet_amd.runner import Runner
    lines, eng = [], _Engine()
    run = Runner(_Model(eng), logger=lines.append, log_interval=2, lr=0.01, warmup=None, layer_stats=dict(on_skip=False))
    assert run.layer_stats == dict(interval=None, on_skip=False, top=1) and eng.enabled is False
    run.train_epoch([BATCH] * 5)
    assert eng.calls == ["step", "step*", "read", "step", "step*", "read", "step"]
    assert lines == [(BASE % i) + SUFFIX for i in (2, 4)]
    assert [(h["iter"], h["step"], h["epoch"]) for h in run.layer_stats_history] == [(2, 2, 1), (4, 4, 1)] and run.layer_stats_history[0]["params"] is ROWS
    # an interval of its own: the history fills at every statistics point, the line carries the suffix where the two meet; under accumulation
    lines, eng = [], _Engine()
    run = Runner(_Model(eng), logger=lines.append, log_interval=2, lr=0.01, warmup=None, accumulate=2, layer_stats=dict(interval=1, on_skip=False))
    run.train_epoch([BATCH] * 4)
    assert eng.calls == ["micro", "micro", "apply*", "read", "micro", "micro", "apply*", "read"]
    assert lines == ["Epoch [1] iter 2 lr 0.01000 loss_cls 0.7500 grad_norm 1.500" + SUFFIX] and len(run.layer_stats_history) == 2


def test_runner_names_the_last_skipped_step_in_the_log_line_and_in_the_error():
    from mvfnet_amd.runner import Runner
    lines, eng = [], _Engine(skips=(2,))
    run = Runner(_Model(eng), logger=lines.append, log_interval=1, lr=0.01, warmup=None, nonfinite_guard={}, layer_stats=dict(interval=3))
    assert eng.enabled is True
    run.iter = 10                                    # a resumed run: the guard's count starts at 0, the runner's iter does not
    run.train_epoch([BATCH] * 3)
    note = " (last: iter 12, backward at %s)" % PARAMS[2]
    assert lines == [(BASE % 11) + " skipped 0", (BASE % 12) + " skipped 1" + note + SUFFIX, (BASE % 13) + " skipped 1" + note]
    lines, eng = [], _Engine(skips=(2, 3))
    run = Runner(_Model(eng), logger=lines.append, log_interval=1, lr=0.01, warmup=None, nonfinite_guard=dict(max_consecutive=2), layer_stats=dict(interval=100))
    with pytest.raises(FloatingPointError) as err:
        run.train_epoch([BATCH] * 4)
    text = str(err.value)
    assert "2 consecutive" in text and "iter 2 and iter 3" in text and text.endswith("those of the last good step (last: iter 3, backward at %s)" % PARAMS[2])


def test_log_line_and_error_text_are_unchanged_with_the_option_off():
    """The stub has none of the option's methods here: a Runner that was not given layer_stats must not miss them."""
    from mvfnet_amd.runner import Runner

    class Plain(_Engine):
        enable_layer_stats = measure_layer_stats = layer_stats = last_skip = None
    lines, eng = [], Plain(skips=(1, 2))
    run = Runner(_Model(eng), logger=lines.append, log_interval=1, lr=0.01, warmup=None, nonfinite_guard=dict(max_consecutive=2))
    assert run.layer_stats is None and run.layer_stats_history == []
    with pytest.raises(FloatingPointError) as err:
        run.train_epoch([BATCH] * 3)
    assert lines == [(BASE % 1) + " skipped 1"]
    assert str(err.value) == ("non-finite gradient norm in 2 consecutive optimizer steps (max_consecutive=2), seen between iter 1 and iter 2 of epoch 1; every one was "
                              "skipped on the device: parameters, optimizer state, averaged weights and BatchNorm statistics are those of the last good step")


# ------------------------------------------------------------------------------------------------ the build
def test_layer_stats_kernels_compile_without_warnings(tmp_path):
    from mvfnet_amd import build
    if not os.path.exists(build.HIPCC):
        pytest.skip("no hipcc on this machine")
    src = os.path.join(build.HERE, "csrc", "layer_stats.hip")
    cmd = [build.HIPCC] + [f for f in build.FLAGS if f != "-shared"] + ["-Werror", "-c", src, "-o", str(tmp_path / "layer_stats.o")]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0 and not p.stdout.strip(), p.stdout.decode()
