"""CPU: the host side of precise BatchNorm -- the argument checks of mvf_bn_stats_accumulate / _finalize / _exchange (csrc/precise_bn.hip; they return before
any launch, from host tables that are only read by the check), the configuration check, checkpoint.averaged_state_dict with calibrated statistics, and the
hook order of the runner (evaluation.PreciseBNHook runs before the evaluation hooks of its epoch)."""
import ctypes as C
import os
from collections import OrderedDict

import pytest
import torch

EINVAL = -1


# ------------------------------------------------------------------------------------------------ the entry points' argument checks
class _Host(object):
    """Two float segments of 4 and 8 elements, a flat fp32 and a flat fp64 array in host memory, and tables over the segments."""

    def __init__(self):
        from mvfnet_amd import _lib
        self.L = _lib
        self.buf = (C.c_float * 64)()
        self.acc = (C.c_double * 16)()
        self.flat = (C.c_float * 16)()
        self.keep = []

    def ptr(self, arr, off=0):
        return C.cast(arr, C.c_void_p).value + off

    def table(self, rows):
        t = (self.L.StatSegment * len(rows))(*[self.L.StatSegment(p, f) for p, f in rows])
        self.keep.append(t)
        return C.addressof(t)

    def good(self):
        return self.table([(self.ptr(self.buf), 0), (self.ptr(self.buf, 64), 4)])      # n = 12


def test_stat_segment_matches_the_header():
    from mvfnet_amd import _lib
    assert C.sizeof(_lib.StatSegment) == 16 and _lib.StatSegment.ptr.offset == 0 and _lib.StatSegment.first.offset == 8
    for name in ("mvf_bn_stats_accumulate", "mvf_bn_stats_finalize", "mvf_bn_stats_exchange"):
        assert name in _lib.declared_symbols() and getattr(_lib.lib, name).restype is C.c_int


def test_argument_failures_return_einval_before_any_launch():
    h = _Host()
    lib, err = h.L.lib, h.L.lib.mvf_last_error
    acc, flat, good = h.ptr(h.acc), h.ptr(h.flat), h.good()
    calls = {
        "accumulate": lambda seg, nseg, n: lib.mvf_bn_stats_accumulate(seg, nseg, n, acc, None),
        "finalize": lambda seg, nseg, n: lib.mvf_bn_stats_finalize(seg, nseg, n, acc, 3, None, None),
        "finalize_flat": lambda seg, nseg, n: lib.mvf_bn_stats_finalize(seg, nseg, n, acc, 3, flat, None),
        "exchange": lambda seg, nseg, n: lib.mvf_bn_stats_exchange(seg, nseg, n, flat, 2, None),
    }
    b = h.ptr(h.buf)
    for name, call in calls.items():
        assert call(None, 2, 12) == EINVAL and b"NULL segment table" in err(), name
        assert call(good, 0, 12) == EINVAL and b"nseg" in err(), name
        assert call(good, -1, 12) == EINVAL and b"nseg" in err(), name
        assert call(good, 2, 0) == EINVAL and b"n=0" in err(), name
        assert call(good, 2, -5) == EINVAL and b"n=-5" in err(), name
        assert call(h.table([(b, 1), (b + 64, 4)]), 2, 12) == EINVAL and b"not at 0" in err(), name
        assert call(h.table([(b, 0), (b + 64, 4), (b + 128, 4)]), 3, 12) == EINVAL and b"ascend" in err(), name          # equal offsets: an empty segment
        assert call(h.table([(b, 0), (b + 64, 8), (b + 128, 4)]), 3, 12) == EINVAL and b"ascend" in err(), name          # descending
        assert call(good, 2, 4) == EINVAL and b"ascend" in err(), name                                                    # the last segment starts at n
        assert call(h.table([(b, 0), (None, 4)]), 2, 12) == EINVAL and b"NULL or misaligned" in err(), name
        assert call(h.table([(b, 0), (b + 66, 4)]), 2, 12) == EINVAL and b"NULL or misaligned" in err(), name
    assert lib.mvf_bn_stats_accumulate(good, 2, 12, None, None) == EINVAL and b"acc" in err()
    assert lib.mvf_bn_stats_accumulate(good, 2, 12, acc + 4, None) == EINVAL and b"acc" in err()
    assert lib.mvf_bn_stats_finalize(good, 2, 12, None, 3, None, None) == EINVAL and b"acc" in err()
    for count in (0, -2):
        assert lib.mvf_bn_stats_finalize(good, 2, 12, acc, count, None, None) == EINVAL and b"count" in err()
        assert lib.mvf_bn_stats_finalize(good, 2, 12, acc, count, flat, None) == EINVAL and b"count" in err()
    assert lib.mvf_bn_stats_exchange(good, 2, 12, None, 0, None) == EINVAL and b"flat" in err()
    for mode in (-1, 3, 7):
        assert lib.mvf_bn_stats_exchange(good, 2, 12, flat, mode, None) == EINVAL and b"mode" in err()
    # a segment that overlaps the flat array of the call
    assert lib.mvf_bn_stats_exchange(good, 2, 12, b + 8, 0, None) == EINVAL and b"overlaps" in err()
    assert lib.mvf_bn_stats_finalize(good, 2, 12, acc, 1, b + 64, None) == EINVAL and b"overlaps" in err()
    assert all(v == 0.0 for v in h.buf) and all(v == 0.0 for v in h.acc) and all(v == 0.0 for v in h.flat)


# ------------------------------------------------------------------------------------------------ configuration
def test_precise_bn_config_check():
    from mvfnet_amd.ema import check_precise_bn
    from mvfnet_amd.runner import Config
    assert check_precise_bn(None) is None
    assert check_precise_bn({}) == dict(num_iters=200, interval=1, weights="live")
    assert check_precise_bn(dict(num_iters=50, weights="both")) == dict(num_iters=50, interval=1, weights="both")
    assert check_precise_bn(Config(interval=5, weights="ema")) == dict(num_iters=200, interval=5, weights="ema")
    with pytest.raises(ValueError, match="unknown key 'momentum'"):
        check_precise_bn(dict(momentum=0.1))
    for key in ("num_iters", "interval"):
        for bad in (0, -1, 1.5, "3", None, True):
            with pytest.raises(ValueError, match=key):
                check_precise_bn({key: bad})
    for bad in ("average", None, 1, ""):
        with pytest.raises(ValueError, match="weights"):
            check_precise_bn(dict(weights=bad))
    with pytest.raises(ValueError, match="precise_bn must be"):
        check_precise_bn(200)


def test_runner_and_train_network_refuse_a_bad_precise_bn_config_before_anything_is_built():
    from mvfnet_amd.evaluation import PreciseBNHook
    from mvfnet_amd.runner import Runner, train_network

    class Untouched(object):
        def __getattr__(self, name):
            raise AssertionError("the model was touched (%s)" % name)
    with pytest.raises(ValueError, match="unknown key"):
        Runner(Untouched(), precise_bn=dict(iters=10))
    with pytest.raises(ValueError, match="num_iters"):
        Runner(Untouched(), precise_bn=dict(num_iters=0))
    with pytest.raises(ValueError, match="needs averaged weights"):
        Runner(Untouched(), precise_bn=dict(weights="ema"))
    opt = dict(type="SGD", lr=0.01)
    with pytest.raises(ValueError, match="weights"):
        train_network(Untouched(), [], dict(precise_bn=dict(weights="averaged"), optimizer=opt))
    with pytest.raises(ValueError, match="interval"):
        train_network(Untouched(), [], dict(precise_bn=dict(interval=0), optimizer=opt))
    with pytest.raises(ValueError, match="needs averaged weights"):
        train_network(Untouched(), [], dict(precise_bn=dict(weights="both"), optimizer=opt))
    with pytest.raises(ValueError, match="weights"):
        PreciseBNHook([], weights="average")
    with pytest.raises(ValueError, match="num_iters"):
        PreciseBNHook([], num_iters=0)


# ------------------------------------------------------------------------------------------------ averaged_state_dict
def _ckpt(bn_stats):
    sd = OrderedDict([("conv.weight", torch.arange(6.0).view(2, 3)), ("bn.weight", torch.ones(2)), ("bn.running_mean", torch.full((2,), 5.0)),
                      ("bn.running_var", torch.full((2,), 2.0)), ("bn.num_batches_tracked", torch.tensor(9)),
                      ("frozen.running_mean", torch.full((2,), -1.0))])
    ema = OrderedDict([("conv.weight", -torch.arange(6.0).view(2, 3)), ("bn.weight", torch.full((2,), 0.5))])
    entry = dict(state_dict=ema, updates=3, momentum=0.1, warmup_steps=0)
    if bn_stats:
        entry["bn_stats"] = OrderedDict([("bn.running_mean", torch.tensor([0.25, -0.0])), ("bn.running_var", torch.tensor([1.5, 3.0]))])
    return dict(meta={}, state_dict=sd, ema=entry)


def test_averaged_state_dict_takes_the_calibrated_statistics_when_the_entry_carries_them(tmp_path):
    from mvfnet_amd.checkpoint import averaged_state_dict
    plain, ck = averaged_state_dict(_ckpt(False)), _ckpt(True)
    # through a file, as a user's checkpoint travels
    path = os.path.join(str(tmp_path), "ck.pth")
    torch.save(ck, path)
    ck = torch.load(path, map_location="cpu", weights_only=False)
    out = averaged_state_dict(ck)
    assert list(out) == list(plain) == list(ck["state_dict"])
    assert torch.equal(out["bn.running_mean"].view(torch.int32), torch.tensor([0.25, -0.0]).view(torch.int32))
    assert torch.equal(out["bn.running_var"], torch.tensor([1.5, 3.0]))
    for k in ("conv.weight", "bn.weight", "bn.num_batches_tracked", "frozen.running_mean"):          # everything else as without them
        assert torch.equal(out[k], plain[k]), k
    assert torch.equal(plain["bn.running_mean"], torch.full((2,), 5.0)) and torch.equal(plain["bn.running_var"], torch.full((2,), 2.0))
    assert torch.equal(ck["state_dict"]["bn.running_mean"], torch.full((2,), 5.0))          # state_dict stays the live model
    out["bn.running_var"].zero_()
    assert torch.equal(ck["ema"]["bn_stats"]["bn.running_var"], torch.tensor([1.5, 3.0]))   # copies
    # a DataParallel-style checkpoint keeps its prefix
    ck = _ckpt(True)
    ck["state_dict"] = OrderedDict(("module." + k, v) for k, v in ck["state_dict"].items())
    assert torch.equal(averaged_state_dict(ck)["module.bn.running_var"], torch.tensor([1.5, 3.0]))
    # what does not fit is refused
    ck = _ckpt(True)
    ck["ema"]["bn_stats"]["other.running_mean"] = torch.zeros(2)
    with pytest.raises(KeyError, match="other.running_mean"):
        averaged_state_dict(ck)
    ck = _ckpt(True)
    ck["ema"]["bn_stats"]["bn.running_var"] = torch.zeros(3)
    with pytest.raises(ValueError, match="bn.running_var"):
        averaged_state_dict(ck)


# ------------------------------------------------------------------------------------------------ hook order
class _Engine(object):
    """Records what the runner and the hooks ask of it."""

    def __init__(self, calls):
        self.calls, self.flat_ema, self.max_norm, self.initial_lr = calls, None, None, None

    def enable_ema(self, **kw):
        self.flat_ema = "on"

    def precise_bn(self, batches, num_iters=200, weights="live"):
        self.calls.append(("precise_bn", weights, num_iters, [tuple(b) for b in batches]))
        return num_iters


class _Model(object):
    training = False

    def __init__(self, calls):
        self.calls = calls

    def train_engine(self, **opt):
        return _Engine(self.calls)

    def train(self, mode=True):
        self.training = mode
        return self


def _eval_hook(calls, **kw):
    from mvfnet_amd.evaluation import EvalTopKAccuracyHook

    class Scored(EvalTopKAccuracyHook):
        def _score(self, runner, prefix):
            calls.append(("eval", prefix))
            return {}
    return Scored([], [0, 1], **kw)


def test_precise_bn_hook_runs_before_the_evaluation_hooks_of_its_epoch():
    from mvfnet_amd.evaluation import PreciseBNHook
    from mvfnet_amd.runner import Runner
    calls = []
    loader = [dict(img_group="x0", label="y0"), dict(img_group="x1", label="y1")]
    # registered AFTER the evaluation hook, over a loader of its own
    run = Runner(_Model(calls), logger=None)
    run.register_hook(_eval_hook(calls))
    hook = run.register_hook(PreciseBNHook(loader, num_iters=7))
    assert run.hooks[0] is hook
    run.train_epoch([])
    assert calls == [("precise_bn", "live", 7, [("x0", "y0"), ("x1", "y1")]), ("eval", "")]
    assert hook.history == [dict(epoch=1, batches=dict(live=7))]
    # Runner(precise_bn=...): over the loader the runner trains from; 'both' = live, then the averaged weights; interval 2 skips the odd epochs
    del calls[:]
    run = Runner(_Model(calls), logger=None, ema=dict(momentum=0.1), precise_bn=dict(num_iters=3, interval=2, weights="both"))
    run.register_hook(_eval_hook(calls, weights="live"))
    run.engine.train_step = lambda *a, **kw: calls.append(("train_step",)) or 0.0
    run.log_interval = 0
    batches = [dict(img_group="a", label="b")]
    run.train_epoch(batches)
    assert calls == [("train_step",), ("eval", "")]
    run.train_epoch(batches)
    assert calls[2:] == [("train_step",), ("precise_bn", "live", 3, [("a", "b")]), ("precise_bn", "ema", 3, [("a", "b")]), ("eval", "")]
    assert run.model.training            # the hook leaves the model in the mode it found it in (train_epoch's)
    # averaged weights asked for, none kept; no loader anywhere
    with pytest.raises(RuntimeError, match="ema_config"):
        PreciseBNHook(loader, weights="ema").after_train_epoch(Runner(_Model([]), logger=None))
    with pytest.raises(RuntimeError, match="no loader"):
        PreciseBNHook().after_train_epoch(Runner(_Model([]), logger=None))
