"""CPU: the host side of the non-finite step guard -- the configuration check (guard.check_nonfinite_guard, refused by Runner / train_network before anything
is built), the C ABI of mvf_sgd_step_guarded / mvf_bn_stats_snapshot / mvf_bn_stats_restore (header, ctypes signatures, exported symbols) and their argument
checks, which return MVF_EINVAL from host pointers before any launch."""
import ctypes as C
import re

import pytest

EINVAL = -1


# ------------------------------------------------------------------------------------------------ configuration
def test_nonfinite_guard_config_check():
    import numpy as np
    from mvfnet_amd.guard import check_nonfinite_guard
    from mvfnet_amd.runner import Config
    assert check_nonfinite_guard(None) is None
    assert check_nonfinite_guard({}) == dict(max_consecutive=100)
    assert check_nonfinite_guard(dict(max_consecutive=3)) == dict(max_consecutive=3)
    assert check_nonfinite_guard(Config(max_consecutive=1)) == dict(max_consecutive=1)
    out = check_nonfinite_guard(dict(max_consecutive=np.int64(7)))
    assert out == dict(max_consecutive=7) and type(out["max_consecutive"]) is int
    for bad in (True, False, 1.0, 2.5, "3", None, 0, -1):
        with pytest.raises(ValueError, match="max_consecutive"):
            check_nonfinite_guard(dict(max_consecutive=bad))
    with pytest.raises(ValueError, match="unknown key 'max_skips'"):
        check_nonfinite_guard(dict(max_skips=3))
    for bad in (True, 100, "on"):
        with pytest.raises(ValueError, match="nonfinite_guard must be"):
            check_nonfinite_guard(bad)


def test_runner_and_train_network_refuse_a_bad_guard_config_before_anything_is_built():
    from mvfnet_amd.runner import Runner, train_network

    class Untouched(object):
        def __getattr__(self, name):
            raise AssertionError("the model was touched (%s)" % name)
    with pytest.raises(ValueError, match="unknown key"):
        Runner(Untouched(), nonfinite_guard=dict(limit=10))
    with pytest.raises(ValueError, match="max_consecutive"):
        Runner(Untouched(), nonfinite_guard=dict(max_consecutive=0))
    with pytest.raises(ValueError, match="max_consecutive"):
        Runner(Untouched(), nonfinite_guard=dict(max_consecutive=True))
    opt = dict(type="SGD", lr=0.01)
    with pytest.raises(ValueError, match="max_consecutive"):
        train_network(Untouched(), [], dict(nonfinite_guard=dict(max_consecutive=1.5), optimizer=opt))
    with pytest.raises(ValueError, match="unknown key"):
        train_network(Untouched(), [], dict(nonfinite_guard=dict(max=1), optimizer=opt))
    with pytest.raises(ValueError, match="nonfinite_guard must be"):
        train_network(Untouched(), [], dict(nonfinite_guard=True, optimizer=opt))


def test_a_runner_without_the_guard_asks_nothing_new_of_its_engine():
    """The fake engine has none of the guard's methods: a Runner that was not given nonfinite_guard must not miss them."""
    from mvfnet_amd.runner import Runner
    lines = []

    class Engine(object):
        flat_ema, max_norm, initial_lr = None, None, None
        norm_out = [1.5]

        def train_step(self, imgs, labels, lr=None):
            return 0.25

    class Model(object):
        def train_engine(self, **opt):
            return Engine()

        def train(self, mode=True):
            return self
    run = Runner(Model(), logger=lines.append, log_interval=1)
    run.train_epoch([dict(img_group="x", label="y")])
    assert len(lines) == 1 and lines[0].endswith("grad_norm 1.500") and "skipped" not in lines[0]


# ------------------------------------------------------------------------------------------------ the C ABI
NEW = {
    "mvf_sgd_step_guarded": 20,
    "mvf_bn_stats_snapshot": 8,
    "mvf_bn_stats_restore": 9,
}


def _prototype(name):
    import os
    from mvfnet_amd import _lib
    hdr = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(_lib.__file__))), "include", "mvfnet_hip.h")
    txt = re.sub(r"/\*.*?\*/", "", open(hdr).read(), flags=re.S)
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, txt)
    assert m, name
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_header_ctypes_and_library_agree_on_the_new_symbols():
    from mvfnet_amd import _lib
    declared = _lib.declared_symbols()
    for name, nargs in NEW.items():
        assert name in declared
        fn = getattr(_lib.lib, name)               # exported by the shared object
        params = _prototype(name)
        assert fn.restype is C.c_int and len(fn.argtypes) == len(params) == nargs, name
        for p, t in zip(params, fn.argtypes):
            if "*" in p:
                assert t is C.c_void_p, (name, p)
            elif p.startswith("float "):
                assert t is C.c_float, (name, p)
            elif p.startswith("int "):
                assert t is C.c_int, (name, p)
            elif p.startswith("long "):
                assert t is C.c_long, (name, p)
            elif p.startswith("size_t "):
                assert t is C.c_size_t, (name, p)
            else:
                raise AssertionError("unexpected parameter %r of %s" % (p, name))
    assert _lib.lib.mvf_abi_version() == 2         # additions only: no structure or existing prototype changed


# ------------------------------------------------------------------------------------------------ argument checks
class _Host(object):
    """Host arrays standing in for the device operands: the checks return before any launch, so nothing is ever dereferenced."""

    def __init__(self):
        from mvfnet_amd import _lib
        self.L = _lib
        self.f = (C.c_float * 256)()                # params [0, 8), grads [8, 16), momentum [16, 24), ema [24, 32), norm_out [32, 34), ws [64, ...)
        self.guard = (C.c_int * 8)()
        self.stats = (C.c_float * 64)()
        self.flat = (C.c_float * 16)()
        self.cnt = (C.c_longlong * 4)()
        self.cnt_copy = (C.c_longlong * 4)()
        self.seg = (_lib.SgdSegment * 2)(_lib.SgdSegment(0, 1.0, 1.0), _lib.SgdSegment(4, 2.0, 0.0))
        b = self.ptr(self.stats)
        self.table = (_lib.StatSegment * 2)(_lib.StatSegment(b, 0), _lib.StatSegment(b + 64, 4))      # n = 12

    @staticmethod
    def ptr(arr, off=0):
        return C.cast(arr, C.c_void_p).value + off

    def untouched(self):
        return (all(v == 0.0 for v in self.f) and all(v == 0 for v in self.guard) and all(v == 0.0 for v in self.stats) and all(v == 0.0 for v in self.flat)
                and all(v == 0 for v in self.cnt) and all(v == 0 for v in self.cnt_copy))


def test_guarded_step_argument_failures_return_einval_before_any_launch():
    h = _Host()
    lib, err = h.L.lib, h.L.lib.mvf_last_error
    p = h.ptr(h.f)
    ws_bytes = lib.mvf_sgd_workspace_bytes(8)
    ws = (C.c_char * ws_bytes)()
    wsp, g, seg = h.ptr(ws), h.ptr(h.guard), h.ptr(h.seg)

    def step(guard, n=8, segments=None, nseg=0, ema=None, ema_m=0.5, params=p, norm=p + 128):
        return lib.mvf_sgd_step_guarded(params, p + 32, p + 64, n, 1.0, 40.0, 0.01, 0.9, 1e-4, 1, 1, segments, nseg, ema, ema_m, guard, norm, wsp, ws_bytes, None)
    for form in (dict(), dict(ema=p + 96), dict(segments=seg, nseg=2), dict(segments=seg, nseg=2, ema=p + 96)):
        assert step(None, **form) == EINVAL and b"NULL guard" in err(), form
        assert step(g + 2, **form) == EINVAL and b"aligned" in err(), form
        for other, name in ((p, b"params"), (p + 32, b"grads"), (p + 64, b"momentum_buf"), (p + 128, b"norm_out"), (wsp, b"workspace")):
            assert step(other, **form) == EINVAL and b"guard and" in err() and name in err(), (form, name)
        assert step(p - 12, **form) == EINVAL and b"params" in err(), form          # the last of the four ints reaches into params
        assert step(p + 128 + 4, **form) == EINVAL and b"norm_out" in err(), form
        for n in (0, -3):
            assert step(g, n=n, **form) == EINVAL and b"bad argument" in err(), (form, n)
        assert step(g, params=None, **form) == EINVAL, form
        assert step(g, norm=None, **form) == EINVAL, form
    assert step(p + 96 + 8, ema=p + 96) == EINVAL and b"ema" in err()
    assert step(seg + 16, segments=seg, nseg=2) == EINVAL and b"segment table" in err()
    for nseg in (0, -1):
        assert step(g, segments=seg, nseg=nseg) == EINVAL and b"bad argument" in err()
    # the average's own checks, as in the _ema entry points
    assert step(g, ema=p + 96 + 2) == EINVAL and b"aligned" in err()
    assert step(g, ema=p + 16) == EINVAL and b"overlap" in err()
    for m in (-0.25, 1.5, float("nan")):
        assert step(g, ema=p + 96, ema_m=m) == EINVAL and b"ema_momentum" in err(), m
    assert h.untouched()


def test_snapshot_and_restore_argument_failures_return_einval_before_any_launch():
    h = _Host()
    lib, err = h.L.lib, h.L.lib.mvf_last_error
    tab, flat, cnt, cpy, g = C.addressof(h.table), h.ptr(h.flat), h.ptr(h.cnt), h.ptr(h.cnt_copy), h.ptr(h.guard)
    calls = {
        "snapshot": lambda seg=tab, nseg=2, n=12, flat=flat, cnt=cnt, ncount=4, cpy=cpy: lib.mvf_bn_stats_snapshot(seg, nseg, n, flat, cnt, ncount, cpy, None),
        "restore": lambda seg=tab, nseg=2, n=12, flat=flat, cnt=cnt, ncount=4, cpy=cpy, guard=g: lib.mvf_bn_stats_restore(seg, nseg, n, flat, cnt, ncount, cpy,
                                                                                                                           guard, None),
    }
    for name, call in calls.items():
        assert call(seg=None) == EINVAL and b"segment table" in err(), name
        assert call(seg=tab + 4) == EINVAL and b"segment table" in err(), name
        for nseg in (0, -1):
            assert call(nseg=nseg) == EINVAL and b"nseg" in err(), name
        for n in (0, -5):
            assert call(n=n) == EINVAL and b"n=" in err(), name
        assert call(n=1) == EINVAL and b"cannot share" in err(), name
        assert call(flat=None) == EINVAL and b"flat" in err(), name
        assert call(flat=flat + 2) == EINVAL and b"flat" in err(), name
        assert call(ncount=-1) == EINVAL and b"ncount" in err(), name
        assert call(cnt=None) == EINVAL and b"counter" in err(), name
        assert call(cpy=None) == EINVAL and b"counter" in err(), name
        assert call(cnt=cnt + 4) == EINVAL and b"counter" in err(), name
        assert call(cpy=cnt + 8) == EINVAL and b"overlap" in err(), name
    restore = calls["restore"]
    assert restore(guard=None) == EINVAL and b"guard" in err()
    assert restore(guard=g + 2) == EINVAL and b"guard" in err()
    for other, what in ((flat, b"flat"), (flat + 44, b"flat"), (cnt, b"counters"), (cpy + 16, b"copy"), (tab, b"segment table"), (tab + 28, b"segment table")):
        assert restore(guard=other) == EINVAL and b"guard and" in err() and what in err(), what
    assert h.untouched()
