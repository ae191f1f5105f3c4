"""CPU: multi-label evaluation -- everything that needs no device: the pair-count restatement of average precision (multilabel_numpy.py) against a sweep
over the thresholds and against scikit-learn where it imports; evaluation.mean_average_precision (the host path) against both; the figures compute()
derives from the kernel's outputs; the header / ctypes declarations and the entry points' argument failures (from host addresses that are never read)."""
import ctypes as C

import numpy as np
import pytest

import multilabel_numpy as mn

AP_BOUND = 1e-12        # sums of at most 300 ratios in [0, 1] in fp64, in different orders: 300 * 2^-53 relative at the very worst


def _case(rows, classes, kind, seed, density=0.3):
    gen = np.random.default_rng(seed * 7919 + rows * 31 + classes)
    if kind == "ties":
        s = gen.integers(-2, 3, (rows, classes)).astype(np.float32)          # five distinct values: heavy ties
    else:
        s = gen.standard_normal((rows, classes)).astype(np.float32)
    return s, (gen.random((rows, classes)) < density).astype(np.uint8)


@pytest.mark.parametrize("kind", ["ties", "gauss"])
def test_pair_counts_equal_the_threshold_sweep_and_the_host_path(kind):
    from mvfnet_amd.evaluation import average_precision, mean_average_precision
    worst = 0.0
    for seed in range(20):
        rows, classes = (1, 7, 64, 65, 300)[seed % 5], (1, 3, 11)[seed % 3]
        s, y = _case(rows, classes, kind, seed)
        ref = mn.average_precision(s, y)
        sweep = mn.average_precision_sweep(s, y)
        ap, positives = average_precision(s, y)
        assert np.array_equal(np.isnan(ref["ap"]), np.isnan(sweep)) and np.array_equal(np.isnan(ref["ap"]), np.isnan(ap))
        assert np.array_equal(positives, ref["positives"]) and np.array_equal(positives, y.sum(axis=0))
        have = positives > 0
        if have.any():
            worst = max(worst, float(np.abs(ref["ap"][have] - sweep[have]).max()), float(np.abs(ref["ap"][have] - ap[have]).max()))
            assert abs(mean_average_precision(s, y) - ref["mAP"]) <= AP_BOUND
        else:
            assert np.isnan(mean_average_precision(s, y)) and np.isnan(ref["mAP"])
    print("worst |AP difference| %.3g (bound %g)" % (worst, AP_BOUND))
    assert worst <= AP_BOUND


def test_against_scikit_learn_where_it_imports():
    metrics = pytest.importorskip("sklearn.metrics")
    for kind in ("ties", "gauss"):
        for seed in range(6):
            s, y = _case(200, 5, kind, seed)
            y[:, 0] = 1                                  # scikit-learn wants a positive in every column it is asked about
            ref = mn.average_precision(s, y)
            for c in range(5):
                if 0 < y[:, c].sum():
                    assert abs(metrics.average_precision_score(y[:, c], s[:, c].astype(np.float64)) - ref["ap"][c]) <= AP_BOUND


def test_edge_cases():
    from mvfnet_amd.evaluation import average_precision, mean_average_precision
    # a worked example: scores 3 2 2 1, positives the first and the last: AP = (1/2) * (1/1 + 2/4)
    s = np.array([[3.0], [2.0], [2.0], [1.0]], dtype=np.float32)
    y = np.array([[1], [0], [0], [1]], dtype=np.uint8)
    ref = mn.average_precision(s, y)
    assert ref["tp"].tolist() == [[1, 0, 0, 2]] and ref["nn"].tolist() == [[1, 0, 0, 4]] and ref["ap"][0] == 0.75 and mean_average_precision(s, y) == 0.75
    # a tie between a positive and a negative counts both at that threshold: (1/1) * 1/2
    assert mn.average_precision(np.array([[1.0], [1.0]], dtype=np.float32), np.array([[1], [0]]))["ap"][0] == 0.5
    # no positive: NaN, left out of the mean; all positives: 1 whatever the scores; every score equal: AP = the positive share
    s, y = _case(50, 4, "gauss", 1)
    y[:, 1], y[:, 2] = 0, 1
    s[:, 3] = 0.25
    ref = mn.average_precision(s, y)
    ap, positives = average_precision(s, y)
    assert np.isnan(ref["ap"][1]) and np.isnan(ap[1]) and ref["ap"][2] == 1.0 and ap[2] == 1.0 and ref["classes_with_positives"] == 3
    assert abs(ref["ap"][3] - y[:, 3].mean()) <= AP_BOUND and abs(ap[3] - y[:, 3].mean()) <= AP_BOUND
    assert abs(ref["mAP"] - np.mean(ref["ap"][[0, 2, 3]])) <= AP_BOUND and abs(mean_average_precision(s, y) - ref["mAP"]) <= AP_BOUND
    # +-inf are ordinary values
    s, y = _case(40, 3, "gauss", 2)
    s[::5, 0], s[1::7, 0], s[::3, 1] = np.inf, -np.inf, -np.inf
    ref, sweep = mn.average_precision(s, y), mn.average_precision_sweep(s, y)
    ap, _ = average_precision(s, y)
    assert np.isfinite(ref["ap"]).all() and np.abs(ref["ap"] - sweep).max() <= AP_BOUND and np.abs(ref["ap"] - ap).max() <= AP_BOUND
    # a row holding a NaN takes part in no class, positives included; the other rows give what they give alone
    s, y = _case(30, 3, "ties", 3)
    s2, y2 = s.copy(), y.copy()
    s2[4, 1] = np.nan
    y2[4] = 1
    ref, alone = mn.average_precision(s2, y2), mn.average_precision(np.delete(s, 4, axis=0), np.delete(y, 4, axis=0))
    ap, positives = average_precision(s2, y2)
    assert (ref["rows"], ref["nan_rows"]) == (29, 1) and np.array_equal(ref["positives"], alone["positives"]) and np.array_equal(positives, alone["positives"])
    assert np.abs(ref["ap"] - alone["ap"]).max() <= AP_BOUND and np.abs(ap - alone["ap"]).max() <= AP_BOUND
    assert (ref["tp"][:, 4] == 0).all() and (ref["nn"][:, 4] == 0).all()
    with pytest.raises(ValueError, match="two \\(videos, classes\\) matrices"):
        average_precision(s, y[:, :2])


def test_figures_from_the_kernels_outputs():
    from mvfnet_amd import _lib
    from mvfnet_amd.metrics import figures_from_ap
    state = np.zeros(_lib.MULTILABEL_STATE_WORDS, dtype=np.int64)
    state[[_lib.MULTILABEL_SLOTS, _lib.MULTILABEL_NAN_ROWS, _lib.MULTILABEL_OVERFLOW, _lib.MULTILABEL_SEEN]] = 10, 2, 0, 10
    fig = figures_from_ap([0.5, np.nan, 1.0], [4, 0, 1], state)
    assert fig["mAP"] == 0.75 and fig["classes_with_positives"] == 2 and (fig["rows"], fig["nan_rows"], fig["overflow"]) == (8, 2, 0)
    assert fig["positives"].dtype == np.int64 and fig["ap"].dtype == np.float64
    assert np.isnan(figures_from_ap([np.nan], [0], state)["mAP"])
    state[[_lib.MULTILABEL_OVERFLOW, _lib.MULTILABEL_SEEN]] = 3, 13
    with pytest.raises(RuntimeError, match="3 of 13 rows did not fit"):
        figures_from_ap([0.5], [1], state)
    assert figures_from_ap([0.5], [1], state, strict=False)["overflow"] == 3


def test_hook_and_metrics_configuration():
    from mvfnet_amd.evaluation import EvalMeanAPHook
    from mvfnet_amd.metrics import DeviceMultiLabelMetrics
    hook = EvalMeanAPHook([], np.eye(3, dtype=bool), interval=2, weights="both", on_device=True)
    assert hook.labels.dtype == np.uint8 and hook.labels.shape == (3, 3) and (hook.interval, hook.weights, hook.on_device) == (2, "both", True)
    with pytest.raises(ValueError, match="weights must be one of"):
        EvalMeanAPHook([], np.eye(3), weights="averaged")
    with pytest.raises(ValueError, match="multi-hot matrix"):
        EvalMeanAPHook([], [0, 1, 2])
    for bad in (dict(num_classes=0, capacity=4), dict(num_classes=3, capacity=0), dict(num_classes=True, capacity=4), dict(num_classes=3, capacity=2.5),
                dict(num_classes=70000, capacity=4)):
        with pytest.raises(ValueError):
            DeviceMultiLabelMetrics(**bad)


def test_header_declarations_and_argument_failures():
    from mvfnet_amd import _lib
    lib = _lib.lib
    declared = _lib.declared_symbols()
    for name in ("mvf_multilabel_record", "mvf_multilabel_ap"):
        assert name in declared and hasattr(lib, name) and getattr(lib, name).restype is C.c_int and getattr(lib, name).argtypes is not None
    hdr = open(_lib.os.path.join(_lib.os.path.dirname(_lib._HERE), "include", "mvfnet_hip.h")).read()
    assert "MVF_MULTILABEL_SLOTS = 0, MVF_MULTILABEL_NAN_ROWS = 1, MVF_MULTILABEL_OVERFLOW = 2, MVF_MULTILABEL_SEEN = 3, MVF_MULTILABEL_STATE_WORDS = 8" in hdr
    assert (_lib.MULTILABEL_SLOTS, _lib.MULTILABEL_NAN_ROWS, _lib.MULTILABEL_OVERFLOW, _lib.MULTILABEL_SEEN, _lib.MULTILABEL_STATE_WORDS) == (0, 1, 2, 3, 8)
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p)
    odd = C.c_void_p(p.value + 2)

    def record(s=p, y=p, rows=2, k=3, rs=p, ry=p, cap=8, st=p):
        return lib.mvf_multilabel_record(s, y, rows, k, rs, ry, cap, st, None)
    for kw in [dict(s=None), dict(y=None), dict(rs=None), dict(ry=None), dict(st=None), dict(s=odd), dict(rs=odd), dict(st=odd)]:
        assert record(**kw) == -1, kw                        # MVF_EINVAL
        assert b"multilabel_record" in lib.mvf_last_error()
    for kw in [dict(k=0), dict(k=-3), dict(rows=-1), dict(cap=0), dict(cap=-4), dict(cap=2 ** 31)]:
        assert record(**kw) == -2, kw                        # MVF_ESHAPE
    assert record(rows=0) == 0                               # nothing to append: no launch

    def ap(rs=p, ry=p, cap=8, k=3, st=p, tp=p, nn=p, out=p, pos=p):
        return lib.mvf_multilabel_ap(rs, ry, cap, k, st, tp, nn, out, pos, None)
    for kw in [dict(rs=None), dict(ry=None), dict(st=None), dict(tp=None), dict(nn=None), dict(out=None), dict(pos=None), dict(rs=odd), dict(tp=odd), dict(nn=odd),
               dict(st=odd), dict(out=odd), dict(pos=odd)]:
        assert ap(**kw) == -1, kw
        assert b"multilabel_ap" in lib.mvf_last_error()
    for kw in [dict(k=0), dict(k=65536), dict(cap=0), dict(cap=2 ** 31)]:
        assert ap(**kw) == -2, kw
    assert all(v == 0.0 for v in buf)
