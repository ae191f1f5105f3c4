"""CPU: sample-wise AP, precision / recall / F1 and the best-F1 thresholds -- the numpy restatements (multilabel_f1_numpy.py) against brute-force
definitions, the host functions of mvfnet_amd.evaluation against the restatements, ties, +-inf, NaN rows, empty classes and rows, the hook's arguments, and
the C entry points' argument failures (from host addresses that are never read)."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

import multilabel_f1_numpy as fn
import multilabel_numpy as mn
from mvfnet_amd import evaluation as ev

TIGHT = 1e-13          # two fp64 sums of at most 157 ratios in [0, 1] in different orders: 157 * 2^-53 = 1.7e-14


def _case(rows, classes, kind, seed=0, density=0.3):
    gen = np.random.default_rng(seed * 7919 + rows * 31 + classes)
    if kind == "ties":
        s = gen.integers(-2, 3, (rows, classes)).astype(np.float32)
    elif kind == "equal":
        s = np.full((rows, classes), 0.5, dtype=np.float32)
    else:
        s = gen.standard_normal((rows, classes)).astype(np.float32)
    return s, (gen.random((rows, classes)) < density).astype(np.uint8)


CASES = [(1, 1, "gauss", 1.0), (7, 3, "ties", 0.5), (40, 65, "gauss", 0.04), (64, 5, "equal", 0.5), (33, 157, "ties", 0.3), (20, 4, "gauss", 0.0),
         (20, 4, "ties", 1.0)]


@pytest.mark.parametrize("rows,classes,kind,density", CASES)
def test_sample_ap_is_average_precision_of_the_transposed_matrix(rows, classes, kind, density):
    s, y = _case(rows, classes, kind, density=density)
    got = fn.sample_ap(s, y)
    ap, positives = ev.average_precision(s.T, y.T)                           # classes and videos change places: one AP per video
    assert np.array_equal(got["positives"], positives) and np.array_equal(np.isnan(got["ap"]), positives == 0)
    have = positives > 0
    assert np.allclose(got["ap"][have], ap[have], rtol=TIGHT, atol=0)
    # and against the independent threshold sweep
    assert np.allclose(got["ap"][have], mn.average_precision_sweep(s.T, y.T)[have], rtol=1e-12, atol=0)
    host_ap, host_pos = ev.sample_average_precision(s, y)
    assert np.array_equal(host_pos, positives) and np.allclose(host_ap[have], got["ap"][have], rtol=TIGHT, atol=0) and np.isnan(host_ap[~have]).all()
    if have.any():
        assert abs(ev.mmit_mean_average_precision(s, y) - got["sample_mAP"]) <= TIGHT and got["rows_with_positives"] == have.sum()
    else:
        assert np.isnan(ev.mmit_mean_average_precision(s, y)) and np.isnan(got["sample_mAP"])


def test_sample_ap_exact_cases_nan_rows_and_inf():
    # one row: scores 4 3 2 1, positives the 1st and 3rd: (1/1 + 2/3) / 2
    got = fn.sample_ap(np.array([[4.0, 3.0, 2.0, 1.0]]), np.array([[1, 0, 1, 0]]))
    assert got["ap"][0] == (1.0 + 2.0 / 3.0) / 2 and got["positives"][0] == 2
    # all scores equal: every positive sees every class, TP / N = |P| / classes
    got = fn.sample_ap(np.zeros((1, 5)), np.array([[1, 1, 0, 0, 0]]))
    assert got["ap"][0] == 2.0 / 5.0
    s, y = _case(30, 6, "gauss", seed=3)
    s[::7, 0], s[1::9, 2] = np.inf, -np.inf
    s[4, 1] = s[29, 5] = np.nan
    y[4] = 1
    y[10] = 0
    got = fn.sample_ap(s, y)
    assert np.isnan(got["ap"][[4, 29, 10]]).all() and (got["positives"][[4, 29, 10]] == 0).all()
    ok = mn.valid_rows(s)
    alone = fn.sample_ap(s[ok], y[ok])
    assert np.array_equal(alone["ap"], got["ap"][ok], equal_nan=True) and alone["sample_mAP"] == got["sample_mAP"]
    host_ap, host_pos = ev.sample_average_precision(s, y)
    assert np.array_equal(host_pos, got["positives"]) and np.allclose(host_ap, got["ap"], rtol=TIGHT, atol=0, equal_nan=True)
    with pytest.raises(ValueError, match="two .videos, classes. matrices"):
        ev.sample_average_precision(s, y[:, :3])


@pytest.mark.parametrize("rows,classes,kind,density", CASES)
def test_prf_counts_are_direct_boolean_counts(rows, classes, kind, density):
    s, y = _case(rows, classes, kind, density=density)
    per_class = np.linspace(-1.5, 1.5, classes).astype(np.float32)
    for kw in (dict(threshold=0.5), dict(threshold=-np.inf), dict(threshold=np.inf), dict(thresholds=per_class)):
        counts = fn.prf_counts(s, y, **kw)
        th = np.full(classes, kw["threshold"], dtype=np.float32) if "threshold" in kw else per_class
        for c in range(classes):
            brute = [0, 0, 0, 0]
            for i in range(rows):
                brute[(0 if y[i, c] else 1) if s[i, c] >= th[c] else (2 if y[i, c] else 3)] += 1
            assert counts[c].tolist() == brute
        assert (counts.sum(axis=1) == rows).all()
        host = ev.precision_recall_f1(s, y, **kw)
        ref = fn.prf_figures(counts)
        assert np.array_equal(host["counts"], counts) and host["counts"].dtype == np.int64
        for k in ("precision", "recall", "f1"):
            assert np.array_equal(host[k], ref[k]), k
        for k in ("micro_precision", "micro_recall", "micro_f1", "macro_f1"):
            assert host[k] == ref[k] or (np.isnan(host[k]) and np.isnan(ref[k])), k


def test_prf_conventions_nan_rows_and_refusals():
    # class 0: never predicted, no positive -> all three ratios 0, left out of macro F1; class 1: TP 1, FP 1, FN 1
    s = np.array([[0.1, 0.9], [0.2, 0.8], [0.3, 0.1]], dtype=np.float32)
    y = np.array([[0, 1], [0, 0], [0, 1]])
    fig = ev.precision_recall_f1(s, y, threshold=0.5)
    assert fig["counts"].tolist() == [[0, 0, 0, 3], [1, 1, 1, 0]]
    assert fig["precision"].tolist() == [0.0, 0.5] and fig["recall"].tolist() == [0.0, 0.5] and fig["f1"].tolist() == [0.0, 0.5]
    assert (fig["micro_precision"], fig["micro_recall"], fig["micro_f1"], fig["macro_f1"]) == (0.5, 0.5, 0.5, 0.5)
    none = ev.precision_recall_f1(s, np.zeros_like(y), threshold=2.0)
    assert none["micro_f1"] == 0.0 and np.isnan(none["macro_f1"])
    # >= : a value equal to the threshold is predicted; the threshold is rounded to fp32 like the record's values
    assert ev.precision_recall_f1(np.array([[np.float32(0.1)]]), np.array([[1]]), threshold=0.1)["counts"].tolist() == [[1, 0, 0, 0]]
    s2 = s.copy()
    s2[1, 0] = np.nan
    assert ev.precision_recall_f1(s2, y, threshold=0.5)["counts"].tolist() == [[0, 0, 0, 2], [1, 0, 1, 0]]
    assert np.array_equal(fn.prf_counts(s2, y, 0.5), ev.precision_recall_f1(s2, y, threshold=0.5)["counts"])
    for kw in (dict(), dict(threshold=0.5, thresholds=[0.5, 0.5]), dict(threshold=float("nan")), dict(threshold="0.5"), dict(threshold=True),
               dict(thresholds=[0.5]), dict(thresholds=[0.5, float("nan")])):
        with pytest.raises(ValueError, match="threshold"):
            ev.precision_recall_f1(s, y, **kw)


@pytest.mark.parametrize("rows,classes,kind,density", CASES)
def test_best_f1_is_the_best_over_every_threshold(rows, classes, kind, density):
    s, y = _case(rows, classes, kind, density=density)
    got = fn.best_f1(s, y)
    sweep = fn.best_f1_sweep(s, y)
    host = ev.best_f1_thresholds(s, y)
    for c in range(classes):
        f, thr = sweep[c]
        if f is None:
            assert (got["best_tp"][c], got["best_n"][c]) == (0, 0) and np.isnan(got["best_threshold"][c]) and np.isnan(got["best_f1"][c])
            continue
        assert Fraction(2 * int(got["best_tp"][c]), int(got["best_n"][c] + got["positives"][c])) == f and float(got["best_threshold"][c]) == thr
        assert got["best_f1"][c] == float(f) or abs(got["best_f1"][c] - float(f)) <= 2e-16
        # the threshold, applied, gives that F1
        fig = fn.prf_figures(fn.prf_counts(s[:, c:c + 1], y[:, c:c + 1], threshold=float(got["best_threshold"][c])))
        assert abs(fig["f1"][0] - float(f)) <= 2e-16
    for k in ("best_tp", "best_n", "positives"):
        assert np.array_equal(host[k], got[k]), k
    assert np.array_equal(host["best_threshold"], got["best_threshold"].astype(np.float64), equal_nan=True)
    assert np.array_equal(host["best_f1"], got["best_f1"], equal_nan=True)
    assert host["macro_best_f1"] == got["macro_best_f1"] or (np.isnan(host["macro_best_f1"]) and np.isnan(got["macro_best_f1"]))


def test_best_f1_exact_cases():
    # scores 4 3 2 1, positives the 1st and 3rd: thresholds 4 -> F = 2/3, 2 -> F = 4/5
    got = fn.best_f1(np.array([[4.0], [3.0], [2.0], [1.0]]), np.array([[1], [0], [1], [0]]))
    assert (got["best_tp"][0], got["best_n"][0], got["best_threshold"][0], got["best_f1"][0]) == (2, 3, 2.0, 0.8)
    # equal F at two thresholds (1 of 1 predicted, |P| = 3: 2/4; 3 of 9: 6/12): the larger score
    s = np.array([9.0, 8, 7, 6, 5, 4, 3, 2, 1, 0])[:, None]
    y = np.array([1, 0, 0, 0, 0, 0, 0, 1, 1, 0])[:, None]
    got = fn.best_f1(s, y)
    assert (got["best_tp"][0], got["best_n"][0], got["best_threshold"][0]) == (1, 1, 9.0) and ev.best_f1_thresholds(s, y)["best_threshold"][0] == 9.0
    # +-inf are values; a NaN row is left out
    s = np.array([[np.inf], [-np.inf], [0.0], [np.nan]], dtype=np.float32)
    y = np.array([[0], [1], [1], [1]])
    got = fn.best_f1(s, y)
    assert (got["best_tp"][0], got["best_n"][0], got["positives"][0]) == (2, 3, 2) and got["best_threshold"][0] == -np.inf
    host = ev.best_f1_thresholds(s, y)
    assert (host["best_tp"][0], host["best_n"][0], host["best_threshold"][0]) == (2, 3, -np.inf)


def test_the_hook_takes_the_new_options_and_keeps_its_defaults():
    labels = np.eye(3)
    h = ev.EvalMeanAPHook([], labels)
    assert (h.sample_map, h.f1_threshold) == (False, None)
    h = ev.EvalMeanAPHook([], labels, sample_map=True, f1_threshold=0.5, weights="both", on_device=True)
    assert (h.sample_map, h.f1_threshold, h.on_device) == (True, 0.5, True)
    for bad in (float("nan"), "0.5", True):
        with pytest.raises(ValueError, match="threshold"):
            ev.EvalMeanAPHook([], labels, f1_threshold=bad)


def test_header_declarations_and_argument_failures():
    from mvfnet_amd import _lib
    lib = _lib.lib
    declared = _lib.declared_symbols()
    for name in ("mvf_multilabel_sample_ap", "mvf_multilabel_prf", "mvf_multilabel_best_f1"):
        assert name in declared and hasattr(lib, name) and getattr(lib, name).restype is C.c_int and getattr(lib, name).argtypes is not None
    assert lib.mvf_abi_version() == 2
    buf = (C.c_double * 64)()
    p = C.cast(buf, C.c_void_p).value
    odd = p + 4                                    # 4-byte aligned, not 8
    nan = float("nan")

    def sample(s=p, y=p, cap=8, k=3, st=p, ap=p, pos=p):
        return lib.mvf_multilabel_sample_ap(s, y, cap, k, st, ap, pos, None)

    def prf(s=p, y=p, cap=8, k=3, st=p, thr=0.5, ths=None, counts=p):
        return lib.mvf_multilabel_prf(s, y, cap, k, st, C.c_float(thr), ths, counts, None)

    def best(s=p, tp=p, nn=p, pos=p, cap=8, k=3, st=p, btp=p, bn=p, bth=p):
        return lib.mvf_multilabel_best_f1(s, tp, nn, pos, cap, k, st, btp, bn, bth, None)
    einval = [(sample, dict(s=None)), (sample, dict(y=None)), (sample, dict(st=None)), (sample, dict(ap=None)), (sample, dict(pos=None)), (sample, dict(st=odd)),
              (sample, dict(ap=odd)), (sample, dict(s=p + 2)), (sample, dict(pos=p + 2)),
              (prf, dict(s=None)), (prf, dict(y=None)), (prf, dict(st=None)), (prf, dict(counts=None)), (prf, dict(thr=nan)), (prf, dict(counts=odd)),
              (prf, dict(st=odd)), (prf, dict(ths=p + 2)), (prf, dict(s=p + 1)),
              (best, dict(s=None)), (best, dict(tp=None)), (best, dict(nn=None)), (best, dict(pos=None)), (best, dict(st=None)), (best, dict(btp=None)),
              (best, dict(bn=None)), (best, dict(bth=None)), (best, dict(pos=odd)), (best, dict(st=odd)), (best, dict(tp=p + 2)), (best, dict(bth=p + 2))]
    for f, kw in einval:
        assert f(**kw) == -1, (f.__name__, kw)     # MVF_EINVAL
        assert b"multilabel_" in lib.mvf_last_error()
    eshape = [(sample, dict(k=0)), (sample, dict(k=65536)), (sample, dict(cap=0)), (sample, dict(cap=2 ** 31)), (prf, dict(k=0)), (prf, dict(k=65536)),
              (prf, dict(cap=0)), (prf, dict(cap=-1)), (best, dict(k=0)), (best, dict(cap=0)), (best, dict(cap=2 ** 30 + 1)), (best, dict(k=65536))]
    for f, kw in eshape:
        assert f(**kw) == -2, (f.__name__, kw)     # MVF_ESHAPE
    assert prf(thr=nan, ths=p, cap=0) == -2        # a NaN scalar beside a vector is no error of its own: the next check answers
    assert all(v == 0.0 for v in buf)
