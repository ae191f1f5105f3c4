"""mvf_multilabel_sample_ap / mvf_multilabel_prf / mvf_multilabel_best_f1 restated in numpy, as include/mvfnet_hip.h states them, by plain comparison: every
positive of a row against every class of the row, every value against its threshold, every positive of a class as a candidate threshold with the F1
fractions compared exactly (Python integers).  Scores are taken as float32, as the record holds them; a row holding a NaN takes part in nothing."""
from fractions import Fraction

import numpy as np

import multilabel_numpy as mn


def sample_ap(scores, labels):
    """-> dict(ap float64 (rows,), NaN for a row without a positive or holding a NaN; positives int64 (rows,); sample_mAP; rows_with_positives).  The sum of
    TP / N runs over the row's positive classes in ascending order."""
    s = np.asarray(scores, dtype=np.float32)
    y = np.asarray(labels) != 0
    rows = s.shape[0]
    ap, positives = np.full(rows, np.nan), np.zeros(rows, dtype=np.int64)
    for i in np.nonzero(mn.valid_rows(s))[0]:
        pos = np.nonzero(y[i])[0]
        if pos.size == 0:
            continue
        ge = s[i][None, :] >= s[i, pos][:, None]                         # (positives, classes)
        n, tp = ge.sum(axis=1), (ge & y[i][None, :]).sum(axis=1)
        ap[i], positives[i] = np.sum(tp.astype(np.float64) / n.astype(np.float64)) / pos.size, pos.size
    have = positives > 0
    return dict(ap=ap, positives=positives, sample_mAP=float(np.mean(ap[have])) if have.any() else float("nan"), rows_with_positives=int(have.sum()))


def prf_counts(scores, labels, threshold=None, thresholds=None):
    """-> int64 (classes, 4): TP, FP, FN, TN of "value >= theta_c", the thresholds as float32."""
    s = np.asarray(scores, dtype=np.float32)
    ok = mn.valid_rows(s)
    s, y = s[ok], (np.asarray(labels) != 0)[ok]
    th = np.full(s.shape[1], threshold, dtype=np.float32) if thresholds is None else np.asarray(thresholds, dtype=np.float32)
    pred = s >= th[None, :]
    return np.stack([(pred & y).sum(axis=0), (pred & ~y).sum(axis=0), (~pred & y).sum(axis=0), (~pred & ~y).sum(axis=0)], axis=1).astype(np.int64)


def prf_figures(counts):
    """The conventions of evaluation.prf_from_counts, restated with Python arithmetic: a ratio with a zero denominator is 0; macro F1 over the classes with
    at least one positive."""
    def ratio(a, b):
        return a / b if b > 0 else 0.0
    tp, fp, fn = (np.asarray(counts)[:, i].astype(np.int64) for i in range(3))
    f1 = np.array([ratio(2.0 * a, 2.0 * a + b + c) for a, b, c in zip(tp, fp, fn)])
    have = (tp + fn) > 0
    a, b, c = float(tp.sum()), float(fp.sum()), float(fn.sum())
    return dict(precision=np.array([ratio(float(x), float(x + z)) for x, z in zip(tp, fp)]), recall=np.array([ratio(float(x), float(x + z)) for x, z in zip(tp, fn)]),
                f1=f1, micro_precision=ratio(a, a + b), micro_recall=ratio(a, a + c), micro_f1=ratio(2 * a, 2 * a + b + c),
                macro_f1=float(np.mean(f1[have])) if have.any() else float("nan"))


def best_f1(scores, labels):
    """-> dict(best_tp, best_n int64 (classes,), best_threshold float32 (classes,), NaN / 0 / 0 for a class without a positive, positives, best_f1 float64).
    The candidates are the positives' scores, from mvf_multilabel_ap's pair counts; F = 2 TP / (N + |P|) compared as a Fraction, ties to the larger score."""
    s = np.asarray(scores, dtype=np.float32)
    tp, nn = mn.pair_counts(s, labels)
    classes = tp.shape[0]
    positives = (nn > 0).sum(axis=1).astype(np.int64)
    btp, bn, bth = np.zeros(classes, dtype=np.int64), np.zeros(classes, dtype=np.int64), np.full(classes, np.nan, dtype=np.float32)
    for c in range(classes):
        cand = np.nonzero(nn[c])[0]
        if cand.size == 0:
            continue
        k = max(cand, key=lambda i: (Fraction(2 * int(tp[c, i]), int(nn[c, i]) + int(positives[c])), float(s[i, c])))
        btp[c], bn[c], bth[c] = tp[c, k], nn[c, k], s[k, c]
    f = np.full(classes, np.nan)
    have = positives > 0
    f[have] = 2.0 * btp[have] / (bn[have] + positives[have])
    return dict(best_tp=btp, best_n=bn, best_threshold=bth, positives=positives, best_f1=f,
                macro_best_f1=float(np.mean(f[have])) if have.any() else float("nan"))


def best_f1_sweep(scores, labels):
    """The best F1 per class by brute force: every distinct score of the class as the threshold (>=), F1 = 2TP / (2TP + FP + FN) as a Fraction.  -> a list of
    (Fraction | None, threshold): the largest F1 and the largest threshold that attains it."""
    s = np.asarray(scores, dtype=np.float32)
    ok = mn.valid_rows(s)
    s, y = s[ok], (np.asarray(labels) != 0)[ok]
    out = []
    for c in range(s.shape[1]):
        npos = int(y[:, c].sum())
        if npos == 0:
            out.append((None, float("nan")))
            continue
        best = None
        for thr in np.unique(s[:, c]):
            pred = s[:, c] >= thr
            tp, fp = int((pred & y[:, c]).sum()), int((pred & ~y[:, c]).sum())
            f = Fraction(2 * tp, 2 * tp + fp + (npos - tp))
            if best is None or (f, float(thr)) > best:
                best = (f, float(thr))
        out.append(best)
    return out
