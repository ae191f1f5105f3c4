"""mvf_multilabel_record / mvf_multilabel_ap restated in numpy, as include/mvfnet_hip.h states them: the pair counts (TP_i, N_i) by plain comparison of
every positive with every row, the fp64 sum of TP_i / N_i, and a second, independent statement of the same average precision as a sweep over the distinct
score thresholds (what scikit-learn's average_precision_score computes)."""
import numpy as np


def valid_rows(scores):
    """Rows that take part: those without a NaN score."""
    return ~np.isnan(np.asarray(scores, dtype=np.float32)).any(axis=1)


def pair_counts(scores, labels):
    """-> tp, nn int64 (classes, rows): TP_i and N_i for each positive i of class c, 0 / 0 elsewhere.  A row holding a NaN takes part in no class."""
    s = np.asarray(scores, dtype=np.float32)
    y = (np.asarray(labels) != 0) & valid_rows(s)[:, None]
    s = np.where(valid_rows(s)[:, None], s, np.float32(np.nan))          # a comparison with a NaN is false
    rows, classes = s.shape
    tp, nn = np.zeros((classes, rows), dtype=np.int64), np.zeros((classes, rows), dtype=np.int64)
    for c in range(classes):
        pos = np.nonzero(y[:, c])[0]
        if pos.size == 0:
            continue
        with np.errstate(invalid="ignore"):
            ge = s[None, :, c] >= s[pos, c][:, None]                     # (positives, rows)
        nn[c, pos] = ge.sum(axis=1)
        tp[c, pos] = (ge & y[None, :, c]).sum(axis=1)
    return tp, nn


def average_precision(scores, labels):
    """-> dict(ap float64 (classes,) with NaN where a class has no positive, positives int64, mAP, classes_with_positives, rows, nan_rows, tp, nn)."""
    tp, nn = pair_counts(scores, labels)
    classes = tp.shape[0]
    ap, positives = np.full(classes, np.nan), (nn > 0).sum(axis=1).astype(np.int64)
    for c in range(classes):
        if positives[c]:
            i = np.nonzero(nn[c])[0]                                     # rows in ascending order
            ap[c] = np.sum(tp[c, i].astype(np.float64) / nn[c, i].astype(np.float64)) / positives[c]
    have = positives > 0
    ok = valid_rows(scores)
    return dict(ap=ap, positives=positives, mAP=float(np.mean(ap[have])) if have.any() else float("nan"), classes_with_positives=int(have.sum()),
                rows=int(ok.sum()), nan_rows=int((~ok).sum()), tp=tp, nn=nn)


def average_precision_sweep(scores, labels):
    """The same AP per class as a sweep over the distinct thresholds in descending order: sum over thresholds of (recall step) * precision, i.e.
    (TP(thr) - TP(previous thr)) / |P| * TP(thr) / N(thr).  No pair counts: an independent statement."""
    s = np.asarray(scores, dtype=np.float64)
    ok = ~np.isnan(s).any(axis=1)
    s, y = s[ok], (np.asarray(labels) != 0)[ok]
    classes = s.shape[1]
    ap = np.full(classes, np.nan)
    for c in range(classes):
        npos = int(y[:, c].sum())
        if npos == 0:
            continue
        acc, prev_tp = 0.0, 0
        for thr in np.unique(s[:, c])[::-1]:
            sel = s[:, c] >= thr
            n, tp = int(sel.sum()), int((sel & y[:, c]).sum())
            acc += (tp - prev_tp) / npos * (tp / n)
            prev_tp = tp
        ap[c] = acc
    return ap
