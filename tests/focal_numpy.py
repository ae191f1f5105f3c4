"""mvf_focal_loss restated in numpy float64, from the text of include/mvfnet_hip.h (no torch softplus: its threshold of 20 costs 2e-9).  Outputs are rounded
to float32 once, as the kernel's are, unless raw=True."""
import numpy as np


def focal_elements(scores, targets, gamma_pos=0.0, gamma_neg=0.0, margin=0.0, alpha=None, class_weight=None, target_threshold=None):
    """Per element: the loss l and its derivative dl/ds, float64.  alpha None or < 0 = off; target_threshold None or NaN = off (the comparison is made on
    the fp32 values).  The settings are rounded to fp32 first: they travel as floats."""
    s = np.asarray(scores, dtype=np.float32).astype(np.float64)
    t32 = np.asarray(targets, dtype=np.float32)
    if target_threshold is not None and not np.isnan(target_threshold):
        t = (t32 > np.float32(target_threshold)).astype(np.float64)
    else:
        t = t32.astype(np.float64)
    gp, gn, m = (float(np.float32(v)) for v in (gamma_pos, gamma_neg, margin))
    if alpha is None or alpha < 0:
        ap = an = 1.0
    else:
        ap = float(np.float32(alpha))
        an = 1.0 - ap
    c = 1.0
    if class_weight is not None:
        c = np.asarray(class_weight, dtype=np.float32).astype(np.float64)[None, :]
        c = np.where(np.isfinite(c), c, np.nan)
    with np.errstate(invalid="ignore", divide="ignore"):
        e = np.exp(-np.abs(s))
        big, small = 1.0 / (1.0 + e), e / (1.0 + e)
        p, pn = np.where(s >= 0, big, small), np.where(s >= 0, small, big)        # sigmoid(s), sigmoid(-s): both from e
        logp = -(np.maximum(-s, 0.0) + np.log1p(e))
        wp = np.ones_like(s) if gp == 0 else pn ** gp
        lpos = -wp * logp
        on = p > m
        pm = np.where(on, p - m, 0.0)
        log1m_on = -(np.maximum(s, 0.0) + np.log1p(e)) if m == 0 else np.log(pn + m)
        log1m = np.where(on, log1m_on, 0.0)
        wn = np.ones_like(s) if gn == 0 else pm ** gn
        lneg = -wn * log1m
        loss = c * (ap * t * lpos + an * (1.0 - t) * lneg)
        dpos = wp * (gp * p * logp - pn)
        dpm = np.where(on, p * pn, 0.0)
        ratio = np.where(on, p if m == 0 else dpm / (pn + m), 0.0)
        dneg = wn * ratio
        if gn != 0:
            dneg = -(gn * (np.ones_like(s) if gn == 1 else pm ** (gn - 1.0)) * dpm) * log1m + dneg
        grad = c * (ap * t * dpos + an * (1.0 - t) * dneg)
    grad = np.where(np.isnan(s), np.nan, grad)
    return loss, grad


def focal_loss(scores, targets, gamma_pos=0.0, gamma_neg=0.0, margin=0.0, alpha=None, class_weight=None, target_threshold=None, sum_classes=False, raw=False):
    """-> dict(dscores (clips, classes), loss_part (clips), loss): what mvf_focal_loss leaves.  raw=True: float64, not rounded."""
    clips, classes = np.asarray(scores).shape
    loss, grad = focal_elements(scores, targets, gamma_pos, gamma_neg, margin, alpha, class_weight, target_threshold)
    D = 1.0 if sum_classes else float(classes)
    loss_part = loss.sum(axis=1) / D
    dscores = grad / (float(clips) * D)
    out_t = (lambda v: v) if raw else (lambda v: np.asarray(v, dtype=np.float64).astype(np.float32))
    loss_part, dscores = out_t(loss_part), out_t(dscores)
    total = out_t(np.asarray(loss_part, dtype=np.float64).sum() / float(clips))          # the mean is taken over the values as they are stored
    return dict(dscores=dscores, loss_part=loss_part, loss=total)
