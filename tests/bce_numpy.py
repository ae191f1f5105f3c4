"""mvf_bce_loss restated in numpy, as include/mvfnet_hip.h states it; dtype = the type all per-row arithmetic runs in (float64 is the reference and the
kernel's own; float32 shows what a single-precision kernel would lose).  Outputs are rounded to float32 once, as the kernel's are, unless raw=True."""
import numpy as np


def bce_elements(scores, targets, pos_weight=None, target_threshold=None, dtype=np.float64):
    """Per element: the loss l and its derivative dl/ds, in `dtype`.  target_threshold None or NaN = off; the comparison is made on the fp32 values."""
    s = np.asarray(scores, dtype=np.float32).astype(dtype)
    t32 = np.asarray(targets, dtype=np.float32)
    if target_threshold is not None and not np.isnan(target_threshold):
        t = (t32 > np.float32(target_threshold)).astype(dtype)
    else:
        t = t32.astype(dtype)
    one = dtype(1.0)
    w = one if pos_weight is None else np.asarray(pos_weight, dtype=np.float32).astype(dtype)[None, :]
    lw = one + (w - one) * t
    e = np.exp(-np.abs(s))
    loss = (one - t) * s + lw * (np.maximum(-s, dtype(0.0)) + np.log1p(e))
    sig = np.where(s >= 0, e / (one + e), one / (one + e))               # sigmoid(-s) without overflow for either sign
    return loss, (one - t) - lw * sig


def bce_loss(scores, targets, pos_weight=None, target_threshold=None, sum_classes=False, dtype=np.float64, raw=False):
    """-> dict(dscores (clips, classes), loss_part (clips), loss): what mvf_bce_loss leaves.  raw=True: the outputs stay in `dtype` (not rounded to
    float32): the reference an error is measured against."""
    clips, classes = np.asarray(scores).shape
    loss, grad = bce_elements(scores, targets, pos_weight, target_threshold, dtype)
    D = dtype(1.0) if sum_classes else dtype(classes)
    loss_part = loss.sum(axis=1) / D
    dscores = grad / (dtype(clips) * D)
    out_t = (lambda v: v) if raw else (lambda v: np.asarray(v, dtype=dtype).astype(np.float32))
    loss_part, dscores = out_t(loss_part), out_t(dscores)
    # the mean is taken over the values as they are stored
    total = out_t(np.asarray(loss_part, dtype=dtype).sum() / dtype(clips))
    return dict(dscores=dscores, loss_part=loss_part, loss=total)


def average_clip_sigmoid(scores):
    """mvf_average_clip_sigmoid in fp64: (1, classes), the mean over the clips of sigmoid(score)."""
    s = np.asarray(scores, dtype=np.float64)
    e = np.exp(-np.abs(s))
    return np.where(s >= 0, 1.0 / (1.0 + e), e / (1.0 + e)).mean(axis=0, keepdims=True)
