"""mvf_distill_loss restated in numpy, as include/mvfnet_hip.h states it; dtype = the type all per-row arithmetic runs in (float64 is the reference; the
kernel's own; float32 shows what a single-precision kernel would lose).  Outputs are rounded to float32 once, as the kernel's are."""
import numpy as np


def _lse(x):
    m = x.max(axis=1, keepdims=True)
    return np.log(np.exp(x - m).sum(axis=1, keepdims=True)) + m


def kd_rows(scores, teacher, temperature, dtype=np.float64):
    """Per clip: kd_i = KL(softmax(z / T) || softmax(s / T)) and the softmaxes p (teacher), q (student), in `dtype`."""
    T = dtype(temperature)
    st, zt = scores.astype(dtype) / T, teacher.astype(dtype) / T
    lse_s, lse_z = _lse(st), _lse(zt)
    p, q = np.exp(zt - lse_z), np.exp(st - lse_s)
    kd = (p * ((zt - st) - (lse_z - lse_s))).sum(axis=1)
    return kd, p, q


def distill_loss(scores, teacher, temperature, alpha, dscores_in, loss_part_in, dtype=np.float64, raw=False):
    """-> dict(dscores (clips, classes), loss_part (clips), loss, terms (2)): what mvf_distill_loss leaves.  temperature and alpha travel as fp32, as through
    the C ABI.  raw=True: the outputs stay in `dtype` (not rounded to float32): the reference an error is measured against."""
    T, a = dtype(np.float32(temperature)), dtype(np.float32(alpha))
    clips = scores.shape[0]
    kd, p, q = kd_rows(scores, teacher, T, dtype)
    keep = dtype(1.0) - a
    loss_part = keep * loss_part_in.astype(dtype) + a * (T * T * kd)
    dscores = keep * dscores_in.astype(dtype) + a * T * (q - p) / dtype(clips)
    out_t = (lambda v: v) if raw else (lambda v: np.asarray(v, dtype=dtype).astype(np.float32))
    loss_part, dscores = out_t(loss_part), out_t(dscores)
    # the mean is taken over the NEW values as they are stored
    loss = out_t(np.asarray(loss_part, dtype=dtype).sum() / dtype(clips))
    terms = out_t(np.array([loss_part_in.astype(dtype).sum() / dtype(clips), (T * T * kd).sum() / dtype(clips)]))
    return dict(dscores=dscores, loss_part=loss_part, loss=loss, terms=terms)


def cross_entropy(scores, labels, dtype=np.float64):
    """The head's part in front of it: per-clip softmax cross-entropy against integer labels and its gradient / clips (mvf_ce_loss)."""
    s = scores.astype(dtype)
    lse = _lse(s)
    clips = s.shape[0]
    part = lse[:, 0] - s[np.arange(clips), labels]
    d = np.exp(s - lse)
    d[np.arange(clips), labels] -= 1.0
    return part, d / clips
