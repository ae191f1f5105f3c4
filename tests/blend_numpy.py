"""fp64 restatement of the batch-blending operations (include/mvfnet_hip.h: mvf_stem_blend, mvf_soft_targets, mvf_ce_loss_soft), shared by
test_blend_cpu.py and test_blend_gpu.py.  The reference project has neither feature; the semantics are the ones the header states.

Table: rows int32 (B, 5) = partner, y0, x0, y1, x1 (half-open box in image pixels, before the pad); wts fp32 (B, 2) = lam_px, lam_lab."""
import numpy as np

COPY_A, COPY_B, BLEND = 0, 1, 2


def blend_ref(xp, rows, wts, pad):
    """xp (B, T, hp, wp, 4): the STORED operand values (any float dtype; taken to fp64).  Returns (v, kind): v fp64 = the blended operand computed from the
    stored values and the fp32 lam_px, kind int8 (B, hp, wp) = COPY_A / COPY_B / BLEND for every pixel of every frame of the clip."""
    x = np.asarray(xp, dtype=np.float64)
    b, t, hp, wp, _ = x.shape
    v = np.empty_like(x)
    kind = np.empty((b, hp, wp), dtype=np.int8)
    yy, xx = np.meshgrid(np.arange(hp), np.arange(wp), indexing="ij")
    for i in range(b):
        p, y0, x0, y1, x1 = (int(k) for k in rows[i])
        lam = float(np.float32(wts[i, 0]))
        box = (yy >= y0 + pad) & (yy < y1 + pad) & (xx >= x0 + pad) & (xx < x1 + pad)
        kind[i] = np.where(box, COPY_B, COPY_A if (lam == 1.0 or p == i) else BLEND)
        mixed = lam * x[i] + (1.0 - lam) * x[p]
        sel = kind[i][None, :, :, None]
        v[i] = np.where(sel == COPY_B, x[p], np.where(sel == COPY_A, x[i], mixed))
    return v, kind


def paste(x, rows, pad=0):
    """The copies of a CutMix table (lam_px = 1) on the host: x (B, ..., H, W, C) channels-last; returns a new array with every clip's box (shifted by
    pad) replaced by its partner's."""
    out = np.array(x, copy=True)
    for i in range(out.shape[0]):
        p, y0, x0, y1, x1 = (int(k) for k in rows[i])
        out[i][..., y0 + pad:y1 + pad, x0 + pad:x1 + pad, :] = x[p][..., y0 + pad:y1 + pad, x0 + pad:x1 + pad, :]
    return out


def paste_nchw(x, rows):
    """paste() for clips stored (B, T, C, H, W)."""
    out = np.array(x, copy=True)
    for i in range(out.shape[0]):
        p, y0, x0, y1, x1 = (int(k) for k in rows[i])
        out[i][..., y0:y1, x0:x1] = x[p][..., y0:y1, x0:x1]
    return out


def soft_targets_ref(labels, rows, wts, classes, eps, dtype=np.float64):
    """t[i, k] = (1 - eps) * (lam_lab_i * [k == y_i] + (1 - lam_lab_i) * [k == y_partner_i]) + eps / K, every step in `dtype` (np.float32 restates the
    kernel's own arithmetic: with eps == 0 the entries are exactly lam_lab, 1.0f - lam_lab, or their fp32 sum).  rows None: smoothing only."""
    labels = np.asarray(labels).reshape(-1)
    b = labels.shape[0]
    ft = np.dtype(dtype).type
    t = np.zeros((b, classes), dtype=dtype)
    for i in range(b):
        lam, p = (ft(np.float32(wts[i, 1])), int(rows[i, 0])) if rows is not None else (ft(1.0), i)
        v = np.zeros(classes, dtype=dtype)
        v[int(labels[i])] += lam
        v[int(labels[p])] += ft(1.0) - lam
        t[i] = v if eps == 0 else (ft(1.0) - ft(eps)) * v + ft(eps) / ft(classes)
    return t


def ce_soft_ref(scores, targets):
    """fp64: loss_part_i = sum_k t_ik (lse_i - s_ik), loss = mean, dscores = (softmax * sum_k t_ik - t) / clips."""
    s, t = np.asarray(scores, dtype=np.float64), np.asarray(targets, dtype=np.float64)
    mx = s.max(1, keepdims=True)
    e = np.exp(s - mx)
    den = e.sum(1, keepdims=True)
    lse = np.log(den) + mx
    loss_part = (t * (lse - s)).sum(1)
    dscores = (e / den * t.sum(1, keepdims=True) - t) / s.shape[0]
    return loss_part, float(loss_part.mean()), dscores
