"""Batch blending for fine-tuning: Mixup and CutMix as mmaction configures them (train_cfg=dict(blending=dict(type='MixupBlending', alpha=.2))).

A blending object only DRAWS the step's table on the host; pixels and labels are blended on the device by mvf_stem_blend / mvf_soft_targets
(csrc/blend.hip), behind every input path of the train engine.  The table, per clip of the batch:

    rows int32 (B, 5): partner, y0, x0, y1, x1     half-open box in image pixels, 0 <= y0 <= y1 <= h, 0 <= x0 <= x1 <= w, 0 <= partner < B
    wts  fp32  (B, 2): lam_px, lam_lab             weight of the clip's own pixel outside the box / of its own label, both in [0, 1]

Inside the box the clip takes its partner's pixels; outside, lam_px * own + (1 - lam_px) * partner.  Mixup: an empty box, lam_px = lam_lab = lambda.  CutMix:
lam_px = 1, a box, lam_lab = 1 - box_area / (h * w).  As in mmaction, one lambda ~ Beta(alpha, alpha) and one random permutation serve the whole batch.
"""
import numbers

import numpy as np

ROW_COLS, WT_COLS = 5, 2


def _alpha(alpha, who):
    if isinstance(alpha, (bool, np.bool_)) or not isinstance(alpha, numbers.Real) or not alpha > 0 or not np.isfinite(alpha):
        raise ValueError("%s: alpha must be a positive number (got %r)" % (who, alpha))
    return float(alpha)


class _Blending(object):
    def __init__(self, alpha, seed=None):
        self.alpha = _alpha(alpha, type(self).__name__)
        self.seed = seed
        self.rng = np.random.default_rng(seed)

    def __repr__(self):
        return "%s(alpha=%g, seed=%r)" % (type(self).__name__, self.alpha, self.seed)


class MixupBlending(_Blending):
    """mixed = lambda * clip + (1 - lambda) * clip[perm], labels likewise (mmaction MixupBlending)."""

    def draw(self, batch, h, w):
        lam = np.float32(self.rng.beta(self.alpha, self.alpha))
        rows = np.zeros((batch, ROW_COLS), dtype=np.int32)
        rows[:, 0] = self.rng.permutation(batch)
        wts = np.full((batch, WT_COLS), lam, dtype=np.float32)
        return rows, wts


class CutmixBlending(_Blending):
    """A box of the partner clip pasted into every frame of the clip; the label weight is the area that stays (mmaction CutmixBlending:
    r = sqrt(1 - lambda), a box of int(w * r) x int(h * r) around a centre uniform in the image, clipped to the image)."""

    def draw(self, batch, h, w):
        lam = float(self.rng.beta(self.alpha, self.alpha))
        perm = self.rng.permutation(batch)
        r = np.sqrt(1.0 - lam)
        cw, ch = int(w * r), int(h * r)
        cx, cy = int(self.rng.integers(w)), int(self.rng.integers(h))
        x0, x1 = int(np.clip(cx - cw // 2, 0, w)), int(np.clip(cx + cw // 2, 0, w))
        y0, y1 = int(np.clip(cy - ch // 2, 0, h)), int(np.clip(cy + ch // 2, 0, h))
        rows = np.empty((batch, ROW_COLS), dtype=np.int32)
        rows[:, 0] = perm
        rows[:, 1:] = (y0, x0, y1, x1)
        wts = np.empty((batch, WT_COLS), dtype=np.float32)
        wts[:, 0] = 1.0
        wts[:, 1] = np.float32(1.0 - float((y1 - y0) * (x1 - x0)) / float(h * w))
        return rows, wts


class ExplicitBlending(object):
    """Hands out a given table every step (tests, or a data loader that draws its own)."""

    def __init__(self, rows, wts):
        self.rows = np.ascontiguousarray(np.asarray(rows), dtype=np.int32)
        self.wts = np.ascontiguousarray(np.asarray(wts), dtype=np.float32)

    def draw(self, batch, h, w):
        return self.rows, self.wts


def check_blend_rows(rows, wts, batch, h, w):
    """ValueError unless (rows, wts) is a table the blend kernels take for a batch of `batch` clips of h x w pixels."""
    rows, wts = np.asarray(rows), np.asarray(wts)
    if rows.shape != (batch, ROW_COLS) or rows.dtype != np.int32:
        raise ValueError("blending rows: int32 (%d, %d) expected, got %s %s" % (batch, ROW_COLS, rows.dtype, rows.shape))
    if wts.shape != (batch, WT_COLS) or wts.dtype != np.float32:
        raise ValueError("blending weights: float32 (%d, %d) expected, got %s %s" % (batch, WT_COLS, wts.dtype, wts.shape))
    partner, y0, x0, y1, x1 = (rows[:, k] for k in range(ROW_COLS))
    if ((partner < 0) | (partner >= batch)).any():
        raise ValueError("blending rows: partner outside [0, %d): %s" % (batch, partner.tolist()))
    if not ((0 <= y0) & (y0 <= y1) & (y1 <= h)).all():
        raise ValueError("blending rows: boxes need 0 <= y0 <= y1 <= %d (y0 %s, y1 %s)" % (h, y0.tolist(), y1.tolist()))
    if not ((0 <= x0) & (x0 <= x1) & (x1 <= w)).all():
        raise ValueError("blending rows: boxes need 0 <= x0 <= x1 <= %d (x0 %s, x1 %s)" % (w, x0.tolist(), x1.tolist()))
    if not ((wts >= 0) & (wts <= 1)).all():              # (a NaN fails both comparisons)
        raise ValueError("blending weights: lam_px / lam_lab must lie in [0, 1]: %s" % wts.tolist())


_TYPES = {"MixupBlending": MixupBlending, "CutmixBlending": CutmixBlending}


def build_blending(cfg):
    """train_cfg['blending'] -> a blending object: dict(type='MixupBlending' | 'CutmixBlending', alpha=..., seed=...), an object with draw(), or None."""
    if cfg is None or hasattr(cfg, "draw"):
        return cfg
    if not hasattr(cfg, "get") or cfg.get("type") is None:
        raise ValueError("blending config: a dict with a 'type' is expected, got %r" % (cfg,))
    args = dict(cfg)
    kind = args.pop("type")
    if kind not in _TYPES:
        raise NotImplementedError("blending type %r: 'MixupBlending' and 'CutmixBlending' are built" % (kind,))
    unknown = sorted(set(args) - {"alpha", "seed", "num_classes"})
    if unknown:
        raise ValueError("blending config: unknown keys %s" % unknown)
    args.pop("num_classes", None)          # mmaction's blendings build one-hot labels themselves; here the head's class count is used
    if "alpha" not in args:
        args["alpha"] = 0.2                # mmaction's default
    return _TYPES[kind](**args)
