"""Stochastic depth (drop path) for fine-tuning, as timm configures it (drop_path_rate; "ResNet strikes back" A1 / A2 train at 0.05):
train_cfg=dict(drop_path=dict(type='DropPath', rate=0.05)).

A drop-path object only DRAWS the step's table on the host; the residual branch is scaled on the device by mvf_bn_apply_bits_rowscale / mvf_gate_rowscale
(csrc/drop_path.hip) inside the train engine's bottlenecks.  The table, for L bottlenecks in dataflow order and a batch of b clips of t frames:

    fp32 (L, b * t): s[i][clip * t + frame], the scale of block i's residual branch for that image

timm's drop_path(x, p, training, scale_by_keep=True) after bn3: out = relu(s * bn3(conv3(a2)) + identity), s = Bernoulli(1 - p_i) / (1 - p_i) (the plain 0 / 1
draw without scale_by_keep), p_i = rate * i / (L - 1): block 0 never drops.  unit='clip' (default) makes one draw per clip, shared by its t frames -- a clip
is one sample, and MVF mixes its frames --; unit='frame' draws per image.  The table holds one value per image either way.
"""
import numbers

import numpy as np

UNITS = ("clip", "frame")


def _rate(rate, who):
    if isinstance(rate, (bool, np.bool_)) or not isinstance(rate, numbers.Real) or not (0.0 <= rate < 1.0):         # (a NaN fails both comparisons)
        raise ValueError("%s: rate must be a number in [0, 1) (got %r)" % (who, rate))
    return float(rate)


class DropPath(object):
    """Linear-in-depth drop path with its own numpy generator."""

    def __init__(self, rate, unit="clip", scale_by_keep=True, seed=None):
        self.rate = _rate(rate, type(self).__name__)
        if unit not in UNITS:
            raise ValueError("DropPath: unit must be 'clip' or 'frame' (got %r)" % (unit,))
        self.unit, self.scale_by_keep, self.seed = unit, bool(scale_by_keep), seed
        self.rng = np.random.default_rng(seed)

    def __repr__(self):
        return "DropPath(rate=%g, unit=%r, scale_by_keep=%r, seed=%r)" % (self.rate, self.unit, self.scale_by_keep, self.seed)

    def rates(self, n_blocks):
        """p_i = rate * i / (L - 1) for the L blocks in dataflow order (a single block: 0)."""
        if n_blocks < 1:
            raise ValueError("DropPath.rates: n_blocks must be >= 1 (got %r)" % (n_blocks,))
        if n_blocks == 1:
            return np.zeros(1, dtype=np.float64)
        return self.rate * np.arange(n_blocks, dtype=np.float64) / float(n_blocks - 1)

    def drops(self, n_blocks):
        """Which blocks take the drop-path kernels: those whose rate is not 0."""
        return tuple(bool(p > 0.0) for p in self.rates(n_blocks))

    def draw(self, n_blocks, b, t):
        """fp32 (n_blocks, b * t).  Every block draws b (clip) or b * t (frame) uniforms, blocks in order, whatever their rate."""
        p = self.rates(n_blocks)
        n = b if self.unit == "clip" else b * t
        keep = self.rng.random((n_blocks, n)) >= p[:, None]                     # P(keep) = 1 - p_i; p = 0 always keeps
        s = keep.astype(np.float32)
        if self.scale_by_keep:
            s *= (1.0 / (1.0 - p)).astype(np.float32)[:, None]                  # rate < 1: every keep probability is positive
        if self.unit == "clip":
            s = np.repeat(s, t, axis=1)
        return np.ascontiguousarray(s, dtype=np.float32)


class ExplicitDropPath(object):
    """Hands out a given (n_blocks, b * t) table every step (tests, or a caller that draws its own); assign .table for another one.  Block 0 never drops, as
    under the linear schedule: its row must be all ones."""

    unit, scale_by_keep = "explicit", True

    def __init__(self, table):
        self.table = table

    def rates(self, n_blocks):
        raise NotImplementedError("ExplicitDropPath carries a table, not rates")

    def drops(self, n_blocks):
        return (False,) + (True,) * (n_blocks - 1)

    def draw(self, n_blocks, b, t):
        table = np.ascontiguousarray(np.asarray(self.table), dtype=np.float32)
        if table.ndim == 2 and table.shape[0] >= 1 and not (table[0] == 1.0).all():
            raise ValueError("ExplicitDropPath: row 0 must be all ones (block 0 never drops)")
        return table


def check_drop_table(table, n_blocks, n_images):
    """ValueError unless `table` is a scale table the drop-path kernels take for n_blocks blocks and n_images images."""
    table = np.asarray(table)
    if table.shape != (n_blocks, n_images) or table.dtype != np.float32:
        raise ValueError("drop path table: float32 (%d, %d) expected, got %s %s" % (n_blocks, n_images, table.dtype, table.shape))
    if not (np.isfinite(table) & (table >= 0)).all():
        raise ValueError("drop path table: finite scales >= 0 expected")
    return table


def build_drop_path(cfg):
    """train_cfg['drop_path'] -> a drop-path object: dict(type='DropPath', rate=..., unit=..., scale_by_keep=..., seed=...), an object with draw(), or None."""
    if cfg is None or hasattr(cfg, "draw"):
        return cfg
    if not hasattr(cfg, "get") or cfg.get("type") is None:
        raise ValueError("drop_path config: a dict with a 'type' is expected, got %r" % (cfg,))
    args = dict(cfg)
    kind = args.pop("type")
    if kind != "DropPath":
        raise ValueError("drop_path type %r: 'DropPath' is built" % (kind,))
    unknown = sorted(set(args) - {"rate", "unit", "scale_by_keep", "seed"})
    if unknown:
        raise ValueError("drop_path config: unknown keys %s" % unknown)
    if "rate" not in args:
        raise ValueError("drop_path config: 'rate' is required")
    return DropPath(**args)
