"""RandomErasing for fine-tuning: timm's transform as PySlowFast (cube=True) and mmaction2 use it (train_cfg=dict(erasing=dict(type='RandomErasing', ...))).

An erasing object only DRAWS the step's table on the host; the pixels are erased on the device by mvf_stem_erase (csrc/erase.hip), in place on the stem
operand, behind every input path of the train engine and before the batch blending.  The table, with planes = batch * t (plane = clip * t + frame):

    boxes int32  (planes, max_boxes, 5): y0, x0, y1, x1, mode    half-open box in image pixels, 0 <= y0 <= y1 <= h, 0 <= x0 <= x1 <= w;
                                                                 mode 0 = unused slot, 1 = constant colour, 2 = per-element N(0, 1) noise
    fill  fp32   (planes, max_boxes, 4): the colour of a mode-1 box in normalised space (channels 0..2; word 3 is ignored)
    key   uint32 (2):                    the step's generator key: the noise of mode 2 is made in the kernel (Philox4x32-10, counter = (x, y, plane, 0))

Where boxes of a plane overlap, the higher slot wins.  The box draw is timm's: a clip is erased with probability `probability`; count ~ U{min_count ..
max_count}; per box up to 10 attempts of area ~ U(min_area, max_area) * h * w / count, aspect = exp(U(log min_aspect, log max_aspect)),
bh = int(round(sqrt(area * aspect))), bw = int(round(sqrt(area / aspect))), accepted when bw < w and bh < h, top ~ U{0 .. h - bh}, left ~ U{0 .. w - bw}.
"""
import math
import numbers

import numpy as np

BOX_COLS, FILL_COLS, KEY_WORDS, MAX_BOXES = 5, 4, 2, 8
MODE_UNUSED, MODE_CONST, MODE_NOISE = 0, 1, 2
_MODES = {"const": MODE_CONST, "rand": MODE_CONST, "pixel": MODE_NOISE}


def _real(v, name, lo=None, hi=None, lo_open=False):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, numbers.Real) or not np.isfinite(v):
        raise ValueError("RandomErasing: %s must be a finite number (got %r)" % (name, v))
    v = float(v)
    if (lo is not None and (v <= lo if lo_open else v < lo)) or (hi is not None and v > hi):
        raise ValueError("RandomErasing: %s=%r is out of range" % (name, v))
    return v


def _count(v, name):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, numbers.Integral) or v < 1:
        raise ValueError("RandomErasing: %s must be an integer >= 1 (got %r)" % (name, v))
    return int(v)


class RandomErasing(object):
    """timm's RandomErasing.  mode 'const': colour 0, the dataset mean in normalised space; 'rand': one N(0, 1) colour per box, drawn on the host; 'pixel':
    per-element N(0, 1) noise, made in the kernel.  cube=True (PySlowFast) gives every frame of a clip the same boxes and, under 'rand', the same colours --
    the noise of 'pixel' still differs per frame, the generator's counter carries the plane --; cube=False draws per frame."""

    def __init__(self, probability=0.25, mode="pixel", min_area=0.02, max_area=1.0 / 3.0, min_aspect=0.3, max_aspect=None, min_count=1, max_count=None,
                 cube=True, seed=None):
        self.probability = _real(probability, "probability", 0.0, 1.0)
        if mode not in _MODES:
            raise ValueError("RandomErasing: mode must be 'pixel', 'rand' or 'const' (got %r)" % (mode,))
        self.mode = mode
        self.min_area = _real(min_area, "min_area", 0.0, 1.0, lo_open=True)
        self.max_area = _real(max_area, "max_area", self.min_area, 1.0)
        self.min_aspect = _real(min_aspect, "min_aspect", 0.0, lo_open=True)
        self.max_aspect = _real(max_aspect, "max_aspect", self.min_aspect) if max_aspect is not None else 1.0 / self.min_aspect
        if self.max_aspect < self.min_aspect:
            raise ValueError("RandomErasing: min_aspect=%r exceeds max_aspect=%r" % (self.min_aspect, self.max_aspect))
        self.min_count = _count(min_count, "min_count")
        self.max_count = _count(max_count, "max_count") if max_count is not None else self.min_count
        if self.max_count < self.min_count:
            raise ValueError("RandomErasing: min_count=%d exceeds max_count=%d" % (self.min_count, self.max_count))
        if self.max_count > MAX_BOXES:
            raise ValueError("RandomErasing: max_count=%d: the kernel takes at most %d boxes per frame" % (self.max_count, MAX_BOXES))
        self.cube = bool(cube)
        self.seed = seed
        self.rng = np.random.default_rng(seed)

    def __repr__(self):
        return "RandomErasing(probability=%g, mode=%r, area=(%g, %g), aspect=(%g, %g), count=(%d, %d), cube=%r, seed=%r)" % (
            self.probability, self.mode, self.min_area, self.max_area, self.min_aspect, self.max_aspect, self.min_count, self.max_count, self.cube, self.seed)

    @property
    def max_boxes(self):
        """The width of every table draw() returns (a launch plan is recorded for it)."""
        return self.max_count

    def _draw_boxes(self, boxes, fill, h, w):
        """One erase decision: fills the slots of boxes (max_boxes, 5) / fill (max_boxes, 4) of one plane."""
        rng = self.rng
        if rng.random() > self.probability:              # (timm: `if random.random() > self.probability: return`)
            return
        count = self.min_count if self.min_count == self.max_count else int(rng.integers(self.min_count, self.max_count + 1))
        log_lo, log_hi = math.log(self.min_aspect), math.log(self.max_aspect)
        slot = 0
        for _ in range(count):
            for _attempt in range(10):
                target = rng.uniform(self.min_area, self.max_area) * (h * w) / count
                aspect = math.exp(rng.uniform(log_lo, log_hi))
                bh, bw = int(round(math.sqrt(target * aspect))), int(round(math.sqrt(target / aspect)))
                if bw < w and bh < h:
                    top, left = int(rng.integers(0, h - bh + 1)), int(rng.integers(0, w - bw + 1))
                    boxes[slot] = (top, left, top + bh, left + bw, _MODES[self.mode])
                    if self.mode == "rand":
                        fill[slot, :3] = rng.standard_normal(3).astype(np.float32)
                    slot += 1
                    break

    def draw(self, batch, t, h, w):
        mb = self.max_count
        boxes = np.zeros((batch, t, mb, BOX_COLS), dtype=np.int32)
        fill = np.zeros((batch, t, mb, FILL_COLS), dtype=np.float32)
        for i in range(batch):
            if self.cube:
                self._draw_boxes(boxes[i, 0], fill[i, 0], h, w)
                boxes[i, 1:], fill[i, 1:] = boxes[i, 0], fill[i, 0]
            else:
                for f in range(t):
                    self._draw_boxes(boxes[i, f], fill[i, f], h, w)
        key = self.rng.integers(0, 1 << 32, size=KEY_WORDS, dtype=np.uint64).astype(np.uint32)
        return boxes.reshape(batch * t, mb, BOX_COLS), fill.reshape(batch * t, mb, FILL_COLS), key


class ExplicitErasing(object):
    """Hands out a given table every step (tests, or a data loader that draws its own)."""

    def __init__(self, boxes, fill, key):
        self.boxes = np.ascontiguousarray(np.asarray(boxes), dtype=np.int32)
        self.fill = np.ascontiguousarray(np.asarray(fill), dtype=np.float32)
        self.key = np.ascontiguousarray(np.asarray(key), dtype=np.uint32)
        self.max_boxes = int(self.boxes.shape[1]) if self.boxes.ndim == 3 else None

    def draw(self, batch, t, h, w):
        return self.boxes, self.fill, self.key


def check_erase_table(boxes, fill, key, planes, h, w):
    """ValueError unless (boxes, fill, key) is a table mvf_stem_erase takes for `planes` frames of h x w pixels."""
    boxes, fill, key = np.asarray(boxes), np.asarray(fill), np.asarray(key)
    if boxes.dtype != np.int32 or boxes.ndim != 3 or boxes.shape[0] != planes or boxes.shape[2] != BOX_COLS or not 1 <= boxes.shape[1] <= MAX_BOXES:
        raise ValueError("erasing boxes: int32 (%d, 1..%d, %d) expected, got %s %s" % (planes, MAX_BOXES, BOX_COLS, boxes.dtype, boxes.shape))
    if fill.dtype != np.float32 or fill.shape != (planes, boxes.shape[1], FILL_COLS):
        raise ValueError("erasing fill: float32 (%d, %d, %d) expected, got %s %s" % (planes, boxes.shape[1], FILL_COLS, fill.dtype, fill.shape))
    if key.dtype != np.uint32 or key.shape != (KEY_WORDS,):
        raise ValueError("erasing key: uint32 (%d,) expected, got %s %s" % (KEY_WORDS, key.dtype, key.shape))
    y0, x0, y1, x1, mode = (boxes[..., k] for k in range(BOX_COLS))
    if not ((0 <= y0) & (y0 <= y1) & (y1 <= h)).all():
        raise ValueError("erasing boxes: boxes need 0 <= y0 <= y1 <= %d" % h)
    if not ((0 <= x0) & (x0 <= x1) & (x1 <= w)).all():
        raise ValueError("erasing boxes: boxes need 0 <= x0 <= x1 <= %d" % w)
    if not ((mode >= MODE_UNUSED) & (mode <= MODE_NOISE)).all():
        raise ValueError("erasing boxes: mode must be 0 (unused), 1 (constant) or 2 (noise): %s" % sorted(set(mode.reshape(-1).tolist())))
    if not np.isfinite(fill).all():
        raise ValueError("erasing fill: non-finite colour")


_TYPES = {"RandomErasing": RandomErasing}
_KEYS = {"probability", "mode", "min_area", "max_area", "min_aspect", "max_aspect", "min_count", "max_count", "cube", "seed"}


def build_erasing(cfg):
    """train_cfg['erasing'] -> an erasing object: dict(type='RandomErasing', probability=..., mode=..., ...), an object with draw(), or None."""
    if cfg is None or hasattr(cfg, "draw"):
        return cfg
    if not hasattr(cfg, "get") or cfg.get("type") is None:
        raise ValueError("erasing config: a dict with a 'type' is expected, got %r" % (cfg,))
    args = dict(cfg)
    kind = args.pop("type")
    if kind not in _TYPES:
        raise NotImplementedError("erasing type %r: 'RandomErasing' is built" % (kind,))
    unknown = sorted(set(args) - _KEYS)
    if unknown:
        raise ValueError("erasing config: unknown keys %s" % unknown)
    return _TYPES[kind](**args)
