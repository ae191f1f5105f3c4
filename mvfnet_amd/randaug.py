"""RandAugment for fine-tuning: timm's transform as the PySlowFast / VideoMAE / mmaction2 recipes name it (`rand-m7-n4-mstd0.5-inc1`), one draw per clip,
applied to every frame of the clip in front of the random-resized crop (train_cfg=dict(randaug=dict(type='RandAugment', config='rand-m7-n4-mstd0.5-inc1'))).

A RandAugment object only DRAWS the step's table on the host; the pixels are changed on the device by mvf_frames_randaug_u8 (csrc/randaug.hip) on the uploaded
uint8 frames, before resize / crop / flip / ColorJitter / Normalize.  The table is int32 (clips, layers, 16), one row per clip and layer:

    word 0       kind: 0 identity, 1 invert, 2 posterize, 3 solarize, 4 solarize-add, 5 autocontrast, 6 equalize, 7 brightness, 8 contrast, 9 color,
                 10 sharpness, 11 affine
    words 1..12  kind 2: mask; 3: thresh; 4: thresh, add; 7 .. 10: the fp32 factor's bits; 11: six fp64 coefficients a .. f of the inverse map, low word first
    word 13      kind 11: the fill colour, three bytes in STORED channel order
    words 14..15 0

include/mvfnet_hip.h states the arithmetic of every kind; it equals Pillow's bit for bit on the fixtures of tests/golden/randaug_cases.npz.

The draw follows timm/data/auto_augment.py (rand_augment_transform, RandAugment, AugmentOp and the level functions): np.random.choice(ops, num_layers) with
replacement; then per layer random.random() > prob skips the op (drawn only when prob < 1, as timm does), the magnitude is random.gauss(m, std) -- or
random.uniform(0, m) when mstd >= 100 --, clipped to [0, magnitude_max], and the op's level function runs, with random.random() > 0.5 negating where timm
negates.  It uses the global `random` and `np.random` generators, as timm does: seed those.  timm is not a dependency of this project and was not installed
where this was written: the rules are restated from its source and were NOT checked against timm itself.  Three deliberate differences: SolarizeAdd's level is
min(110, int(110 L)) (timm caps at 128, the same for magnitude_max <= 10), Rotate always goes through the affine map (Pillow transposes at exactly 180
degrees, which magnitude_max < 60 never reaches), and `inc0` in the config string selects the plain op list (timm tests the string, so any `inc` selects the
increasing one there).

Not built: bicubic interpolation, YUV / addressed input, AutoAugment / AugMix policies, per-op choice weights (`w` in the config string).
"""
import math
import numbers
import random
import re

import numpy as np

TABLE_WORDS, MAX_LAYERS = 16, 8
(K_IDENTITY, K_INVERT, K_POSTERIZE, K_SOLARIZE, K_SOLARIZE_ADD, K_AUTOCONTRAST, K_EQUALIZE, K_BRIGHTNESS, K_CONTRAST, K_COLOR, K_SHARPNESS,
 K_AFFINE) = range(12)
STAT_KINDS = (K_AUTOCONTRAST, K_EQUALIZE, K_CONTRAST)
WS_PER_FRAME = 3 * 256 + 16                     # MVF_RANDAUG_WS_PER_FRAME
ORDER_BGR, ORDER_RGB = 0, 1

RAND_TRANSFORMS = ("AutoContrast", "Equalize", "Invert", "Rotate", "Posterize", "Solarize", "SolarizeAdd", "Color", "Contrast", "Brightness", "Sharpness",
                   "ShearX", "ShearY", "TranslateXRel", "TranslateYRel")
RAND_INCREASING_TRANSFORMS = ("AutoContrast", "Equalize", "Invert", "Rotate", "PosterizeIncreasing", "SolarizeIncreasing", "SolarizeAdd", "ColorIncreasing",
                              "ContrastIncreasing", "BrightnessIncreasing", "SharpnessIncreasing", "ShearX", "ShearY", "TranslateXRel", "TranslateYRel")
_ENHANCE = {"Color": K_COLOR, "Contrast": K_CONTRAST, "Brightness": K_BRIGHTNESS, "Sharpness": K_SHARPNESS}
_SIZED = ("Rotate", "TranslateXRel", "TranslateYRel")            # their matrix depends on the frame size
OP_NAMES = ("Identity", "TranslateX", "TranslateY") + RAND_TRANSFORMS + tuple(n for n in RAND_INCREASING_TRANSFORMS if n not in RAND_TRANSFORMS)
_BUILT = "built: interpolation 'bilinear'; ops %s" % ", ".join(OP_NAMES)


def _affine_words(row, coeffs, fill, order):
    row[0] = K_AFFINE
    row[1:13] = np.asarray(coeffs, dtype=np.float64).view(np.int32)
    rgb = [int(v) for v in fill]
    if len(rgb) != 3 or not all(0 <= v <= 255 for v in rgb):
        raise ValueError("RandAugment: fill must be three values in 0 .. 255 (RGB), got %r" % (fill,))
    b = rgb if order == ORDER_RGB else rgb[::-1]
    row[13] = b[0] | b[1] << 8 | b[2] << 16


def rotate_matrix(deg, h, w):
    """The matrix Pillow's Image.rotate(deg) hands to its affine transform (no expand, default centre); 0 degrees is the identity."""
    angle = deg % 360.0
    if angle == 0:
        return (1.0, 0.0, 0.0, 0.0, 1.0, 0.0)
    cx, cy = w / 2.0, h / 2.0
    angle = -math.radians(angle)
    m = [round(math.cos(angle), 15), round(math.sin(angle), 15), 0.0, round(-math.sin(angle), 15), round(math.cos(angle), 15), 0.0]
    a, b, c, d, e, f = m
    m[2], m[5] = a * -cx + b * -cy + c, d * -cx + e * -cy + f
    m[2] += cx
    m[5] += cy
    return tuple(m)


def op_row(name, arg, h, w, fill=(124, 116, 104), order=ORDER_BGR):
    """One op as its int32 (16,) table row.  `arg` is what timm's level function hands the op: degrees (Rotate), the shear factor, the fraction of the width /
    height (Translate?Rel) or pixels (TranslateX / TranslateY), the enhance factor, the bits kept (Posterize), the threshold (Solarize), the addend
    (SolarizeAdd, threshold 128); ignored by Identity, AutoContrast, Equalize and Invert.  (h, w) is the frame's own size, `fill` RGB, `order` the stored
    channel order of the frames (0 = BGR, 1 = RGB)."""
    if order not in (ORDER_BGR, ORDER_RGB):
        raise ValueError("RandAugment: order must be 0 (BGR) or 1 (RGB), got %r" % (order,))
    row = np.zeros(TABLE_WORDS, dtype=np.int32)
    base = name[:-len("Increasing")] if name.endswith("Increasing") else name
    if name == "Identity":
        pass
    elif name == "Invert":
        row[0] = K_INVERT
    elif name == "AutoContrast":
        row[0] = K_AUTOCONTRAST
    elif name == "Equalize":
        row[0] = K_EQUALIZE
    elif base == "Posterize":
        bits = int(arg)
        if bits >= 8:                                   # (timm: `if bits_to_keep >= 8: return img`)
            return row
        if bits < 0:
            raise ValueError("RandAugment: Posterize keeps 0 .. 8 bits, got %r" % (arg,))
        row[0], row[1] = K_POSTERIZE, ~(2 ** (8 - bits) - 1) & 255
    elif base == "Solarize":
        row[0], row[1] = K_SOLARIZE, min(256, max(0, int(arg)))
    elif name == "SolarizeAdd":
        row[0], row[1], row[2] = K_SOLARIZE_ADD, 128, min(255, max(0, int(arg)))
    elif base in _ENHANCE:
        f = np.float32(arg)
        if not np.isfinite(f):
            raise ValueError("RandAugment: %s factor %r" % (name, arg))
        row[0], row[1] = _ENHANCE[base], np.array([f], dtype=np.float32).view(np.int32)[0]
    elif name == "Rotate":
        _affine_words(row, rotate_matrix(float(arg), h, w), fill, order)
    elif name == "ShearX":
        _affine_words(row, (1, float(arg), 0, 0, 1, 0), fill, order)
    elif name == "ShearY":
        _affine_words(row, (1, 0, 0, float(arg), 1, 0), fill, order)
    elif name in ("TranslateXRel", "TranslateX"):
        _affine_words(row, (1, 0, float(arg) * w if name.endswith("Rel") else float(arg), 0, 1, 0), fill, order)
    elif name in ("TranslateYRel", "TranslateY"):
        _affine_words(row, (1, 0, 0, 0, 1, float(arg) * h if name.endswith("Rel") else float(arg)), fill, order)
    else:
        raise ValueError("RandAugment: unknown op %r (%s)" % (name, _BUILT))
    return row


def stats_mask(table):
    """Bit k set = some clip's layer k needs the statistics pass (autocontrast, equalize, contrast)."""
    kinds = np.asarray(table)[:, :, 0]
    return int(sum(1 << k for k in range(kinds.shape[1]) if np.isin(kinds[:, k], STAT_KINDS).any()))


def _number(v, name, lo=None, hi=None):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, numbers.Real) or math.isnan(v):
        raise ValueError("RandAugment: %s must be a number (got %r)" % (name, v))
    if (lo is not None and v < lo) or (hi is not None and v > hi):
        raise ValueError("RandAugment: %s=%r is out of range" % (name, v))
    return float(v)


def parse_config(config):
    """timm's config string ('rand-m7-n4-mstd0.5-inc1') -> keyword arguments of RandAugment.  Keys: m n mstd mmax inc p."""
    parts = str(config).split("-")
    if parts[0] != "rand":
        raise ValueError("RandAugment: the config string must start with 'rand' (got %r)" % (config,))
    out = {}
    for c in parts[1:]:
        cs = re.split(r"(\d.*)", c)
        if len(cs) < 2:
            continue
        key, val = cs[:2]
        try:
            if key == "mstd":
                out["magnitude_std"] = float(val)
            elif key == "mmax":
                out["magnitude_max"] = int(val)
            elif key == "inc":
                out["increasing"] = bool(int(val))
            elif key == "m":
                out["magnitude"] = int(val)
            elif key == "n":
                out["num_layers"] = int(val)
            elif key == "p":
                out["prob"] = float(val)
            else:
                raise ValueError("RandAugment: unknown key %r in %r (built: m n mstd mmax inc p)" % (key, config))
        except ValueError as e:
            if "RandAugment" in str(e):
                raise
            raise ValueError("RandAugment: bad value %r for %r in %r" % (val, key, config))
    return out


class RandAugment(object):
    """timm's RandAugment; draw() makes one table per step, one row per clip and layer."""

    def __init__(self, config=None, num_layers=4, magnitude=7, magnitude_std=0.5, increasing=True, prob=0.5, magnitude_max=10, translate_pct=0.45,
                 fill=(124, 116, 104), interpolation="bilinear", ops=None):
        if config is not None:
            kw = dict(num_layers=num_layers, magnitude=magnitude, magnitude_std=magnitude_std, increasing=increasing, prob=prob, magnitude_max=magnitude_max)
            kw.update(parse_config(config))
            num_layers, magnitude, magnitude_std, increasing, prob, magnitude_max = (kw[k] for k in ("num_layers", "magnitude", "magnitude_std", "increasing",
                                                                                                      "prob", "magnitude_max"))
        if interpolation != "bilinear":
            raise ValueError("RandAugment: interpolation %r (%s)" % (interpolation, _BUILT))
        if isinstance(num_layers, (bool, np.bool_)) or not isinstance(num_layers, numbers.Integral) or not 1 <= num_layers <= MAX_LAYERS:
            raise ValueError("RandAugment: num_layers must be an integer in 1 .. %d (got %r)" % (MAX_LAYERS, num_layers))
        self.num_layers = int(num_layers)
        self.magnitude = _number(magnitude, "magnitude", 0.0)
        self.magnitude_std = _number(magnitude_std, "magnitude_std", 0.0)
        self.increasing = bool(increasing)
        self.prob = _number(prob, "prob", 0.0, 1.0)
        self.magnitude_max = _number(magnitude_max, "magnitude_max", 0.0)
        self.translate_pct = _number(translate_pct, "translate_pct", 0.0)
        self.fill = tuple(int(v) for v in fill)
        _affine_words(np.zeros(TABLE_WORDS, dtype=np.int32), (1, 0, 0, 0, 1, 0), self.fill, ORDER_RGB)        # a bad fill is refused here
        self.ops = tuple(ops) if ops is not None else (RAND_INCREASING_TRANSFORMS if self.increasing else RAND_TRANSFORMS)
        if not self.ops:
            raise ValueError("RandAugment: an empty op list")
        for name in self.ops:
            op_row(name, 1, 8, 8, self.fill)            # unknown names are refused here

    def __repr__(self):
        return "RandAugment(num_layers=%d, magnitude=%g, magnitude_std=%g, increasing=%r, prob=%g, magnitude_max=%g, translate_pct=%g, fill=%r)" % (
            self.num_layers, self.magnitude, self.magnitude_std, self.increasing, self.prob, self.magnitude_max, self.translate_pct, self.fill)

    def level(self, name, magnitude):
        """timm's level function of op `name`: the op's argument at `magnitude` (draws the sign where timm negates); None for the ops without one."""
        L = magnitude / 10.0

        def negate(v):
            return -v if random.random() > 0.5 else v
        if name in ("Identity", "AutoContrast", "Equalize", "Invert"):
            return None
        if name == "Rotate":
            return negate(L * 30.0)
        if name in ("ShearX", "ShearY"):
            return negate(L * 0.3)
        if name in ("TranslateXRel", "TranslateYRel"):
            return negate(L * self.translate_pct)
        if name.endswith("Increasing") and name[:-len("Increasing")] in _ENHANCE:
            return max(0.1, 1.0 + negate(L * 0.9))
        if name in _ENHANCE:
            return L * 1.8 + 0.1
        if name == "PosterizeIncreasing":
            return 4 - int(L * 4)
        if name == "Posterize":
            return int(L * 4)
        if name == "SolarizeIncreasing":
            return 256 - min(256, int(L * 256))
        if name == "Solarize":
            return min(256, int(L * 256))
        if name == "SolarizeAdd":
            return min(110, int(L * 110))
        raise ValueError("RandAugment: op %r has no level function (%s)" % (name, _BUILT))

    def draw(self, batch, t, sizes, order=ORDER_BGR):
        """-> (table int32 (batch, num_layers, 16), statistics mask).  sizes = (h, w) or per-frame (batch * t, 2) rows (hs_i, ws_i)."""
        sizes = np.asarray(sizes, dtype=np.int64)
        sizes = np.broadcast_to(sizes.reshape(-1, 2), (batch * t, 2)) if sizes.size == 2 else sizes.reshape(batch * t, 2)
        per_clip = sizes.reshape(batch, t, 2)
        table = np.zeros((batch, self.num_layers, TABLE_WORDS), dtype=np.int32)
        for i in range(batch):
            names = np.random.choice(self.ops, self.num_layers)
            for k, name in enumerate(names):
                name = str(name)
                if self.prob < 1.0 and random.random() > self.prob:
                    continue
                m = self.magnitude
                if self.magnitude_std >= 100:
                    m = random.uniform(0, m)
                elif self.magnitude_std > 0:
                    m = random.gauss(m, self.magnitude_std)
                m = max(0.0, min(m, self.magnitude_max))
                arg = self.level(name, m)
                if name in _SIZED and (per_clip[i] != per_clip[i, 0]).any():
                    raise ValueError("RandAugment: %s depends on the frame size, and the frames of clip %d differ in size" % (name, i))
                h, w = (int(v) for v in per_clip[i, 0])
                table[i, k] = op_row(name, arg, h, w, self.fill, order)
        return table, stats_mask(table)


class ExplicitAugment(object):
    """Hands out a given table every step (tests, or a data loader that draws its own)."""

    def __init__(self, table):
        self.table = np.ascontiguousarray(np.asarray(table), dtype=np.int32)

    def draw(self, batch, t, sizes, order=ORDER_BGR):
        return self.table, stats_mask(self.table) if self.table.ndim == 3 else 0


def check_randaug_table(table, batch, layers=None):
    """ValueError unless `table` is one mvf_frames_randaug_u8 takes for `batch` clips (and `layers` layers, when given)."""
    table = np.asarray(table)
    if table.dtype != np.int32 or table.ndim != 3 or table.shape[0] != batch or table.shape[2] != TABLE_WORDS or not 1 <= table.shape[1] <= MAX_LAYERS or (
            layers is not None and table.shape[1] != layers):
        raise ValueError("randaug table: int32 (%d, %s, %d) expected, got %s %s" % (batch, layers if layers is not None else "1..%d" % MAX_LAYERS, TABLE_WORDS,
                                                                                    table.dtype, table.shape))
    kind = table[..., 0]
    if not ((kind >= 0) & (kind <= K_AFFINE)).all():
        raise ValueError("randaug table: kinds must be 0 .. %d: %s" % (K_AFFINE, sorted(set(kind.reshape(-1).tolist()))))
    if (table[..., 14:] != 0).any():
        raise ValueError("randaug table: words 14..15 must be 0")
    w1, w2 = table[..., 1], table[..., 2]
    if ((kind == K_POSTERIZE) & ((w1 < 0) | (w1 > 255))).any():
        raise ValueError("randaug table: a posterize mask outside 0 .. 255")
    if (np.isin(kind, (K_SOLARIZE, K_SOLARIZE_ADD)) & ((w1 < 0) | (w1 > 256))).any():
        raise ValueError("randaug table: a solarize threshold outside 0 .. 256")
    if ((kind == K_SOLARIZE_ADD) & ((w2 < 0) | (w2 > 255))).any():
        raise ValueError("randaug table: a solarize addend outside 0 .. 255")
    blend = np.isin(kind, (K_BRIGHTNESS, K_CONTRAST, K_COLOR, K_SHARPNESS))
    if not np.isfinite(np.ascontiguousarray(w1).view(np.float32)[blend]).all():
        raise ValueError("randaug table: a non-finite blend factor")
    co = np.ascontiguousarray(table[..., 1:13]).view(np.float64)
    if not np.isfinite(co[kind == K_AFFINE]).all():
        raise ValueError("randaug table: a non-finite affine coefficient")
    if ((kind == K_AFFINE) & ((table[..., 13] < 0) | (table[..., 13] > 0xFFFFFF))).any():
        raise ValueError("randaug table: the fill colour is three bytes")


_TYPES = {"RandAugment": RandAugment}
_KEYS = {"config", "num_layers", "magnitude", "magnitude_std", "increasing", "prob", "magnitude_max", "translate_pct", "fill", "interpolation", "ops"}


def build_randaug(cfg):
    """train_cfg['randaug'] -> an augment object: dict(type='RandAugment', config='rand-m7-n4-mstd0.5-inc1', ...), an object with draw(), or None."""
    if cfg is None or hasattr(cfg, "draw"):
        return cfg
    if not hasattr(cfg, "get") or cfg.get("type") is None:
        raise ValueError("randaug config: a dict with a 'type' is expected, got %r" % (cfg,))
    args = dict(cfg)
    kind = args.pop("type")
    if kind not in _TYPES:
        raise NotImplementedError("randaug type %r: 'RandAugment' is built" % (kind,))
    unknown = sorted(set(args) - _KEYS)
    if unknown:
        raise ValueError("randaug config: unknown keys %s" % unknown)
    return _TYPES[kind](**args)


def apply(frames, table, t, sizes=None, order=ORDER_BGR, out=None):
    """mvf_frames_randaug_u8 over `frames` (..., hs, ws, 3) uint8 on the GPU, flattened to n frames with clips of t consecutive frames: `table` is the
    host int32 (n / t, layers, 16) table (validated here), `sizes` None, or (n, 2) rows (hs_i, ws_i) on the host or the device.  Returns `out` (allocated when
    None), shaped like `frames`; `frames` is not written.  Owns the second buffer and the workspace (allocated per call: the train engine keeps persistent ones of its own)."""
    import torch
    from ._lib import check, lib
    if frames.dtype != torch.uint8 or not frames.is_cuda or frames.dim() < 3 or frames.shape[-1] != 3:
        raise ValueError("randaug.apply: a CUDA uint8 tensor (..., hs, ws, 3) is expected, got %s %s" % (frames.dtype, tuple(frames.shape)))
    f = frames.reshape((-1,) + tuple(frames.shape[-3:])).contiguous()
    n, hs, ws = (int(v) for v in f.shape[:3])
    if t < 1 or n % t:
        raise ValueError("randaug.apply: %d frames are not clips of %d" % (n, t))
    table = np.ascontiguousarray(np.asarray(table))
    check_randaug_table(table, n // t)
    layers = int(table.shape[1])
    dev = f.device
    table_d = torch.from_numpy(table).to(dev)
    sizes_d = None
    if sizes is not None:
        sizes_d = torch.as_tensor(sizes).to(device=dev, dtype=torch.int32).reshape(-1, 2).contiguous()
        if sizes_d.shape[0] != n:
            raise ValueError("randaug.apply: sizes needs one (hs_i, ws_i) row per frame: %d rows for %d frames" % (sizes_d.shape[0], n))
        if bool(((sizes_d[:, 0] < 1) | (sizes_d[:, 0] > hs) | (sizes_d[:, 1] < 1) | (sizes_d[:, 1] > ws)).any()):
            raise ValueError("randaug.apply: a frame size outside the %dx%d extent" % (hs, ws))
    if out is None:
        out = torch.empty_like(f)
    elif out.dtype != torch.uint8 or out.numel() != f.numel() or not out.is_contiguous() or out.device != dev:
        raise ValueError("randaug.apply: the output buffer %s %s does not hold %s" % (out.dtype, tuple(out.shape), tuple(f.shape)))
    tmp = torch.empty(f.numel(), dtype=torch.uint8, device=dev)
    ws_buf = torch.empty(n * WS_PER_FRAME, dtype=torch.uint8, device=dev)
    check(lib.mvf_frames_randaug_u8(f.data_ptr(), n, hs, ws, int(t), int(order), None if sizes_d is None else sizes_d.data_ptr(), table_d.data_ptr(), layers,
                                    stats_mask(table), out.data_ptr(), tmp.data_ptr(), ws_buf.data_ptr(), ws_buf.numel(),
                                    torch.cuda.current_stream().cuda_stream), "mvf_frames_randaug_u8")
    return out.view(frames.shape) if out.numel() == frames.numel() else out
