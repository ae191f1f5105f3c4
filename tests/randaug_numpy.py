"""numpy restatement of mvf_frames_randaug_u8 (include/mvfnet_hip.h states the arithmetic): uint8 in, uint8 out, per op and for a layer sequence.  Written
from the header's text, not from the kernel: whole-image array expressions, one op at a time."""
import numpy as np

(IDENTITY, INVERT, POSTERIZE, SOLARIZE, SOLARIZE_ADD, AUTOCONTRAST, EQUALIZE, BRIGHTNESS, CONTRAST, COLOR, SHARPNESS, AFFINE) = range(12)


def grey(img, order):
    """The grey image, int64 (h, w); order 0 = BGR, 1 = RGB."""
    v = img.astype(np.int64)
    r, g, b = (v[..., 0], v[..., 1], v[..., 2]) if order else (v[..., 2], v[..., 1], v[..., 0])
    return (r * 19595 + g * 38470 + b * 7471 + 0x8000) >> 16


def blend(d, f, p):
    """fp32, every operation rounded on its own: v = d + f * (p - d); truncated, after a clamp when f is outside [0, 1]."""
    d, p, f = np.asarray(d, dtype=np.float32), np.asarray(p, dtype=np.float32), np.float32(f)
    v = d + f * (p - d)
    assert v.dtype == np.float32
    if not 0.0 <= f <= 1.0:
        v = np.clip(v, np.float32(0), np.float32(255))
    return v.astype(np.int64).astype(np.uint8)


def autocontrast_lut(ch):
    lo, hi = int(ch.min()), int(ch.max())
    i = np.arange(256, dtype=np.float64)
    if hi <= lo:
        return i.astype(np.uint8)
    scale = 255.0 / (hi - lo)
    off = -lo * scale
    return np.clip((i * scale + off).astype(np.int64), 0, 255).astype(np.uint8)


def equalize_lut(ch):
    h = np.bincount(ch.reshape(-1), minlength=256).astype(np.int64)
    nz = h[h > 0]
    ident = np.arange(256, dtype=np.uint8)
    if nz.size <= 1:
        return ident
    step = int(nz.sum() - nz[-1]) // 255
    if step == 0:
        return ident
    acc = step // 2 + np.concatenate([[0], np.cumsum(h)[:-1]])
    return np.minimum(255, acc // step).astype(np.uint8)


def smooth(img):
    """(2 acc + 13) / 26 on the interior, acc = the 3 x 3 sum with centre weight 5; the border (or an image under 3 x 3) is the image."""
    out = img.copy()
    h, w = img.shape[:2]
    if h < 3 or w < 3:
        return out
    v = img.astype(np.int64)
    acc = 4 * v[1:-1, 1:-1]
    for dy in range(3):
        for dx in range(3):
            acc = acc + v[dy:dy + h - 2, dx:dx + w - 2]
    out[1:-1, 1:-1] = (2 * acc + 13) // 26
    return out


def affine(img, co, fill):
    """fill = the three bytes in stored order."""
    h, w = img.shape[:2]
    a, b, c, d, e, f = (float(v) for v in co)
    ys, xs = np.meshgrid(np.arange(h, dtype=np.float64) + 0.5, np.arange(w, dtype=np.float64) + 0.5, indexing="ij")
    xin = (a * xs + b * ys) + c
    yin = (d * xs + e * ys) + f
    inside = (xin >= 0) & (xin < w) & (yin >= 0) & (yin < h)
    xin, yin = np.where(inside, xin, 0.5) - 0.5, np.where(inside, yin, 0.5) - 0.5
    fx, fy = np.floor(xin), np.floor(yin)
    dx, dy = (xin - fx)[..., None], (yin - fy)[..., None]
    x0, y0 = fx.astype(np.int64), fy.astype(np.int64)
    xa, xq = np.clip(x0, 0, w - 1), np.clip(x0 + 1, 0, w - 1)
    ya = np.clip(y0, 0, h - 1)
    second = (y0 + 1 >= 0) & (y0 + 1 < h)
    yb = np.where(second, y0 + 1, ya)
    v = img.astype(np.float64)
    pa, qa, pb, qb = v[ya, xa], v[ya, xq], v[yb, xa], v[yb, xq]
    v1 = pa + (qa - pa) * dx
    v2 = np.where(second[..., None], pb + (qb - pb) * dx, v1)
    res = (v1 + (v2 - v1) * dy).astype(np.int64).astype(np.uint8)
    return np.where(inside[..., None], res, np.asarray(fill, dtype=np.uint8)[None, None, :])


def apply_row(img, row, order=0):
    """One op (an int32 (16,) table row) on one image (h, w, 3) uint8 in stored order."""
    row = np.asarray(row, dtype=np.int32)
    kind, w1, w2 = int(row[0]), int(row[1]), int(row[2])
    fac = row[1:2].view(np.float32)[0]
    v = img.astype(np.int64)
    if img.size == 0 or kind == IDENTITY:
        return img.copy()
    if kind == INVERT:
        return (255 - v).astype(np.uint8)
    if kind == POSTERIZE:
        return (v & w1).astype(np.uint8)
    if kind == SOLARIZE:
        return np.where(v < w1, v, 255 - v).astype(np.uint8)
    if kind == SOLARIZE_ADD:
        return np.where(v < w1, np.minimum(255, v + w2), v).astype(np.uint8)
    if kind in (AUTOCONTRAST, EQUALIZE):
        lut = autocontrast_lut if kind == AUTOCONTRAST else equalize_lut
        return np.stack([lut(img[..., c])[img[..., c]] for c in range(3)], axis=-1)
    if kind == BRIGHTNESS:
        return blend(0, fac, img)
    if kind == CONTRAST:
        s, n = int(grey(img, order).sum()), img.shape[0] * img.shape[1]
        return blend((2 * s + n) // (2 * n), fac, img)
    if kind == COLOR:
        return blend(grey(img, order)[..., None], fac, img)
    if kind == SHARPNESS:
        return blend(smooth(img), fac, img)
    if kind == AFFINE:
        return affine(img, np.ascontiguousarray(row[1:13]).view(np.float64), [(int(row[13]) >> (8 * c)) & 255 for c in range(3)])
    raise ValueError("kind %d" % kind)


def apply_layers(frames, table, t, sizes=None, order=0):
    """frames (n, hs, ws, 3) uint8, table (n / t, layers, 16): every layer in turn on each frame's own hs_i x ws_i image; the padding keeps its bytes."""
    out = np.array(frames, dtype=np.uint8, copy=True)
    for i in range(out.shape[0]):
        h, w = (int(v) for v in sizes[i]) if sizes is not None else out.shape[1:3]
        img = out[i, :h, :w]
        for row in table[i // t]:
            img = apply_row(img, row, order)
        out[i, :h, :w] = img
    return out
