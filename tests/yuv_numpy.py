"""numpy statement of the YUV 4:2:0 input of mvf_frames_yuv420_gather_resample_u8 (include/mvfnet_hip.h): the 20-bit integer conversion
of one (Y, U, V) triple, chroma replicated from sample (y >> 1, x >> 1), the I420 / NV12 frame layouts with a pitch -- planes or a frame
buffer -> the stored-order packed uint8 frames the packed-frame exports take -- plus helpers that build such buffers from random planes.

TEST INFRASTRUCTURE ONLY -- never imported by mvfnet_amd."""
import numpy as np

I420, NV12 = 0, 1
BGR, RGB = 0, 1
# standard -> (y_off, cY, cVR, cVG, cUG, cUB): BT.601 limited, BT.601 full (yuvj420p), BT.709 limited
COEF = {0: (16, 1.164, 1.596, 0.813, 0.391, 2.018),
        1: (0, 1.0, 1.402, 0.714136, 0.344136, 1.772),
        2: (16, 1.164384, 1.792741, 0.532909, 0.213249, 2.112402)}


def constants(standard):
    """(y_off, CY, CVR, CVG, CUG, CUB): every coefficient rint(c * 2^20)."""
    c = COEF[standard]
    return (int(c[0]),) + tuple(int(np.rint(v * float(1 << 20))) for v in c[1:])


def convert(y, u, v, standard):
    """Integer arrays (Y, U, V) of one shape -> (R, G, B) uint8: int32 arithmetic, arithmetic shift, saturation."""
    y_off, cy, cvr, cvg, cug, cub = constants(standard)
    y, u, v = (np.asarray(a).astype(np.int32) for a in (y, u, v))
    yp = np.maximum(0, y - y_off) * np.int32(cy) + np.int32(1 << 19)
    u = u - 128
    v = v - 128
    r = (yp + np.int32(cvr) * v) >> 20
    g = (yp - np.int32(cvg) * v - np.int32(cug) * u) >> 20
    b = (yp + np.int32(cub) * u) >> 20
    return tuple(np.clip(c, 0, 255).astype(np.uint8) for c in (r, g, b))


def convert_float(y, u, v, standard):
    """The float definition the integer formula approximates: the decimal coefficients in float64, rounded to nearest, saturated."""
    y_off, cy, cvr, cvg, cug, cub = COEF[standard]
    y, u, v = (np.asarray(a).astype(np.float64) for a in (y, u, v))
    yp = np.maximum(0.0, y - y_off) * cy
    u = u - 128.0
    v = v - 128.0
    return tuple(np.clip(np.rint(c), 0, 255).astype(np.uint8) for c in (yp + cvr * v, yp - cvg * v - cug * u, yp + cub * u))


def planes_to_packed(y, u, v, standard=0, order=BGR):
    """Y (n, h, w), U, V (n, >= ceil(h / 2), >= ceil(w / 2)) uint8 -> (n, h, w, 3) uint8 packed frames in stored `order`."""
    n, h, w = y.shape
    yy, xx = np.arange(h)[:, None] >> 1, np.arange(w)[None, :] >> 1
    r, g, b = convert(y, u[:, yy, xx], v[:, yy, xx], standard)
    return np.stack((b, g, r) if order == BGR else (r, g, b), axis=-1)


def split(buf, layout):
    """(n, 3 * hs / 2, pitch) uint8 frame buffers -> Y (n, hs, pitch), U, V (n, hs / 2, pitch / 2), pitch padding included."""
    n, rows3, pitch = buf.shape
    hs = rows3 // 3 * 2
    assert rows3 * 2 == hs * 3 and hs % 2 == 0 and pitch % 2 == 0
    flat = buf.reshape(n, -1)
    y, c = flat[:, :hs * pitch].reshape(n, hs, pitch), flat[:, hs * pitch:]
    if layout == I420:
        q = (hs // 2) * (pitch // 2)
        return y, c[:, :q].reshape(n, hs // 2, pitch // 2), c[:, q:].reshape(n, hs // 2, pitch // 2)
    uv = c.reshape(n, hs // 2, pitch // 2, 2)
    return y, uv[..., 0], uv[..., 1]


def to_packed(buf, layout, standard=0, order=BGR, width=None):
    """(..., 3 * hs / 2, pitch) uint8 YUV 4:2:0 frames -> (n, hs, width, 3) uint8: the packed frames they stand for."""
    buf = np.asarray(buf)
    y, u, v = split(buf.reshape((-1,) + buf.shape[-2:]), layout)
    width = y.shape[2] if width is None else width
    return planes_to_packed(y[:, :, :width], u, v, standard, order)


def random_planes(n, h, w, seed):
    """Uniform random Y (n, h, w), U, V (n, ceil(h / 2), ceil(w / 2)): every byte value occurs, so Y < 16 and saturation do."""
    rng = np.random.RandomState(seed)
    ch, cw = (h + 1) // 2, (w + 1) // 2
    return tuple(rng.randint(0, 256, size=s).astype(np.uint8) for s in ((n, h, w), (n, ch, cw), (n, ch, cw)))


def pack(y, u, v, layout, pitch=None, hs=None, fill_seed=None):
    """Planes -> (n, 3 * hs / 2, pitch) uint8 frame buffers in `layout`; hs and pitch default to the luma size rounded up to even.  The bytes
    no pixel owns (pitch and height padding) are zero, or random with `fill_seed` (nothing may depend on them)."""
    n, h, w = y.shape
    hs = h + h % 2 if hs is None else hs
    pitch = w + w % 2 if pitch is None else pitch
    assert hs % 2 == 0 and pitch % 2 == 0 and hs >= h and pitch >= w
    if fill_seed is None:
        buf = np.zeros((n, hs * 3 // 2, pitch), dtype=np.uint8)
    else:
        buf = np.random.RandomState(fill_seed).randint(0, 256, size=(n, hs * 3 // 2, pitch)).astype(np.uint8)
    by, bu, bv = split(buf, layout)                              # views of buf
    by[:, :h, :w] = y
    bu[:, :u.shape[1], :u.shape[2]] = u
    bv[:, :v.shape[1], :v.shape[2]] = v
    return buf
