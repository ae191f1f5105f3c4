"""fp64 restatement of mvf_stem_erase (include/mvfnet_hip.h), shared by test_erase_cpu.py and test_erase_gpu.py.  The reference project has no such
feature; the semantics are the ones the header states.

Table: boxes int32 (planes, max_boxes, 5) = y0, x0, y1, x1, mode (half-open box in image pixels, before the pad; mode 1 = constant colour, 2 = noise, anything
else = unused; the higher slot wins); fill fp32 (planes, max_boxes, 4); key uint32 (2).  Noise: Philox4x32-10(counter = (x, y, plane, 0), key), two Box-Muller
pairs from the four words."""
import numpy as np

UNTOUCHED, CONST, NOISE = 0, 1, 2
_M0, _M1, _W0, _W1, _MASK = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85, 0xFFFFFFFF


def philox4x32_10(counter, key):
    """counter: four broadcastable integer arrays (or ints), key: two integers < 2^32 -> four uint64 arrays holding the 32-bit output words."""
    c0, c1, c2, c3 = np.broadcast_arrays(*[np.asarray(c, dtype=np.uint64) & np.uint64(_MASK) for c in counter])
    k0, k1 = int(key[0]) & _MASK, int(key[1]) & _MASK
    m0, m1, mask, s32 = np.uint64(_M0), np.uint64(_M1), np.uint64(_MASK), np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c0, m1 * c2                         # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> s32) ^ c1 ^ np.uint64(k0), p1 & mask, (p0 >> s32) ^ c3 ^ np.uint64(k1), p0 & mask
        k0, k1 = (k0 + _W0) & _MASK, (k1 + _W1) & _MASK
    return c0, c1, c2, c3


def normals(words, dtype=np.float64):
    """The three N(0, 1) values of the header from the four Philox words, every step in `dtype` (np.float32 restates the kernel's own arithmetic with numpy's
    functions): stacked on a new last axis."""
    ft = np.dtype(dtype).type
    w0, w1, w2, w3 = (np.asarray(w, dtype=np.uint64) for w in words)
    inv24, two_pi, s8, one = ft(2.0 ** -24), ft(2.0 * np.pi), np.uint64(8), np.uint64(1)
    u1, u2 = ((w0 >> s8) + one).astype(dtype) * inv24, (w1 >> s8).astype(dtype) * inv24
    u3, u4 = ((w2 >> s8) + one).astype(dtype) * inv24, (w3 >> s8).astype(dtype) * inv24
    r1, r2 = np.sqrt(ft(-2.0) * np.log(u1)), np.sqrt(ft(-2.0) * np.log(u3))
    t1, t2 = two_pi * u2, two_pi * u4
    out = np.stack([r1 * np.cos(t1), r1 * np.sin(t1), r2 * np.cos(t2)], axis=-1)
    assert out.dtype == np.dtype(dtype)
    return out


def plane_noise(planes, h, w, key, dtype=np.float64):
    """(planes, h, w, 3): the noise of every image pixel of every plane."""
    p, y, x = np.meshgrid(np.arange(planes), np.arange(h), np.arange(w), indexing="ij")
    return normals(philox4x32_10((x, y, p, 0), key), dtype)


def erase_ref(xp, boxes, fill, key, pad):
    """xp (planes, hp, wp, 4): the STORED operand values (any float dtype; taken to fp64).  Returns (v, kind): v fp64 = the erased operand before the rounding
    to the storage type (untouched elements: the stored value; constant: the fp32 colour; noise: the fp64 normal), kind int8 (planes, hp, wp, 4) per element.
    The fourth channel, the border and the padding columns are UNTOUCHED everywhere (an erased pixel's fourth channel is stored as the zero it is)."""
    x = np.asarray(xp, dtype=np.float64)
    planes, hp, wp, _ = x.shape
    boxes, fill = np.asarray(boxes), np.asarray(fill)
    h = hp - 2 * pad
    w = wp - 2 * pad                                        # (clamping to the padded width's interior; tables of the tests stay inside the image)
    v = x.copy()
    kind = np.zeros(x.shape, dtype=np.int8)
    noise = plane_noise(planes, h, w, key)
    for p in range(planes):
        for k in range(boxes.shape[1]):
            y0, x0, y1, x1, mode = (int(c) for c in boxes[p, k])
            if mode not in (CONST, NOISE):
                continue
            y0, y1 = (min(max(c, 0), h) for c in (y0, y1))
            x0, x1 = (min(max(c, 0), w) for c in (x0, x1))
            if y1 <= y0 or x1 <= x0:
                continue
            ys, xs = slice(y0 + pad, y1 + pad), slice(x0 + pad, x1 + pad)
            kind[p, ys, xs, :3] = mode
            v[p, ys, xs, :3] = noise[p, y0:y1, x0:x1] if mode == NOISE else np.asarray(fill[p, k, :3], dtype=np.float32).astype(np.float64)
    return v, kind


def erase_nchw(clips, boxes, fill, key, noise_hw3=None):
    """The same erase on clips stored (B, T, 3, H, W) fp32, on the host: constant boxes take the fp32 colour; noise boxes take `noise_hw3`
    (planes, H, W, 3) fp32 values handed in (the device's own noise, where bit equality is wanted).  Returns a new array."""
    out = np.array(clips, dtype=np.float32, copy=True)
    b, t, _, h, w = out.shape
    flat = out.reshape(b * t, 3, h, w)
    for p in range(b * t):
        for k in range(boxes.shape[1]):
            y0, x0, y1, x1, mode = (int(c) for c in boxes[p, k])
            if mode == CONST:
                flat[p, :, y0:y1, x0:x1] = np.asarray(fill[p, k, :3], dtype=np.float32)[:, None, None]
            elif mode == NOISE:
                flat[p, :, y0:y1, x0:x1] = np.transpose(noise_hw3[p, y0:y1, x0:x1], (2, 0, 1))
    return flat.reshape(out.shape)
