"""fp64 reference of the channels-last MVF stencil primitives (mvf_nhwc_stencil*, mvf_nhwc_tapgrad: csrc/mvf_nhwc.hip) for tests/test_stencil_variants_gpu.py,
written from shifted arrays (np.pad + slices) and numpy only; proved against oracle/mvf_numpy.py in tests/test_stencil_ref_cpu.py.

Tensors are 2-d [m, pitch] with m = nt * h * w rows in (clip, t, h, w) order, as the kernels see them; the gate bits are [m, pitch / 4] bytes, bit j of byte k
= channel 4k + j."""
import collections

import numpy as np

# nt frames of h x w pixels in clips of T, the first cs channels are the slice; mode = bit 1 (T view, always taken) | 2 (H view) | 4 (W view)
Desc = collections.namedtuple("Desc", "nt h w T cs mode")
VIEW_H, VIEW_W = 2, 4


def _neighbours(s, axis):
    """(s[i - 1], s[i + 1]) along `axis`, zeros outside."""
    pad = [(0, 0)] * s.ndim
    pad[axis] = (1, 1)
    p = np.pad(s, pad)
    n = s.shape[axis]
    return np.take(p, np.arange(0, n), axis=axis), np.take(p, np.arange(2, n + 2), axis=axis)


def _axes(desc):
    """the view axes of the (clips, T, h, w, cs) tensor, with their tap slot"""
    return [(1, "t")] + ([(2, "h")] if desc.mode & VIEW_H else []) + ([(3, "w")] if desc.mode & VIEW_W else [])


def unpack_bits(bits, cs):
    """[m, >= cs / 4] bytes -> [m, cs] of 0.0 / 1.0"""
    bits = np.asarray(bits, dtype=np.uint8)
    c = np.arange(cs)
    return ((bits[:, c // 4] >> (c % 4).astype(np.uint8)) & 1).astype(np.float64)


def hswish(u):
    return u * np.minimum(np.maximum(u + 3.0, 0.0), 6.0) / 6.0


def stencil(x, desc, wt, wh=None, ww=None, flip=0, scale=None, shift=None, addend=None, addend_c=0, addend_bits=None, out_gate_bits=None):
    """(y, A), both [m, cs] fp64: y = ([hswish(scale * v + shift)] + gated addend) * output gate with v = the sum of the present 3-tap views of x[:, :cs];
    A = the same expression on absolute values (1.5 = max |hswish'| in front of the activation's argument): what a rounding error of y is proportional to."""
    x = np.asarray(x, dtype=np.float64)
    m, cs = desc.nt * desc.h * desc.w, desc.cs
    assert x.shape[0] == m and x.shape[1] >= cs and desc.nt % desc.T == 0
    s = x[:, :cs].reshape(desc.nt // desc.T, desc.T, desc.h, desc.w, cs)
    taps = dict(t=wt, h=wh, w=ww)
    v, a = np.zeros_like(s), np.zeros_like(s)
    for axis, slot in _axes(desc):
        k = np.asarray(taps[slot], dtype=np.float64).reshape(cs, 3)
        if flip:
            k = k[:, ::-1]
        lo, hi = _neighbours(s, axis)
        v += k[:, 0] * lo + k[:, 1] * s + k[:, 2] * hi
        a += np.abs(k[:, 0]) * np.abs(lo) + np.abs(k[:, 1]) * np.abs(s) + np.abs(k[:, 2]) * np.abs(hi)
    v, a = v.reshape(m, cs), a.reshape(m, cs)
    if scale is not None:
        scale, shift = np.asarray(scale, dtype=np.float64), np.asarray(shift, dtype=np.float64)
        v = hswish(scale * v + shift)
        a = 1.5 * (np.abs(scale) * a + np.abs(shift))
    if addend is not None:
        addend = np.asarray(addend, dtype=np.float64)
        assert addend.shape == (m, addend_c) and addend_c >= cs
        on = unpack_bits(addend_bits, cs) if addend_bits is not None else 1.0
        v = v + addend[:, :cs] * on
        a = a + np.abs(addend[:, :cs]) * on
    else:
        assert addend_bits is None
    if out_gate_bits is not None:
        g = unpack_bits(out_gate_bits, cs)
        v, a = v * g, a * g
    return v, a


def stats(y_stored, K=None):
    """per-channel (sum(y - K), sum((y - K)^2)) over the rows of y_stored [m, cs]; K = None is 0"""
    d = np.asarray(y_stored, dtype=np.float64) - (0.0 if K is None else np.asarray(K, dtype=np.float64))
    return d.sum(axis=0), (d * d).sum(axis=0)


def tapgrad(x, dy, desc):
    """(dwt, dwh, dww), each [cs, 3] fp64: dw[c, j] = sum_p dy[p, c] * x[p + (j - 1) along the view axis, c] (the centre tap is the same sum in every view);
    the gradient of a view whose mode bit is off is zero.  tapgrad(|x|, |dy|, desc) is the sum of |terms|."""
    x, dy = np.asarray(x, dtype=np.float64), np.asarray(dy, dtype=np.float64)
    m, cs = desc.nt * desc.h * desc.w, desc.cs
    assert x.shape[0] == m and dy.shape[0] == m and x.shape[1] >= cs and dy.shape[1] >= cs
    shape = (desc.nt // desc.T, desc.T, desc.h, desc.w, cs)
    s, g = x[:, :cs].reshape(shape), dy[:, :cs].reshape(shape)
    dw = dict(t=np.zeros((cs, 3)), h=np.zeros((cs, 3)), w=np.zeros((cs, 3)))
    for axis, slot in _axes(desc):
        lo, hi = _neighbours(s, axis)
        for j, nb in enumerate((lo, s, hi)):
            dw[slot][:, j] = (g * nb).sum(axis=(0, 1, 2, 3))
    return dw["t"], dw["h"], dw["w"]
