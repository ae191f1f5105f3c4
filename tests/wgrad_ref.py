"""Independent fp64 reference of the channels-last conv weight gradient (mvf_conv2d_nhwc_wgrad, include/mvfnet_hip.h), written from the entry point's
semantics as explicit tap loops over a zero-padded array -- no autograd, no im2col index arithmetic of the kernels.  Proved against
torch.nn.grad.conv2d_weight / autograd in tests/test_wgrad_ref_cpu.py.

    dW[co, ci, kh, kw] = sum_{n, oh, ow} dz[n, oh, ow, co] * X[n, oh * s - pad + kh, ow * s - pad + kw, ci]          (X = 0 outside the h x w map)

The operand as the entry point defines it: `x` is a buffer of pixels with a PITCH (x_pix_stride elements from one pixel to the next; >= cin for a channel
slice of a wider tensor, < cin for the stem's overlapping view); with a split operand, channel ci < split_c is read from `x2` at column ci with pitch
x2_pix_stride and channel ci >= split_c from `x` at column ci with pitch x_pix_stride."""
import numpy as np


def gather_channels(buf, n, h, w, pitch, c0, c1):
    """X[n, ih, iw, ci - c0] = buf_n[(ih * w + iw) * pitch + ci] for ci in [c0, c1): `buf` holds n equally long images, flat."""
    flat = np.asarray(buf, dtype=np.float64).reshape(n, -1)
    assert flat.shape[1] >= h * w * pitch, "the buffer is shorter than n x h x w pixels of this pitch"
    idx = (np.arange(h * w) * pitch)[:, None] + np.arange(c0, c1)[None, :]
    over = int(idx.max()) + 1 - flat.shape[1] if idx.size else 0
    if over > 0:
        # only an overlapping view (pitch < channels: the stem's) may run past the image with its LAST pixels' channels; no tap of a valid call reads
        # them, and they are NaN here so that one that did would show
        assert pitch < c1, "the last pixel's channels run past the image"
        flat = np.concatenate([flat, np.full((n, over), np.nan)], axis=1)
    return flat[:, idx].reshape(n, h, w, c1 - c0)


def operand(x, n, h, w, cin, x_pix_stride, x2=None, split_c=0, x2_pix_stride=0):
    """The (n, h, w, cin) tensor the weight gradient contracts with, assembled from x (and x2 below split_c)."""
    if not split_c:
        return gather_channels(x, n, h, w, x_pix_stride, 0, cin)
    assert x2 is not None and 0 < split_c < cin
    return np.concatenate([gather_channels(x2, n, h, w, x2_pix_stride, 0, split_c), gather_channels(x, n, h, w, x_pix_stride, split_c, cin)], axis=3)


def wgrad_taps(dz, X, kh, kw, stride, pad):
    """(dW, absref), both (cout, cin, kh, kw): dW as in the module docstring, absref = the same sum over |dz| * |X| (the scale an accumulation error is
    relative to, for diagnostics).  dz (n, ho, wo, cout), X (n, h, w, cin), fp64."""
    dz = np.asarray(dz, dtype=np.float64)
    X = np.asarray(X, dtype=np.float64)
    n, ho, wo, cout = dz.shape
    n2, h, w, cin = X.shape
    assert n == n2
    lo = pad
    hi_h = max(0, (ho - 1) * stride - pad + kh - h)          # rows / columns a tap reaches past the map
    hi_w = max(0, (wo - 1) * stride - pad + kw - w)
    Xp = np.zeros((n, lo + h + hi_h, lo + w + hi_w, cin))
    Xp[:, lo:lo + h, lo:lo + w, :] = X
    dW = np.zeros((cout, cin, kh, kw))
    absref = np.zeros((cout, cin, kh, kw))
    dz2 = dz.reshape(-1, cout)
    adz2 = np.abs(dz2)
    for i in range(kh):
        for j in range(kw):
            # output pixel (oh, ow) reads padded row oh * s + i (= input row oh * s - pad + i), padded column ow * s + j
            win = Xp[:, i:i + (ho - 1) * stride + 1:stride, j:j + (wo - 1) * stride + 1:stride, :].reshape(-1, cin)
            dW[:, :, i, j] = dz2.T @ win
            absref[:, :, i, j] = adz2.T @ np.abs(win)
    return dW, absref


def wgrad(dz, x, n, h, w, cin, kh, kw, stride, pad, x_pix_stride=None, x2=None, split_c=0, x2_pix_stride=0):
    """The weight gradient of the entry point's plain form (kw_packed == kw_real, cin_packed == cin_real): (dW, absref), (cout, cin, kh, kw)."""
    X = operand(x, n, h, w, cin, cin if x_pix_stride is None else x_pix_stride, x2, split_c, x2_pix_stride)
    return wgrad_taps(dz, X, kh, kw, stride, pad)


def wgrad_stem(dz, xp, n, hp, wp, kw_packed=8, cin_packed=4, kw_real=7, cin_real=3, kh=7, stride=2):
    """The stem's packed view: xp = the zero-padded channels-last input (n, hp, wp, cin_packed); a kh x 1 conv of stride `stride`, no padding, over
    kw_packed * cin_packed "channels" of pixel pitch cin_packed (channel c = pixel offset c // cin_packed, real channel c % cin_packed) -- a pixel step of
    the view is ONE input pixel, so the view's column stride of `stride` is the real conv's.  The packed gradient (cout, kw_packed * cin_packed, kh, 1) is
    unpacked to (cout, cin_real, kh, kw_real): packed taps >= kw_real and packed channels >= cin_real are dropped."""
    cv = kw_packed * cin_packed
    dWp, absp = wgrad(dz, xp, n, hp, wp, cv, kh, 1, stride, 0, x_pix_stride=cin_packed)

    def unpack(a):
        a = a[:, :, :, 0].reshape(a.shape[0], kw_packed, cin_packed, kh)          # (co, kw, ci, kh)
        return np.ascontiguousarray(a.transpose(0, 2, 3, 1)[:, :cin_real, :, :kw_real])
    return unpack(dWp), unpack(absp)
