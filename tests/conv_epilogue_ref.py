"""fp64 reference of the implicit-GEMM conv's training epilogues (csrc/conv_nhwc.hip), written from the DOCUMENTED semantics -- include/mvfnet_hip.h and the
ConvArgs comments -- not from the kernel's code.  CPU only (numpy / torch double).

Every function starts from the operands AS STORED (x, the packed weights, residual, z ...: already rounded to the storage type and read back as fp64),
computes in fp64 and rounds exactly where the documentation says the kernel rounds: the stored tensor once, and the recomputed z3 of the BatchNorm-apply /
BatchNorm-backward epilogues once.  Tensors are channels-last, flattened to [M][C] with M = n * ho * wo; packed weights are [cout][kh][kw][cin]; sign / gate
bits are [M][C / 4] bytes, bit j of byte k = channel 4k + j; partial sums are CHANNEL-MAJOR [C][rows][2], one row per 128 output rows (mvf_conv2d_stats_rows)."""
import numpy as np
import torch
import torch.nn.functional as F

ROWS = 128          # output rows per statistics partial


def rnd(a, dtype):
    """fp64 -> storage type (one rounding, through fp32 as the kernels' accumulators are) -> fp64.  dtype: "f32" | "bf16"."""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).float()
    if dtype == "bf16":
        t = t.bfloat16()
    return t.double().numpy()


def ulp(a, dtype):
    """Spacing of the storage type at |a| (fp64 array)."""
    s = np.spacing(np.abs(np.asarray(a, dtype=np.float64)).astype(np.float32)).astype(np.float64)
    return s * 65536.0 if dtype == "bf16" else s


def unpack_bits(bits, c):
    """[M][c / 4] bytes -> [M][c] of 0 / 1: bit j of byte k gates channel 4k + j (only the low four bits of a byte are used)."""
    b = np.asarray(bits, dtype=np.uint8)
    assert b.shape[1] * 4 == c
    return ((b[:, :, None] >> np.arange(4, dtype=np.uint8)[None, None, :]) & 1).reshape(b.shape[0], c).astype(np.float64)


def pack_bits(mask):
    """[M][c] booleans -> [M][c / 4] bytes in the same layout."""
    m = np.asarray(mask).astype(np.uint8)
    m4 = m.reshape(m.shape[0], m.shape[1] // 4, 4)
    return (m4[:, :, 0] | (m4[:, :, 1] << 1) | (m4[:, :, 2] << 2) | (m4[:, :, 3] << 3)).astype(np.uint8)


def pack_dgrad(w_oihw):
    """mvf_pack_conv_weight_dgrad's layout (include/mvfnet_hip.h): packed[ci][kh'][kw'][co] = w[co][ci][KH-1-kh'][KW-1-kw']."""
    w = np.asarray(w_oihw, dtype=np.float64)
    return np.ascontiguousarray(w[:, :, ::-1, ::-1].transpose(1, 2, 3, 0))


def out_size(h, k, stride, pad, in_dil=1):
    """The largest output extent mvf_conv_desc_t allows (a strided data gradient may ask for dil - 1 fewer)."""
    dil = max(in_dil, 1)
    return ((h - 1) * dil + 1 + 2 * pad - k) // stride + 1 + (dil - 1)


def conv(x, wp, stride=1, pad=0, in_dil=1, ho=None, wo=None):
    """x [n][h][w][cin], wp [cout][kh][kw][cin] (fp64) -> [n * ho * wo][cout] fp64.  in_dil = s > 1: x is read as if zero-upsampled by s."""
    xt = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).permute(0, 3, 1, 2)
    dil = max(in_dil, 1)
    if dil > 1:
        n, c, h, w = xt.shape
        up = torch.zeros(n, c, (h - 1) * dil + 1 + (dil - 1), (w - 1) * dil + 1 + (dil - 1), dtype=torch.float64)
        up[:, :, 0:(h - 1) * dil + 1:dil, 0:(w - 1) * dil + 1:dil] = xt
        xt = up
    wt = torch.from_numpy(np.ascontiguousarray(wp, dtype=np.float64)).permute(0, 3, 1, 2)
    y = F.conv2d(xt, wt, stride=stride, padding=pad)
    ho = y.shape[2] if ho is None else ho
    wo = y.shape[3] if wo is None else wo
    assert ho <= y.shape[2] and wo <= y.shape[3]
    y = y[:, :, :ho, :wo].permute(0, 2, 3, 1)
    return np.ascontiguousarray(y.numpy()).reshape(-1, wp.shape[0])


def partials(rows_of, v1, v2):
    """Channel-major [C][rows][2]: per-128-row column sums of v1 and v2 over the row runs `rows_of` (a list of index arrays, one per run: the whole tensor,
    or the parity classes of a strided data gradient back to back)."""
    out = []
    for idx in rows_of:
        for r0 in range(0, len(idx), ROWS):
            sel = idx[r0:r0 + ROWS]
            out.append(np.stack([v1[sel].sum(0), v2[sel].sum(0)], axis=1))       # [C][2]
    return np.ascontiguousarray(np.stack(out, axis=1))                            # [C][rows][2]


def row_runs(n, ho, wo, in_dil=1):
    """The runs of output rows that share partial rows, in mvf_conv2d_stats_rows order: everything, or -- in_dil = s > 1 -- the s * s parity classes
    (oh % s, ow % s), each in (image, oh, ow) order."""
    m = np.arange(n * ho * wo).reshape(n, ho, wo)
    s = max(in_dil, 1)
    if s == 1:
        return [m.reshape(-1)]
    runs = []
    for ph in range(s):
        for pw in range(s):
            r = m[:, ph::s, pw::s].reshape(-1)
            if r.size:
                runs.append(r)
    return runs


def stats_rows(n, ho, wo, in_dil=1):
    return sum((len(r) + ROWS - 1) // ROWS for r in row_runs(n, ho, wo, in_dil))


# ------------------------------------------------------------------------------------------------ entry points
def fwd_stats(x, wp, dtype, shift=None, acc=None, **geom):
    """mvf_conv2d_nhwc_fwd_stats: z = conv rounded once to the storage type; partials of (z_stored - shift) and its square."""
    z = rnd(_acc(acc, x, wp, geom), dtype)
    k = 0.0 if shift is None else np.asarray(shift, dtype=np.float64)[None, :]
    n, ho, wo = _nhw(x, wp, geom)
    return z, partials(row_runs(n, ho, wo), z - k, (z - k) ** 2)


def fwd(x, wp, dtype, bias=None, res=None, relu=False, acc=None, **geom):
    """mvf_conv2d_nhwc_fwd_ws: act(conv + bias + residual), rounded once."""
    v = _acc(acc, x, wp, geom)
    if bias is not None:
        v = v + np.asarray(bias, dtype=np.float64)[None, :]
    if res is not None:
        v = v + res
    if relu:
        v = np.maximum(v, 0.0)
    return rnd(v, dtype)


def fwd_resmask(x, wp, dtype, res, res_bits=None, out_gate=None, res_c0=0, bias=None, colsums=False, acc=None, **geom):
    """mvf_conv2d_nhwc_fwd_resmask[_gate[_colsums]]: the residual is read only for channels >= res_c0 and gated by res_bits; the OUTPUT gate applies to
    channels >= res_c0 only; the column sums (y, y^2) are those of what is stored, every channel."""
    v = _acc(acc, x, wp, geom)
    c = v.shape[1]
    hi = (np.arange(c) >= res_c0)[None, :]
    if bias is not None:
        v = v + np.asarray(bias, dtype=np.float64)[None, :]
    r = np.where(hi, res, 0.0)
    if res_bits is not None:
        r = r * unpack_bits(res_bits, c)
    v = v + r
    if out_gate is not None:
        v = np.where(hi, v * unpack_bits(out_gate, c), v)
    y = rnd(v, dtype)
    if not colsums:
        return y
    n, ho, wo = _nhw(x, wp, geom)
    return y, partials(row_runs(n, ho, wo), y, y * y)


def dgrad_bnsums(dz, wd, dtype, z, mean, invstd, scale, shift, bias=None, acc=None, **geom):
    """mvf_conv2d_nhwc_dgrad_bnsums[_split]: y = the transposed convolution (a conv of dz with the data-gradient pack, in_dil = the forward stride)
    [+ bias], rounded once; gm = y_stored * [scale * z + shift > 0]; partials of gm and gm * xhat, xhat = (z - mean) * invstd.  A split operand is passed
    concatenated: dz = [x2 | x] along the channels."""
    v = _acc(acc, dz, wd, geom)
    if bias is not None:
        v = v + np.asarray(bias, dtype=np.float64)[None, :]
    y = rnd(v, dtype)
    f = lambda a: np.asarray(a, dtype=np.float64)[None, :]        # noqa: E731
    gm = y * ((f(scale) * z + f(shift)) > 0)
    xhat = (z - f(mean)) * f(invstd)
    n, ho, wo = _nhw(dz, wd, geom)
    return y, partials(row_runs(n, ho, wo, geom.get("in_dil", 1)), gm, gm * xhat)


def gate_margin(z, scale, shift):
    """|scale * z + shift| -- the test repairs z until this exceeds 1e-3 everywhere, so the gate is the same in any arithmetic."""
    return np.abs(np.asarray(scale, dtype=np.float64)[None, :] * z + np.asarray(shift, dtype=np.float64)[None, :])


def fwd_bnapply(x, wp, dtype, scale, shift, res, rscale=None, rshift=None, round_z3=True, acc=None, **geom):
    """mvf_conv2d_nhwc_fwd_bnapply: z3 = conv rounded to the storage type; t = scale * z3 + shift + res', res' = res or rscale * res + rshift;
    out = relu(t) rounded; bits = [out > 0].  Returns a dict with out, bits, t, z3 and res'."""
    f = lambda a: np.asarray(a, dtype=np.float64)[None, :]        # noqa: E731
    z3 = _acc(acc, x, wp, geom)
    if round_z3:
        z3 = rnd(z3, dtype)
    r = res if rscale is None else f(rscale) * res + f(rshift)
    t = f(scale) * z3 + f(shift) + r
    out = rnd(np.maximum(t, 0.0), dtype)
    return dict(out=out, bits=pack_bits(out > 0), t=t, z3=z3, res=r)


def fwd_bnbwd(x, wp, dtype, g, bits, mean, invstd, gamma=None, dgamma=None, dbeta=None, round_z3=True, z3_ulps=0, acc=None, **geom):
    """mvf_conv2d_nhwc_fwd_bnbwd_sums (mode 10) and _apply (mode 9) on the rounded recomputed z3 (moved by z3_ulps storage ulps: the sensitivity probe of
    the test), gm = g * bit:
        sums: partials of gm and gm * (z3 - mean) * invstd
        dz  : gamma * invstd * (gm - dbeta / M - (z3 - mean) * invstd * dgamma / M), rounded once (only with gamma / dgamma / dbeta)."""
    f = lambda a: np.asarray(a, dtype=np.float64)[None, :]        # noqa: E731
    z3 = _acc(acc, x, wp, geom)
    if round_z3:
        z3 = rnd(z3, dtype)
    if z3_ulps:
        z3 = z3 + z3_ulps * ulp(z3, dtype)
    m, c = z3.shape
    gm = g * unpack_bits(bits, c)
    xhat = (z3 - f(mean)) * f(invstd)
    n, ho, wo = _nhw(x, wp, geom)
    out = dict(z3=z3, gm=gm, sums=partials(row_runs(n, ho, wo), gm, gm * xhat))
    if gamma is not None:
        dz = f(gamma) * f(invstd) * (gm - f(dbeta) / m - xhat * f(dgamma) / m)
        out["dz_exact"] = dz
        out["dz"] = rnd(dz, dtype)
    return out


def _acc(acc, x, wp, geom):
    """The fp64 convolution, or the caller's copy of it (acc: the same conv(x, wp, **geom), computed once for several entry points)."""
    return conv(x, wp, **geom) if acc is None else np.array(acc, dtype=np.float64)


def _nhw(x, wp, geom):
    n, h, w, _ = x.shape
    kh, kw = wp.shape[1], wp.shape[2]
    s, p, d = geom.get("stride", 1), geom.get("pad", 0), geom.get("in_dil", 1)
    ho = geom.get("ho") or out_size(h, kh, s, p, d)
    wo = geom.get("wo") or out_size(w, kw, s, p, d)
    return n, ho, wo
