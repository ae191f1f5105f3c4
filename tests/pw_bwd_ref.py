"""fp64 reference (numpy only) of the fused pointwise-conv backward entry points -- csrc/pw_bwd_fused.hip (mvf_conv1x1_bwd_fused), csrc/pw_sums_pair.hip
(mvf_conv1x1_bnbwd_sums_pair), csrc/pw_sums.hip (the statistics-only / BatchNorm-backward-sums passes of a conv that is never stored) and csrc/bnbwd_wgrad.hip
(mvf_bn_bwd_apply_wgrad, mvf_bn_bwd_pair_wgrad) -- COMPOSED from the references the rest of the hot path is tested with, not restated: conv_epilogue_ref
(rnd, ulp, unpack_bits, fwd_bnbwd, dgrad_bnsums), bn_pool_ref (bn_bwd / bn_bwd_pair with their A terms) and wgrad_ref (wgrad + absref).  Proved against torch
float64 autograd of the bottleneck tail, with the roundings switched off, by tests/test_pw_bwd_ref_cpu.py.

Everything is a matrix [M][channels] of the operands AS STORED (bf16 values held in fp64); the per-channel vectors are the fp32 values the kernels are given.
`rounding=True` rounds where the documentation of the kernels says they round (the recomputed conv output, dz, the data gradient: once each, to bf16);
`rounding=False` rounds nowhere (the autograd comparison).  Sums are returned PER ELEMENT (v1, v2 [M][C]): a test adds them over exactly the rows a launch
plan assigns to a workgroup (rows_sum / blocks_sum).

Besides the values the functions return what bounds a kernel's deviation FROM THE REFERENCE ALONE: `und_z`, the elements of the conv output whose exact
value lies within `acc_err` of a bf16 rounding midpoint (an fp32 accumulator may round them to the other neighbour), and `und_dz` likewise for dz
(within 8 * 2^-24 * A of a midpoint, plus what an undecided z moves it)."""
import numpy as np

import bn_pool_ref as B
import conv_epilogue_ref as E
import wgrad_ref as W

ACC_REL = 2e-5           # the project's bound of an fp32 accumulator against the exact convolution, of the tensor's largest magnitude (test_conv_gpu.py)
ST = "bf16"


def f64(a):
    return np.asarray(a, dtype=np.float64)


def _x4(a):
    """[M][C] -> the channels-last tensor (1, M, 1, C) the conv references take."""
    return f64(a)[None, :, None, :]


def _w4(w):
    """[Cout][Cin] -> packed (Cout, 1, 1, Cin)."""
    return f64(w)[:, None, None, :]


def conv1x1(a, w):
    """The exact pointwise convolution: [M][K] x [C][K] -> [M][C]."""
    return f64(a) @ f64(w).T


def rnd(a, rounding=True):
    return E.rnd(a, ST) if rounding else f64(a)


def midpoint_gap(exact, rounded):
    """Distance of `exact` from the nearest bf16 rounding midpoint on the side of `rounded` it lies on (rounded = rnd(exact))."""
    exact, rounded = f64(exact), f64(rounded)
    u = E.ulp(rounded, ST)
    mant, _ = np.frexp(np.abs(rounded))
    below = np.where(mant == 0.5, 0.5 * u, u)                       # the spacing towards zero halves at a power of two
    half = 0.5 * np.where(np.abs(exact) >= np.abs(rounded), u, below)
    return half - np.abs(exact - rounded)


def undecided_z(exact, rounded):
    return midpoint_gap(exact, rounded) < ACC_REL * float(np.abs(exact).max())


def rows_sum(v, bounds):
    """[M][C] per-element terms -> [C][len(bounds)] sums over the row ranges [(begin, end), ...]."""
    return np.stack([f64(v)[b:e].sum(axis=0) for b, e in bounds], axis=1)


def blocks_sum(v, blocks_of, blk=32):
    """[M][C] -> [C][len(blocks_of)]: sums over lists of 32-row block indices (csrc/pw_sums.hip's walk)."""
    v = f64(v)
    out = []
    for blocks in blocks_of:
        idx = np.concatenate([np.arange(b * blk, min((b + 1) * blk, v.shape[0])) for b in blocks]) if len(blocks) else np.zeros(0, dtype=np.int64)
        out.append(v[idx].sum(axis=0))
    return np.stack(out, axis=1)


# ---------------------------------------------------------------------------------------------------------------- sums on a recomputed conv
def conv_bnbwd_sums(a, w, g, bits, mean, invstd, rounding=True, acc=None):
    """bn's backward sums on the recomputed z = rnd(conv1x1(a, w)): v1 = gm, v2 = gm (z - mean) invstd, gm = g * sign bit (pw_sums.hip MODE 1, one branch
    of pw_sums_pair.hip).  allow2: what ONE undecided rounding of z moves v2 by, |gm| invstd ulp(z), zero at decided elements."""
    acc = conv1x1(a, w) if acc is None else f64(acc)
    fb = E.fwd_bnbwd(_x4(a), _w4(w), ST, f64(g), bits, mean, invstd, round_z3=rounding, acc=acc)
    z, gm = fb["z3"], fb["gm"]
    xhat = (z - f64(mean)[None, :]) * f64(invstd)[None, :]
    und = undecided_z(acc, z) if rounding else np.zeros(z.shape, dtype=bool)
    return dict(acc=acc, z=z, gm=gm, xhat=xhat, v1=gm, v2=gm * xhat, und_z=und, allow2=np.where(und, np.abs(gm) * np.abs(f64(invstd))[None, :] * E.ulp(z, ST), 0.0))


def conv_stats(a, w, shift=None, rounding=True, acc=None):
    """The statistics-only pass (pw_sums.hip MODE 0): v1 = z - K, v2 = (z - K)^2 of z = rnd(conv1x1(a, w)); K = shift or 0."""
    acc = conv1x1(a, w) if acc is None else f64(acc)
    if rounding:
        z, _ = E.fwd_stats(_x4(a), _w4(w), ST, shift, acc=acc)
    else:
        z = acc
    k = 0.0 if shift is None else f64(shift)[None, :]
    und = undecided_z(acc, z) if rounding else np.zeros(z.shape, dtype=bool)
    u = E.ulp(z, ST)
    return dict(acc=acc, z=z, v1=z - k, v2=(z - k) ** 2, und_z=und, allow1=np.where(und, u, 0.0), allow2=np.where(und, 2.0 * np.abs(z - k) * u + u * u, 0.0))


# ---------------------------------------------------------------------------------------------------------------- gated sums of a stored gradient
def gated_sums(y, z, mean, invstd, scale, shift):
    """The next BatchNorm's backward sums over a STORED gradient y: gq = y [scale z + shift > 0]; v1 = gq, v2 = gq (z - mean) invstd."""
    f = lambda t: f64(t)[None, :]        # noqa: E731
    gq = f64(y) * ((f(scale) * f64(z) + f(shift)) > 0)
    return gq, gq * ((f64(z) - f(mean)) * f(invstd))


# ---------------------------------------------------------------------------------------------------------------- the one-pass backward of conv3
def conv1x1_bwd_fused(a, w, g, bits, gamma, mean, invstd, dgamma, dbeta, z_in=None, in_mean=None, in_invstd=None, in_scale=None, in_shift=None, rounding=True,
                      acc=None):
    """mvf_conv1x1_bwd_fused.  z3 = rnd(conv1x1(a, w)); dz3 = rnd(gamma invstd (gm - dbeta / M - (z3 - mean) invstd dgamma / M)); dW = dz3^T a;
    dx = rnd(dz3 W); with z_in: v1 / v2 = the gated sums of bn_in over dx.  Returns a dict; the allowances of the undecided roundings:
    allow_dx [M][K] = sum_c u_dz |W[c][k]| with u_dz [M][C] = und_dz ulp(dz3) + und_z ulp(z3) |d dz3 / d z3| (a weight-gradient allowance over rows r is
    u_dz[r]^T |a[r]|)."""
    a, w, g = f64(a), f64(w), f64(g)
    m = a.shape[0]
    acc = conv1x1(a, w) if acc is None else f64(acc)
    fb = E.fwd_bnbwd(_x4(a), _w4(w), ST, g, bits, mean, invstd, gamma=gamma, dgamma=dgamma, dbeta=dbeta, round_z3=rounding, acc=acc)
    z3, dz_exact = fb["z3"], fb["dz_exact"]
    bn = B.bn_bwd(g, z3, bits, 4, f64(gamma), f64(mean), f64(invstd), dgamma=dgamma, dbeta=dbeta)
    assert np.allclose(bn["dz"], dz_exact, rtol=1e-12, atol=1e-300)          # the two references this is composed from agree
    dz = rnd(dz_exact, rounding)
    out = dict(acc=acc, z3=z3, gm=fb["gm"], dz_exact=dz_exact, dz=dz, A_dz=bn["A_dz"])
    if rounding:
        und_z = undecided_z(acc, z3)
        moved = np.abs(f64(gamma) * f64(invstd) * f64(invstd) * f64(dgamma) / m)[None, :] * E.ulp(z3, ST)
        und_dz = midpoint_gap(dz_exact, dz) < 8.0 * 2.0 ** -24 * bn["A_dz"] + np.where(und_z, moved, 0.0)
        # one ulp of each undecided element through its effect: the rounding of dz3 itself, and -- an undecided z3 -- ulp(z3) |d dz3 / d z3|, which is MORE than
        # an ulp of a small dz3 (a gated-off element's dz3 of ~ 0.01 moves by tens of its ulps when z3 = 4 rounds the other way)
        u_dz = np.where(und_dz, E.ulp(dz, ST), 0.0) + np.where(und_z, moved, 0.0)
    else:
        und_z = und_dz = np.zeros(z3.shape, dtype=bool)
        u_dz = np.zeros(z3.shape)
    out.update(und_z=und_z, und_dz=und_dz, u_dz=u_dz, allow_dx=u_dz @ np.abs(w))
    dx_exact = dz @ w
    if rounding and z_in is not None:
        y, _ = E.dgrad_bnsums(_x4(dz), f64(w.T)[:, None, None, :], ST, f64(z_in), in_mean, in_invstd, in_scale, in_shift, acc=dx_exact)
    else:
        y = rnd(dx_exact, rounding)
    out.update(dx_exact=dx_exact, dx=y)
    if z_in is not None:
        out["v1"], out["v2"] = gated_sums(y, z_in, in_mean, in_invstd, in_scale, in_shift)
    return out


def wgrad(dz, x, rows=None):
    """(dW, absref) [C][K] of a pointwise conv over the rows [begin, end) (None: all): wgrad_ref.wgrad on the (1, rows, 1, .) tensors."""
    dz, x = f64(dz), f64(x)
    if rows is not None:
        dz, x = dz[rows[0]:rows[1]], x[rows[0]:rows[1]]
    n = dz.shape[0]
    dw, ab = W.wgrad(dz[None, :, None, :], x, 1, n, 1, x.shape[1], 1, 1, 1, 0)
    return dw[:, :, 0, 0], ab[:, :, 0, 0]


# ---------------------------------------------------------------------------------------------------------------- BatchNorm backward apply + weight gradient
def bn_bwd_apply_wgrad(g, z, operand, mode, gamma, mean, invstd, scale, shift, dgamma, dbeta, rounding=True):
    """mvf_bn_bwd_apply_wgrad's dz (mask mode 2: gate scale z + shift > 0; 4: sign bits): bn_pool_ref.bn_bwd fed the given dgamma / dbeta.  Returns its dict
    with dz_exact, dz (rounded once) and A_dz.  The weight gradient is wgrad() of the STORED dz."""
    r = B.bn_bwd(f64(g), f64(z), operand, mode, f64(gamma), f64(mean), f64(invstd), None if scale is None else f64(scale), None if shift is None else f64(shift),
                 dgamma, dbeta)
    r["dz_exact"] = r["dz"]
    r["dz"] = rnd(r["dz_exact"], rounding)
    return r


def bn_bwd_pair_wgrad(g, z_a, z_b, bits, gamma_a, mean_a, invstd_a, gamma_b, mean_b, invstd_b, sums_a=None, sums_b=None, rounding=True):
    """mvf_bn_bwd_pair_wgrad: both BatchNorms of relu(bn_a(z_a) + bn_b(z_b)) under the same sign bits (bn_pool_ref.bn_bwd_pair); sums_* = (dgamma, dbeta) the
    apply pass is fed (a kernel's own), None: the reference's."""
    ra, rb = B.bn_bwd_pair(f64(g), f64(z_a), f64(z_b), bits, f64(gamma_a), f64(mean_a), f64(invstd_a), f64(gamma_b), f64(mean_b), f64(invstd_b), sums_a, sums_b)
    for r in (ra, rb):
        r["dz_exact"] = r["dz"]
        r["dz"] = rnd(r["dz_exact"], rounding)
    return ra, rb
