"""fp64 reference (numpy only) of the four glue kernels of csrc/bn_dzfree.hip, written from the definition of what each one stands for in the backward of
out = relu(bn3(conv3(a2)) + identity) (Bottleneck.forward under torch autograd, bn3 on batch statistics) -- not from the kernels' algebra:

    z3 = a2 W^T,  dz3 = a (gm - d0 - kx (z3 - mean)),  a = gamma invstd, d0 = dbeta / m, kx = invstd dgamma / m          (gm = g * [out > 0])

  prep       the affine map (gm, a2) -> da2 = dz3 W, PROBED with unit vectors: [gm | a2] bd^T + bias == da2
  wgrad_fix  dW = dz3^T a2 from what the kernel is given: Q = gm^T a2, A2 = a2^T a2, the column means of a2
  sums       dbeta = sum_m gm, dgamma = sum_m gm (z3 - mean) invstd, from Q and the producers' partial column sums
  gram_stats batch statistics of z3 from A2 and the column means, and what torch.nn.BatchNorm2d does with them

Proved against torch float64 autograd by tests/test_dzfree_ref_cpu.py; tests/test_dzfree_kernels_gpu.py compares every kernel with it.  Matrices are [M][C]
(channels last); W is [c][k] (c output channels of the pointwise conv3, k input channels).  Besides each result the functions return `A`, the sum of the
absolute values of the terms of the element's expression: an fp32 evaluation in any order errs by a small multiple of 2^-24 A."""
import numpy as np

from bn_pool_ref import round_bf16  # noqa: F401  (the storage rounding, shared)


def coefficients(gamma, mean, invstd, dgamma, dbeta, m):
    """a, d0, kx of the BatchNorm backward dz = a (gm - d0 - kx (z - mean))."""
    return gamma * invstd, dbeta / float(m), invstd * dgamma / float(m)


def dz3(gm, z3, gamma, mean, invstd, dgamma, dbeta, m):
    a, d0, kx = coefficients(gamma, mean, invstd, dgamma, dbeta, m)
    return a * (gm - d0 - kx * (z3 - mean))


def prep(wd, gamma, mean, invstd, dgamma, dbeta, m):
    """wd [k][c] = W^T (the data-gradient pack).  bd [k][c + k], bias [k] with [gm | a2] bd^T + bias = dz3(gm, a2 W^T) W for every (gm, a2): the constant is the
    map's value at zero, column i of the matrix its value at the i-th unit vector less that constant.
    A_scale [k][c] = |a_c W[c][k]|; A_G [k][k] = sum_c |e_c W[c][j] W[c][k]|, e = a kx; A_bias [k] = sum_c |t_c W[c][k]|, t = a (d0 - kx mean)."""
    w = np.asarray(wd, dtype=np.float64).T
    c, k = w.shape

    def dz(gm, a2):
        return dz3(gm, a2 @ w.T, gamma, mean, invstd, dgamma, dbeta, m)

    dz0 = dz(np.zeros((1, c)), np.zeros((1, k)))
    bias = (dz0 @ w)[0]
    bd = np.empty((k, c + k))
    bd[:, :c] = ((dz(np.eye(c), np.zeros((c, k))) - dz0) @ w).T         # (the difference is taken per channel, before the product: untouched channels cancel exactly)
    bd[:, c:] = ((dz(np.zeros((k, c)), np.eye(k)) - dz0) @ w).T
    a, d0, kx = coefficients(gamma, mean, invstd, dgamma, dbeta, m)
    aw = np.abs(w)
    return dict(bd=bd, bias=bias, A_scale=(np.abs(a)[:, None] * aw).T, A_G=aw.T @ (np.abs(a * kx)[:, None] * aw), A_bias=np.abs(a * (d0 - kx * mean)) @ aw)


def wgrad_fix(q, w, a2gram, a_mean, gamma, mean, invstd, dgamma, dbeta, m):
    """dW [c][k] = sum_m dz3[m][c] a2[m][k] with the sums over m taken from q = gm^T a2, a2gram = a2^T a2 and sa = m a_mean:
    sum_m z3[m][c] a2[m][k] = (W A2)[c][k].  wa2 [c][k] = sum_j |W[c][j] A2[j][k]| is returned for the bound of the kernel's two-term split of A2."""
    a, d0, kx = (v[:, None] for v in coefficients(gamma, mean, invstd, dgamma, dbeta, m))
    sa = float(m) * a_mean[None, :]
    mu = mean[:, None]
    dw = a * (q - d0 * sa - kx * (w @ a2gram - mu * sa))
    wa2 = np.abs(w) @ np.abs(a2gram)
    big_a = np.abs(a) * (np.abs(q) + np.abs(d0 * sa) + np.abs(kx) * (wa2 + np.abs(mu * sa)))
    return dict(dw=dw, A=big_a, wa2=wa2, split=np.abs(a * kx) * wa2)


def column_sums(part_lo, rows_lo, c_split, part_hi, rows_hi, c):
    """sum_m gm[m][ch] and its sum of absolute terms from the two runs of partial rows: part_lo [c_split][rows_lo][2] for channels < c_split, part_hi
    [c][rows_hi][2] indexed by the ABSOLUTE channel for the rest; element [..][0] only."""
    s, a = np.empty(c), np.empty(c)
    for ch in range(c):
        rows = part_lo[ch, :rows_lo, 0] if ch < c_split else part_hi[ch, :rows_hi, 0]
        s[ch], a[ch] = rows.sum(), np.abs(rows).sum()
    return s, a


def sums(q, w, mean, invstd, part_lo, rows_lo, c_split, part_hi, rows_hi):
    """dbeta[c] = sum_m gm[m][c]; dgamma[c] = sum_m gm[m][c] (z3[m][c] - mean_c) invstd_c with sum_m gm z3 = sum_k W[c][k] Q[c][k]."""
    c = w.shape[0]
    dbeta, a_db = column_sums(part_lo, rows_lo, c_split, part_hi, rows_hi, c)
    dgamma = invstd * ((w * q).sum(axis=1) - mean * dbeta)
    return dict(dgamma=dgamma, dbeta=dbeta, A_dbeta=a_db, A_dgamma=np.abs(invstd) * (np.abs(w * q).sum(axis=1) + np.abs(mean) * a_db))


def gram_stats(a2gram, a_mean, w, m, gamma, beta, eps, momentum, running_mean=None, running_var=None):
    """Batch statistics of z3 = a2 W^T: mean_c = W[c] . abar, var_c = W[c] (A2 / m - abar abar^T) W[c]^T (biased), invstd, scale = gamma invstd,
    shift = beta - mean scale, and the running statistics of torch.nn.BatchNorm2d after one step (unbiased variance; one row keeps the divisor 1).
    A_mean = sum_k |W[c][k] abar_k|; A_var = sum_jk |W_cj| (|A2_jk| / m + |abar_j abar_k|) |W_ck|."""
    mf = float(m)
    mean = w @ a_mean
    gc = a2gram / mf - np.outer(a_mean, a_mean)
    var = np.einsum("cj,jk,ck->c", w, gc, w)
    aw = np.abs(w)
    a_var = np.einsum("cj,jk,ck->c", aw, np.abs(a2gram) / mf + np.abs(np.outer(a_mean, a_mean)), aw)
    invstd = 1.0 / np.sqrt(np.maximum(var, 0.0) + eps)           # (a variance is not negative: only synthetic A2 / abar that belong to no a2 could make it so)
    scale = gamma * invstd
    out = dict(mean=mean, var=var, invstd=invstd, scale=scale, shift=beta - mean * scale, A_mean=aw @ np.abs(a_mean), A_var=a_var)
    unbias = mf / max(mf - 1.0, 1.0)
    if running_mean is not None:
        out["running_mean"] = (1.0 - momentum) * running_mean + momentum * mean
        out["A_running_mean"] = np.abs((1.0 - momentum) * running_mean) + momentum * out["A_mean"]
    if running_var is not None:
        out["running_var"] = (1.0 - momentum) * running_var + momentum * var * unbias
        out["A_running_var"] = np.abs((1.0 - momentum) * running_var) + momentum * unbias * a_var
    return out
