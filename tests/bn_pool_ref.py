"""fp64 reference (numpy only) of the training-mode BatchNorm and stem max-pool operations of csrc/train_ops.hip, written from the semantics of the model
they implement -- torch BatchNorm2d in training mode (biased variance to normalise, unbiased into running_var), Bottleneck.forward's
relu(bn3(z3) + identity | bn_d(z_d)), MVF's hard-swish u * relu6(u + 3) / 6, the stem's maxpool3x3/2(relu(bn(z))) -- and from calculus, not from the kernels.
Proved against torch in float64 by tests/test_bn_pool_ref_cpu.py; tests/test_bn_pool_kernels_gpu.py compares every kernel variant with it.

Matrices are [M][C] (channels last), pool tensors [n][h][w][c].  Besides each result the functions return what a test needs to BOUND an fp32 evaluation of
the same expression: `A`, the sum of the absolute values of the expression's terms (an fp32 evaluation in any order errs by a small multiple of 2^-24 A), and
`undecided`, the elements whose pre-activation lies so close to a kink of the activation that fp32 may land on the other side."""
import numpy as np

UNDECIDED_REL = 2.0 ** -20


# ---------------------------------------------------------------------------------------------------------------- storage types
def round_bf16(x):
    """Round-to-nearest-even to bfloat16, returned as float64 (finite values)."""
    f = np.ascontiguousarray(x, dtype=np.float32)
    u = f.view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).astype(np.float64).reshape(np.shape(x))


def round_storage(x, dtype):
    """x rounded to the storage type ("f32" | "bf16") as float64."""
    return round_bf16(x) if dtype == "bf16" else np.asarray(x, dtype=np.float32).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------------- activations
def hswish(u):
    return u * np.clip(u + 3.0, 0.0, 6.0) / 6.0


def hswish_grad(u):
    """d/du [u relu6(u + 3) / 6]; relu6' = 0 at the kinks (autograd of hardtanh uses strict inequalities)."""
    return np.clip(u + 3.0, 0.0, 6.0) / 6.0 + np.where((u > -3.0) & (u < 3.0), u / 6.0, 0.0)


def act_fwd(u, act):
    return u if act == 0 else (np.maximum(u, 0.0) if act == 1 else hswish(u))


def undecided(u, mag, thresholds):
    """|u - t| <= 2^-20 max(1, mag) for a threshold t: an fp32 evaluation of u may fall on the other side of t."""
    w = UNDECIDED_REL * np.maximum(1.0, mag)
    und = np.zeros(u.shape, dtype=bool)
    for t in thresholds:
        und |= np.abs(u - t) <= w
    return und


def pack_bits(positive):
    """[M][C] booleans -> [M][C/4] bytes, bit j of byte k <=> element 4k + j."""
    m, c = positive.shape
    p = positive.reshape(m, c // 4, 4).astype(np.uint8)
    return p[..., 0] | (p[..., 1] << 1) | (p[..., 2] << 2) | (p[..., 3] << 3)


def unpack_bits(bits, c):
    m = bits.shape[0]
    b = np.asarray(bits, dtype=np.uint8).reshape(m, c // 4, 1)
    return ((b >> np.arange(4, dtype=np.uint8)) & 1).reshape(m, c).astype(bool)


# ---------------------------------------------------------------------------------------------------------------- forward statistics
def _stats_from_moments(mean, var, m, gamma, beta, eps, momentum, running_mean, running_var):
    invstd = 1.0 / np.sqrt(var + eps)
    scale = gamma * invstd
    shift = beta - mean * scale
    out = dict(mean=mean, var=var, invstd=invstd, scale=scale, shift=shift, running_mean=None, running_var=None)
    if running_mean is not None:
        out["running_mean"] = (1.0 - momentum) * running_mean + momentum * mean
    if running_var is not None:
        out["running_var"] = (1.0 - momentum) * running_var + momentum * var * m / max(m - 1, 1)      # unbiased; one row keeps the divisor 1
    return out


def bn_stats(z, gamma, beta, eps, momentum, running_mean=None, running_var=None):
    """Batch statistics of z [M][C]: mean, biased var, invstd = 1 / sqrt(var + eps), scale = gamma invstd, shift = beta - mean scale, new running statistics."""
    z = np.asarray(z, dtype=np.float64)
    m = z.shape[0]
    mean = z.mean(axis=0)
    var = ((z - mean) ** 2).mean(axis=0)                          # two-pass: no cancellation
    return _stats_from_moments(mean, var, m, gamma, beta, eps, momentum, running_mean, running_var)


def finalize(part, layout):
    """Per-channel sums of the partial pairs: layout "cm" = channel-major [C][rows][2], "rm" = row-major [rows][C][2].  Returns (s1 [C], s2 [C])."""
    part = np.asarray(part, dtype=np.float64)
    s = part.sum(axis=1 if layout == "cm" else 0)
    return s[:, 0], s[:, 1]


def bn_stats_from_sums(s1, s2, m, k, gamma, beta, eps, momentum, running_mean=None, running_var=None):
    """The same outputs from shifted sums s1 = sum(z - k), s2 = sum((z - k)^2) (k = 0: plain sums)."""
    d = s1 / m
    var = np.maximum(s2 / m - d * d, 0.0)
    return _stats_from_moments(k + d, var, m, gamma, beta, eps, momentum, running_mean, running_var)


def conditioning(z, k):
    """1 + (mean - k)^2 / var per channel: the factor by which sum((z - k)^2) / M - (mean - k)^2 amplifies the relative error of its two terms."""
    z = np.asarray(z, dtype=np.float64)
    mean = z.mean(axis=0)
    var = ((z - mean) ** 2).mean(axis=0)
    return 1.0 + (mean - k) ** 2 / np.maximum(var, 1e-300)


# ---------------------------------------------------------------------------------------------------------------- apply
def bn_apply(z, scale, shift, r=None, rscale=None, rshift=None, act=0):
    """out = act(z scale + shift [+ r | + r rscale + rshift]), act 0 none / 1 ReLU / 2 hard-swish.  Returns a dict: out, bits (sign bits of out), colmeans,
    u (the pre-activation), A (for out), undecided (sign of out: u near 0)."""
    z = np.asarray(z, dtype=np.float64)
    u = z * scale + shift
    a_u = np.abs(z * scale) + np.abs(shift)
    if r is not None:
        r = np.asarray(r, dtype=np.float64)
        if rscale is not None:
            u = u + (r * rscale + rshift)
            a_u = a_u + np.abs(r * rscale) + np.abs(rshift)
        else:
            u = u + r
            a_u = a_u + np.abs(r)
    out = act_fwd(u, act)
    # hard-swish: |d out / d u| <= 1.5, and the products u * relu6(u + 3) * (1 / 6) round on their own
    a_out = a_u if act != 2 else 1.5 * a_u + np.abs(out)
    return dict(out=out, bits=pack_bits(out > 0), colmeans=out.mean(axis=0), u=u, A=a_out, A_u=a_u, undecided=undecided(u, a_u, (0.0,)))


# ---------------------------------------------------------------------------------------------------------------- backward
def bn_mask(g, z, mask_operand, mode, scale=None, shift=None):
    """gm = g act'(.) for the five mask modes: 0 none, 1 [mask_operand > 0] (the forward output), 2 [scale z + shift > 0], 3 hard-swish'(scale z + shift),
    4 sign bits ([M][C/4] bytes).  Returns (gm, A of gm, undecided)."""
    g = np.asarray(g, dtype=np.float64)
    z = np.asarray(z, dtype=np.float64)
    none = np.zeros(g.shape, dtype=bool)
    if mode == 0:
        return g, np.abs(g), none
    if mode == 1:
        return np.where(np.asarray(mask_operand, dtype=np.float64) > 0, g, 0.0), np.abs(g), none
    if mode == 4:
        return np.where(unpack_bits(mask_operand, g.shape[1]), g, 0.0), np.abs(g), none
    u = z * scale + shift
    a_u = np.abs(z * scale) + np.abs(shift)
    if mode == 2:
        return np.where(u > 0, g, 0.0), np.abs(g), undecided(u, a_u, (0.0,))
    assert mode == 3
    d = hswish_grad(u)
    # |d hswish' / d u| = 1/3 inside the kinks
    return g * d, np.abs(g) * (np.abs(d) + a_u / 3.0), undecided(u, a_u, (-3.0, 3.0))


def bn_bwd(g, z, mask_operand, mode, gamma, mean, invstd, scale=None, shift=None, dgamma=None, dbeta=None):
    """Backward of y = gamma (z - mean) invstd + beta under batch statistics, for the upstream gradient gm = g act'(.):
    dbeta = sum gm, dgamma = sum gm xhat, dz = gamma invstd (gm - dbeta / M - xhat dgamma / M).  dgamma / dbeta given: dz is formed from THOSE (a kernel's own
    sums), so that an apply pass is judged on its own.  Returns a dict: gm, dgamma, dbeta, dz, A_gm, A_dz, undecided, and abs_dbeta / abs_dgamma = the sums of
    |gm| and |gm xhat| (what an fp32 summation error is proportional to)."""
    z = np.asarray(z, dtype=np.float64)
    m = z.shape[0]
    gm, a_gm, und = bn_mask(g, z, mask_operand, mode, scale, shift)
    xhat = (z - mean) * invstd
    db, dg = gm.sum(axis=0), (gm * xhat).sum(axis=0)
    use_dg = dg if dgamma is None else np.asarray(dgamma, dtype=np.float64)
    use_db = db if dbeta is None else np.asarray(dbeta, dtype=np.float64)
    dz = gamma * invstd * (gm - use_db / m - xhat * use_dg / m)
    a_xhat = (np.abs(z) + np.abs(mean)) * np.abs(invstd)
    a_dz = np.abs(gamma * invstd) * (a_gm + np.abs(use_db) / m + a_xhat * np.abs(use_dg) / m)
    return dict(gm=gm, dgamma=dg, dbeta=db, dz=dz, A_gm=a_gm, A_dz=a_dz, undecided=und, abs_dbeta=np.abs(gm).sum(axis=0), abs_dgamma=(np.abs(gm) * a_xhat).sum(axis=0),
                xhat=xhat)


def bn_bwd_pair(g, z_a, z_b, bits, gamma_a, mean_a, invstd_a, gamma_b, mean_b, invstd_b, sums_a=None, sums_b=None):
    """out = relu(bn_a(z_a) + bn_b(z_b)): both BatchNorms receive g gated by the sign bits of out."""
    a = bn_bwd(g, z_a, bits, 4, gamma_a, mean_a, invstd_a, **(dict(dgamma=sums_a[0], dbeta=sums_a[1]) if sums_a else {}))
    b = bn_bwd(g, z_b, bits, 4, gamma_b, mean_b, invstd_b, **(dict(dgamma=sums_b[0], dbeta=sums_b[1]) if sums_b else {}))
    return a, b


# ---------------------------------------------------------------------------------------------------------------- stem: maxpool3x3/2 pad 1 over relu(bn(z))
def pool_out(h):
    return (h - 1) // 2 + 1


def maxpool_bn_relu_fwd(z, scale, shift):
    """y = maxpool3x3, stride 2, pad 1 of relu(z scale + shift), z [n][h][w][c]; argmax byte = window position dy * 3 + dx of the FIRST maximum in scan order (rows,
    then columns; taps outside the image are skipped).  Returns a dict: y, argmax (uint8), a (the activation), u, A (of y: its winner's), undecided (of the
    ReLU gate, per INPUT element)."""
    z = np.asarray(z, dtype=np.float64)
    n, h, w, c = z.shape
    ho, wo = pool_out(h), pool_out(w)
    u = z * scale + shift
    a_u = np.abs(z * scale) + np.abs(shift)
    a = np.maximum(u, 0.0)
    hp, wp = 2 * ho + 1, 2 * wo + 1
    pad = np.full((n, hp, wp, c), -np.inf)
    pad[:, 1:h + 1, 1:w + 1] = a
    pad_a = np.zeros((n, hp, wp, c))
    pad_a[:, 1:h + 1, 1:w + 1] = a_u
    y = np.full((n, ho, wo, c), -np.inf)
    am = np.zeros((n, ho, wo, c), dtype=np.uint8)
    ay = np.zeros((n, ho, wo, c))
    for k in range(9):
        dy, dx = divmod(k, 3)
        v = pad[:, dy:dy + 2 * ho:2, dx:dx + 2 * wo:2]
        better = v > y                                             # strict: the first maximum stays
        y = np.where(better, v, y)
        am = np.where(better, np.uint8(k), am)
        ay = np.where(better, pad_a[:, dy:dy + 2 * ho:2, dx:dx + 2 * wo:2], ay)
    return dict(y=y, argmax=am, a=a, u=u, A=ay, A_u=a_u, undecided=undecided(u, a_u, (0.0,)))


def maxpool_gather(argmax, g, h, w):
    """ga [n][h][w][c] = sum over the windows whose argmax is this pixel of g[window] (the pool's backward).  Returns (ga, sum of |g| likewise)."""
    g = np.asarray(g, dtype=np.float64)
    n, ho, wo, c = g.shape
    hp, wp = max(2 * ho + 1, h + 2), max(2 * wo + 1, w + 2)
    ga, aa = np.zeros((n, hp, wp, c)), np.zeros((n, hp, wp, c))
    for k in range(9):
        dy, dx = divmod(k, 3)
        sel = argmax == k
        ga[:, dy:dy + 2 * ho:2, dx:dx + 2 * wo:2] += np.where(sel, g, 0.0)
        aa[:, dy:dy + 2 * ho:2, dx:dx + 2 * wo:2] += np.where(sel, np.abs(g), 0.0)
    assert not ga[:, 0].any() and not ga[:, :, 0].any() and not ga[:, h + 1:].any() and not ga[:, :, w + 1:].any(), "an argmax byte points outside the image"
    return ga[:, 1:h + 1, 1:w + 1].copy(), aa[:, 1:h + 1, 1:w + 1].copy()


def maxpool_bn_relu_bwd(argmax, g, h, w, z=None, gamma=None, mean=None, invstd=None, scale=None, shift=None, dgamma=None, dbeta=None, stored=None):
    """ga as maxpool_gather.  With z and the statistics also the backward of the BatchNorm under relu and pool: the result of bn_bwd (mask mode 2) on ga over
    the n h w rows.  stored: the rounding of the storage type (round_bf16), applied to ga before the gate -- the BatchNorm backward reads ga as it is STORED."""
    ga, a_ga = maxpool_gather(argmax, g, h, w)
    out = dict(ga=ga, A_ga=a_ga)
    if z is not None:
        c = ga.shape[-1]
        gs = stored(ga) if stored is not None else ga
        bn = bn_bwd(gs.reshape(-1, c), np.asarray(z, dtype=np.float64).reshape(-1, c), None, 2, gamma, mean, invstd, scale, shift, dgamma, dbeta)
        # gm is itself a sum of up to four g: its terms' absolute values (a_ga) stand in A where bn_bwd counted |ga| (they differ where the four cancel)
        extra = np.maximum(a_ga - np.abs(gs), 0.0).reshape(-1, c)
        bn["A_gm"] = bn["A_gm"] + extra
        bn["A_dz"] = bn["A_dz"] + np.abs(gamma * invstd) * extra
        out["bn"] = bn
    return out
