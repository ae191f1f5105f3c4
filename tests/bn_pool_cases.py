"""The inputs of tests/test_bn_pool_kernels_gpu.py (numpy only, seeded, built once per case and never modified), shared with tests/test_bn_pool_ref_cpu.py,
which checks on the CPU every condition the GPU module relies on: the share of undecided elements per case, the exactness of the lattice inputs, the
conditioning factors of the statistics cases.  Operands are rounded to the storage type here; the fp64 reference is evaluated on exactly these values."""
import numpy as np

import bn_pool_ref as R

EPS, MOMENTUM = 1e-5, 0.1
DTYPES = ("f32", "bf16")
# [M][C] matrices: (M, C, storage types).  C = 4: one channel group, 256 row lanes; 12: three groups on a 4-wide block (an idle lane column); 260: two blocks
# along the channels, the second ragged; 2048: four blocks at 16-byte bf16 lanes.  M = 1; 37 (one short row block); 53 (at C = 64 some row lanes make an ODD
# number of trips under both lane widths: 53 = 3 x 16 + 5 = 32 + 21 -> the unrolled loops end in their single-row tail); 300 (several row blocks at
# C = 64); 2049 at C = 4 (two row blocks of 256 lanes x 8 rows).
MATRICES = (
    (1, 4, DTYPES), (37, 4, DTYPES), (2049, 4, DTYPES),
    (37, 12, DTYPES), (300, 12, DTYPES),
    (1, 64, DTYPES), (37, 64, DTYPES), (53, 64, DTYPES), (300, 64, DTYPES),
    (37, 260, DTYPES), (300, 260, DTYPES),
    (37, 2048, ("bf16",)), (300, 2048, ("bf16",)),
)
POOL_SHAPES = ((2, 9, 12, 8), (1, 1, 1, 4), (2, 5, 4, 64), (2, 8, 12, 64), (1, 8, 8, 256), (3, 7, 16, 64), (2, 6, 6, 12))
FINALIZE_ROWS = (1, 3, 255, 1023, 1024, 1500)
FINALIZE_CHANNELS = (4, 6, 64)
UNDECIDED_SHARE = 1e-4

# seeds moved on until the case has no undecided element (M = 1: scale z + shift = beta + (z - mean) scale with scale ~ 316 |gamma|, a wide window around
# every kink; tests/test_bn_pool_ref_cpu.py checks the outcome)
SEED_BUMP = {(1, 64): 1}
_cache = {}


def f32(x):
    """Rounded to fp32, as float64: the per-channel parameters the kernels read."""
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def matrix_case(m, c, dtype):
    """Operands of the apply / backward legs for one [M][C] shape and storage type.  The statistics the kernels are GIVEN (mean, invstd, scale, shift) are the
    fp64 batch statistics of z rounded to fp32, and the reference uses those rounded values: each kernel is judged on its own."""
    key = ("matrix", m, c, dtype)
    if key in _cache:
        return _cache[key]
    rng = np.random.default_rng(1000 * c + m + (7 if dtype == "bf16" else 0) + 100000 * SEED_BUMP.get((m, c), 0))
    o = dict(m=m, c=c, dtype=dtype)
    o["z"] = R.round_storage(rng.standard_normal((m, c)) * 2 + rng.standard_normal(c) * 3, dtype)       # per-channel means of ~ 3 / 2 standard deviations
    o["zb"] = R.round_storage(rng.standard_normal((m, c)) + rng.standard_normal(c), dtype)              # the second BatchNorm of the pair
    o["r"] = R.round_storage(rng.standard_normal((m, c)) * 2, dtype)
    o["gwide"] = R.round_storage(rng.standard_normal((m, c + 8)), dtype)                                 # g = its first c columns; every column holds data
    for k in ("gamma", "gamma_b", "rscale"):
        o[k] = f32((rng.random(c) + 0.5) * np.where(rng.random(c) < 0.25, -1.0, 1.0))
    for k in ("beta", "beta_b", "rshift"):
        o[k] = f32(rng.standard_normal(c))
    o["running_mean"], o["running_var"] = f32(rng.standard_normal(c) * 0.1), f32(rng.random(c) + 0.5)
    for suf, zk, gk, bk in (("", "z", "gamma", "beta"), ("_b", "zb", "gamma_b", "beta_b")):
        st = R.bn_stats(o[zk], o[gk], o[bk], EPS, MOMENTUM)
        o["mean" + suf], o["invstd" + suf] = f32(st["mean"]), f32(st["invstd"])
        o["scale" + suf] = f32(o[gk] * o["invstd" + suf])
        o["shift" + suf] = f32(o[bk] - o["mean" + suf] * o["scale" + suf])
    _cache[key] = o
    return o


# the statistics leg: name -> (mean in standard deviations, K relative to the mean in standard deviations | None = K = 0 (running_mean NULL), bound scaled by
# the conditioning factor?)
STATS_KINDS = {
    "mean3_k": (3.0, "running", False),            # K = a running mean near 0 (as the existing test)
    "mean3_k0": (3.0, None, False),
    "mean30_knear": (30.0, "near", False),         # ill-conditioned data, K within one standard deviation of the mean: what the shifted sums exist for
    "mean30_k0": (30.0, None, True),               # the same data with K = 0: the bound scales by 1 + (mean - K)^2 / var
}


def stats_case(m, c, dtype, kind):
    key = ("stats", m, c, dtype, kind)
    if key in _cache:
        return _cache[key]
    nsig, kmode, scaled = STATS_KINDS[kind]
    rng = np.random.default_rng(77 * c + m + (3 if dtype == "bf16" else 0))
    sd = 2.0
    sign = np.where(rng.random(c) < 0.5, -1.0, 1.0)
    cmean = sign * nsig * sd * (0.75 + 0.5 * rng.random(c))
    o = dict(m=m, c=c, dtype=dtype, kind=kind)
    o["z"] = R.round_storage(rng.standard_normal((m, c)) * sd + cmean, dtype)
    o["gamma"], o["beta"] = f32(rng.random(c) + 0.5), f32(rng.standard_normal(c))
    o["running_var"] = f32(rng.random(c) + 0.5)
    if kmode is None:
        o["running_mean"] = None
    elif kmode == "near":
        o["running_mean"] = f32(cmean + sd * (rng.random(c) * 1.6 - 0.8))
    else:
        o["running_mean"] = f32(rng.standard_normal(c) * 0.1)
    k = 0.0 if o["running_mean"] is None else o["running_mean"]
    # (var + eps: what invstd is conditioned on)
    zz = o["z"]
    var = ((zz - zz.mean(axis=0)) ** 2).mean(axis=0)
    o["factor"] = float((1.0 + (zz.mean(axis=0) - k) ** 2 / (var + EPS)).max())
    o["scaled"] = scaled
    o["ref"] = R.bn_stats(zz, o["gamma"], o["beta"], EPS, MOMENTUM, o["running_mean"], o["running_var"])
    _cache[key] = o
    return o


def finalize_case(c, nblk):
    """Synthetic channel-major partials [C][nblk][2] of shifted sums with a per-channel offset: summed row-major they land in the wrong channel, visibly."""
    key = ("fin", c, nblk)
    if key in _cache:
        return _cache[key]
    rng = np.random.default_rng(31 * c + nblk)
    per = 7                                                                              # rows of the [M][C] matrix behind one partial row
    ch = np.arange(c, dtype=np.float64)
    part = np.empty((c, nblk, 2))
    part[:, :, 0] = rng.standard_normal((c, nblk)) * 2 + (ch[:, None] % 5 - 2) * 1.5     # sum (z - K) over 7 rows
    part[:, :, 1] = per * (1.0 + ch[:, None] % 7) + rng.random((c, nblk)) * 3 + 12       # sum (z - K)^2: var >= ~1 for every channel
    o = dict(c=c, nblk=nblk, m=per * nblk, part=f32(part))
    o["gamma"], o["beta"] = f32(rng.random(c) + 0.5), f32(rng.standard_normal(c))
    o["running_mean"], o["running_var"] = f32(rng.standard_normal(c)), f32(rng.random(c) + 0.5)
    s1, s2 = R.finalize(o["part"], "cm")
    o["s1"], o["s2"] = s1, s2
    o["ref"] = R.bn_stats_from_sums(s1, s2, o["m"], o["running_mean"], o["gamma"], o["beta"], EPS, MOMENTUM, o["running_mean"], o["running_var"])
    _cache[key] = o
    return o


def pool_case(shape, dtype, family):
    """Stem inputs z [n][h][w][c], g [n][ho][wo][c] and the per-channel BatchNorm parameters.
    lattice: z and g multiples of 1/4 in [-2, 2], scale +-2^k (k = -1, 0, 1; negative on some channels), shift a multiple of 1/8 in [-1, 1], mean a multiple of
    1/4, invstd = gamma = 1: every activation, gathered gradient and backward sum is exact in fp32 AND in bf16 whatever the order or fusion of the operations,
    ties (positive ones too) are plentiful, and channels with shift = -4 make windows of zeros only.
    random: batch statistics of Gaussian z (fp64, rounded to fp32)."""
    key = ("pool", shape, dtype, family)
    if key in _cache:
        return _cache[key]
    n, h, w, c = shape
    ho, wo = R.pool_out(h), R.pool_out(w)
    rng = np.random.default_rng(sum(shape) * 13 + (5 if dtype == "bf16" else 0) + (1 if family == "lattice" else 0))
    o = dict(shape=shape, dtype=dtype, family=family, ho=ho, wo=wo, m=n * h * w)
    if family == "lattice":
        o["z"] = rng.integers(-8, 9, (n, h, w, c)) / 4.0
        o["g"] = rng.integers(-8, 9, (n, ho, wo, c)) / 4.0
        o["scale"] = 2.0 ** rng.integers(-1, 2, c) * np.where(np.arange(c) % 3 == 1, -1.0, 1.0)
        o["shift"] = rng.integers(-8, 9, c) / 8.0
        o["shift"][c - 1] = -4.0                                                        # scale z + shift <= -2: every window of this channel is all zeros
        o["scale"][c - 1] = 1.0
        o["mean"] = rng.integers(-4, 5, c) / 4.0
        o["invstd"], o["gamma"] = np.ones(c), np.ones(c)
    else:
        o["z"] = R.round_storage(rng.standard_normal((n, h, w, c)) * 2 + rng.standard_normal(c), dtype)
        o["g"] = R.round_storage(rng.standard_normal((n, ho, wo, c)), dtype)
        o["gamma"] = f32((rng.random(c) + 0.5) * np.where(np.arange(c) % 5 == 2, -1.0, 1.0))
        beta = f32(rng.standard_normal(c) * 0.5)
        st = R.bn_stats(o["z"].reshape(-1, c), o["gamma"], beta, EPS, MOMENTUM)
        o["mean"], o["invstd"] = f32(st["mean"]), f32(st["invstd"])
        o["scale"] = f32(o["gamma"] * o["invstd"])
        o["shift"] = f32(beta - o["mean"] * o["scale"])
    _cache[key] = o
    return o
