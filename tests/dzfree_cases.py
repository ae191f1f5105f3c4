"""The inputs of tests/test_dzfree_kernels_gpu.py (numpy only, seeded, built once per case and never modified), shared with tests/test_dzfree_ref_cpu.py,
which checks on the CPU every condition the GPU module relies on (the exactness of the lattice inputs, the conditioning of the offset family, the layout of
the partial rows).  Every operand of the four glue kernels of csrc/bn_dzfree.hip is made HERE, in fp64 from one (gm, a2, W) triple with few rows, and rounded
once to the type the kernel reads it in -- A2, a_mean, Q, the partial column sums, dgamma and dbeta included -- so that no producer kernel stands between a
test and the kernel it judges; the fp64 reference (tests/dzfree_ref.py) is evaluated on exactly these rounded values."""
import numpy as np

import dzfree_ref as R

EPS, MOMENTUM = 1e-5, 0.1
# (c, k) of mvf_bn_bwd_dzfree_prep (c % 256, c <= 4096, k % 32).  (256, 32): one G workgroup, one 64-channel trip per wave (the prefetch's `more` is false at
# once); (512, 64): four G blocks, two off the diagonal, two trips; (768, 96): three trips (the prefetch's steady state), 9 blocks; (1280, 160): five trips, 25
# blocks; (4096, 32): the upper bound, exactly 64 KiB of dynamic LDS, eight strides of the bias loop; (1024, 256): layer3.
PREP_SHAPES = ((256, 32), (512, 64), (768, 96), (1280, 160), (4096, 32), (1024, 256))
PREP_ROWS = {(256, 32): (1, 37), (512, 64): (37, 300)}                 # m per shape (default: 37)
# (c, k) of mvf_bn_bwd_dzfree_wgrad (c % 32, k % 64).  (32, 64): two blocks in one workgroup, two idle waves, one trip; (96, 64): 6 blocks, a ragged last
# workgroup; (64, 192): three trips.
WGRAD_SHAPES = ((32, 64), (96, 64), (64, 192), (160, 128), (256, 64))
WGRAD_ROWS = {(32, 64): (1, 37), (96, 64): (37, 300)}
# mvf_bn_bwd_dzfree_sums (k % 4, any c): one active lane (k = 4), a ragged first stride (12, 260), a third stride (516); c = 1, 5, 6, 130: ragged workgroups
SUMS_C = (1, 5, 6, 64, 130)
SUMS_K = (4, 12, 256, 260, 516)
SUMS_ROWS = ((1, 65), (63, 64), (130, 1), (64, 63))                      # (rows_lo, rows_hi): one row, both sides of the 64-lane stride, a third stride
SUMS_M = 300
# (c, k) of mvf_bn_train_stats_gram (c % 32, k % 32): (96, 32) a ragged workgroup (three waves), (160, 96) / (128, 160) several column blocks
GRAM_SHAPES = ((32, 32), (96, 32), (160, 96), (128, 160), (512, 64))
GRAM_F64_MAX_ROWS = 16                                                     # up to here the library takes the fp64 one-wave-per-channel kernel (few rows: see bn_dzfree.hip)
GRAM_ROWS = (1, 2, 16, 17, 37, 1568)                                       # ... so 16 | 17 are the two sides of that switch
GRAM_FAMILIES = ("plain", "zero_row", "offset3")
LATTICE_M = 64                                                             # 1 / m is a power of two

# Bounds of the reduced quantities (rel_l2 against the fp64 reference): 4 x the largest figure measured on an MI355X (profiles/dzfree_errors.txt, made by
# tools/dzfree_errors_table.py), kept within [4 * 2^-24, the bound tests/test_dzfree_gpu.py uses for the quantity] (CAPS).  A quantity without an entry is
# held to its cap.
FLOOR = 4 * 2.0 ** -24
CAPS = {"G_block": 6e-3, "bias": 6e-3, "dw": 6e-3, "dgamma": 2e-4, "dbeta": 1e-5, "gram_mean": 2e-5, "gram_invstd": 2e-5, "gram_scale": 2e-5, "gram_shift": 2e-5,
        "gram_running_mean": 2e-5, "gram_running_var": 2e-5}
BOUNDS = {
    "G_block": 6.00e-03,                # measured 2.56e-3 (one bf16 rounding of each scaled operand and one of the output): 4 x is above the cap
    "bias": 4.56e-07,
    "dw": 6.57e-06,
    "dbeta": 2.38e-07,
    "dgamma": 1.07e-06,
    "gram_mean": 3.62e-07,
    "gram_invstd": 4.39e-06,
    "gram_scale": 4.98e-06,
    "gram_shift": 9.44e-06,
    "gram_running_mean": 3.62e-07,
    "gram_running_var": 7.94e-06,
}


def bound(q):
    return min(max(BOUNDS.get(q, CAPS[q]), FLOOR), CAPS[q])


_cache = {}


def f32(x):
    """Rounded to fp32, as float64."""
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def bf16_bits(x):
    """The bf16 bit patterns (uint16) of values that are bf16 numbers already."""
    return (np.ascontiguousarray(x, dtype=np.float32).view(np.uint32) >> 16).astype(np.uint16)


def triple(m, c, k, family="plain", seed=0):
    """One (gm, a2, W) triple in bf16 and everything the glue kernels are handed for it, each rounded ONCE from fp64 to fp32.
    plain: a2 = relu(N(0, 1)); offset3: a2 = relu(N(0, 1)) + 3 (|mean| / std of a2 about 5: the uncentred forms cancel); zero_row: row c / 2 + 1 of W is zero."""
    key = ("triple", m, c, k, family, seed)
    if key in _cache:
        return _cache[key]
    rng = np.random.default_rng(100003 * c + 101 * k + m + 7919 * seed + GRAM_FAMILIES.index(family))
    o = dict(m=m, c=c, k=k, family=family)
    w = R.round_bf16(rng.standard_normal((c, k)) * np.sqrt(2.0 / k))
    if family == "zero_row":
        o["zero_row"] = c // 2 + 1 if c > 1 else 0
        w[o["zero_row"]] = 0.0
    o["w"] = w
    o["wd"] = np.ascontiguousarray(w.T)                                       # the data-gradient pack of a pointwise conv: wd[k][c] = W[c][k]
    o["a2"] = R.round_bf16(np.maximum(rng.standard_normal((m, k)), 0.0) + (3.0 if family == "offset3" else 0.0))
    o["gm"] = R.round_bf16(rng.standard_normal((m, c)) * (rng.random((m, c)) < 0.5))
    z3 = o["a2"] @ w.T
    o["mean"] = f32(z3.mean(axis=0))
    o["invstd"] = f32(1.0 / np.sqrt(z3.var(axis=0) + EPS))
    o["gamma"] = f32((rng.random(c) + 0.5) * np.where(rng.random(c) < 0.25, -1.0, 1.0))
    o["beta"] = f32(rng.standard_normal(c) * 0.2)
    o["dbeta"] = f32(o["gm"].sum(axis=0))
    o["dgamma"] = f32((o["gm"] * (z3 - o["mean"]) * o["invstd"]).sum(axis=0))
    o["gram"] = f32(o["a2"].T @ o["a2"])
    o["a_mean"] = f32(o["a2"].mean(axis=0))
    o["q"] = f32(o["gm"].T @ o["a2"])
    o["running_mean"], o["running_var"] = f32(rng.standard_normal(c) * 0.1), f32(rng.random(c) + 0.5)
    # what the composed checks compare with: dz3 from the very fp32 coefficients the kernels read, z3 unrounded
    o["dz3"] = R.dz3(o["gm"], z3, o["gamma"], o["mean"], o["invstd"], o["dgamma"], o["dbeta"], m)
    _cache[key] = o
    return o


def frozen(o):
    """The same case under frozen statistics: the engine passes dgamma = dbeta = 0."""
    z = dict(o)
    z["dgamma"], z["dbeta"] = np.zeros(o["c"]), np.zeros(o["c"])
    z["dz3"] = R.dz3(o["gm"], o["a2"] @ o["w"].T, o["gamma"], o["mean"], o["invstd"], z["dgamma"], z["dbeta"], o["m"])
    return z


def scaling_restatement(o):
    """bd[k][c'] as the kernel states it, in numpy float32: bf16_rne(fl32(fl32(gamma invstd) * wd)) -- the bits."""
    a = np.float32(o["gamma"]) * np.float32(o["invstd"])
    return bf16_bits(R.round_bf16((np.float32(o["wd"]) * a[None, :]).astype(np.float32)))


def partial_rows(gm, c, c_split, rows_lo, rows_hi, seed, f32=f32):
    """The producers' partial column sums of gm, cut at arbitrary row boundaries (sorted random cut points; rows_x chunks each): part_lo [c_split][rows_lo][2]
    with exactly c_split channels, part_hi [c][rows_hi][2] indexed by the absolute channel with the channels below c_split NaN; element [..][1] NaN everywhere
    (the kernel must not read it).  None for an empty range.  f32: the rounding of a stored partial sum (the CPU proof of the reference turns it off)."""
    rng = np.random.default_rng(seed)
    m = gm.shape[0]

    def chunks(rows):
        cuts = np.concatenate([[0], np.sort(rng.choice(np.arange(1, m), rows - 1, replace=False)), [m]]).astype(int)
        return np.stack([gm[cuts[i]:cuts[i + 1]].sum(axis=0) for i in range(rows)], axis=1)         # [c][rows]

    lo = hi = None
    if c_split > 0:
        lo = np.full((c_split, rows_lo, 2), np.nan)
        lo[:, :, 0] = f32(chunks(rows_lo)[:c_split])
    if c_split < c:
        hi = np.full((c, rows_hi, 2), np.nan)
        hi[c_split:, :, 0] = f32(chunks(rows_hi)[c_split:])
    return lo, hi


def splits(c):
    """c_split values per channel count: none, all, and splits that are no multiple of 4 (both ranges inside one 4-channel workgroup)."""
    return (0, c) + {64: (6,), 5: (3,), 130: (67,), 6: (1,)}.get(c, ())


# ---------------------------------------------------------------------------------------------------------------- lattice families
def _pow2(rng, lo, hi, n, signed=True):
    v = 2.0 ** rng.integers(lo, hi + 1, n)
    return v * np.where(rng.random(n) < 0.5, -1.0, 1.0) if signed else v


def _wlat(rng, c, k, values=(0.0, 0.5, -0.5, 1.0, -1.0, 2.0, -2.0)):
    return rng.choice(np.asarray(values), (c, k))


def _lattice_bn(rng, c, m):
    """Per-channel signed powers of two: gamma, mean, dgamma / m, dbeta / m; invstd a positive one."""
    return dict(gamma=_pow2(rng, -1, 1, c), invstd=_pow2(rng, -1, 1, c, signed=False), mean=_pow2(rng, -2, 2, c), dgamma=m * _pow2(rng, -2, 1, c),
                dbeta=m * _pow2(rng, -2, 1, c))


def lattice_prep(c=768, k=96):
    """Dyadic operands of mvf_bn_bwd_dzfree_prep: every product and every partial sum of G, the scaling part and the bias is an fp32 number in any order."""
    key = ("lat_prep", c, k)
    if key not in _cache:
        rng = np.random.default_rng(4242)
        o = dict(c=c, k=k, m=LATTICE_M, w=_wlat(rng, c, k), **_lattice_bn(rng, c, LATTICE_M))
        o["wd"] = np.ascontiguousarray(o["w"].T)
        _cache[key] = o
    return _cache[key]


def lattice_wgrad(c=64, k=192):
    """... of mvf_bn_bwd_dzfree_wgrad: A2 symmetric integers of up to 11 bits (beyond the 8 of its bf16 `hi` term: the `lo` term carries the rest)."""
    key = ("lat_wgrad", c, k)
    if key not in _cache:
        rng = np.random.default_rng(4243)
        o = dict(c=c, k=k, m=LATTICE_M, w=_wlat(rng, c, k), **_lattice_bn(rng, c, LATTICE_M))
        t = rng.integers(-511, 512, (k, k)).astype(np.float64)
        o["gram"] = t + t.T
        o["a_mean"] = rng.integers(-4, 5, k).astype(np.float64)
        o["q"] = rng.integers(-64, 65, (c, k)).astype(np.float64)
        _cache[key] = o
    return _cache[key]


def lattice_sums(c=130, k=516, c_split=67, rows_lo=63, rows_hi=64):
    key = ("lat_sums", c, k, c_split, rows_lo, rows_hi)
    if key not in _cache:
        rng = np.random.default_rng(4244)
        o = dict(c=c, k=k, c_split=c_split, rows_lo=rows_lo, rows_hi=rows_hi, w=_wlat(rng, c, k), mean=_pow2(rng, -2, 2, c), invstd=_pow2(rng, -1, 1, c, signed=False))
        o["q"] = rng.integers(-32, 33, (c, k)).astype(np.float64)
        o["part_lo"] = np.full((c_split, rows_lo, 2), np.nan)
        o["part_lo"][:, :, 0] = rng.integers(-16, 17, (c_split, rows_lo))
        o["part_hi"] = np.full((c, rows_hi, 2), np.nan)
        o["part_hi"][c_split:, :, 0] = rng.integers(-16, 17, (c - c_split, rows_hi))
        _cache[key] = o
    return _cache[key]


LATTICE_GRAM_ROWS, LATTICE_GRAM_MOMENTUM = (2, 32), 0.5            # 2: the few-rows fp64 kernel (m / (m - 1) = 2, everything exact); 32: the matrix-core kernel


def lattice_running_var(o, var):
    """running_var of a lattice case from the exact variance, as fp32 states it: fl(fl(var fl(m / (m - 1))) / 2 + running_var / 2) -- the halves are exact, so
    fused or not the sum is rounded once; at m = 2 nothing is rounded at all."""
    ub = np.float32(o["m"] / (o["m"] - 1.0)).astype(np.float64)
    t = np.asarray(var * ub, dtype=np.float32).astype(np.float64)
    return f32(o["momentum"] * t + (1.0 - o["momentum"]) * o["running_var"])


def lattice_gram(m=2, c=96, k=32):
    """... of mvf_bn_train_stats_gram: m = 2 or 32 (1 / m a power of two), momentum 1/2; A2 / m - abar abar^T has six diagonal entries of 20 significant bits (they need the `mid` AND the
    `lo` term of the three-term split), the other diagonal entries 10 bits (the `mid` term); it is strictly diagonally dominant, so every variance is positive."""
    key = ("lat_gram", m, c, k)
    if key not in _cache:
        rng = np.random.default_rng(4245)
        o = dict(c=c, k=k, m=m, momentum=LATTICE_GRAM_MOMENTUM, w=_wlat(rng, c, k, (0.0, 0.0, 0.0, 0.5, -0.5, 1.0, -1.0)))
        o["w"][:, :6] = rng.choice(np.asarray((0.0, 0.5, -0.5)), (c, 6))               # the columns that meet the 20-bit entries: the sums stay below 2^24 units
        o["zero_row"] = c // 2 + 1
        o["w"][o["zero_row"]] = 0.0
        am = rng.integers(-3, 4, k).astype(np.float64)
        t = rng.integers(-4, 5, (k, k)).astype(np.float64)
        gc = (t + t.T) / 2.0
        diag = 513.0 + 2 * rng.integers(0, 256, k)                                 # odd, 10 bits
        diag[:6] = 2.0 ** 19 + 2 * rng.integers(0, 2 ** 18, 6) + 1                  # odd, 20 bits
        gc[np.arange(k), np.arange(k)] = diag
        o["a_mean"] = am
        o["gram"] = (gc + np.outer(am, am)) * m
        o["gamma"], o["beta"] = _pow2(rng, -1, 1, c), rng.integers(-4, 5, c) / 4.0
        o["running_mean"], o["running_var"] = rng.integers(-8, 9, c).astype(np.float64), rng.integers(1, 9, c).astype(np.float64)
        _cache[key] = o
    return _cache[key]
