"""Case tables, input construction, launch-plan ports and comparison functions of tests/test_pw_bwd_kernels_gpu.py (numpy only, seeded, built once per case and
never modified), shared with tests/test_pw_bwd_ref_cpu.py, which checks on the CPU every condition the GPU module relies on: the gate margins, the 1 %
allowance conditions, the plan ports against hand-computed splits, and that the comparison functions reject the ways these kernels can go wrong.

Inputs keep the reductions well conditioned: mean = the batch mean of the reference's rounded conv output (or of the stored BatchNorm input) + 0.05 randn,
invstd = 1 / sqrt(var + 1e-5) of the same tensor, g = round_bf16(randn + 0.25 xhat + 0.1) -- so dgamma is a sum of mostly positive terms, not noise --, sign
bits random in the low nibble of each byte, gamma in [0.5, 1.5); dgamma / dbeta handed to an apply pass are the fp64 sums of the same case cast to fp32.
A gate taken from an input (mask mode 2, bn2's gate of the fused kernel) is decided in any arithmetic: z is repaired until |scale z + shift| > 1e-3."""
import os

import numpy as np

import bn_pool_ref as B
import conv_epilogue_ref as E
import pw_bwd_ref as R

EPS = 1e-5
CH = 64
NC, NK = 256, 64
GATE_MARGIN = 1e-3
FLOOR = 4 * 2.0 ** -24        # no measured bound goes below the rounding of an fp32 result
# the existing tests' bounds of the reduced quantities (test_pw_bwd_fused_gpu.py, test_train_gpu.py, test_bn_pool_kernels_gpu.py): no measured bound goes above
CAPS = {"fused": 2e-5, "pair_s1": 3e-6, "pair_s2": 2e-5, "pw_sums": 2e-6, "pair_wgrad": 5e-5}
ALLOW_SHARE = 0.01           # every allowance stays below this share of the largest magnitude of the quantity it is added to

# row counts of the three chunk walkers under the default policy (tests/test_pw_bwd_ref_cpu.py has the splits they give, by hand)
ROWS = (17, 64, 209, 465, 3665, 40017)
ROWS_SMALL = ROWS[:-1]
PITCH_ROWS = (209, 465)
LEG_ROWS = (17, 209, 401, 448, 465)
LEGS = {"one_workgroup": dict(pwbf_wgs=1, bnwg_wgs=1), "two_workgroups": dict(pwbf_wgs=2, bnwg_wgs=2)}
# operand placements: name -> (pitch as a function of the channel count, column offset)
A_PLACE = {"contig": (lambda k: k, 0), "k+8": (lambda k: k + 8, 0), "slice": (lambda k: 4 * k, 64)}
G_PLACE = {"contig": lambda c: c, "c+8": lambda c: c + 8, "2c": lambda c: 2 * c}
# (mask mode, c, k) of mvf_bn_bwd_apply_wgrad: every instance of bnbwd_wgrad_launch with one BatchNorm
BNWG_SHAPES = ((4, 256, 64), (4, 512, 64), (4, 256, 128), (2, 64, 256), (2, 64, 512), (2, 128, 256), (2, 256, 256))
# (c, k, with x_b) of mvf_bn_bwd_pair_wgrad
PAIR_WGRAD_SHAPES = ((256, 64, True), (256, 64, False), (256, 128, False), (512, 128, False))
PW_SUMS_ROWS = (2048, 2047, 1920, 2225, 40017)
SLAB_SPLITS = (1, 2, 7, 29)
_cache = {}


def f32(x):
    return np.asarray(x, dtype=np.float32).astype(np.float64)


def rb(x):
    return E.rnd(x, "bf16")


# ------------------------------------------------------------------------------------------------ the launch plans (ports of the library's)
def policy_int(name, dflt):
    """csrc/common.h mvf_policy_int on this process's MVF_POLICY."""
    for item in os.environ.get("MVF_POLICY", "").replace(";", ",").split(","):
        if "=" in item:
            k, v = item.split("=", 1)
            if k.strip().lower() == name.lower():
                return int(v.strip())
    return dflt


def ceil_to(x, q):
    return (x + q - 1) // q * q


def fused_plan(m, c=NC, k=NK, wgs=None):
    """pw_bwd_fused_plan -> (workgroups, rows per workgroup); (0, 0): not built."""
    if c != NC or k != NK or m <= 0 or m * NC * 2 >= 0x7ffffff0:
        return 0, 0
    wgs = max(1, policy_int("pwbf_wgs", 256)) if wgs is None else wgs
    rows = max(ceil_to((m + wgs - 1) // wgs, CH), 2 * CH)
    return (m + rows - 1) // rows, rows


def bnwg_tile(c, k, nbn, mode):
    """bnbwd_wgrad_tile -> (CT, KT) or None."""
    if mode == 4 and c % 256 == 0 and (k == 64 or (k == 128 and nbn == 1)):
        return 256, k
    if mode == 4 and nbn == 2 and c % 256 == 0 and k == 128:
        return 256, 128
    if mode == 2 and nbn == 1 and c == 64 and k % 256 == 0:
        return 64, 256
    if mode == 2 and nbn == 1 and c % 128 == 0 and c <= 256 and k % 256 == 0:
        return 128, 256
    return None


def bnwg_plan(m, c, k, nbn, mode, wgs=None):
    """mvf_bn_bwd_wgrad_splits / bnbwd_wgrad_plan -> (row splits, rows per split, column tiles, k tiles); zeros: not built."""
    t = bnwg_tile(c, k, nbn, mode)
    if m <= 0 or c <= 0 or k <= 0 or m * max(c, k) * 2 >= 0x7ffffff0 or t is None:
        return 0, 0, 0, 0
    ct, kt = c // t[0], k // t[1]
    wgs = policy_int("bnwg_wgs", 256) if wgs is None else wgs
    want = wgs // (ct * kt) if wgs // (ct * kt) > 0 else 1
    rows = max(ceil_to((m + want - 1) // want, CH), 4 * CH)
    return (m + rows - 1) // rows, rows, ct, kt


def split_bounds(m, rows):
    return [(b, min(m, b + rows)) for b in range(0, m, rows)]


def chunks_of(m, rows):
    """Chunks each workgroup walks."""
    return [(e - b + CH - 1) // CH for b, e in split_bounds(m, rows)]


def pw_sums_nwg(m, n, stats_rows, cus, per_cu=None):
    """pw_sums_launch's workgroups per channel half; 0: the shape goes to the implicit GEMM."""
    if policy_int("pw_sums", 1) == 0 or n not in (128, 256) or m <= 0:
        return 0
    nblocks = (m + 31) // 32
    per_cu = policy_int("pw_sums_wgs", 3) if per_cu is None else per_cu
    nwg = min((nblocks + 3) // 4, per_cu * cus // (n // 128))
    nwg = min(nwg, stats_rows // 2)
    nwg = nwg // 8 * 8
    return nwg if nwg >= 8 else 0


def pw_sums_blocks(m, nwg):
    """The 32-row blocks each workgroup's four waves walk: blk = wg * 4 + wave, += 4 * nwg."""
    nblocks = (m + 31) // 32
    return [[b for wave in range(4) for b in range(wg * 4 + wave, nblocks, 4 * nwg)] for wg in range(nwg)]


def stats_rows(m):
    return (m + 127) // 128


# ------------------------------------------------------------------------------------------------ inputs
def _stats(z, rng):
    mean = f32(z.mean(axis=0) + 0.05 * rng.standard_normal(z.shape[1]))
    invstd = f32(1.0 / np.sqrt(z.var(axis=0) + EPS))
    return mean, invstd


def _g_for(z, mean, invstd, rng):
    xhat = (z - mean[None, :]) * invstd[None, :]
    return rb(rng.standard_normal(z.shape) + 0.25 * xhat + 0.1)


def _bits(rng, m, c):
    return rng.integers(0, 16, (m, c // 4), dtype=np.uint8)


def _repair(z, scale, shift):
    """z (bf16 values) moved where the gate scale z + shift lies within 2e-3 of zero, to the side it was on."""
    for _ in range(6):
        t = scale[None, :] * z + shift[None, :]
        bad = np.abs(t) < 2.0 * GATE_MARGIN
        if not bad.any():
            break
        target = np.where(t >= 0, 0.05, -0.05)
        z = np.where(bad, rb((target - shift[None, :]) / scale[None, :]), z)
    return z


def _gated_bn(rng, m, c, spread=1.2):
    """A stored pre-activation z [m][c] with its BatchNorm (a quarter of the weights negative) and a decided gate."""
    z = rb(rng.standard_normal((m, c)) * spread + 0.1 * rng.standard_normal(c))
    gamma = f32((rng.random(c) + 0.5) * np.where(rng.random(c) < 0.25, -1.0, 1.0))
    beta = f32(rng.standard_normal(c) * 0.3)
    noise = 0.05 * rng.standard_normal(c)
    for _ in range(6):
        mean = f32(z.mean(axis=0) + noise)
        invstd = f32(1.0 / np.sqrt(z.var(axis=0) + EPS))
        scale = f32(gamma * invstd)
        shift = f32(beta - mean * scale)
        if float(E.gate_margin(z, scale, shift).min()) > GATE_MARGIN:
            break
        z = _repair(z, scale, shift)
    return dict(z=z, gamma=gamma, mean=mean, invstd=invstd, scale=scale, shift=shift)


def conv_case(m, seed=0):
    """Operands of mvf_conv1x1_bwd_fused and mvf_conv1x1_bnbwd_sums_pair at m rows (64 -> 256 channels), with the reference's sums."""
    key = ("conv", m, seed)
    if key in _cache:
        return _cache[key]
    rng = np.random.default_rng(100003 * seed + m)
    o = dict(m=m, seed=seed)
    for suf in ("", "_b"):                                        # conv3 on a2; the downsample conv on the block input
        a = rb(np.maximum(rng.standard_normal((m, NK)), 0.0)) if not suf else rb(rng.standard_normal((m, NK)))
        w = rb(rng.standard_normal((NC, NK)) * (2.0 / NK) ** 0.5)
        acc = R.conv1x1(a, w)
        mean, invstd = _stats(rb(acc), rng)
        o["a" + suf], o["w" + suf], o["acc" + suf], o["mean" + suf], o["invstd" + suf] = a, w, acc, mean, invstd
    o["g"] = _g_for(rb(o["acc"]), o["mean"], o["invstd"], rng)
    # the pair's gradient is correlated with BOTH branches' xhat (with conv3's alone, bn_d's dgamma is noise that grows as sqrt(M) under an allowance
    # that grows as M: 1.04 % at M = 40017)
    xhat_b = (rb(o["acc_b"]) - o["mean_b"][None, :]) * o["invstd_b"][None, :]
    o["g_pair"] = rb(rng.standard_normal((m, NC)) + 0.25 * (rb(o["acc"]) - o["mean"][None, :]) * o["invstd"][None, :] + 0.25 * xhat_b + 0.1)
    o["bits"] = _bits(rng, m, NC)
    o["gamma"] = f32(rng.random(NC) + 0.5)
    o["bn2"] = _gated_bn(rng, m, NK)
    o["sums"] = R.conv_bnbwd_sums(o["a"], o["w"], o["g"], o["bits"], o["mean"], o["invstd"], acc=o["acc"])
    o["pair_a"] = R.conv_bnbwd_sums(o["a"], o["w"], o["g_pair"], o["bits"], o["mean"], o["invstd"], acc=o["acc"])
    o["pair_b"] = R.conv_bnbwd_sums(o["a_b"], o["w_b"], o["g_pair"], o["bits"], o["mean_b"], o["invstd_b"], acc=o["acc_b"])
    o["dbeta"], o["dgamma"] = f32(o["sums"]["v1"].sum(axis=0)), f32(o["sums"]["v2"].sum(axis=0))
    _cache[key] = o
    return o


def fused_ref(m, seed=0, with_bn=True):
    key = ("fused_ref", m, seed, with_bn)
    if key not in _cache:
        o = conv_case(m, seed)
        b = o["bn2"]
        kw = dict(z_in=b["z"], in_mean=b["mean"], in_invstd=b["invstd"], in_scale=b["scale"], in_shift=b["shift"]) if with_bn else {}
        _cache[key] = R.conv1x1_bwd_fused(o["a"], o["w"], o["g"], o["bits"], o["gamma"], o["mean"], o["invstd"], o["dgamma"], o["dbeta"], acc=o["acc"], **kw)
    return _cache[key]


def bnwg_case(m, c, k, mode, pair=False, seed=0):
    """Operands of mvf_bn_bwd_apply_wgrad (mask mode 2 / 4) and, pair=True, of mvf_bn_bwd_pair_wgrad at [m][c] with a k-channel conv input."""
    key = ("bnwg", m, c, k, mode, pair, seed)
    if key in _cache:
        return _cache[key]
    rng = np.random.default_rng(7919 * seed + 31 * c + 7 * k + m + (1 if pair else 0))
    o = dict(m=m, c=c, k=k, mode=mode)
    if mode == 2:
        o.update(_gated_bn(rng, m, c, spread=2.0))
        o["bits"] = None
    else:
        o["z"] = rb(rng.standard_normal((m, c)) * 2 + rng.standard_normal(c) * 1.5)
        o["mean"], o["invstd"] = _stats(o["z"], rng)
        o["gamma"] = f32(rng.random(c) + 0.5)
        o["scale"] = o["shift"] = None
        o["bits"] = _bits(rng, m, c)
    o["g"] = _g_for(o["z"], o["mean"], o["invstd"], rng)
    o["x"] = rb(np.maximum(rng.standard_normal((m, k)), 0.0))
    ref = B.bn_bwd(o["g"], o["z"], o["bits"], mode, o["gamma"], o["mean"], o["invstd"], o["scale"], o["shift"])
    o["dgamma"], o["dbeta"] = f32(ref["dgamma"]), f32(ref["dbeta"])
    if pair:
        o["z_b"] = rb(rng.standard_normal((m, c)) + rng.standard_normal(c))
        o["mean_b"], o["invstd_b"] = _stats(o["z_b"], rng)
        o["gamma_b"] = f32(rng.random(c) + 0.5)
        o["x_b"] = rb(rng.standard_normal((m, k)))
        o["ref_pair"] = R.bn_bwd_pair_wgrad(o["g"], o["z"], o["z_b"], o["bits"], o["gamma"], o["mean"], o["invstd"], o["gamma_b"], o["mean_b"], o["invstd_b"])
    _cache[key] = o
    return o


def pw_sums_case(m, n, seed=0):
    """Operands of the two passes of csrc/pw_sums.hip: a [m][64], w [n][64]; K = a running mean near the batch mean; bn's statistics; g, sign bits."""
    key = ("pw_sums", m, n, seed)
    if key in _cache:
        return _cache[key]
    rng = np.random.default_rng(65537 * seed + 3 * n + m)
    o = dict(m=m, n=n)
    o["a"] = rb(np.maximum(rng.standard_normal((m, NK)), 0.0))
    o["w"] = rb(rng.standard_normal((n, NK)) * (2.0 / NK) ** 0.5)
    o["acc"] = R.conv1x1(o["a"], o["w"])
    z = rb(o["acc"])
    o["mean"], o["invstd"] = _stats(z, rng)
    o["kshift"] = f32(z.mean(axis=0) + 0.05 * rng.standard_normal(n))
    o["g"] = _g_for(z, o["mean"], o["invstd"], rng)
    o["bits"] = _bits(rng, m, n)
    o["ref"] = {"k0": R.conv_stats(o["a"], o["w"], None, acc=o["acc"]), "k": R.conv_stats(o["a"], o["w"], o["kshift"], acc=o["acc"]),
                "bwd": R.conv_bnbwd_sums(o["a"], o["w"], o["g"], o["bits"], o["mean"], o["invstd"], acc=o["acc"])}
    _cache[key] = o
    return o


def slab_case(nsplit, c=NC, k=NK):
    rng = np.random.default_rng(nsplit)
    return f32(rng.standard_normal((nsplit, c, k)) * (1.0 + np.arange(nsplit)[:, None, None]))


def pitched(a, pitch, off, seed=1):
    """[M][C] -> the [M][pitch] allocation that holds it at columns [off, off + C), finite data in every other column."""
    m, c = a.shape
    if pitch == c and off == 0:
        return np.ascontiguousarray(a)
    buf = rb(np.random.default_rng(seed).standard_normal((m, pitch)) * 3.0)
    buf[:, off:off + c] = a
    return buf


# ------------------------------------------------------------------------------------------------ the case lists
def fused_cases():
    """(m, seed, z_in given, a placement, g placement)."""
    out = [(m, 0, True, "contig", "contig") for m in ROWS]
    out += [(m, 0, False, "contig", "contig") for m in (17, 209, 465)]
    out += [(465, 1, True, "contig", "contig")]
    for m in PITCH_ROWS:
        out += [(m, 0, True, "k+8", "c+8"), (m, 0, True, "slice", "2c"), (m, 0, False, "slice", "c+8")]
    return out


def pair_cases():
    """(m, seed, branches, a placement, x placement, g placement)."""
    out = [(m, 0, 2, "contig", "contig", "contig") for m in ROWS]
    out += [(m, 0, 1, "contig", "contig", "contig") for m in (17, 209, 465)]
    out += [(465, 1, 2, "contig", "contig", "contig")]
    for m in PITCH_ROWS:
        out += [(m, 0, 2, "k+8", "slice", "2c"), (m, 0, 2, "slice", "k+8", "contig"), (m, 0, 1, "k+8", "contig", "2c")]
    return out


def bnwg_cases():
    """(mode, c, k, m, g placement, x placement)."""
    out = []
    for mode, c, k in BNWG_SHAPES:
        out += [(mode, c, k, m, "contig", "contig") for m in ROWS_SMALL]
        for m in PITCH_ROWS:
            out += [(mode, c, k, m, "c+8", "k+8"), (mode, c, k, m, "2c", "slice")]
    out.append((4, 256, 64, 40017, "contig", "contig"))
    return out


def pair_wgrad_cases():
    """(c, k, with x_b, m, g placement, x placement)."""
    out = []
    for c, k, xb in PAIR_WGRAD_SHAPES:
        out += [(c, k, xb, m, "contig", "contig") for m in ROWS_SMALL]
        out += [(c, k, xb, 465, "c+8", "slice")]
    return out


def pw_sums_cases():
    """(m, n, x placement, pass: k0 | k | bwd, pw_sums_wgs or None)."""
    out = []
    for n in (128, 256):
        for what in ("k0", "k", "bwd"):
            out += [(m, n, "contig", what, None) for m in PW_SUMS_ROWS]
            out += [(2225, n, "k+8", what, None), (2225, n, "slice", what, None), (40017, n, "contig", what, 1)]
    return out


# ------------------------------------------------------------------------------------------------ comparisons (what the GPU module asserts with)
def _fmt(x):
    return "%.3g" % x


def cmp_elem(what, got, ref, a_terms):
    """A stored bf16 tensor whose inputs are all observable: |got - ref| <= 2^-8 |ref| + 8 * 2^-24 * A, every element."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), "%s: %d of %d elements are not finite (never written?)" % (what, int((~np.isfinite(got)).sum()), got.size)
    tol = 2.0 ** -8 * np.abs(ref) + 8.0 * 2.0 ** -24 * a_terms
    bad = np.abs(got - ref) > tol
    if bad.any():
        i = np.unravel_index(np.argmax(np.where(bad, np.abs(got - ref) / np.maximum(tol, 1e-300), 0.0)), got.shape)
        raise AssertionError("%s: %d of %d elements beyond the bound; worst at %s: got %.9g, ref %.9g, bound %.3g" % (what, int(bad.sum()), got.size, i, got[i], ref[i], tol[i]))
    return float((np.abs(got - ref) / np.maximum(tol, 1e-300)).max())


def allowance_share(allow, ref):
    """Largest allowance as a share of the largest magnitude of what it is added to."""
    return float(np.max(allow)) / max(float(np.abs(ref).max()), 1e-300) if np.size(allow) else 0.0


def cmp_tensor(what, got, ref, base, allow=None, l2=True):
    """|got - ref| <= base max|ref| + allow elementwise and, l2, ||got - ref|| <= base ||ref|| + ||allow||.  Returns the measured figures (net = outside the
    allowance, relative); raises AssertionError beyond the bound."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), "%s: %d of %d values are not finite (never written?)" % (what, int((~np.isfinite(got)).sum()), got.size)
    al = np.zeros(ref.shape) if allow is None else np.asarray(allow, dtype=np.float64)
    scale, norm = max(float(np.abs(ref).max()), 1e-300), max(float(np.sqrt((ref ** 2).sum())), 1e-300)
    d = np.abs(got - ref)
    fig = dict(rel_err=float(d.max()) / scale, rel_l2=float(np.sqrt((d ** 2).sum())) / norm, net_err=float(np.maximum(d - al, 0.0).max()) / scale,
               net_l2=max(float(np.sqrt((d ** 2).sum())) - float(np.sqrt((al ** 2).sum())), 0.0) / norm, allow=float(al.max()) / scale, bound=base)
    if fig["net_err"] > base or (l2 and fig["net_l2"] > base):
        i = np.unravel_index(np.argmax(d - al), d.shape)
        raise AssertionError("%s: rel_err %s rel_l2 %s, outside the allowance (%s of the scale) %s / %s, bound %s; worst at %s: got %.9g, ref %.9g" % (
            what, _fmt(fig["rel_err"]), _fmt(fig["rel_l2"]), _fmt(fig["allow"]), _fmt(fig["net_err"]), _fmt(fig["net_l2"]), _fmt(base), i, got[i], ref[i]))
    return fig


def part_rows(what, part, nwg, check_remainder_col=1):
    """Partial rows [C][rows][2] as these kernels leave them -- rows [0, nwg) the fp32 value of a workgroup's fp64 sum, rows [nwg, 2 nwg) its remainder, rows
    beyond exactly zero -> [C][nwg][2] in fp64.  The layout is asserted: everything finite, a remainder at most half an fp32 ulp of its value, and the
    remainders of the second sum (products rounded in fp32: generically inexact) present, not zeros."""
    part = np.asarray(part, dtype=np.float64)
    assert part.ndim == 3 and part.shape[2] == 2 and part.shape[1] >= 2 * nwg, (what, part.shape, nwg)
    assert np.isfinite(part).all(), "%s: %d partial sums are not finite (never written?)" % (what, int((~np.isfinite(part)).sum()))
    val, rem, rest = part[:, :nwg], part[:, nwg:2 * nwg], part[:, 2 * nwg:]
    assert not rest.any(), "%s: rows beyond 2 x %d workgroups are not zero" % (what, nwg)
    half = 0.5 * np.spacing(np.abs(val).astype(np.float32)).astype(np.float64)
    assert (np.abs(rem) <= half).all(), "%s: %d remainders exceed half an ulp of their value row (value / remainder rows misplaced?)" % (what, int((np.abs(rem) > half).sum()))
    live = val[:, :, check_remainder_col] != 0
    if live.sum() >= 16:
        zero = float((rem[:, :, check_remainder_col][live] == 0).mean())
        assert zero < 0.5, "%s: %.0f %% of the remainders of sum %d are exactly zero (the remainder row dropped?)" % (what, 100 * zero, check_remainder_col)
    return val + rem


def kernel_layout(t64):
    """fp64 sums [C][nwg][2] -> the partial rows a kernel leaves: [C][2 nwg][2] fp32 value rows then remainder rows (the CPU test corrupts these)."""
    val = f32(t64)
    return np.concatenate([val, f32(t64 - val)], axis=1)
