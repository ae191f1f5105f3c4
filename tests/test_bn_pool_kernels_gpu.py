"""GPU: every kernel variant of the training BatchNorm and stem max-pool entry points of csrc/train_ops.hip through the C ABI against the INDEPENDENT fp64
reference tests/bn_pool_ref.py (proved against torch float64 in tests/test_bn_pool_ref_cpu.py), at the smallest shapes that reach each variant, in both
storage types.  After every call the host-side launch record (mvf_bn_last_launch) says which form ran: under the default policy each case asserts the lane
width, the column plan (derived here from a port of col_plan), the mask mode and its specialisation, the finalize form and the pool form; one child process per
forced policy (bn_spec=0, pool_fwd_block=0, pool_bwd_block=0) re-runs the backward / pool cases and asserts through the record that the forced form ran.

Conventions (those of test_wgrad_families_gpu.py): operands are rounded to the storage type on the CPU (tests/bn_pool_cases.py) and the reference is evaluated
on exactly those values; outputs are NaN before the call; the workspace is exactly mvf_bn_workspace_bytes of NaN plus a 4 KiB canary that must be unchanged;
a tensor with a pitch holds data in every column of the pitch.

Bounds.
  Elementwise outputs (apply out, gm, dz, pool y and ga), A = the sum of the absolute values of the terms of the element's fp64 expression (bn_pool_ref returns
  it): fp32 storage |got - ref| <= 8 * 2^-24 * A; bf16 storage |got - ref| <= 2^-8 |ref| + 8 * 2^-24 * A (one stored rounding).  For dz the reference is fed the
  KERNEL's dgamma / dbeta, so the apply pass is judged on its own.
  Reduced quantities (statistics, dgamma, dbeta, column means, pool sums): helpers.rel_err and rel_l2 against the reference, bound = 4 x the largest value
  measured over all cases of that quantity and storage type (the per-block fp32 sums reorder across lane widths and plans), never above the 5e-5 of the existing
  tests and never below 4 x 2^-24 (a result's own fp32 rounding): BOUNDS below, measured values in profiles/bn_pool_errors.txt (MVF_BN_POOL_ERRORS=file dumps them; tools/bn_pool_errors_table.py).
  Statistics with an ill-conditioned sum: the data with mean = 30 standard deviations and K = 0 (running_mean NULL) forms var = sum(z^2) / M - mean^2 from two
  terms 1 + mean^2 / var (~ 900) times larger than their difference; the bound of the var-derived quantities (invstd, scale, shift, running_var) is multiplied
  by that conditioning factor 1 + (mean - K)^2 / (var + eps) (bn_pool_cases.stats_case states it per case), for that case alone.  With K = running_mean near the
  mean the plain bound holds: that is what the shifted sums are for.  One row per channel (M = 1) meets the plain bounds too: its variance is zero, and the
  finalize kernel says so instead of taking the fp32 rounding of (z - K)^2 for it (it did, which left invstd up to 15 % off 1 / sqrt(eps); this module found it).
  Undecided mask elements (modes 2 and 3, the sign bits, the pool's ReLU gate): fp64 pre-activation within 2^-20 max(1, |s z| + |b|) of a kink.  They are left
  out of the elementwise checks and their |g| is added to the slack of the sums, in their own channel only; at most 1e-4 of a case's elements (checked on the CPU, for these very inputs,
  by tests/test_bn_pool_ref_cpu.py); the lattice family has none."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bn_pool_cases as K
import bn_pool_ref as R
from helpers import policy_env, rel_err, rel_l2

pytestmark = pytest.mark.gpu

COVERAGE_ENV = "MVF_BN_POOL_COVERAGE"     # a file: one JSON line per recorded call (the forced legs' children)
ERRORS_ENV = "MVF_BN_POOL_ERRORS"         # a file: one JSON line per measured reduced quantity (tooling: profiles/bn_pool_errors.txt)
CAP = 5e-5
# (quantity, storage type) -> 4 x the largest rel_err / rel_l2 measured over all cases (profiles/bn_pool_errors.txt, section 4), capped at 5e-5; never below
# 4 x 2^-24 (the rounding of the fp32 result itself: the bf16 pool sums of these sizes are exact before it)
BOUNDS = {
    ("mean", "f32"): 5.40e-07,
    ("invstd", "f32"): 1.12e-05,
    ("scale", "f32"): 1.12e-05,
    ("shift", "f32"): 1.01e-05,
    ("running_var", "f32"): 3.29e-06,
    ("running_mean", "f32"): 6.23e-07,
    ("mean", "bf16"): 6.17e-07,
    ("invstd", "bf16"): 9.39e-06,
    ("scale", "bf16"): 9.87e-06,
    ("shift", "bf16"): 9.63e-06,
    ("running_var", "bf16"): 5.26e-06,
    ("running_mean", "bf16"): 7.14e-07,
    ("finalize_mean", "f32"): 2.38e-07,
    ("finalize_invstd", "f32"): 3.27e-07,
    ("finalize_scale", "f32"): 4.31e-07,
    ("finalize_shift", "f32"): 5.36e-07,
    ("finalize_running_mean", "f32"): 3.09e-07,
    ("finalize_running_var", "f32"): 2.91e-07,
    ("finalize_dbeta", "f32"): 2.38e-07,
    ("finalize_dgamma", "f32"): 2.38e-07,
    ("colmeans", "f32"): 3.40e-07,
    ("colmeans", "bf16"): 2.38e-07,
    ("dbeta", "f32"): 5.86e-07,
    ("dgamma", "f32"): 6.84e-07,
    ("dbeta", "bf16"): 9.35e-07,
    ("dgamma", "bf16"): 8.36e-07,
    ("pool_dbeta", "f32"): 7.13e-07,
    ("pool_dgamma", "f32"): 6.27e-07,
    ("pool_dbeta", "bf16"): 2.38e-07,
    ("pool_dgamma", "bf16"): 5.30e-07,
}
POLICY = os.environ.get("MVF_POLICY", "").lower()
FORCED = {k: ("%s=0" % k) in POLICY.replace(" ", "") for k in ("bn_spec", "pool_fwd_block", "pool_bwd_block")}
DEFAULT_POLICY = not any(k in POLICY for k in FORCED)
CANARY = 4096
EINVAL, EWS, EUNSUPPORTED = -1, -3, -5
_records = []


def _bound(q, dtype):
    return min(BOUNDS.get((q, dtype), CAP), CAP)


# ------------------------------------------------------------------------------------------------ the plan the library must choose (port of col_plan)
def col_plan(m, c, vn=4, blocks=2048):
    cq = c // vn
    cqb = 1
    while cqb < cq and cqb < 64:
        cqb *= 2
    rl = 256 // cqb
    gx = (cq + cqb - 1) // cqb
    want = max(1, blocks // gx)
    rows = max((m + want - 1) // want, rl * 8)
    rows = (rows + rl - 1) // rl * rl
    return dict(cqb=cqb, rows=rows, gx=gx, gy=(m + rows - 1) // rows)


def _vn(dtype, c, *ok):
    """Lane width the library must take: fp32 4; bf16 8 when c % 8 == 0 and every other condition (pitch % 8, 16-byte alignment) holds, else 4."""
    return 8 if dtype == "bf16" and c % 8 == 0 and all(ok) else 4


# ------------------------------------------------------------------------------------------------ device buffers
def _tt(dtype):
    return torch.bfloat16 if dtype == "bf16" else torch.float32


def _dev(a, dtype, off=0):
    """fp64 numpy (already rounded to the storage type) -> device tensor; off: elements between a 256-byte aligned allocation and the first element."""
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(_tt(dtype))
    if not off:
        return t.cuda()
    buf = torch.zeros(t.numel() + off + 8, dtype=_tt(dtype), device="cuda")
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def _nan(shape, dtype, off=0):
    n = int(np.prod(shape))
    buf = torch.full((n + off + 8,), float("nan"), dtype=_tt(dtype), device="cuda")
    return buf[off:off + n].view(shape)


def _p(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).float().cuda()


def _nanv(c):
    return torch.full((c,), float("nan"), device="cuda")


def _bytes(a, off=0):
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8))
    buf = torch.zeros(t.numel() + off + 8, dtype=torch.uint8, device="cuda")
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    return v


def P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _np(t):
    return t.double().cpu().numpy()


class _Ws(object):
    """Exactly `nbytes` of NaN workspace plus a canary that must come back unchanged."""

    def __init__(self, nbytes):
        self.n = nbytes
        self.t = torch.empty(nbytes + CANARY, dtype=torch.uint8, device="cuda")
        self.t[:nbytes] = 0xFF
        self.t[nbytes:] = 0xA5

    def check(self):
        torch.cuda.synchronize()
        assert bool((self.t[self.n:] == 0xA5).all()), "the workspace was written past its published size"


def _ws(m, c, mult=1):
    from mvfnet_amd import _lib
    nb = _lib.lib.mvf_bn_workspace_bytes(m, c)
    assert nb > 0 and nb % 256 == 0
    return _Ws(mult * nb)


def _dt(dtype):
    return 0 if dtype == "f32" else 1


# ------------------------------------------------------------------------------------------------ the record
def _rec(case):
    from mvfnet_amd import _lib
    info = _lib.BnLaunchInfo()
    _lib.check(_lib.lib.mvf_bn_last_launch(C.byref(info)))
    r = dict(case=case, entry=_lib.BN_ENTRIES[info.entry], dtype=info.dtype, vn=info.vn, cqb=info.cqb, rows=info.rows, gx=info.gx, gy=info.gy, mask_mode=info.mask_mode,
             spec=info.specialised, finalize=_lib.BN_FINALIZE_FORMS[info.finalize], part_rows=info.part_rows, pool=_lib.POOL_FORMS[info.pool], launches=info.launches)
    _records.append(r)
    if os.environ.get(COVERAGE_ENV):
        with open(os.environ[COVERAGE_ENV], "a") as f_:
            f_.write(json.dumps(r) + "\n")
    return r


def _want(rec, **kv):
    got = {k_: rec[k_] for k_ in kv}
    assert got == kv, "launch record of %s: %s, expected %s (whole record %s)" % (rec["case"], got, kv, rec)


def _want_plan(rec, m, c, vn, blocks):
    _want(rec, vn=vn, **col_plan(m, c, vn, blocks))


def _refused(rc, rc_want, case, entry, *outs):
    from mvfnet_amd import _lib
    assert rc == rc_want, (case, rc, _lib.lib.mvf_last_error())
    rec = _rec(case)
    _want(rec, entry=entry, launches=0, vn=0, finalize="none", pool="none", part_rows=0)
    torch.cuda.synchronize()
    for o in outs:
        assert bool(torch.isnan(o.float()).all()), "%s: a refused call wrote an output" % case


# ------------------------------------------------------------------------------------------------ comparisons
def _elem(case, what, got, ref, a, dtype, skip=None):
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == ref.shape, (case, what, got.shape, ref.shape)
    assert np.isfinite(got).all(), "%s %s: %d of %d elements are not finite (never written?)" % (case, what, int((~np.isfinite(got)).sum()), got.size)
    tol = 8.0 * 2.0 ** -24 * a + (2.0 ** -8 * np.abs(ref) if dtype == "bf16" else 0.0)
    bad = np.abs(got - ref) > tol
    if skip is not None:
        assert skip.mean() <= K.UNDECIDED_SHARE, (case, what, float(skip.mean()))
        bad &= ~skip
    if bad.any():
        i = np.unravel_index(np.argmax(np.where(bad, np.abs(got - ref) / np.maximum(tol, 1e-300), 0)), got.shape)
        raise AssertionError("%s %s %s: %d of %d elements beyond the bound; worst at %s: got %.9g, ref %.9g, bound %.3g" % (case, what, dtype, int(bad.sum()), got.size, i,
                                                                                                                      got[i], ref[i], tol[i] if np.ndim(tol) else tol))


def _reduced(case, q, dtype, got, ref, factor=1.0, slack=None):
    """A reduced quantity against the reference: rel_err and rel_l2 printed, dumped and asserted <= bound x factor.  slack: per-channel ABSOLUTE allowance (the
    undecided elements' weights, _slack), granted to the channels that hold such elements and to no other: |got - ref|[c] <= bound x factor x max |ref| + slack[c],
    and in the 2-norm ||got - ref|| <= bound x factor x ||ref|| + ||slack||."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    assert np.isfinite(got).all(), "%s %s: not finite (never written, or summed from an unwritten partial row)" % (case, q)
    e, l2 = rel_err(got, ref), rel_l2(got, ref)
    b = _bound(q, dtype)
    sl = np.zeros(ref.shape) if slack is None else slack
    # the figures the bound is asserted on: the error outside the slack, on the scale of the tensor
    e_net = float(np.maximum(np.abs(got - ref) - sl, 0.0).max()) / max(float(np.abs(ref).max()), 1e-30) if ref.any() else float(np.maximum(np.abs(got - ref) - sl, 0.0).max())
    l2_net = max(float(np.sqrt(((got - ref) ** 2).sum())) - float(np.sqrt((sl ** 2).sum())), 0.0) / max(float(np.sqrt((ref ** 2).sum())), 1e-30)
    if os.environ.get(ERRORS_ENV):
        with open(os.environ[ERRORS_ENV], "a") as f_:
            f_.write(json.dumps(dict(case=case, quantity=q, dtype=dtype, rel_err=e, rel_l2=l2, net_err=e_net, net_l2=l2_net, factor=factor, slack_channels=int((sl > 0).sum()),
                                     bound=b, policy=os.environ.get("MVF_POLICY", ""))) + "\n")
    print("%s %s %s: rel_err %.3g rel_l2 %.3g, outside the slack of %d channels %.3g / %.3g (bound %.3g x factor %.3g)" % (case, q, dtype, e, l2, int((sl > 0).sum()), e_net, l2_net, b,
                                                                                                                      factor))
    assert e_net <= b * factor and l2_net <= b * factor, "%s %s %s: rel_err %.3g, rel_l2 %.3g (outside the slack: %.3g, %.3g), bound %.3g x %.3g" % (case, q, dtype, e, l2, e_net,
                                                                                                                                                 l2_net, b, factor)


def _slack(und, weight):
    """Per-channel absolute slack of a sum for its undecided elements: the sum of their weights (|g|, |g xhat|) in that channel; zero elsewhere."""
    return np.where(und, weight, 0.0).reshape(-1, und.shape[-1]).sum(axis=0)


# ------------------------------------------------------------------------------------------------ statistics
def _mc(lst=K.MATRICES):
    return [pytest.param(m, c, dt, id="m%d_c%d_%s" % (m, c, dt)) for m, c, dts in lst for dt in dts]


def _run_stats(m, c, dtype, kind, off=0):
    from mvfnet_amd import _lib
    lib = _lib.lib
    o = K.stats_case(m, c, dtype, kind)
    case = "stats_%s_m%d_c%d%s" % (kind, m, c, "_off" if off else "")
    z = _dev(o["z"], dtype, off)
    rm, rv = _p(o["running_mean"]), _p(o["running_var"])
    outs = [_nanv(c) for _ in range(4)]
    ws = _ws(m, c)
    gam, bet = _p(o["gamma"]), _p(o["beta"])                      # (every device operand stays referenced until the results are read)
    rc = lib.mvf_bn_train_stats(P(z), m, c, P(gam), P(bet), C.c_float(K.EPS), C.c_float(K.MOMENTUM), P(rm), P(rv), *[P(t) for t in outs], P(ws.t), ws.n,
                                _dt(dtype), None)
    assert rc == 0, lib.mvf_last_error()
    rec = _rec(case)
    ws.check()
    vn = _vn(dtype, c, off == 0)
    if DEFAULT_POLICY:
        _want(rec, entry="train_stats", finalize="row_major", launches=2, part_rows=col_plan(m, c, vn)["gy"], dtype=_dt(dtype), mask_mode=-1)
        _want_plan(rec, m, c, vn, 2048)
    ref = o["ref"]
    f = o["factor"] if o["scaled"] else 1.0
    for q, t, fq in (("mean", outs[0], 1.0), ("invstd", outs[1], f), ("scale", outs[2], f), ("shift", outs[3], f), ("running_var", rv, f)):
        _reduced(case, q, dtype, _np(t), ref[q], fq)
    if rm is not None:
        _reduced(case, "running_mean", dtype, _np(rm), ref["running_mean"])
    return rec


def _stats_params():
    """Every matrix x kind; one row has no standard deviation to place a mean 30 of them away, so M = 1 runs the two regular kinds only."""
    return [pytest.param(m, c, dt, kind, id="m%d_c%d_%s-%s" % (m, c, dt, kind)) for m, c, dts in K.MATRICES for dt in dts for kind in K.STATS_KINDS
            if not (m == 1 and kind.startswith("mean30"))]


@pytest.mark.parametrize("m,c,dtype,kind", _stats_params())
def test_train_statistics(m, c, dtype, kind):
    """mvf_bn_train_stats with running_mean given (K = running_mean) and NULL (K = 0), at means of ~ 3 and of 30 standard deviations.  M = 1: the variance is
    exactly zero, invstd = 1 / sqrt(eps) and running_var decays by the momentum alone, at the ordinary bounds."""
    rec = _run_stats(m, c, dtype, kind)
    if (m, c) == (300, 64) or (m, c) == (2049, 4):
        assert rec["gy"] > 1, rec


# ------------------------------------------------------------------------------------------------ finalize layouts
@pytest.mark.parametrize("nblk", K.FINALIZE_ROWS)
@pytest.mark.parametrize("c", K.FINALIZE_CHANNELS)
def test_finalize_layouts(c, nblk):
    """mvf_bn_train_finalize / mvf_bn_bwd_finalize on channel-major partials [C][nblk][2]: a wave per channel below 1024 rows (C = 6: a ragged last workgroup),
    a workgroup per channel from 1024 on.  (The row-major form is what every mvf_bn_train_stats / mvf_bn_bwd_reduce case runs.)"""
    from mvfnet_amd import _lib
    lib = _lib.lib
    o = K.finalize_case(c, nblk)
    case = "finalize_c%d_rows%d" % (c, nblk)
    form = "cm_workgroup" if nblk >= 1024 else "cm_wave"
    part = _p(o["part"])
    rm, rv = _p(o["running_mean"]), _p(o["running_var"])
    outs = [_nanv(c) for _ in range(4)]
    gam, bet = _p(o["gamma"]), _p(o["beta"])
    rc = lib.mvf_bn_train_finalize(P(part), nblk, o["m"], c, P(gam), P(bet), C.c_float(K.EPS), C.c_float(K.MOMENTUM), P(rm), P(rv), *[P(t) for t in outs], None)
    assert rc == 0, lib.mvf_last_error()
    _want(_rec(case), entry="train_finalize", finalize=form, part_rows=nblk, launches=1, vn=0, pool="none")
    for q, t in (("mean", outs[0]), ("invstd", outs[1]), ("scale", outs[2]), ("shift", outs[3]), ("running_mean", rm), ("running_var", rv)):
        _reduced(case, "finalize_" + q, "f32", _np(t), o["ref"][q])
    dg, db = _nanv(c), _nanv(c)
    rc = lib.mvf_bn_bwd_finalize(P(part), nblk, c, P(dg), P(db), None)
    assert rc == 0, lib.mvf_last_error()
    _want(_rec(case), entry="bwd_finalize", finalize=form, part_rows=nblk, launches=1, vn=0, pool="none")
    _reduced(case, "finalize_dbeta", "f32", _np(db), o["s1"])
    _reduced(case, "finalize_dgamma", "f32", _np(dg), o["s2"])


# ------------------------------------------------------------------------------------------------ apply
RESIDUALS = ("none", "r", "r_scaled")


def _apply_ref(o, act, res):
    kw = {} if res == "none" else (dict(r=o["r"]) if res == "r" else dict(r=o["r"], rscale=o["rscale"], rshift=o["rshift"]))
    return R.bn_apply(o["z"], o["scale"], o["shift"], act=act, **kw)


def _run_apply(m, c, dtype, act, res, with_bits, z_off=0, out_off=0, bits_off=0):
    from mvfnet_amd import _lib
    lib = _lib.lib
    o = K.matrix_case(m, c, dtype)
    case = "apply_m%d_c%d_act%d_%s%s%s" % (m, c, act, res, "_bits" if with_bits else "", "_off%d%d%d" % (z_off, out_off, bits_off) if z_off or out_off or bits_off else "")
    ref = _apply_ref(o, act, res)
    z, r = _dev(o["z"], dtype, z_off), (_dev(o["r"], dtype) if res != "none" else None)
    out = _nan((m, c), dtype, out_off)
    bits = _bytes(np.full((m, c // 4), 0xEE, dtype=np.uint8), bits_off) if with_bits else None
    rs, rb = (_p(o["rscale"]), _p(o["rshift"])) if res == "r_scaled" else (None, None)
    sc, sh = _p(o["scale"]), _p(o["shift"])
    rc = lib.mvf_bn_apply_bits(P(z), m, c, P(sc), P(sh), P(r), P(rs), P(rb), act, P(out), P(bits), _dt(dtype), None)
    assert rc == 0, lib.mvf_last_error()
    rec = _rec(case)
    vn = _vn(dtype, c, z_off == 0, out_off == 0, bits_off % 2 == 0)
    _want(rec, entry="apply", launches=1, finalize="none", pool="none", dtype=_dt(dtype))
    _want_plan(rec, m, c, vn, 4096)
    got = _np(out)
    _elem(case, "out", got, ref["out"], ref["A"], dtype)
    if with_bits:
        b = bits.cpu().numpy()
        assert np.array_equal(b, R.pack_bits(got > 0)), "%s: the sign bits are not those of the stored output" % case
        agree = (R.unpack_bits(b, c) == (ref["out"] > 0)) | ref["undecided"]
        assert agree.all(), "%s: %d sign bits differ from the reference at decided elements" % (case, int((~agree).sum()))
    return rec


@pytest.mark.parametrize("m,c,dtype", _mc())
def test_apply_and_sign_bits(m, c, dtype):
    """mvf_bn_apply_bits: act 0 / 1 / 2 x no residual / residual / residual with rscale and rshift x with and without sign bits."""
    for act in (0, 1, 2):
        for res in RESIDUALS:
            for with_bits in (False, True):
                _run_apply(m, c, dtype, act, res, with_bits)


@pytest.mark.parametrize("m,c,dtype", _mc([t for t in K.MATRICES if t[1] % 8 == 0]))
def test_apply_with_column_means(m, c, dtype):
    """mvf_bn_apply_colmeans (c % 8 == 0), act 1 and 2: out as mvf_bn_apply, the means against the fp64 column means of the STORED output."""
    from mvfnet_amd import _lib
    lib = _lib.lib
    o = K.matrix_case(m, c, dtype)
    for act in (1, 2):
        case = "colmeans_m%d_c%d_act%d" % (m, c, act)
        ref = _apply_ref(o, act, "none")
        out, means = _nan((m, c), dtype), _nanv(c)
        ws = _ws(m, c)
        z, sc, sh = _dev(o["z"], dtype), _p(o["scale"]), _p(o["shift"])
        rc = lib.mvf_bn_apply_colmeans(P(z), m, c, P(sc), P(sh), act, P(out), P(means), P(ws.t), ws.n, _dt(dtype), None)
        assert rc == 0, lib.mvf_last_error()
        rec = _rec(case)
        ws.check()
        vn = _vn(dtype, c)
        _want(rec, entry="apply_colmeans", launches=2, finalize="row_major", part_rows=col_plan(m, c, vn, 4096)["gy"])
        _want_plan(rec, m, c, vn, 4096)
        got = _np(out)
        _elem(case, "out", got, ref["out"], ref["A"], dtype)
        _reduced(case, "colmeans", dtype, _np(means), got.mean(axis=0))


# ------------------------------------------------------------------------------------------------ backward
PITCHES = ("contig", "c+8", "c+4")


def _g_of(o, pitch, dtype, off=0):
    c = o["c"]
    gw = o["gwide"]
    if pitch == "contig":
        return _dev(gw[:, :c], dtype, off), c
    if pitch == "c+8":
        return _dev(gw, dtype, off), c + 8
    return _dev(gw[:, :c + 4], dtype, off), c + 4


def _mask_operands(o, dtype):
    """The forward whose output the masks of modes 1 and 4 come from: relu(bn(z) + r), stored in the storage type."""
    ap = R.bn_apply(o["z"], o["scale"], o["shift"], r=o["r"], act=1)
    y = R.round_storage(ap["out"], dtype)
    return y, R.pack_bits(y > 0)


def _forced_spec(rec):
    if FORCED["bn_spec"]:
        assert rec["spec"] == 0, "policy bn_spec=0 did not reach the run-time mask select: %s" % rec
    elif DEFAULT_POLICY:
        assert rec["spec"] == 1, rec


def _run_backward(m, c, dtype, pitch, modes=(0, 1, 2, 3, 4), z_off=0, dz_off=0, bits_off=0, pair=True):
    from mvfnet_amd import _lib
    lib = _lib.lib
    o = K.matrix_case(m, c, dtype)
    tag = "m%d_c%d_%s%s" % (m, c, pitch, "_off%d%d%d" % (z_off, dz_off, bits_off) if z_off or dz_off or bits_off else "")
    g, gp = _g_of(o, pitch, dtype)
    gnp = o["gwide"][:, :c]
    z = _dev(o["z"], dtype, z_off)
    y, bits = _mask_operands(o, dtype)
    yd, bd = _dev(y, dtype), _bytes(bits, bits_off)
    par = {k_: _p(o[k_]) for k_ in ("gamma", "mean", "invstd", "scale", "shift", "gamma_b", "mean_b", "invstd_b")}
    wide_apply = lambda mode: _vn(dtype, c, gp % 8 == 0, z_off == 0, dz_off == 0, mode != 4 or bits_off % 2 == 0)      # noqa: E731
    for mode in modes:
        operand, oper_np = (yd, y) if mode == 1 else ((bd, bits) if mode == 4 else (None, None))
        case = "bwd_mode%d_%s" % (mode, tag)
        ref = R.bn_bwd(gnp, o["z"], oper_np, mode, o["gamma"], o["mean"], o["invstd"], o["scale"], o["shift"])
        und = ref["undecided"]
        sl_db = _slack(und, np.abs(gnp))
        sl_dg = _slack(und, np.abs(gnp) * np.abs(ref["xhat"]))
        for with_gm in (False, True):
            gm = _nan((m, c), dtype) if with_gm else None
            dg, db = _nanv(c), _nanv(c)
            ws = _ws(m, c)
            rc = lib.mvf_bn_bwd_reduce(P(g), gp, P(z), P(operand), m, c, P(par["mean"]), P(par["invstd"]), P(par["scale"]), P(par["shift"]), mode, P(gm), P(dg), P(db), P(ws.t),
                                       ws.n, _dt(dtype), None)
            assert rc == 0, lib.mvf_last_error()
            rec = _rec(case + ("_gm" if with_gm else ""))
            ws.check()
            _want(rec, entry="bwd_reduce", mask_mode=mode, launches=2, finalize="row_major", part_rows=col_plan(m, c, 4)["gy"], dtype=_dt(dtype))
            _want_plan(rec, m, c, 4, 2048)                        # (this kernel always takes the 8-byte bf16 lanes)
            _forced_spec(rec)
            _reduced(case, "dbeta", dtype, _np(db), ref["dbeta"], slack=sl_db)
            _reduced(case, "dgamma", dtype, _np(dg), ref["dgamma"], slack=sl_dg)
            if with_gm:
                _elem(case, "gm", _np(gm), ref["gm"], ref["A_gm"], dtype, und)
        # the apply pass, fed the kernel's own sums
        ref_k = R.bn_bwd(gnp, o["z"], oper_np, mode, o["gamma"], o["mean"], o["invstd"], o["scale"], o["shift"], _np(dg), _np(db))
        entries = ("masked", "plain") if mode in (0, 2, 3) else ("masked",)
        for ent in entries:
            dz = _nan((m, c), dtype, dz_off)
            if ent == "masked":
                rc = lib.mvf_bn_bwd_apply_masked(P(g), gp, P(z), P(operand), m, c, P(par["gamma"]), P(par["mean"]), P(par["invstd"]), P(par["scale"]), P(par["shift"]), P(dg), P(db),
                                                 mode, P(dz), _dt(dtype), None)
            else:
                rc = lib.mvf_bn_bwd_apply(P(g), gp, P(z), m, c, P(par["gamma"]), P(par["mean"]), P(par["invstd"]), P(par["scale"]), P(par["shift"]), P(dg), P(db), mode, P(dz),
                                          _dt(dtype), None)
            assert rc == 0, lib.mvf_last_error()
            rec = _rec(case + "_apply_" + ent)
            _want(rec, entry="bwd_apply", mask_mode=mode, launches=1, finalize="none", dtype=_dt(dtype))
            _want_plan(rec, m, c, wide_apply(mode), 4096)
            _forced_spec(rec)
            _elem(case, "dz (%s)" % ent, _np(dz), ref_k["dz"], ref_k["A_dz"], dtype, und)
    if not pair:
        return
    # the pair: both BatchNorms of relu(bn_a(z_a) + bn_b(z_b)) under the same sign bits
    case = "bwd_pair_" + tag
    zb = _dev(o["zb"], dtype, z_off)
    ra, rb = R.bn_bwd_pair(gnp, o["z"], o["zb"], bits, o["gamma"], o["mean"], o["invstd"], o["gamma_b"], o["mean_b"], o["invstd_b"])
    sums = [_nanv(c) for _ in range(4)]
    dza, dzb = _nan((m, c), dtype, dz_off), _nan((m, c), dtype, dz_off)
    ws = _ws(m, c, 2)
    rc = lib.mvf_bn_bwd_pair(P(g), gp, P(z), P(zb), P(bd), m, c, P(par["gamma"]), P(par["mean"]), P(par["invstd"]), P(sums[0]), P(sums[1]), P(par["gamma_b"]), P(par["mean_b"]),
                             P(par["invstd_b"]), P(sums[2]), P(sums[3]), P(dza), P(dzb), P(ws.t), ws.n, _dt(dtype), None)
    assert rc == 0, lib.mvf_last_error()
    rec = _rec(case)
    ws.check()
    _want(rec, entry="bwd_pair", mask_mode=4, launches=3, finalize="row_major", part_rows=col_plan(m, c, 4)["gy"])
    _want_plan(rec, m, c, wide_apply(4), 4096)
    for (dgt, dbt, dzt, rr, gk, mk, ik, zk) in ((sums[0], sums[1], dza, ra, "gamma", "mean", "invstd", "z"), (sums[2], sums[3], dzb, rb, "gamma_b", "mean_b", "invstd_b", "zb")):
        _reduced(case, "dbeta", dtype, _np(dbt), rr["dbeta"])
        _reduced(case, "dgamma", dtype, _np(dgt), rr["dgamma"])
        rk = R.bn_bwd(gnp, o[zk], bits, 4, o[gk], o[mk], o[ik], dgamma=_np(dgt), dbeta=_np(dbt))
        _elem(case, "dz of " + zk, _np(dzt), rk["dz"], rk["A_dz"], dtype)


@pytest.mark.parametrize("pitch", PITCHES)
@pytest.mark.parametrize("m,c,dtype", _mc())
def test_backward(m, c, dtype, pitch):
    """mvf_bn_bwd_reduce (with and without gm_out), mvf_bn_bwd_apply_masked, mvf_bn_bwd_apply (modes 0, 2, 3) for the five mask modes, then mvf_bn_bwd_pair;
    g contiguous, a channel slice of a tensor 8 columns wider (bf16 stays in 16-byte lanes) and 4 columns wider (the record must show 8-byte lanes)."""
    _run_backward(m, c, dtype, pitch)


@pytest.mark.parametrize("m,c", [(53, 64), (300, 64), (37, 2048)], ids=str)
def test_bf16_alignment_fallback(m, c):
    """bf16 operands that start 8 bytes into a 16-byte aligned buffer (z, out, dz in turn) and sign bits at an odd address: the library falls back to 8-byte
    lanes (the record says vn = 4; asserted from the plan port) and the results meet the same bounds."""
    for kw in (dict(z_off=4), dict(out_off=4), dict(bits_off=1)):
        rec = _run_apply(m, c, "bf16", 1, "r", True, **kw)
        assert rec["vn"] == 4, rec
    assert _run_apply(m, c, "bf16", 1, "r", True)["vn"] == 8
    assert _run_stats(m, c, "bf16", "mean3_k", off=4)["vn"] == 4
    for kw in (dict(z_off=4), dict(dz_off=4), dict(bits_off=1)):
        first = len(_records)
        _run_backward(m, c, "bf16", "contig", modes=(4, 2), **kw)                     # (the expected width of every call is asserted inside, from the same conditions)
        recs = [r for r in _records[first:] if r["entry"] in ("bwd_apply", "bwd_pair") and not ("bits_off" in kw and r["mask_mode"] == 2)]
        assert len(recs) >= 2 and all(r["vn"] == 4 for r in recs), recs


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_outputs_untouched():
    from mvfnet_amd import _lib
    lib = _lib.lib
    m, c, dtype = 37, 64, "bf16"
    o = K.matrix_case(m, c, dtype)
    z, g = _dev(o["z"], dtype), _dev(o["gwide"][:, :c], dtype)
    y, bits = _mask_operands(o, dtype)
    bd = _bytes(bits)
    par = {k_: _p(o[k_]) for k_ in ("gamma", "mean", "invstd", "scale", "shift")}
    f = C.c_float
    ws = _ws(m, c)
    outs = [_nanv(c) for _ in range(6)]
    out, dz, dz2 = _nan((m, c), dtype), _nan((m, c), dtype), _nan((m, c), dtype)
    a = [P(par["gamma"]), P(par["mean"]), P(par["invstd"]), P(par["scale"]), P(par["shift"])]
    _refused(lib.mvf_bn_train_stats(P(z), m, 62, a[0], a[0], f(K.EPS), f(0.1), None, None, *[P(t) for t in outs[:4]], P(ws.t), ws.n, 1, None), EINVAL, "stats c % 4",
             "train_stats", *outs[:4])
    _refused(lib.mvf_bn_train_stats(P(z), m, c, a[0], a[0], f(K.EPS), f(0.1), None, None, *[P(t) for t in outs[:4]], P(ws.t), ws.n - 1, 1, None), EWS, "stats ws - 1",
             "train_stats", *outs[:4])
    _refused(lib.mvf_bn_apply_bits(P(z), m, c, a[3], a[4], P(z), a[3], None, 1, P(out), None, 1, None), EINVAL, "rscale without rshift", "apply", out)
    _refused(lib.mvf_bn_apply_bits(P(z), m, 62, a[3], a[4], None, None, None, 1, P(out), None, 1, None), EINVAL, "apply c % 4", "apply", out)
    _refused(lib.mvf_bn_apply_colmeans(P(z), m, 12, a[3], a[4], 1, P(out), P(outs[0]), P(ws.t), ws.n, 1, None), EINVAL, "colmeans c % 8", "apply_colmeans", out, outs[0])
    red = lambda mode, operand, sc, sh, gp, cc=c, nb=ws.n: lib.mvf_bn_bwd_reduce(P(g), gp, P(z), operand, m, cc, a[1], a[2], sc, sh, mode, P(dz2), P(outs[4]), P(outs[5]), P(ws.t), nb,  # noqa: E731
                                                                                 1, None)
    for mode in (1, 4):
        _refused(red(mode, None, a[3], a[4], c), EINVAL, "reduce mode %d without ymask" % mode, "bwd_reduce", dz2, outs[4], outs[5])
    for mode in (2, 3):
        _refused(red(mode, None, None, a[4], c), EINVAL, "reduce mode %d without scale" % mode, "bwd_reduce", dz2, outs[4], outs[5])
        _refused(red(mode, None, a[3], None, c), EINVAL, "reduce mode %d without shift" % mode, "bwd_reduce", dz2, outs[4], outs[5])
    _refused(red(0, None, a[3], a[4], c - 4), EINVAL, "reduce g_pitch < c", "bwd_reduce", dz2, outs[4], outs[5])
    _refused(red(0, None, a[3], a[4], c, cc=62), EINVAL, "reduce c % 4", "bwd_reduce", dz2, outs[4], outs[5])
    _refused(red(0, None, a[3], a[4], c, nb=ws.n - 1), EWS, "reduce ws - 1", "bwd_reduce", dz2, outs[4], outs[5])
    dgb = [P(par["mean"]), P(par["shift"])]                       # (any finite vectors stand in for dgamma / dbeta)
    app = lambda mode, operand, sc, sh, gp: lib.mvf_bn_bwd_apply_masked(P(g), gp, P(z), operand, m, c, a[0], a[1], a[2], sc, sh, dgb[0], dgb[1], mode, P(dz), 1, None)   # noqa: E731
    for mode in (1, 4):
        _refused(app(mode, None, a[3], a[4], c), EINVAL, "apply mode %d without ymask" % mode, "bwd_apply", dz)
        _refused(lib.mvf_bn_bwd_apply(P(g), c, P(z), m, c, a[0], a[1], a[2], a[3], a[4], dgb[0], dgb[1], mode, P(dz), 1, None), EINVAL, "mvf_bn_bwd_apply mode %d" % mode,
                 "bwd_apply", dz)
    for mode in (2, 3):
        _refused(app(mode, None, None, None, c), EINVAL, "apply mode %d without scale / shift" % mode, "bwd_apply", dz)
    _refused(app(0, None, a[3], a[4], c - 4), EINVAL, "apply g_pitch < c", "bwd_apply", dz)
    ws2 = _ws(m, c, 2)
    _refused(lib.mvf_bn_bwd_pair(P(g), c, P(z), P(z), P(bd), m, c, a[0], a[1], a[2], P(outs[0]), P(outs[1]), a[0], a[1], a[2], P(outs[2]), P(outs[3]), P(dz), P(dz2), P(ws2.t),
                                 ws2.n - 1, 1, None), EWS, "pair ws - 1", "bwd_pair", dz, dz2, *outs[:4])
    ws.check()
    ws2.check()
    # pool sums with 256 % (c / 4) != 0: test_pool_random[(2, 6, 6, 12)]
    assert lib.mvf_bn_last_launch(None) == EINVAL


# ------------------------------------------------------------------------------------------------ max pool
def _pool_expect(shape, dtype):
    n, h, w, c = shape
    vc = 4 if dtype == "f32" else 8
    fwd = "block" if (h % 4 == 0 and w % 4 == 0 and c % vc == 0 and not FORCED["pool_fwd_block"]) else "element"
    bwd = "rows" if w * (c // 4) >= 256 else "element"
    blk = h % 2 == 0 and w % 2 == 0 and c % vc == 0 and 256 % (c // vc) == 0 and c <= 256 and not FORCED["pool_bwd_block"]
    sums_ok = 256 % (c // 4) == 0
    return dict(fwd=fwd, bwd=bwd, sums="block" if blk else "rows_sums", apply="block" if blk else "rows_apply", sums_ok=sums_ok)


def _run_pool(shape, dtype, family):
    from mvfnet_amd import _lib
    lib = _lib.lib
    n, h, w, c = shape
    o = K.pool_case(shape, dtype, family)
    ho, wo, m = o["ho"], o["wo"], o["m"]
    case = "pool_%s_%dx%dx%dx%d" % ((family,) + shape)
    exp = _pool_expect(shape, dtype)
    exact = family == "lattice"
    st = (lambda x: R.round_storage(x, dtype))
    z, g = _dev(o["z"], dtype), _dev(o["g"], dtype)
    par = {k_: _p(o[k_]) for k_ in ("gamma", "mean", "invstd", "scale", "shift")}
    # forward
    y = _nan((n, ho, wo, c), dtype)
    am = torch.full((n, ho, wo, c), 0xEE, dtype=torch.uint8, device="cuda")
    rc = lib.mvf_maxpool_bn_relu_fwd(P(z), n, h, w, c, P(par["scale"]), P(par["shift"]), P(y), P(am), _dt(dtype), None)
    assert rc == 0, lib.mvf_last_error()
    _want(_rec(case + "_fwd"), entry="pool_fwd", pool=exp["fwd"], launches=1, vn=0, finalize="none")
    fw = R.maxpool_bn_relu_fwd(o["z"], o["scale"], o["shift"])
    amk = am.cpu().numpy()
    assert amk.max() < 9, "%s: an argmax byte was not written" % case
    if exact:
        assert np.array_equal(_np(y), fw["y"]), "%s: y differs from the exact result" % case
        assert np.array_equal(amk, fw["argmax"]), "%s: %d argmax bytes are not the first maximum in scan order" % (case, int((amk != fw["argmax"]).sum()))
    else:
        _elem(case, "y", _np(y), fw["y"], fw["A"], dtype)
        # the byte names a tap INSIDE the image whose activation is the stored maximum (a near tie may choose another tap than the reference's, never a smaller one)
        hp, wp = 2 * ho + 1, 2 * wo + 1
        pad_a, pad_A = np.full((n, hp, wp, c), np.nan), np.zeros((n, hp, wp, c))
        pad_a[:, 1:h + 1, 1:w + 1], pad_A[:, 1:h + 1, 1:w + 1] = fw["a"], fw["A_u"]
        at, At = np.full(fw["y"].shape, np.nan), np.zeros(fw["y"].shape)
        for k_ in range(9):
            dy, dx = divmod(k_, 3)
            at = np.where(amk == k_, pad_a[:, dy:dy + 2 * ho:2, dx:dx + 2 * wo:2], at)
            At = np.where(amk == k_, pad_A[:, dy:dy + 2 * ho:2, dx:dx + 2 * wo:2], At)
        assert np.isfinite(at).all(), "%s: %d argmax bytes name a tap outside the image" % (case, int((~np.isfinite(at)).sum()))
        _elem(case, "activation at the argmax tap against the stored y", _np(y), at, At, dtype)
    # backward, judged on the KERNEL's argmax bytes (equal to the reference's in the lattice family)
    rb = R.maxpool_bn_relu_bwd(amk, o["g"], h, w, o["z"], o["gamma"], o["mean"], o["invstd"], o["scale"], o["shift"], stored=st)
    und = rb["bn"]["undecided"].reshape(n, h, w, c)
    assert exact or und.mean() <= K.UNDECIDED_SHARE
    ga = _nan((n, h, w, c), dtype)
    rc = lib.mvf_maxpool_bn_relu_bwd(P(am), P(g), n, h, w, c, P(ga), _dt(dtype), None)
    assert rc == 0, lib.mvf_last_error()
    _want(_rec(case + "_bwd"), entry="pool_bwd", pool=exp["bwd"], launches=1)

    def check_ga(t, what):
        if exact:
            assert np.array_equal(_np(t), rb["ga"]), "%s: %s differs from the exact result" % (case, what)
        else:
            _elem(case, what, _np(t), rb["ga"], rb["A_ga"], dtype)
    check_ga(ga, "ga")
    nblk = lib.mvf_maxpool_bwd_sums_rows(n, h)
    assert nblk == (n * h + 7) // 8
    dz = _nan((n, h, w, c), dtype)
    if not exp["sums_ok"]:
        part = torch.full((c, nblk, 2), float("nan"), device="cuda")
        ga2 = _nan((n, h, w, c), dtype)
        _refused(lib.mvf_maxpool_bn_relu_bwd_sums(P(am), P(g), n, h, w, c, P(ga2), P(z), P(par["mean"]), P(par["invstd"]), P(par["scale"]), P(par["shift"]), P(part), _dt(dtype), None),
                 EUNSUPPORTED, case + "_sums", "pool_bwd_sums", part, ga2)
        _refused(lib.mvf_maxpool_bn_relu_bwd_apply(P(am), P(g), n, h, w, c, P(z), P(par["gamma"]), P(par["mean"]), P(par["invstd"]), P(par["scale"]), P(par["shift"]),
                                                   P(par["mean"]), P(par["mean"]), P(dz), _dt(dtype), None), EUNSUPPORTED, case + "_apply", "pool_bwd_apply", dz)
        return
    bn = rb["bn"]
    gst = np.abs(st(rb["ga"]))
    sl_db = _slack(und, gst)
    sl_dg = _slack(und, gst * np.abs(bn["xhat"]).reshape(n, h, w, c))
    sums = None
    for with_ga in (True, False):
        part = _Ws(c * nblk * 8)
        ga2 = _nan((n, h, w, c), dtype) if with_ga else None
        rc = lib.mvf_maxpool_bn_relu_bwd_sums(P(am), P(g), n, h, w, c, P(ga2), P(z), P(par["mean"]), P(par["invstd"]), P(par["scale"]), P(par["shift"]), P(part.t), _dt(dtype), None)
        assert rc == 0, lib.mvf_last_error()
        _want(_rec(case + "_sums" + ("_ga" if with_ga else "")), entry="pool_bwd_sums", pool=exp["sums"], part_rows=nblk, launches=1, mask_mode=2)
        part.check()
        if with_ga:
            check_ga(ga2, "ga of the sums form")
        dg, db = _nanv(c), _nanv(c)
        rc = lib.mvf_bn_bwd_finalize(P(part.t), nblk, c, P(dg), P(db), None)
        assert rc == 0, lib.mvf_last_error()
        _want(_rec(case + "_finalize"), entry="bwd_finalize", finalize="cm_wave", part_rows=nblk)
        if exact:
            assert np.array_equal(_np(db), bn["dbeta"]) and np.array_equal(_np(dg), bn["dgamma"]), "%s: the sums are not exact" % case
        else:
            _reduced(case, "pool_dbeta", dtype, _np(db), bn["dbeta"], slack=sl_db)
            _reduced(case, "pool_dgamma", dtype, _np(dg), bn["dgamma"], slack=sl_dg)
        sums = (_np(dg), _np(db)) if sums is None else sums
        if not with_ga:
            assert np.array_equal(_np(dg), sums[0]) and np.array_equal(_np(db), sums[1]), "%s: the sums change with a materialised ga" % case
    # the re-gathering apply form.  lattice: zero sums, gamma = invstd = 1 -> dz IS the ReLU-masked gradient, bit for bit
    dgk, dbk = (np.zeros(c), np.zeros(c)) if exact else sums
    rk = R.maxpool_bn_relu_bwd(amk, o["g"], h, w, o["z"], o["gamma"], o["mean"], o["invstd"], o["scale"], o["shift"], dgk, dbk, stored=st)["bn"]
    dgd, dbd = _p(dgk), _p(dbk)
    rc = lib.mvf_maxpool_bn_relu_bwd_apply(P(am), P(g), n, h, w, c, P(z), P(par["gamma"]), P(par["mean"]), P(par["invstd"]), P(par["scale"]), P(par["shift"]), P(dgd), P(dbd),
                                           P(dz), _dt(dtype), None)
    assert rc == 0, lib.mvf_last_error()
    _want(_rec(case + "_apply"), entry="pool_bwd_apply", pool=exp["apply"], launches=1, mask_mode=2)
    if exact:
        assert np.array_equal(_np(dz), rk["gm"].reshape(n, h, w, c)), "%s: the ReLU-masked gradient differs from the exact result" % case
    else:
        _elem(case, "dz", _np(dz), rk["dz"].reshape(n, h, w, c), rk["A_dz"].reshape(n, h, w, c), dtype, und)


@pytest.mark.parametrize("dtype", K.DTYPES)
@pytest.mark.parametrize("shape", K.POOL_SHAPES, ids=str)
def test_pool_lattice(shape, dtype):
    """Exact inputs: y, the argmax byte (first maximum in scan order, positive ties and all-zero windows included), ga, the backward sums and the ReLU-masked
    gradient bit for bit, in every pool form the shape reaches."""
    _run_pool(shape, dtype, "lattice")


@pytest.mark.parametrize("dtype", K.DTYPES)
@pytest.mark.parametrize("shape", K.POOL_SHAPES, ids=str)
def test_pool_random(shape, dtype):
    """Gaussian inputs with batch statistics: y, ga, dgamma / dbeta of the sums form + mvf_bn_bwd_finalize (with and without a materialised ga), dz of the apply form."""
    _run_pool(shape, dtype, "random")


# ------------------------------------------------------------------------------------------------ forced policy legs
# leg -> (policy, the cases the child re-runs, check(records) that the forced form ran and the form it replaces did not)
LEGS = {
    "bn_spec=0": (dict(bn_spec=0), "test_backward", lambda rs: {r["spec"] for r in rs if r["entry"] in ("bwd_reduce", "bwd_apply") and r["launches"]} == {0} and
                  {r["mask_mode"] for r in rs if r["entry"] == "bwd_reduce"} == {0, 1, 2, 3, 4}),
    "pool_fwd_block=0": (dict(pool_fwd_block=0), "test_pool", lambda rs: {r["pool"] for r in rs if r["entry"] == "pool_fwd"} == {"element"} and
                         "block" in {r["pool"] for r in rs if r["entry"] == "pool_bwd_sums"}),
    "pool_bwd_block=0": (dict(pool_bwd_block=0), "test_pool", lambda rs: {r["pool"] for r in rs if r["entry"] == "pool_bwd_sums" and r["launches"]} == {"rows_sums"} and
                         {r["pool"] for r in rs if r["entry"] == "pool_bwd_apply" and r["launches"]} == {"rows_apply"} and
                         "block" in {r["pool"] for r in rs if r["entry"] == "pool_fwd"}),
}
_leg_results = {}


def _abnormal(rc):
    return rc < 0 or rc in (124, 134, 137, 139)


def _run_leg(leg, tmp_dir):
    """This module's backward or pool cases again in a fresh child process under the leg's policy (the switches are read once per process).  The children run
    serially, each under its own time limit; after a child that exits abnormally (a signal, an abort, its time limit) no further child is started."""
    if leg in _leg_results:
        return _leg_results[leg]
    stopped = [k_ for k_, v in _leg_results.items() if _abnormal(v[0])]
    if stopped:
        _leg_results[leg] = (1, "not started: the child of leg %s exited abnormally" % stopped[0], [])
        return _leg_results[leg]
    policy, select, _ = LEGS[leg]
    cov = os.path.join(str(tmp_dir), "coverage_%d.jsonl" % list(LEGS).index(leg))
    env = policy_env(**policy)
    env[COVERAGE_ENV] = cov
    try:
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-m", "gpu", "-k", select, "-p", "no:cacheprovider"], env=env, capture_output=True,
                           text=True, timeout=300)
        rc, tail = r.returncode, r.stdout[-3000:] + r.stderr[-2000:]
    except subprocess.TimeoutExpired as e:
        rc, tail = 124, "time limit: %s" % e
    recs = [json.loads(line) for line in open(cov)] if os.path.exists(cov) else []
    _leg_results[leg] = (rc, tail, recs)
    return _leg_results[leg]


@pytest.fixture(scope="module")
def leg_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("bn_pool_legs")


@pytest.mark.parametrize("leg", list(LEGS))
def test_forced_policy_legs(leg, leg_dir):
    if not DEFAULT_POLICY:
        pytest.skip("a forced leg's child does not start children of its own")
    rc, tail, recs = _run_leg(leg, leg_dir)
    assert rc == 0, tail
    assert recs and LEGS[leg][2](recs), "policy %s did not reach the forms it names: %s" % (leg, sorted({(r["entry"], r["spec"], r["pool"]) for r in recs}))


# ------------------------------------------------------------------------------------------------ coverage under the default policy
def test_coverage_summary_of_the_default_policy():
    """Every form is reached at least once under the default policy (a minimal set of the cases above, run here so that the test stands alone): both bf16 lane
    widths, the five mask modes specialised, the three finalize forms, the five pool forms.  Prints the summary."""
    if not DEFAULT_POLICY:
        pytest.skip("the forms of the default policy")
    first = len(_records)
    _run_backward(300, 64, "bf16", "contig", pair=True)
    _run_backward(37, 12, "bf16", "contig", modes=(2,), pair=False)
    _run_stats(300, 64, "f32", "mean3_k")
    for nblk in (1023, 1024):
        test_finalize_layouts(4, nblk)
    for shape in ((2, 5, 4, 64), (2, 8, 12, 64), (3, 7, 16, 64)):
        _run_pool(shape, "bf16", "lattice")
    rs = [r for r in _records[first:] if r["launches"]]
    seen = dict(bf16_lane_widths=sorted({r["vn"] for r in rs if r["dtype"] == 1 and r["vn"]}),
                mask_modes_specialised=sorted({r["mask_mode"] for r in rs if r["entry"] in ("bwd_reduce", "bwd_apply") and r["spec"] == 1}),
                finalize_forms=sorted({r["finalize"] for r in rs} - {"none"}), pool_forms=sorted({r["pool"] for r in rs} - {"none"}))
    print("coverage under the default policy (reached):")
    for k_, v in seen.items():
        print("  %s: %s" % (k_, ", ".join(str(x) for x in v)))
    assert seen == dict(bf16_lane_widths=[4, 8], mask_modes_specialised=[0, 1, 2, 3, 4], finalize_forms=["cm_wave", "cm_workgroup", "row_major"],
                        pool_forms=["block", "element", "rows", "rows_apply", "rows_sums"]), seen
