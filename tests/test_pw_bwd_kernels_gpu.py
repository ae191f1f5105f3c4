"""GPU: the five fused pointwise-conv backward kernels through the C ABI against the INDEPENDENT fp64 reference tests/pw_bwd_ref.py (proved against torch
float64 autograd in tests/test_pw_bwd_ref_cpu.py): mvf_conv1x1_bwd_fused (csrc/pw_bwd_fused.hip), mvf_conv1x1_bnbwd_sums_pair (csrc/pw_sums_pair.hip), the
two passes of csrc/pw_sums.hip (reached through mvf_conv2d_nhwc_fwd_stats with y = NULL and mvf_conv2d_nhwc_fwd_bnbwd_sums), mvf_bn_bwd_apply_wgrad and
mvf_bn_bwd_pair_wgrad (csrc/bnbwd_wgrad.hip, all seven template instances) and mvf_wgrad_slab_reduce -- at the smallest row counts that reach each state of
the chunk pipelines (tests/pw_bwd_cases.py), under the default launch plans in this process and under forced one- and two-workgroup plans in one child
process per leg (the switches are read once per process).  The bit-identity tests between fused and un-fused paths (tests/test_pw_bwd_fused_gpu.py,
tests/test_train_gpu.py) complement this module and stay.

Conventions (those of test_bn_pool_kernels_gpu.py and test_wgrad_families_gpu.py).  Operands are rounded to bf16 on the CPU and the reference is evaluated on
exactly those values.  Every output is NaN before the call.  Slab buffers are exactly splits * c * k floats (mvf_bn_bwd_wgrad_slab_bytes where the entry
documents that), partial-row buffers exactly [c][rows][2], each followed by a 4 KiB NaN canary that must be unchanged.  A pitched tensor holds finite data in
every column of the pitch; a sliced operand starts at a column offset (a multiple of 8 elements) inside a wider allocation.  Inputs keep the reductions well
conditioned (pw_bwd_cases: mean / invstd are the batch statistics of the reference's rounded conv output, g is correlated with xhat, dgamma / dbeta handed to an
apply pass are the fp64 sums of the case).  Gates taken from an input (mask mode 2, bn2's gate of the fused kernel): z is repaired on the CPU until
|scale z + shift| > 1e-3, asserted before the launch; no element is left out of any comparison.  Plans: every case asserts that mvf_conv1x1_bwd_fused_splits /
mvf_bn_bwd_wgrad_splits return what the Python ports in pw_bwd_cases give under the policy of this process (CU count from torch), and for pw_sums that the
conv launch record names the family the port expects.

Bounds.
  dz of bnbwd_wgrad (every input observable; the pair form is fed the KERNEL's dgamma / dbeta): |got - ref| <= 2^-8 |ref| + 8 * 2^-24 * A.
  Weight gradients from a stored dz (bnbwd_wgrad): wgrad_ref on the kernel's own dz, rel_err and rel_l2 < 2e-6, per slab over that split's rows and for
  the reduced dw.
  Sums: per workgroup, value row + remainder row, against the fp64 sum over exactly the rows / blocks the plan port assigns to it; rows beyond 2 nwg of the
  pw_sums layout exactly zero; sums over a tensor the kernel stored (bn2's over dx) are taken over the stored values.
  Quantities behind a conv output or dz3 that is never stored: the allowance of the undecided roundings comes from the reference alone (pw_bwd_ref: z3
  within 2e-5 max|z3| of a rounding midpoint, dz3 within 8 * 2^-24 A plus what an undecided z3 moves it; one ulp of its effect each: ulp(dz3) |W| or
  ulp(dz3) |a2| for an undecided dz3 and ulp(z3) |d dz3 / d z3| |W| or |a2| for an undecided z3), on top of 6e-3 (dx) or 2e-6 (slabs, dw); every
  allowance < 1 % of the largest magnitude it is added to, asserted before the launch (largest measured: 0.5 %).
  Reduced quantities with no derived bound (partial rows, finalized dgamma / dbeta, the pw_sums statistics): BOUNDS = 4 x the largest error measured over
  all cases and legs (the summation order changes with the plan), never above the existing tests' bounds (CAPS) and never below 4 * 2^-24;
  profiles/pw_bwd_errors.txt has the measurements (MVF_PW_BWD_ERRORS=file dumps them, tools/pw_bwd_errors_table.py prints the table).

What the module found is in the docstrings of the tests concerned."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import conv_epilogue_ref as E
import pw_bwd_cases as K
import pw_bwd_ref as R
from helpers import policy_env, policy_set

pytestmark = pytest.mark.gpu

ERRORS_ENV = "MVF_PW_BWD_ERRORS"            # a file: one JSON line per measured quantity (tooling: profiles/pw_bwd_errors.txt)
LEG_ENV = "MVF_PW_BWD_LEG"                  # set in a forced leg's child: the leg's name
FLOOR, CAPS = K.FLOOR, K.CAPS
# (kernel, quantity) -> 4 x the largest figure of profiles/pw_bwd_errors.txt (tools/pw_bwd_errors_table.py prints this table)
BOUNDS = {
    ("fused", "bn2_part_s1"): 2.38e-07,
    ("fused", "bn2_part_s2"): 3.63e-07,
    ("fused", "bn2_dbeta"): 2.38e-07,
    ("fused", "bn2_dgamma"): 3.94e-07,
    ("pair", "part_s1"): 2.38e-07,
    ("pair", "part_s2"): 2.38e-07,
    ("pair", "dbeta"): 2.38e-07,
    ("pair", "dgamma"): 2.38e-07,
    ("pair_wgrad", "dbeta"): 2.38e-07,
    ("pair_wgrad", "dgamma"): 4.95e-07,
    ("pw_sums", "k0_part_s1"): 2.38e-07,
    ("pw_sums", "k0_part_s2"): 2.38e-07,
    ("pw_sums", "k0_total_s1"): 2.38e-07,
    ("pw_sums", "k0_total_s2"): 2.38e-07,
    ("pw_sums", "k_part_s1"): 2.38e-07,
    ("pw_sums", "k_part_s2"): 2.38e-07,
    ("pw_sums", "k_total_s1"): 2.38e-07,
    ("pw_sums", "k_total_s2"): 2.38e-07,
    ("pw_sums", "bwd_part_s1"): 2.38e-07,
    ("pw_sums", "bwd_part_s2"): 2.38e-07,
    ("pw_sums", "bwd_total_s1"): 2.38e-07,
    ("pw_sums", "bwd_total_s2"): 2.38e-07,
}
CANARY = 4096
EINVAL, ESHAPE, EWS, EUNSUPPORTED = -1, -2, -3, -5
_reached = set()
_tag = {}


def _bound(kernel, q, cap):
    return max(FLOOR, min(BOUNDS.get((kernel, q), CAPS[cap]), CAPS[cap]))


def _note(kernel, case, q, fig):
    rec = dict(kernel=kernel, case=case, quantity=q, policy=os.environ.get("MVF_POLICY", ""), **fig)
    rec.update(_tag)
    if os.environ.get(ERRORS_ENV):
        with open(os.environ[ERRORS_ENV], "a") as f_:
            f_.write(json.dumps(rec) + "\n")
    print("%s %s %s: %s" % (kernel, case, q, " ".join("%s %.3g" % kv for kv in sorted(fig.items()))))


def _cmp(kernel, case, q, got, ref, base, allow=None, l2=True):
    """pw_bwd_cases.cmp_tensor with the figures printed and dumped BEFORE the assertion."""
    try:
        fig = K.cmp_tensor("%s %s %s" % (kernel, case, q), got, ref, base, allow, l2)
    except AssertionError:
        g_, r_ = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
        if g_.shape == r_.shape and np.isfinite(g_).all():
            d = np.abs(g_ - r_)
            al = np.zeros(r_.shape) if allow is None else allow
            s = max(float(np.abs(r_).max()), 1e-300)
            _note(kernel, case, q, dict(rel_err=float(d.max()) / s, net_err=float(np.maximum(d - al, 0).max()) / s, allow=float(np.max(al)) / s, bound=base, failed=1.0))
        raise
    _note(kernel, case, q, fig)
    return fig


def _red(kernel, case, q, bq, cap, got, ref, allow=None):
    """A reduced quantity with a MEASURED bound: BOUNDS[(kernel, bq)] within [4 * 2^-24, CAPS[cap]]; the dump names the key (tools/pw_bwd_errors_table.py)."""
    global _tag
    _tag = dict(bound_key=bq, cap=cap)
    try:
        return _cmp(kernel, case, q, got, ref, _bound(kernel, bq, cap), allow)
    finally:
        _tag = {}


# ------------------------------------------------------------------------------------------------ device buffers
def P(t):
    return C.c_void_p(t if isinstance(t, int) else t.data_ptr()) if t is not None else C.c_void_p(0)


def _bf(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(torch.bfloat16).cuda()


def _fp(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).float().cuda()


def _u8(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).cuda()


class _Placed(object):
    """A bf16 operand [M][C] inside its [M][pitch] allocation at a column offset: .ptr is the address of element (0, 0) of the operand."""

    def __init__(self, a, pitch, off=0):
        self.buf = _bf(K.pitched(a, pitch, off))
        self.pitch = pitch
        self.ptr = self.buf.data_ptr() + 2 * off


def _place_x(a, place):
    pf, off = K.A_PLACE[place]
    return _Placed(a, pf(a.shape[1]), off)


def _place_g(a, place):
    return _Placed(a, K.G_PLACE[place](a.shape[1]))


class _Out(object):
    """n elements of NaN (fp32 or bf16) followed by a 4 KiB NaN canary that must come back unchanged."""

    def __init__(self, n, dtype=torch.float32):
        es = 4 if dtype == torch.float32 else 2
        self.n = n
        self.t = torch.full((n + CANARY // es,), float("nan"), dtype=dtype, device="cuda")
        self.bits = self.t[n:].clone().view(torch.int16)

    def np(self, shape=None):
        torch.cuda.synchronize()
        assert torch.equal(self.t[self.n:].view(torch.int16), self.bits), "the canary behind an output was written"
        a = self.t[:self.n].double().cpu().numpy()
        return a if shape is None else a.reshape(shape)

    def untouched(self):
        return bool(np.isnan(self.np()).all())


def _lib():
    from mvfnet_amd import _lib
    return _lib.lib


def _ok(rc, what):
    assert rc == 0, "%s: rc %d: %s" % (what, rc, _lib().mvf_last_error())


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _finalize(part_t, rows, c):
    dg, db = torch.full((c,), float("nan"), device="cuda"), torch.full((c,), float("nan"), device="cuda")
    _ok(_lib().mvf_bn_bwd_finalize(P(part_t), rows, c, P(dg), P(db), None), "bn_bwd_finalize")
    torch.cuda.synchronize()
    return dg.double().cpu().numpy(), db.double().cpu().numpy()


def _share(case, what, allow, ref):
    s = K.allowance_share(allow, ref)
    assert s < K.ALLOW_SHARE, "%s: the allowance of %s is %.3g of the largest magnitude" % (case, what, s)
    return s


# ------------------------------------------------------------------------------------------------ mvf_conv1x1_bwd_fused
def _run_fused(m, seed, with_bn, a_place, g_place):
    lib = _lib()
    o, ref = K.conv_case(m, seed), K.fused_ref(m, seed, with_bn)
    b2 = o["bn2"]
    case = "m%d_s%d_%s_a-%s_g-%s" % (m, seed, "zin" if with_bn else "nozin", a_place, g_place)
    ns, rows = K.fused_plan(m)
    assert lib.mvf_conv1x1_bwd_fused_splits(m, K.NC, K.NK) == ns and ns > 0, (case, lib.mvf_conv1x1_bwd_fused_splits(m, K.NC, K.NK), ns)
    bounds = K.split_bounds(m, rows)
    # conditions, from the reference alone
    assert float(E.gate_margin(b2["z"], b2["scale"], b2["shift"]).min()) > K.GATE_MARGIN
    _share(case, "dx", ref["allow_dx"], ref["dx"])
    slab_ref = [R.wgrad(ref["dz"], o["a"], be) for be in bounds]
    slab_allow = [ref["u_dz"][b:e].T @ np.abs(o["a"][b:e]) for b, e in bounds]
    for (dw_, _), al in zip(slab_ref, slab_allow):
        _share(case, "a slab", al, dw_)
    dw_ref = R.wgrad(ref["dz"], o["a"])[0]
    dw_allow = ref["u_dz"].T @ np.abs(o["a"])
    _share(case, "dw", dw_allow, dw_ref)
    a, g = _place_x(o["a"], a_place), _place_g(o["g"], g_place)
    w, bits, z2 = _bf(o["w"]), _u8(o["bits"]), _bf(b2["z"])
    par = {k_: _fp(o[k_]) for k_ in ("gamma", "mean", "invstd", "dgamma", "dbeta")}
    p2 = {k_: _fp(b2[k_]) for k_ in ("mean", "invstd", "scale", "shift")}
    dx, spart, slabs = _Out(m * K.NK, torch.bfloat16), _Out(K.NK * 2 * ns * 2), _Out(ns * K.NC * K.NK)
    n_ = (lambda t: P(t) if with_bn else None)
    _ok(lib.mvf_conv1x1_bwd_fused(P(a.ptr), a.pitch, P(w), P(g.ptr), g.pitch, P(bits), m, K.NC, K.NK, P(par["gamma"]), P(par["mean"]), P(par["invstd"]), P(par["dgamma"]),
                                  P(par["dbeta"]), n_(z2), n_(p2["mean"]), n_(p2["invstd"]), n_(p2["scale"]), n_(p2["shift"]), P(dx.t), n_(spart.t), 2 * ns if with_bn else 0,
                                  P(slabs.t), slabs.n * 4, 1, None), case)
    _reached.add("fused:%s" % ("z_in" if with_bn else "no_z_in"))
    got_dx = dx.np((m, K.NK))
    _cmp("fused", case, "dx", got_dx, ref["dx"], 6e-3, ref["allow_dx"], l2=False)
    got_slabs = slabs.np((ns, K.NC, K.NK))
    worst = None
    for i, ((dw_, _), al) in enumerate(zip(slab_ref, slab_allow)):
        fig = K.cmp_tensor("fused %s slab %d of %d (rows %s)" % (case, i, ns, bounds[i]), got_slabs[i], dw_, 2e-6, al)
        worst = fig if worst is None else {k_: max(worst[k_], fig[k_]) for k_ in fig}
    _note("fused", case, "slabs (largest over %d)" % ns, worst)
    dw = _Out(K.NC * K.NK)
    _ok(lib.mvf_wgrad_slab_reduce(P(slabs.t), ns, K.NC, K.NK, P(dw.t), None), "slab_reduce")
    _cmp("fused", case, "dw", dw.np((K.NC, K.NK)), dw_ref, 2e-6, dw_allow)
    if not with_bn:
        assert spart.untouched(), "%s: z_in = NULL wrote the partial rows" % case
        return
    # bn2's sums over what the kernel STORED
    v1, v2 = R.gated_sums(got_dx, b2["z"], b2["mean"], b2["invstd"], b2["scale"], b2["shift"])
    got = K.part_rows("fused %s sums_part" % case, spart.np((K.NK, 2 * ns, 2)), ns)
    _red("fused", case, "bn2_part_s1", "bn2_part_s1", "fused", got[:, :, 0], R.rows_sum(v1, bounds))
    _red("fused", case, "bn2_part_s2", "bn2_part_s2", "fused", got[:, :, 1], R.rows_sum(v2, bounds))
    dg2, db2 = _finalize(spart.t, 2 * ns, K.NK)
    _red("fused", case, "bn2_dbeta", "bn2_dbeta", "fused", db2, v1.sum(axis=0))
    _red("fused", case, "bn2_dgamma", "bn2_dgamma", "fused", dg2, v2.sum(axis=0))


@pytest.mark.parametrize("m,seed,with_bn,a_place,g_place", K.fused_cases(), ids=lambda v: str(v))
def test_conv1x1_bwd_fused(m, seed, with_bn, a_place, g_place):
    """dx, every weight-gradient slab, the reduced dw, bn2's partial rows per workgroup and the finalized sums; z_in = NULL leaves sums_part NaN.
    Found at M = 40017 (the first three-chunk walk): with ulp(dz3) alone as an undecided element's contribution, slab 1 of 209 lay 2.57e-6 of its scale
    outside the allowance (bound 2e-6).  Not the kernel: an fp32 evaluation of the same expressions in numpy gives the kernel's value to 8 digits.  Where
    z3 ~ 4 is undecided and the element is gated off, dz3 ~ 0.01 moves by ulp(z3) |d dz3 / d z3| = up to 45 of ITS ulps, so that term is part of an
    undecided z3's effect (pw_bwd_ref.conv1x1_bwd_fused); with it the same evaluation stays within 1e-11 and the allowance below 0.5 %."""
    _run_fused(m, seed, with_bn, a_place, g_place)


# ------------------------------------------------------------------------------------------------ mvf_conv1x1_bnbwd_sums_pair
def _run_pair(m, seed, branches, a_place, x_place, g_place):
    lib = _lib()
    o = K.conv_case(m, seed)
    case = "m%d_s%d_br%d_a-%s_x-%s_g-%s" % (m, seed, branches, a_place, x_place, g_place)
    ns, rows = K.fused_plan(m)
    assert lib.mvf_conv1x1_bwd_fused_splits(m, K.NC, K.NK) == ns and ns > 0
    bounds = K.split_bounds(m, rows)
    refs = [o["pair_a"], o["pair_b"]][:branches]
    for r in refs:
        _share(case, "a partial of sum gm xhat", R.rows_sum(r["allow2"], bounds), R.rows_sum(r["v2"], bounds))
        _share(case, "dgamma", r["allow2"].sum(axis=0), r["v2"].sum(axis=0))
    a, x, g = _place_x(o["a"], a_place), _place_x(o["a_b"], x_place), _place_g(o["g_pair"], g_place)
    wa, wb, bits = _bf(o["w"]), _bf(o["w_b"]), _u8(o["bits"])
    par = {k_: _fp(o[k_]) for k_ in ("mean", "invstd", "mean_b", "invstd_b")}
    pa, pb = _Out(K.NC * 2 * ns * 2), _Out(K.NC * 2 * ns * 2)
    two = branches == 2
    _ok(lib.mvf_conv1x1_bnbwd_sums_pair(P(a.ptr), a.pitch, P(wa), P(x.ptr) if two else None, x.pitch if two else 0, P(wb) if two else None, P(g.ptr), g.pitch, P(bits), m,
                                        K.NC, K.NK, P(par["mean"]), P(par["invstd"]), P(par["mean_b"]) if two else None, P(par["invstd_b"]) if two else None, P(pa.t),
                                        P(pb.t) if two else None, 2 * ns, 1, None), case)
    _reached.add("pair:%d" % branches)
    if two:          # the one-branch form is bit-identical to branch a of the pair
        p1 = _Out(K.NC * 2 * ns * 2)
        _ok(lib.mvf_conv1x1_bnbwd_sums_pair(P(a.ptr), a.pitch, P(wa), None, 0, None, P(g.ptr), g.pitch, P(bits), m, K.NC, K.NK, P(par["mean"]), P(par["invstd"]), None, None,
                                            P(p1.t), None, 2 * ns, 1, None), case + " (x_in = NULL)")
        torch.cuda.synchronize()
        assert torch.equal(p1.t[:p1.n], pa.t[:pa.n]), "%s: the one-branch sums differ from branch a of the pair" % case
    else:
        assert pb.untouched()
    for name, part, r in (("a", pa, o["pair_a"]), ("b", pb, o["pair_b"]))[:branches]:
        got = K.part_rows("pair %s part_%s" % (case, name), part.np((K.NC, 2 * ns, 2)), ns)
        _red("pair", case, "part_%s_s1" % name, "part_s1", "pair_s1", got[:, :, 0], R.rows_sum(r["v1"], bounds))
        _red("pair", case, "part_%s_s2" % name, "part_s2", "pair_s2", got[:, :, 1], R.rows_sum(r["v2"], bounds), R.rows_sum(r["allow2"], bounds))
        dg, db = _finalize(part.t, 2 * ns, K.NC)
        _red("pair", case, "dbeta_%s" % name, "dbeta", "pair_s1", db, r["v1"].sum(axis=0))
        _red("pair", case, "dgamma_%s" % name, "dgamma", "pair_s2", dg, r["v2"].sum(axis=0), r["allow2"].sum(axis=0))


@pytest.mark.parametrize("m,seed,branches,a_place,x_place,g_place", K.pair_cases(), ids=lambda v: str(v))
def test_conv1x1_bnbwd_sums_pair(m, seed, branches, a_place, x_place, g_place):
    """Both branches' partial rows per workgroup and the finalized dgamma / dbeta; x_in = NULL bit-identical to branch a."""
    _run_pair(m, seed, branches, a_place, x_place, g_place)


# ------------------------------------------------------------------------------------------------ csrc/bnbwd_wgrad.hip
def _check_slabs(kernel, case, slabs, ns, c, k, bounds, dz_got, x, reduce_too=True):
    got = slabs.np()[:ns * c * k].reshape(ns, c, k)
    worst = None
    for i, be in enumerate(bounds):
        fig = K.cmp_tensor("%s %s slab %d of %d (rows %s)" % (kernel, case, i, ns, be), got[i], R.wgrad(dz_got, x, be)[0], 2e-6)
        worst = fig if worst is None else {k_: max(worst[k_], fig[k_]) for k_ in fig}
    _note(kernel, case, "slabs (largest over %d)" % ns, worst)
    dw = _Out(c * k)
    _ok(_lib().mvf_wgrad_slab_reduce(P(slabs.t), ns, c, k, P(dw.t), None), "slab_reduce")
    _cmp(kernel, case, "dw", dw.np((c, k)), R.wgrad(dz_got, x)[0], 2e-6)


def _run_bnwg(mode, c, k, m, g_place, x_place):
    lib = _lib()
    o = K.bnwg_case(m, c, k, mode)
    case = "mode%d_c%d_k%d_m%d_g-%s_x-%s" % (mode, c, k, m, g_place, x_place)
    ns, rows, ct, kt = K.bnwg_plan(m, c, k, 1, mode)
    assert lib.mvf_bn_bwd_wgrad_splits(m, c, k, 1, mode) == ns and ns > 0, (case, lib.mvf_bn_bwd_wgrad_splits(m, c, k, 1, mode), ns)
    nbytes = lib.mvf_bn_bwd_wgrad_slab_bytes(m, c, k, 1, mode)
    assert nbytes >= ns * c * k * 4 and nbytes % 4 == 0
    if mode == 2:
        assert float(E.gate_margin(o["z"], o["scale"], o["shift"]).min()) > K.GATE_MARGIN
    g, x = _place_g(o["g"], g_place), _place_x(o["x"], x_place)
    z, bits = _bf(o["z"]), _u8(o["bits"])
    par = {k_: _fp(o[k_]) for k_ in ("gamma", "mean", "invstd", "scale", "shift", "dgamma", "dbeta")}
    dz, slabs = _Out(m * c, torch.bfloat16), _Out(nbytes // 4)
    _ok(lib.mvf_bn_bwd_apply_wgrad(P(g.ptr), g.pitch, P(z), P(bits), m, c, P(par["gamma"]), P(par["mean"]), P(par["invstd"]), P(par["scale"]), P(par["shift"]), P(par["dgamma"]),
                                   P(par["dbeta"]), mode, P(dz.t), P(x.ptr), x.pitch, k, P(slabs.t), nbytes, 1, None), case)
    tile = K.bnwg_tile(c, k, 1, mode)
    _reached.add("bnwg:%dx%d:nbn1:nx1:mode%d" % (tile[0], tile[1], mode))
    ref = R.bn_bwd_apply_wgrad(o["g"], o["z"], o["bits"], mode, o["gamma"], o["mean"], o["invstd"], o["scale"], o["shift"], o["dgamma"], o["dbeta"])
    assert not ref["undecided"].any() or mode != 2
    got = dz.np((m, c))
    _note("bnwg", case, "dz", dict(worst_over_bound=K.cmp_elem("bnwg %s dz" % case, got, ref["dz_exact"], ref["A_dz"])))
    _check_slabs("bnwg", case, slabs, ns, c, k, K.split_bounds(m, rows), got, o["x"])


@pytest.mark.parametrize("mode,c,k,m,g_place,x_place", K.bnwg_cases(), ids=lambda v: str(v))
def test_bn_bwd_apply_wgrad(mode, c, k, m, g_place, x_place):
    """dz elementwise, every slab against the weight gradient of the kernel's own stored dz over that split's rows, and the reduced dw."""
    _run_bnwg(mode, c, k, m, g_place, x_place)


def _run_pair_wgrad(c, k, with_xb, m, g_place, x_place):
    lib = _lib()
    o = K.bnwg_case(m, c, k, 4, pair=True)
    case = "c%d_k%d_%s_m%d_g-%s_x-%s" % (c, k, "xb" if with_xb else "noxb", m, g_place, x_place)
    ns, rows, ct, kt = K.bnwg_plan(m, c, k, 2, 4)
    assert lib.mvf_bn_bwd_wgrad_splits(m, c, k, 2, 4) == ns and ns > 0
    nbytes = lib.mvf_bn_bwd_wgrad_slab_bytes(m, c, k, 2, 4)
    wsb = 2 * lib.mvf_bn_workspace_bytes(m, c)
    g, xa, xb = _place_g(o["g"], g_place), _place_x(o["x"], x_place), _place_x(o["x_b"], x_place)
    za, zb, bits = _bf(o["z"]), _bf(o["z_b"]), _u8(o["bits"])
    par = {k_: _fp(o[k_]) for k_ in ("gamma", "mean", "invstd", "gamma_b", "mean_b", "invstd_b")}
    sums = [_Out(c) for _ in range(4)]
    dza, dzb = _Out(m * c, torch.bfloat16), _Out(m * c, torch.bfloat16)
    sa, sb, ws = _Out(nbytes // 4), _Out(nbytes // 4), _Out(wsb // 4)
    _ok(lib.mvf_bn_bwd_pair_wgrad(P(g.ptr), g.pitch, P(za), P(zb), P(bits), m, c, P(par["gamma"]), P(par["mean"]), P(par["invstd"]), P(sums[0].t), P(sums[1].t),
                                  P(par["gamma_b"]), P(par["mean_b"]), P(par["invstd_b"]), P(sums[2].t), P(sums[3].t), P(dza.t), P(dzb.t), P(xa.ptr), xa.pitch,
                                  P(xb.ptr) if with_xb else None, xb.pitch if with_xb else 0, k, P(sa.t), P(sb.t) if with_xb else None, nbytes, P(ws.t), wsb, 1, None), case)
    tile = K.bnwg_tile(c, k, 2, 4)
    _reached.add("bnwg:%dx%d:nbn2:nx%d:mode4" % (tile[0], tile[1], 2 if with_xb else 1))
    ws.np()
    got = [s.np() for s in sums]
    ra, rb_ = o["ref_pair"]
    for name, r, dg, db in (("a", ra, got[0], got[1]), ("b", rb_, got[2], got[3])):
        _red("pair_wgrad", case, "dbeta_%s" % name, "dbeta", "pair_wgrad", db, r["dbeta"])
        _red("pair_wgrad", case, "dgamma_%s" % name, "dgamma", "pair_wgrad", dg, r["dgamma"])
    ka, kb = R.bn_bwd_pair_wgrad(o["g"], o["z"], o["z_b"], o["bits"], o["gamma"], o["mean"], o["invstd"], o["gamma_b"], o["mean_b"], o["invstd_b"], (got[0], got[1]),
                                 (got[2], got[3]))
    bounds = K.split_bounds(m, rows)
    ga, gb = dza.np((m, c)), dzb.np((m, c))
    _note("pair_wgrad", case, "dz_a", dict(worst_over_bound=K.cmp_elem("pair_wgrad %s dz_a" % case, ga, ka["dz_exact"], ka["A_dz"])))
    _note("pair_wgrad", case, "dz_b", dict(worst_over_bound=K.cmp_elem("pair_wgrad %s dz_b" % case, gb, kb["dz_exact"], kb["A_dz"])))
    _check_slabs("pair_wgrad", case + " conv a", sa, ns, c, k, bounds, ga, o["x"])
    if with_xb:
        _check_slabs("pair_wgrad", case + " conv b", sb, ns, c, k, bounds, gb, o["x_b"])
    else:
        assert sb.untouched()


@pytest.mark.parametrize("c,k,with_xb,m,g_place,x_place", K.pair_wgrad_cases(), ids=lambda v: str(v))
def test_bn_bwd_pair_wgrad(c, k, with_xb, m, g_place, x_place):
    """The sums against the reference, both dz fed the kernel's own sums, the slabs of one or both convs and their reduced dw."""
    _run_pair_wgrad(c, k, with_xb, m, g_place, x_place)


# ------------------------------------------------------------------------------------------------ csrc/pw_sums.hip through the conv ABI
def _conv_family():
    from mvfnet_amd import _lib
    info = _lib.ConvLaunchInfo()
    _lib.check(_lib.lib.mvf_conv2d_last_launch(C.byref(info)))
    return _lib.CONV_FAMILIES[info.family]


def _run_pw_sums(m, n, x_place, what, wgs):
    from mvfnet_amd import _lib
    lib = _lib.lib
    o = K.pw_sums_case(m, n)
    r = o["ref"][what]
    case = "m%d_n%d_x-%s_%s%s" % (m, n, x_place, what, "" if wgs is None else "_wgs%d" % wgs)
    x = _place_x(o["a"], x_place)
    d = _lib.ConvDesc(1, m, 1, K.NK, n, 1, 1, 1, 0, m, 1, x.pitch, 1, 0, 0, 0, 0, 0)
    rows = lib.mvf_conv2d_stats_rows(C.byref(d))
    assert rows == K.stats_rows(m)
    w, g, bits = _bf(o["w"]), _bf(o["g"]), _u8(o["bits"])
    par = {k_: _fp(o[k_]) for k_ in ("mean", "invstd", "kshift")}
    part = _Out(n * rows * 2)
    with policy_set(**({} if wgs is None else dict(pw_sums_wgs=wgs))):
        nwg = K.pw_sums_nwg(m, n, rows, _cus())
        if what == "bwd":
            _ok(lib.mvf_conv2d_nhwc_fwd_bnbwd_sums(C.byref(d), P(x.ptr), None, P(w), P(g), P(bits), P(par["mean"]), P(par["invstd"]), P(part.t), None, 0, None), case)
        else:
            _ok(lib.mvf_conv2d_nhwc_fwd_stats(C.byref(d), P(x.ptr), None, P(w), None, P(part.t), P(par["kshift"]) if what == "k" else None, None, 0, None), case)
    fam = _conv_family()
    assert (fam == "pw_sums") == (nwg > 0), "%s: the launch record says %s, the plan port %d workgroups" % (case, fam, nwg)
    a1 = r.get("allow1", np.zeros(r["v1"].shape))
    a2 = r["allow2"]
    got_all = part.np((n, rows, 2))
    if nwg:
        _reached.add("pw_sums:%s:n%d" % ("mode1" if what == "bwd" else "mode0", n))
        blocks = K.pw_sums_blocks(m, nwg)
        ref1, ref2 = R.blocks_sum(r["v1"], blocks), R.blocks_sum(r["v2"], blocks)
        al1, al2 = R.blocks_sum(a1, blocks), R.blocks_sum(a2, blocks)
        got = K.part_rows("pw_sums %s" % case, got_all, nwg)
    else:            # the implicit GEMM's layout: one partial row per 128 output rows (tests/test_conv_epilogues_gpu.py has its own tests; its bounds)
        runs = [(b, min(m, b + 128)) for b in range(0, m, 128)]
        ref1, ref2, al1, al2 = (R.rows_sum(v, runs) for v in (r["v1"], r["v2"], a1, a2))
        assert np.isfinite(got_all).all()
        got = got_all
    _share(case, "a partial of sum 1", al1, ref1)
    _share(case, "a partial of sum 2", al2, ref2)
    if not nwg:
        _cmp("implicit_gemm", case, what + "_part_s1", got[:, :, 0], ref1, 1e-4, al1)
        _cmp("implicit_gemm", case, what + "_part_s2", got[:, :, 1], ref2, 1e-4 if what == "bwd" else 1e-5, al2)
    else:
        _red("pw_sums", case, what + "_part_s1", what + "_part_s1", "pw_sums", got[:, :, 0], ref1, al1)
        _red("pw_sums", case, what + "_part_s2", what + "_part_s2", "pw_sums", got[:, :, 1], ref2, al2)
        tot = got_all.sum(axis=1)
        _red("pw_sums", case, what + "_total_s1", what + "_total_s1", "pw_sums", tot[:, 0], r["v1"].sum(axis=0), a1.sum(axis=0))
        _red("pw_sums", case, what + "_total_s2", what + "_total_s2", "pw_sums", tot[:, 1], r["v2"].sum(axis=0), a2.sum(axis=0))
    return nwg


@pytest.mark.parametrize("m,n,x_place,what,wgs", K.pw_sums_cases(), ids=lambda v: str(v))
def test_pw_sums(m, n, x_place, what, wgs):
    """The statistics pass (K = NULL, K = a running mean near the batch mean) and the BatchNorm-backward sums of a conv that stores nothing: the partial-row
    layout (value rows, remainder rows, zero rows), the block walk of every workgroup, the ragged last block, both N, pitched and sliced inputs.  M = 1920
    (15 partial rows: fewer than 8 workgroups) goes to the implicit GEMM and is still checked.  M = 2047 has 16 partial rows like M = 2048 and does reach
    csrc/pw_sums.hip, with a ragged last block: the port and the launch record agree on that."""
    nwg = _run_pw_sums(m, n, x_place, what, wgs)
    if wgs is None:
        assert nwg == {2048: 8, 2047: 8, 1920: 0, 2225: 8, 40017: 152}[m], nwg


# ------------------------------------------------------------------------------------------------ mvf_wgrad_slab_reduce
@pytest.mark.parametrize("nsplit", K.SLAB_SPLITS)
def test_wgrad_slab_reduce(nsplit):
    """Synthetic slabs against their fp64 sum: a fixed-order fp32 sum of nsplit terms errs by at most nsplit * 2^-24 * sum |terms| per element."""
    s = K.slab_case(nsplit)
    t = _fp(s)
    dw = _Out(K.NC * K.NK)
    _ok(_lib().mvf_wgrad_slab_reduce(P(t), nsplit, K.NC, K.NK, P(dw.t), None), "slab_reduce")
    got, ref = dw.np((K.NC, K.NK)), s.sum(axis=0)
    tol = nsplit * 2.0 ** -24 * np.abs(s).sum(axis=0)
    assert np.isfinite(got).all() and (np.abs(got - ref) <= tol).all(), float((np.abs(got - ref) / tol).max())
    _reached.add("slab_reduce")


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_the_outputs_untouched():
    """Arguments the entries reject before any launch (csrc/train_ops.hip): a non-zero return code and outputs still NaN.  mvf_bn_bwd_wgrad_splits is 0 for
    (96, 64) and (1024, 256, mode 2); for (256, 128, two BatchNorms) it is NOT 0 -- that shape is built with x_b = NULL -- and the call WITH x_b is what is
    refused."""
    lib = _lib()
    m = 209
    o = K.conv_case(m)
    b2 = o["bn2"]
    ns, _ = K.fused_plan(m)
    a, a72, g, w, bits, z2 = _bf(o["a"]), _bf(K.pitched(o["a"], 72, 0)), _bf(o["g"]), _bf(o["w"]), _u8(o["bits"]), _bf(b2["z"])
    par = [_fp(o[k_]) for k_ in ("gamma", "mean", "invstd", "dgamma", "dbeta")]
    p2 = [_fp(b2[k_]) for k_ in ("mean", "invstd", "scale", "shift")]
    dx, spart, slabs = _Out(m * K.NK, torch.bfloat16), _Out(K.NK * 2 * ns * 2), _Out(ns * K.NC * K.NK)

    def fused(a_ptr=a.data_ptr(), ap=K.NK, gp=K.NC, mm=m, c=K.NC, k=K.NK, rows=2 * ns, sb=slabs.n * 4, dt=1, g_ptr=g.data_ptr()):
        rc = lib.mvf_conv1x1_bwd_fused(P(a_ptr), ap, P(w), P(g_ptr), gp, P(bits), mm, c, k, *[P(t) for t in par], P(z2), *[P(t) for t in p2], P(dx.t), P(spart.t), rows,
                                       P(slabs.t), sb, dt, None)
        assert dx.untouched() and spart.untouched() and slabs.untouched(), "a refused call wrote an output"
        return rc
    assert fused(dt=0) == EUNSUPPORTED
    assert fused(a_ptr=a72.data_ptr(), ap=68) == ESHAPE                     # a pitch that is no multiple of 8
    assert fused(a_ptr=a.data_ptr() + 8) == ESHAPE                          # an operand 8 bytes into its 16-byte lane
    assert fused(g_ptr=g.data_ptr() + 8) == ESHAPE
    assert fused(rows=2 * ns + 1) == EINVAL and fused(rows=ns) == EINVAL
    assert fused(sb=slabs.n * 4 - 4) == EWS
    assert fused(c=512, k=128, ap=128, gp=512) == EUNSUPPORTED and fused(c=256, k=128, ap=128) == EUNSUPPORTED
    assert lib.mvf_conv1x1_bwd_fused_splits(m, 512, 128) == 0 and lib.mvf_conv1x1_bwd_fused_splits(m, 256, 128) == 0
    big = 0x7ffffff0 // (2 * 520) + 1                                       # m * g_pitch * 2 >= 0x7ffffff0 while m * 256 * 2 is below: refused on the numbers alone
    assert big * 256 * 2 < 0x7ffffff0 <= big * 520 * 2 and lib.mvf_conv1x1_bwd_fused_splits(big, K.NC, K.NK) > 0
    nsb = lib.mvf_conv1x1_bwd_fused_splits(big, K.NC, K.NK)
    assert fused(mm=big, gp=520, rows=2 * nsb, sb=1 << 40) == ESHAPE
    # the sums pair
    pa, pb = _Out(K.NC * 2 * ns * 2), _Out(K.NC * 2 * ns * 2)
    q = [_fp(o[k_]) for k_ in ("mean", "invstd", "mean_b", "invstd_b")]
    xb, wb = _bf(o["a_b"]), _bf(o["w_b"])          # (any finite g serves a call that is refused)

    def pair(a_ptr=a.data_ptr(), ap=K.NK, xp=K.NK, gp=K.NC, mm=m, rows=2 * ns, dt=1):
        rc = lib.mvf_conv1x1_bnbwd_sums_pair(P(a_ptr), ap, P(w), P(xb), xp, P(wb), P(g), gp, P(bits), mm, K.NC, K.NK, *[P(t) for t in q], P(pa.t), P(pb.t), rows, dt, None)
        assert pa.untouched() and pb.untouched(), "a refused call wrote an output"
        return rc
    assert pair(dt=0) == EUNSUPPORTED
    assert pair(xp=68) == ESHAPE and pair(a_ptr=a.data_ptr() + 8) == ESHAPE
    assert pair(rows=2 * ns + 2) == EINVAL
    assert pair(mm=big, gp=520, rows=2 * nsb) == ESHAPE
    # BatchNorm backward + weight gradient
    assert lib.mvf_bn_bwd_wgrad_splits(m, 96, 64, 1, 4) == 0 and lib.mvf_bn_bwd_wgrad_splits(m, 1024, 256, 1, 2) == 0
    assert lib.mvf_bn_bwd_wgrad_splits(m, 256, 128, 2, 4) == K.bnwg_plan(m, 256, 128, 2, 4)[0] > 0
    c, k = 256, 64
    ob = K.bnwg_case(m, c, k, 4, pair=True)
    nsw = K.bnwg_plan(m, c, k, 1, 4)[0]
    nbytes = lib.mvf_bn_bwd_wgrad_slab_bytes(m, c, k, 1, 4)
    gg, z, zb_, bb, x, x2 = _bf(ob["g"]), _bf(ob["z"]), _bf(ob["z_b"]), _u8(ob["bits"]), _bf(ob["x"]), _bf(ob["x_b"])
    pr = {k_: _fp(ob[k_]) for k_ in ("gamma", "mean", "invstd", "dgamma", "dbeta", "gamma_b", "mean_b", "invstd_b")}
    dz, dzb, sl, sl2 = _Out(m * c, torch.bfloat16), _Out(m * c, torch.bfloat16), _Out(nbytes // 4), _Out(nbytes // 4)

    def app(g_ptr=gg.data_ptr(), gp=c, xp=k, cc=c, kk=k, mode=4, sb=nbytes, dt=1, mm=m):
        rc = lib.mvf_bn_bwd_apply_wgrad(P(g_ptr), gp, P(z), P(bb), mm, cc, P(pr["gamma"]), P(pr["mean"]), P(pr["invstd"]), None, None, P(pr["dgamma"]), P(pr["dbeta"]), mode,
                                        P(dz.t), P(x), xp, kk, P(sl.t), sb, dt, None)
        assert dz.untouched() and sl.untouched(), "a refused call wrote an output"
        return rc
    assert app(dt=0) == EUNSUPPORTED
    assert app(gp=c + 4) == ESHAPE and app(xp=k + 4) == ESHAPE and app(g_ptr=gg.data_ptr() + 8) == ESHAPE
    assert app(sb=nsw * c * k * 4 - 4) == EWS
    assert app(cc=96, gp=96) == EUNSUPPORTED
    assert app(mode=2) == EINVAL                                            # mode 2 without scale / shift
    assert app(mode=1) == EUNSUPPORTED
    bigw = 0x7ffffff0 // (2 * 520) + 1
    assert app(mm=bigw, gp=520, sb=1 << 40) == ESHAPE
    wsb = 2 * lib.mvf_bn_workspace_bytes(m, c)
    ws = _Out(wsb // 4)
    sums = [_Out(c) for _ in range(4)]

    def pairw(kk=k, with_xb=True, xp=k, wb_=wsb, dt=1, sb=nbytes):
        rc = lib.mvf_bn_bwd_pair_wgrad(P(gg), c, P(z), P(zb_), P(bb), m, c, P(pr["gamma"]), P(pr["mean"]), P(pr["invstd"]), P(sums[0].t), P(sums[1].t), P(pr["gamma_b"]),
                                       P(pr["mean_b"]), P(pr["invstd_b"]), P(sums[2].t), P(sums[3].t), P(dz.t), P(dzb.t), P(x), xp, P(x2) if with_xb else None, xp, kk,
                                       P(sl.t), P(sl2.t), sb, P(ws.t), wb_, dt, None)
        assert dz.untouched() and dzb.untouched() and sl.untouched() and sl2.untouched() and all(s.untouched() for s in sums) and ws.untouched(), "a refused call wrote an output"
        return rc
    assert pairw(dt=0) == EUNSUPPORTED
    assert pairw(wb_=wsb - 1) == EWS
    assert pairw(xp=k + 4) == ESHAPE
    assert pairw(sb=nsw * c * k * 4 - 4) == EWS
    assert pairw(kk=128, xp=128, sb=1 << 40) == EUNSUPPORTED               # (256, 128) with x_b: both convs are contracted for k = 64 only
    assert lib.mvf_wgrad_slab_reduce(None, 1, c, k, P(dz.t), None) == EINVAL and lib.mvf_wgrad_slab_reduce(P(sl.t), 0, c, k, P(dz.t), None) == EINVAL
    assert dz.untouched()


# ------------------------------------------------------------------------------------------------ forced split plans
# leg -> row count -> the chunks each workgroup of the fused / pair walker must walk (by hand; the bnbwd_wgrad walker at one column tile walks the same)
LEG_CHUNKS = {
    "one_workgroup": {17: [1], 209: [4], 401: [7], 448: [7], 465: [8]},
    "two_workgroups": {17: [1], 209: [2, 2], 401: [4, 3], 448: [4, 3], 465: [4, 4]},
}


@pytest.mark.parametrize("m", K.LEG_ROWS)
def test_rows_of_the_forced_legs(m):
    """The row counts of the forced legs through every chunk walker: here under the plan of this process; in a leg's child under the forced plan, asserted
    through the splits functions (a leg whose port and library disagree fails)."""
    leg = os.environ.get(LEG_ENV)
    if leg:
        lib = _lib()
        assert K.policy_int("pwbf_wgs", 256) == K.policy_int("bnwg_wgs", 256) == K.LEGS[leg]["pwbf_wgs"]
        ns, rows = K.fused_plan(m)
        assert K.chunks_of(m, rows) == LEG_CHUNKS[leg][m] and lib.mvf_conv1x1_bwd_fused_splits(m, K.NC, K.NK) == ns == len(LEG_CHUNKS[leg][m])
        nw, rw, _, _ = K.bnwg_plan(m, 256, 64, 1, 4)
        assert lib.mvf_bn_bwd_wgrad_splits(m, 256, 64, 1, 4) == nw
        sizes = [e - b for b, e in K.split_bounds(m, rw)]
        assert sizes == ([m] if leg == "one_workgroup" or m <= 256 else [256, m - 256]), (leg, m, sizes)          # (two: 256 | 145, 256 | 192, 256 | 209)
    _run_fused(m, 0, True, "contig", "contig")
    _run_fused(m, 0, False, "k+8", "c+8")
    _run_pair(m, 0, 2, "contig", "contig", "contig")
    for mode, c, k in K.BNWG_SHAPES:
        _run_bnwg(mode, c, k, m, "contig", "contig")
    for c, k, xb in K.PAIR_WGRAD_SHAPES:
        _run_pair_wgrad(c, k, xb, m, "contig", "contig")


_leg_results = {}


def _abnormal(rc):
    return rc < 0 or rc in (124, 134, 137, 139)


def _run_leg(leg):
    """test_rows_of_the_forced_legs again in a fresh child process under the leg's policy.  The children run serially, each under its own time limit; after a
    child that exits abnormally (a signal, an abort, its time limit) no further child is started."""
    if leg in _leg_results:
        return _leg_results[leg]
    stopped = [k_ for k_, v in _leg_results.items() if _abnormal(v[0])]
    if stopped:
        _leg_results[leg] = (1, "not started: the child of leg %s exited abnormally" % stopped[0])
        return _leg_results[leg]
    env = policy_env(**K.LEGS[leg])
    env[LEG_ENV] = leg
    try:
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-m", "gpu", "-k", "test_rows_of_the_forced_legs", "-p", "no:cacheprovider"],
                           env=env, capture_output=True, text=True, timeout=300)
        rc, tail = r.returncode, r.stdout[-3000:] + r.stderr[-2000:]
    except subprocess.TimeoutExpired as e:
        rc, tail = 124, "time limit: %s" % e
    _leg_results[leg] = (rc, tail)
    return _leg_results[leg]


@pytest.mark.parametrize("leg", list(K.LEGS))
def test_forced_split_plans(leg):
    """pwbf_wgs = bnwg_wgs = 1: one workgroup walks 1, 4, 7, 7 and 8 chunks (odd and even counts, ragged and exact tails, both buffer parities at the tail);
    = 2: splits 256 | 145 and 256 | 209."""
    assert not os.environ.get(LEG_ENV), "a leg's child starts no children of its own"
    rc, tail = _run_leg(leg)
    assert rc == 0, tail
    assert "5 passed" in tail, tail


# ------------------------------------------------------------------------------------------------ what was reached
REACHED = {"fused:z_in", "fused:no_z_in", "pair:1", "pair:2", "slab_reduce", "pw_sums:mode0:n128", "pw_sums:mode0:n256", "pw_sums:mode1:n128", "pw_sums:mode1:n256",
           "bnwg:256x64:nbn1:nx1:mode4", "bnwg:256x128:nbn1:nx1:mode4", "bnwg:64x256:nbn1:nx1:mode2", "bnwg:128x256:nbn1:nx1:mode2", "bnwg:256x64:nbn2:nx2:mode4",
           "bnwg:256x64:nbn2:nx1:mode4", "bnwg:256x128:nbn2:nx1:mode4"}


def test_every_entry_point_and_instance_is_reached():
    """Every entry point, every bnbwd_wgrad instance, both pw_sums modes and both N (a minimal set of the cases above, run here so that the test stands
    alone).  Prints the reached set."""
    _reached.clear()
    m = 209
    _run_fused(m, 0, True, "contig", "contig")
    _run_fused(m, 0, False, "contig", "contig")
    _run_pair(m, 0, 2, "contig", "contig", "contig")
    _run_pair(m, 0, 1, "contig", "contig", "contig")
    for mode, c, k in K.BNWG_SHAPES:
        _run_bnwg(mode, c, k, m, "contig", "contig")
    for c, k, xb in K.PAIR_WGRAD_SHAPES:
        _run_pair_wgrad(c, k, xb, m, "contig", "contig")
    for n in (128, 256):
        for what in ("k", "bwd"):
            _run_pw_sums(2048, n, "contig", what, None)
    test_wgrad_slab_reduce(2)
    print("reached: %s" % ", ".join(sorted(_reached)))
    assert _reached == REACHED, (sorted(REACHED - _reached), sorted(_reached - REACHED))
