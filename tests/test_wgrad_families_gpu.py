"""GPU: every kernel path of the conv weight gradient (mvf_conv2d_nhwc_wgrad / _wgs: csrc/wgrad_nhwc.hip, wgrad3x3_c64.hip, wgrad_stem.hip) through the C ABI
against the INDEPENDENT fp64 reference tests/wgrad_ref.py (proved against torch in tests/test_wgrad_ref_cpu.py), at the smallest shapes at which the kernels
can still go wrong, in both storage types -- in this process under the default launch policy, and again in one child process per forced policy so that every
family x tile x storage type x split-operand instance is reached.  After every call the host-side launch record (mvf_conv2d_wgrad_last_launch) says which
kernel ran and with which pixel split; under the default policy each case asserts the family, tile, nsplit, rows per split and XCD map it was chosen for.

Operands are rounded to the storage type on the CPU and the reference is evaluated on exactly those values, so the only admissible error is fp32
accumulation.  dw is NaN before the call, the workspace is exactly mvf_conv2d_wgrad_workspace_bytes of NaN plus a 4 KiB canary that must be unchanged.

Bound: helpers.rel_err < 2e-6 AND helpers.rel_l2 < 2e-6 for both storage types and every family -- the project's own bound for fp32 accumulation
(test_fp32_weight_gradient_on_the_bf16_matrix_cores_..., which holds at up to 3136 pixels per split; every split here is shorter) -- except the direct
stem kernel, which keeps the 2e-5 of its existing test.  Measured values: profiles/wgrad_errors.txt."""
import collections
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import wgrad_ref as R
from helpers import policy_env, rel_err, rel_l2

pytestmark = pytest.mark.gpu

COVERAGE_ENV = "MVF_WGRAD_COVERAGE"       # a file: this module appends one JSON line per weight-gradient call (the forced legs' children; tooling)
ERRORS_ENV = "MVF_WGRAD_ERRORS"           # a file: one JSON line per measured error (tooling: profiles/wgrad_errors.txt)
BOUND, BOUND_STEM = 2e-6, 2e-5
# the plans asserted per case are those of the DEFAULT policy: a child of a forced leg (or a caller's own MVF_POLICY) checks the arithmetic only
DEFAULT_POLICY = not any(k in os.environ.get("MVF_POLICY", "").lower() for k in ("wgrad", "gram_wgs", "f32_x3"))

# n h w = the input map; xps = pixel pitch of x (0: cin); split = split_c, x2ps = pitch of x2
Geo = collections.namedtuple("Geo", "n h w cin cout k stride xps split x2ps")
# what the launch record must say under the default policy
Plan = collections.namedtuple("Plan", "family tile nsplit xcd_rr")


def _g(n, h, w, cin, cout, k, stride, xps=0, split=0, x2ps=0):
    return Geo(n, h, w, cin, cout, k, stride, xps or cin, split, x2ps)


def _gid(g):
    s = "n%d_%dx%d_c%d_o%d_k%d_s%d" % g[:7]
    if g.xps != g.cin:
        s += "_pitch%d" % g.xps
    if g.split:
        s += "_split%d_pitch%d" % (g.split, g.x2ps)
    return s


def _out_hw(g):
    p = g.k // 2
    return (g.h + 2 * p - g.k) // g.stride + 1, (g.w + 2 * p - g.k) // g.stride + 1


T64, T128x64, T128, T256 = (64, 128), (128, 64), (128, 128), (256, 256)
# Every default plan below has 256-row splits: plan_split never goes below 256 rows, and no shape here has more than 256 rows per workgroup aimed at.
# (geometry, {storage type: plan})
POINTWISE = [
    (_g(2, 9, 7, 64, 256, 1, 1), dict(bf16=Plan("bf16_reg", T128x64, 1, 0), f32=Plan("x3", T128x64, 1, 0))),             # M = 126: one ragged chunk; K <= 64
    (_g(3, 6, 6, 128, 96, 1, 1), dict(bf16=Plan("bf16_pipe/3", T128, 1, 0), f32=Plan("x3", T128, 1, 0))),               # ragged cout tile
    (_g(5, 5, 5, 32, 64, 1, 1), dict(bf16=Plan("bf16_reg", T64, 1, 0), f32=Plan("x3", T64, 1, 0))),                     # tile wider than K; K < 128: no bf16 DMA
    (_g(1, 14, 14, 256, 1024, 1, 1), dict(bf16=Plan("t256_p4", T256, 1, 0), f32=Plan("x3", T128, 1, 0))),               # M = 196: 3 full 64-row chunks + 4 rows
    (_g(3, 10, 10, 512, 256, 1, 1), dict(bf16=Plan("t256_p4", T256, 2, 0), f32=Plan("x3", T128, 2, 0))),                # M = 300: 256 + 44, shorter than the pipeline
    (_g(2, 10, 13, 256, 256, 1, 1), dict(bf16=Plan("t256_p4", T256, 2, 0), f32=Plan("x3", T128, 2, 0))),                # M = 260: a 4-row last split
    (_g(2, 32, 32, 64, 64, 1, 1), dict(bf16=Plan("bf16_reg", T64, 8, 1), f32=Plan("x3", T64, 8, 1))),                   # M = 2048: 8 splits -> round-robin XCD map
    (_g(150, 1, 1, 64, 64, 1, 1), dict(bf16=Plan("bf16_reg", T64, 1, 0), f32=Plan("x3", T64, 1, 0))),                   # 1 x 1 maps
]
CONV3 = [
    (_g(2, 9, 9, 32, 64, 3, 1), dict(bf16=Plan("bf16_pipe/3", T64, 1, 0), f32=Plan("x3", T64, 1, 0))),
    (_g(2, 7, 7, 132, 36, 3, 1), dict(bf16=Plan("bf16_widen", T64, 1, 0), f32=Plan("x3", T64, 1, 0))),                  # bf16 cin % 8 != 0: the widening kernel
    (_g(3, 2, 33, 64, 96, 3, 1), dict(bf16=Plan("bf16_pipe/3", T128, 1, 0), f32=Plan("x3", T128, 1, 0))),
    (_g(2, 13, 11, 256, 256, 3, 2), dict(bf16=Plan("t256_p4", T256, 1, 0), f32=Plan("x3", T128, 1, 0))),                # stride 2, odd map
    (_g(5, 13, 11, 128, 64, 3, 2), dict(bf16=Plan("bf16_pipe/3", T64, 1, 0), f32=Plan("x3", T64, 1, 0))),
]
# beyond the shapes the issue lists: the widening kernel's other two tiles, and x_pix_stride > cin on the implicit GEMM (three loaders)
EXTRA = [
    (_g(2, 7, 7, 132, 132, 3, 1), dict(bf16=Plan("bf16_widen", T128, 1, 0), f32=Plan("x3", T128, 1, 0))),
    (_g(3, 5, 5, 36, 132, 1, 1), dict(bf16=Plan("bf16_widen", T128x64, 1, 0), f32=Plan("x3", T128x64, 1, 0))),
    (_g(3, 6, 6, 128, 96, 1, 1, xps=136), dict(bf16=Plan("bf16_pipe/3", T128, 1, 0), f32=Plan("x3", T128, 1, 0))),
    (_g(5, 5, 5, 32, 64, 1, 1, xps=48), dict(bf16=Plan("bf16_reg", T64, 1, 0), f32=Plan("x3", T64, 1, 0))),
    (_g(3, 2, 33, 64, 96, 3, 1, xps=72), dict(bf16=Plan("bf16_pipe/3", T128, 1, 0), f32=Plan("x3", T128, 1, 0))),
    (_g(2, 10, 13, 256, 256, 1, 1, xps=264), dict(bf16=Plan("t256_p4", T256, 2, 0), f32=Plan("x3", T128, 2, 0))),
]
# direct 3x3 (bf16, 64 -> 64 channels): nsplit = one slab per workgroup = min(512, n * ceil(h / 3) bands); the last is refused by the predicate (w > 56)
DIRECT3 = [
    (_g(3, 7, 12, 64, 64, 3, 1), Plan("c3x3_c64", (64, 576), 9, 0)),
    (_g(1, 5, 4, 64, 64, 3, 1), Plan("c3x3_c64", (64, 576), 2, 0)),                 # minimum width
    (_g(1, 4, 56, 64, 64, 3, 1), Plan("c3x3_c64", (64, 576), 2, 0)),                # maximum width
    (_g(4, 13, 8, 64, 64, 3, 1, xps=128), Plan("c3x3_c64", (64, 576), 20, 0)),      # a channel slice of a wider tensor
    (_g(1, 4, 60, 64, 64, 3, 1), Plan("bf16_pipe/3", T64, 1, 0)),                   # w = 60: the implicit GEMM
]
# the stem (bf16; (n, h, w) of the IMAGE): nsplit = min(768, n * ho / 2 bands); wo = 20 is refused by the predicate: M = 800, two tiles, 256 workgroups aimed at
STEM = [
    ((2, 32, 32), Plan("stem", (64, 224), 16, 0)),                                    # wo = 16, the minimum
    ((3, 64, 64), Plan("stem", (64, 224), 48, 0)),
    ((5, 32, 64), Plan("stem", (64, 224), 40, 0)),
    ((2, 40, 40), Plan("bf16_pipe/3", T64, 4, 0)),
]
# split operand, pointwise, M = 300; x2 pitch = split_c + 8.  The last is beyond the issue's list: the 64-wide tile with a split the LDS-DMA loaders take
SPLIT = [
    (_g(3, 10, 10, 256, 64, 1, 1, split=64, x2ps=72), dict(bf16=Plan("bf16_reg", T64, 2, 0), f32=Plan("x3", T64, 2, 0))),           # split % tile width != 0
    (_g(3, 10, 10, 256, 128, 1, 1, split=128, x2ps=136), dict(bf16=Plan("bf16_pipe/3", T128, 2, 0), f32=Plan("x3", T128, 2, 0))),   # LDS-DMA
    (_g(3, 10, 10, 512, 256, 1, 1, split=256, x2ps=264), dict(bf16=Plan("t256_p4", T256, 2, 0), f32=Plan("x3", T128, 2, 0))),       # the 256 x 256 tile
    (_g(3, 10, 10, 256, 64, 1, 1, split=128, x2ps=136), dict(bf16=Plan("bf16_pipe/3", T64, 2, 0), f32=Plan("x3", T64, 2, 0))),
]
GRAM = [(64, dict(bf16=Plan("bf16_reg", T64, 2, 0), f32=Plan("x3", T64, 2, 0))), (256, dict(bf16=Plan("t256_p4", T256, 2, 0), f32=Plan("x3", T128, 2, 0)))]
WGS_SHAPE = _g(2, 32, 32, 64, 64, 1, 1)
WS_CASE = _g(2, 100, 100, 512, 512, 1, 1)
DTYPES = ["f32", "bf16"]


def _cases(lst):
    return [pytest.param(g, plans, id=_gid(g)) for g, plans in lst]


# ------------------------------------------------------------------------------------------------ operands and references (one per shape and storage type, shared, never modified)
_ops_cache = {}


def _round(t, dtype):
    return t.to(torch.bfloat16 if dtype == "bf16" else torch.float32)


def _ops(g, dtype):
    key = (g, dtype)
    if key in _ops_cache:
        return _ops_cache[key]
    gen = torch.Generator().manual_seed(sum(g))
    ho, wo = _out_hw(g)
    o = {"ho": ho, "wo": wo, "m": g.n * ho * wo}
    o["x"] = _round(torch.randn(g.n, g.h, g.w, g.xps, generator=gen), dtype)            # (every column of the pitch holds data: a pitch mistake shows)
    o["dz"] = _round(torch.randn(g.n, ho, wo, g.cout, generator=gen), dtype)
    o["x2"] = _round(torch.randn(g.n, g.h, g.w, g.x2ps, generator=gen), dtype) if g.split else None
    x2 = o["x2"].double().numpy() if g.split else None
    o["ref"], o["absref"] = R.wgrad(o["dz"].double().numpy(), o["x"].double().numpy(), g.n, g.h, g.w, g.cin, g.k, g.k, g.stride, g.k // 2, x_pix_stride=g.xps,
                                    x2=x2, split_c=g.split, x2_pix_stride=g.x2ps)
    o["gpu"] = {k_: (v.cuda() if isinstance(v, torch.Tensor) else None) for k_, v in o.items() if k_ in ("x", "dz", "x2")}
    _ops_cache[key] = o
    return o


def _stem_ops(shape):
    """The stem's operand as mvf_stem_prep lays it out, (n, h + 6, w + 8, 4) bf16, zero padded -- with data in the fourth channel and in the two columns only
    the eighth packed tap reads: both are dropped by the unpacking (kw_real = 7, cin_real = 3)."""
    key = ("stem", shape)
    if key in _ops_cache:
        return _ops_cache[key]
    n, h, w = shape
    gen = torch.Generator().manual_seed(h * 7 + w)
    hp, wp, ho, wo = h + 6, w + 8, h // 2, w // 2
    xp = torch.zeros(n, hp, wp, 4)
    xp[:, 3:3 + h, 3:3 + w, :3] = torch.randn(n, h, w, 3, generator=gen)
    xp[:, :, :, 3] = torch.randn(n, hp, wp, generator=gen)
    xp[:, :, w + 6:, :] = torch.randn(n, hp, 2, 4, generator=gen)
    o = {"hp": hp, "wp": wp, "ho": ho, "wo": wo, "m": n * ho * wo}
    o["x"] = xp.to(torch.bfloat16)
    o["dz"] = torch.randn(n, ho, wo, 64, generator=gen).to(torch.bfloat16)
    o["ref"], o["absref"] = R.wgrad_stem(o["dz"].double().numpy(), o["x"].double().numpy(), n, hp, wp)
    o["gpu"] = {"x": o["x"].cuda(), "dz": o["dz"].cuda(), "x2": None}
    _ops_cache[key] = o
    return o


# ------------------------------------------------------------------------------------------------ the call
def _P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _desc(g, dtype):
    from mvfnet_amd import _lib
    ho, wo = _out_hw(g)
    return _lib.ConvDesc(g.n, g.h, g.w, g.cin, g.cout, g.k, g.k, g.stride, g.k // 2, ho, wo, g.xps, _lib.MVF_F32 if dtype == "f32" else _lib.MVF_BF16, 0, g.split, g.x2ps,
                         0, 0, 0)


def _stem_desc(n, o):
    from mvfnet_amd import _lib
    return _lib.ConvDesc(n, o["hp"], o["wp"], 32, 64, 7, 1, 2, 0, o["ho"], o["wo"], 4, _lib.MVF_BF16, 0, 0, 0, 0, 0, 0)


CANARY = 4096


def _record(entry, shape, dtype):
    from mvfnet_amd import _lib
    info = _lib.WgradLaunchInfo()
    _lib.check(_lib.lib.mvf_conv2d_wgrad_last_launch(C.byref(info)))
    fam = _lib.WGRAD_FAMILIES[info.family]
    if fam == "bf16_pipe":
        fam += "/%d" % info.stages
    rec = dict(entry=entry, shape=shape, dtype=dtype, family=fam, tile=[info.tile_co, info.tile_k], rec_dtype=info.dtype, nsplit=info.nsplit, rows=info.rows_per_split,
               xcd_rr=info.xcd_rr, split=info.split_operand, gram=info.gram, wgs_target=info.wgs_target, launches=info.launches)
    if os.environ.get(COVERAGE_ENV):
        with open(os.environ[COVERAGE_ENV], "a") as f_:
            f_.write(json.dumps(rec) + "\n")
    return rec


def _call(entry, shape, dtype, d, G, dw_shape, packed, wgs=None, ws_short=0, expect_rc=0):
    """One weight-gradient call: dw all NaN before, the workspace exactly as published (NaN) + a canary tail.  Returns (dw as fp64 numpy, launch record)."""
    from mvfnet_amd import _lib
    lib = _lib.lib
    nbytes = lib.mvf_conv2d_wgrad_workspace_bytes(C.byref(d))
    assert nbytes > 0 and nbytes % 256 == 0
    ws = torch.empty(nbytes + CANARY, dtype=torch.uint8, device="cuda")
    ws[:nbytes] = 0xFF                                   # (fp32 NaN: a slab region that is summed without having been written shows in dw)
    ws[nbytes:] = 0xA5
    dw = torch.full(dw_shape, float("nan"), device="cuda")
    args = (C.byref(d), _P(G["dz"]), _P(G["x"]), _P(G["x2"])) + tuple(packed) + (_P(dw), _P(ws), nbytes - ws_short)
    rc = lib.mvf_conv2d_nhwc_wgrad(*(args + (None,))) if wgs is None else lib.mvf_conv2d_nhwc_wgrad_wgs(*(args + (wgs, None)))
    rec = _record(entry, shape, dtype)
    torch.cuda.synchronize()
    assert bool((ws[nbytes:] == 0xA5).all()), "the workspace was written past mvf_conv2d_wgrad_workspace_bytes"
    got = dw.double().cpu().numpy()
    if expect_rc:
        assert rc == expect_rc, (rc, lib.mvf_last_error())
        assert rec["launches"] == 0 and rec["family"] == "none", rec
        assert np.isnan(got).all(), "a refused call wrote dw"
        return got, rec
    assert rc == 0, lib.mvf_last_error()
    assert rec["launches"] == 2 and rec["family"] != "none", rec
    assert rec["rec_dtype"] == (_lib.MVF_F32 if dtype == "f32" else _lib.MVF_BF16)
    assert np.isfinite(got).all(), "%d of %d dw elements are not finite (never written, or summed from an unwritten slab)" % (int((~np.isfinite(got)).sum()), got.size)
    return got, rec


def _compare(entry, shape, dtype, rec, got, o):
    bound = BOUND_STEM if rec["family"] == "stem" else BOUND
    ref = o["ref"]
    e_max, e_l2 = rel_err(got, ref), rel_l2(got, ref)
    # (diagnostics: the worst element's error against ITS OWN sum of |dz| |x| -- what an fp32 accumulation error is proportional to)
    e_abs = float((np.abs(got - ref) / np.maximum(o["absref"], 1e-30)).max())
    if os.environ.get(ERRORS_ENV):
        with open(os.environ[ERRORS_ENV], "a") as f_:
            f_.write(json.dumps(dict(entry=entry, shape=shape, dtype=dtype, family=rec["family"], tile=rec["tile"], split=rec["split"], nsplit=rec["nsplit"], rows=rec["rows"],
                                     rel_err=e_max, rel_l2=e_l2, rel_abs=e_abs, bound=bound, policy=os.environ.get("MVF_POLICY", ""))) + "\n")
    print("%s %s %s %s tile %s nsplit %d x %d rows: rel_err %.3g rel_l2 %.3g (bound %.3g), vs sum|dz||x| %.3g" % (entry, shape, dtype, rec["family"], rec["tile"], rec["nsplit"],
                                                                                                              rec["rows"], e_max, e_l2, bound, e_abs))
    assert e_max < bound and e_l2 < bound, "%s %s %s on %s: rel_err %.3g, rel_l2 %.3g (bound %.3g)" % (entry, shape, dtype, rec, e_max, e_l2, bound)


def _assert_plan(rec, plan, rows=256, split=0, gram=0, wgs_target=None):
    if not DEFAULT_POLICY:
        return
    assert (rec["family"], tuple(rec["tile"]), rec["nsplit"], rec["xcd_rr"]) == tuple(plan), (rec, plan)
    assert rec["rows"] == rows and rec["split"] == split and rec["gram"] == gram, rec
    if wgs_target is not None:
        assert rec["wgs_target"] == wgs_target, rec


def _default_target(rec):
    """The workgroup count the library's own plan aims at (csrc/wgrad_nhwc.hip wgrad_impl): 128 for the 256 x 256 tile, 256 for the other bf16 GEMMs, 768 for
    fp32 on the bf16 matrix cores; the direct kernels have none."""
    if rec["family"] in ("c3x3_c64", "stem"):
        return 0
    return 128 if rec["family"].startswith("t256") else (768 if rec["family"] == "x3" else 256)


def _run_geo(entry, g, dtype, plan, **kw):
    o = _ops(g, dtype)
    got, rec = _call(entry, _gid(g), dtype, _desc(g, dtype), o["gpu"], (g.cout, g.cin, g.k, g.k), (g.k, g.cin, g.k, g.cin))
    _compare(entry, _gid(g), dtype, rec, got, o)
    _assert_plan(rec, plan, split=1 if g.split else 0, wgs_target=_default_target(rec), **kw)
    return got, rec


# ------------------------------------------------------------------------------------------------ in-process cases
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("g,plans", _cases(POINTWISE + CONV3 + EXTRA))
def test_implicit_gemm(g, plans, dtype):
    _run_geo("wgrad", g, dtype, plans[dtype])


@pytest.mark.parametrize("g,plan", [pytest.param(g_, p_, id=_gid(g_)) for g_, p_ in DIRECT3])
def test_direct_3x3(g, plan):
    """csrc/wgrad3x3_c64.hip, one fp32 slab per workgroup; a width the predicate refuses reports the implicit GEMM and meets the same bound."""
    _run_geo("wgrad_3x3_c64", g, "bf16", plan, rows=0 if plan.family == "c3x3_c64" else 256)


@pytest.mark.parametrize("shape,plan", [pytest.param(s_, p_, id="n%d_%dx%d" % s_) for s_, p_ in STEM])
def test_stem(shape, plan):
    """csrc/wgrad_stem.hip through the packed view (7 x 1 taps over 32 "channels" of the padded NHWC4 input -> (64, 3, 7, 7)); wo % 16 != 0 is refused by the
    predicate and runs the same view on the implicit GEMM."""
    o = _stem_ops(shape)
    sid = "stem_n%d_%dx%d" % shape
    got, rec = _call("wgrad_stem", sid, "bf16", _stem_desc(shape[0], o), o["gpu"], (64, 3, 7, 7), (7, 3, 8, 4))
    _compare("wgrad_stem", sid, "bf16", rec, got, o)
    _assert_plan(rec, plan, rows=0 if plan.family == "stem" else 256, wgs_target=_default_target(rec))


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("g,plans", _cases(SPLIT))
def test_split_operand(g, plans, dtype):
    """Channels below split_c from x2 (its own pitch), the others from x at the SAME column."""
    _run_geo("wgrad_split", g, dtype, plans[dtype])


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("c,plans", [pytest.param(c_, p_, id="c%d" % c_) for c_, p_ in GRAM])
def test_gram(c, plans, dtype):
    """dz and x the same pointer: a^T a, on the Gram plan (policy gram_wgs = 32 workgroups aimed at)."""
    g = _g(3, 10, 10, c, c, 1, 1)
    o = _ops(g, dtype)
    G = dict(o["gpu"], dz=o["gpu"]["x"])
    a = o["x"].double().numpy().reshape(-1, c)
    oo = dict(ref=(a.T @ a).reshape(c, c, 1, 1), absref=(np.abs(a).T @ np.abs(a)).reshape(c, c, 1, 1))
    got, rec = _call("wgrad_gram", _gid(g), dtype, _desc(g, dtype), G, (c, c, 1, 1), (1, c, 1, c))
    _compare("wgrad_gram", _gid(g), dtype, rec, got, oo)
    s = got[:, :, 0, 0]
    assert np.abs(s - s.T).max() / np.abs(oo["ref"]).max() < BOUND
    assert rec["gram"] == 1
    _assert_plan(rec, plans[dtype], gram=1, wgs_target=32)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("wgs", [8, 256, 4096])
def test_caller_named_workgroup_count(wgs, dtype):
    g = WGS_SHAPE
    o = _ops(g, dtype)
    got, rec = _call("wgrad_wgs%d" % wgs, _gid(g), dtype, _desc(g, dtype), o["gpu"], (g.cout, g.cin, 1, 1), (1, g.cin, 1, g.cin), wgs=wgs)
    _compare("wgrad_wgs%d" % wgs, _gid(g), dtype, rec, got, o)
    assert rec["wgs_target"] == wgs and rec["gram"] == 0
    _assert_plan(rec, Plan("bf16_reg" if dtype == "bf16" else "x3", T64, 8, 1))


@pytest.mark.parametrize("wgs", [7, 4097])
def test_caller_named_workgroup_count_out_of_range_is_refused(wgs):
    g = WGS_SHAPE
    o = _ops(g, "bf16")
    _call("wgrad_wgs_refused", _gid(g), "bf16", _desc(g, "bf16"), o["gpu"], (g.cout, g.cin, 1, 1), (1, g.cin, 1, g.cin), wgs=wgs, expect_rc=-1)


def test_refusals_leave_no_launch_and_dw_untouched():
    g = POINTWISE[1][0]
    o = _ops(g, "bf16")
    pk = (1, g.cin, 1, g.cin)
    d = _desc(g, "bf16")
    d.cin = 126                                                      # cin % 4 != 0 (the buffers are those of cin = 128)
    d.x_pix_stride = 128
    _call("refused_cin", _gid(g), "bf16", d, o["gpu"], (g.cout, 126, 1, 1), (1, 126, 1, 126), expect_rc=-2)
    _call("refused_ws", _gid(g), "bf16", _desc(g, "bf16"), o["gpu"], (g.cout, g.cin, 1, 1), pk, ws_short=1, expect_rc=-3)
    _call("refused_packed", _gid(g), "bf16", _desc(g, "bf16"), o["gpu"], (g.cout, g.cin, 1, 1), (1, g.cin, 2, g.cin), expect_rc=-1)
    _call("refused_packed_real", _gid(g), "bf16", _desc(g, "bf16"), o["gpu"], (g.cout, g.cin, 1, 1), (2, g.cin, 1, g.cin), expect_rc=-1)
    g3 = CONV3[2][0]
    o3 = _ops(g3, "bf16")
    d3 = _desc(g3, "bf16")
    d3.split_c, d3.x2_pix_stride = 32, 64                            # a split operand with a 3x3
    _call("refused_split_3x3", _gid(g3), "bf16", d3, dict(o3["gpu"], x2=o3["gpu"]["x"]), (g3.cout, g3.cin, 3, 3), (3, g3.cin, 3, g3.cin), expect_rc=-1)
    from mvfnet_amd import _lib
    assert _lib.lib.mvf_conv2d_wgrad_last_launch(None) == -1


@pytest.mark.parametrize("dtype", DTYPES)
def test_wgs_4096_runs_in_the_published_workspace(dtype):
    """M = 20000, cin = cout = 512, wgs = 4096: 256 workgroups per tile would be 79 splits of 256 rows, the published workspace (planned for 1024 workgroups)
    holds 63 slabs.  The count is one to AIM at: the call runs with 63 splits of 320 rows -- the smallest multiple of 64 that fits -- instead of returning
    MVF_EWS (which it did before this case existed)."""
    g = WS_CASE
    o = _ops(g, dtype)
    got, rec = _call("wgrad_wgs4096_ws", _gid(g), dtype, _desc(g, dtype), o["gpu"], (g.cout, g.cin, 1, 1), (1, g.cin, 1, g.cin), wgs=4096)
    _compare("wgrad_wgs4096_ws", _gid(g), dtype, rec, got, o)
    _assert_plan(rec, Plan("bf16_pipe/3" if dtype == "bf16" else "x3", T128, 63, 0), rows=320, wgs_target=4096)
    del _ops_cache[(g, dtype)]                                       # (80 MB of operands: not kept for the rest of the session)


# ------------------------------------------------------------------------------------------------ forced legs
def _fams(recs, **match):
    return {r["family"] for r in recs if all(r[k_] == v_ for k_, v_ in match.items())}


def _implicit_default_entry(recs):
    return [r for r in recs if r["launches"] and r["wgs_target"] and not r["gram"] and not r["entry"].startswith("wgrad_wgs") and not r["family"].startswith("t256")]


# leg -> (policy, check(records) that the forced policy reached the kernels it names -- and kept the others out)
LEGS = {
    "wgrad_dma=0": (dict(wgrad_dma=0), lambda rs: not _fams(rs) & {"bf16_dma2", "bf16_pipe/3", "bf16_pipe/4"} and "bf16_reg" in _fams(rs, tile=[128, 128])),
    "wgrad_dma=2": (dict(wgrad_dma=2), lambda rs: "bf16_pipe/3" in _fams(rs, tile=[128, 64]) and "bf16_reg" not in _fams(rs, split=0)),
    "wgrad_dma=3": (dict(wgrad_dma=3), lambda rs: _fams(rs, split=1, dtype="bf16") <= {"bf16_reg", "t256_p4"} and "bf16_pipe/3" in _fams(rs, split=0)),
    "wgrad_stages=2": (dict(wgrad_stages=2), lambda rs: "bf16_dma2" in _fams(rs) and not _fams(rs) & {"bf16_pipe/3", "bf16_pipe/4"}),
    "wgrad_stages=4": (dict(wgrad_stages=4), lambda rs: "bf16_pipe/4" in _fams(rs) and "bf16_pipe/3" not in _fams(rs)),
    "wgrad_x3=0": (dict(wgrad_x3=0), lambda rs: "f32_dma" in _fams(rs) and "x3" not in _fams(rs)),
    "wgrad_x3=0,wgrad_dma_f32=0": (dict(wgrad_x3=0, wgrad_dma_f32=0), lambda rs: _fams(rs, dtype="f32") == {"none", "f32_reg"} or _fams(rs, dtype="f32") == {"f32_reg"}),
    "wgrad_p4=0": (dict(wgrad_p4=0), lambda rs: "t256_2b" in _fams(rs) and "t256_p4" not in _fams(rs)),
    "wgrad_big=0": (dict(wgrad_big=0), lambda rs: not _fams(rs) & {"t256_2b", "t256_p4"}),
    "wgrad3x3_direct=0,wgrad_stem_direct=0": (dict(wgrad3x3_direct=0, wgrad_stem_direct=0), lambda rs: not _fams(rs) & {"c3x3_c64", "stem"}),
    # more bands than workgroups at small shapes: 4-row bands on 8 workgroups (n13x8: 4 x 4 = 16 bands), 1-row bands on 4 (every stem shape)
    "wgrad3x3_r=4,wgrad3x3_wgs=8,wgrad_stem_r=1,wgrad_stem_wgs=4": (dict(wgrad3x3_r=4, wgrad3x3_wgs=8, wgrad_stem_r=1, wgrad_stem_wgs=4),
                                                                   lambda rs: {r["nsplit"] for r in rs if r["family"] == "stem"} == {4} and
                                                                   sorted(r["nsplit"] for r in rs if r["family"] == "c3x3_c64") == [1, 2, 6, 8]),
    "wgrad_wgs=64": (dict(wgrad_wgs=64), lambda rs: {r["wgs_target"] for r in _implicit_default_entry(rs)} == {64}),
    "wgrad_wgs=4096": (dict(wgrad_wgs=4096), lambda rs: {r["wgs_target"] for r in _implicit_default_entry(rs)} == {4096}),
}
_leg_results = {}


def _run_leg(leg, tmp_dir):
    """This file's in-process cases again in a fresh child process under the leg's policy (the policies are read once per process); memoised."""
    if leg not in _leg_results:
        cov = os.path.join(str(tmp_dir), "coverage_%d.jsonl" % list(LEGS).index(leg))
        env = policy_env(**LEGS[leg][0])
        env[COVERAGE_ENV] = cov
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-m", "gpu", "-k",
                            "not forced and not coverage_matrix and not published_workspace", "-p", "no:cacheprovider"], env=env, capture_output=True, text=True, timeout=600)
        recs = [json.loads(line) for line in open(cov)] if os.path.exists(cov) else []
        _leg_results[leg] = (r.returncode, r.stdout[-3000:] + r.stderr[-2000:], recs)
    return _leg_results[leg]


@pytest.fixture(scope="module")
def leg_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("wgrad_legs")


@pytest.mark.parametrize("leg", list(LEGS))
def test_families_under_forced_policies(leg, leg_dir):
    rc, tail, recs = _run_leg(leg, leg_dir)
    assert rc == 0, tail
    assert recs
    assert LEGS[leg][1](recs), "policy %s did not reach the kernels it names: %s" % (leg, sorted({(r["family"], tuple(r["tile"]), r["dtype"], r["split"], r["nsplit"],
                                                                                                   r["wgs_target"]) for r in recs}))


# (family, tile, storage type, split operand) that must have been reached across the legs
def _rows(fam, dt, *tile_splits):
    return [(fam, t, dt, s) for t, ss in tile_splits for s in ss]


MATRIX = (
    _rows("x3", "f32", (T64, (0, 1)), (T128x64, (0,)), (T128, (0, 1))) +
    _rows("f32_dma", "f32", (T64, (0, 1)), (T128x64, (0,)), (T128, (0, 1))) +
    _rows("f32_reg", "f32", (T64, (0, 1)), (T128x64, (0,)), (T128, (0, 1))) +
    _rows("bf16_widen", "bf16", (T64, (0,)), (T128x64, (0,)), (T128, (0,))) +
    _rows("bf16_reg", "bf16", (T64, (0, 1)), (T128x64, (0,)), (T128, (0, 1))) +
    _rows("bf16_dma2", "bf16", (T64, (0, 1)), (T128, (0, 1))) +
    _rows("bf16_pipe/3", "bf16", (T64, (0, 1)), (T128x64, (0,)), (T128, (0, 1))) +
    _rows("bf16_pipe/4", "bf16", (T64, (0, 1)), (T128, (0, 1))) +
    _rows("t256_2b", "bf16", (T256, (0, 1))) +
    _rows("t256_p4", "bf16", (T256, (0, 1))) +
    _rows("c3x3_c64", "bf16", ((64, 576), (0,))) +
    _rows("stem", "bf16", ((64, 224), (0,)))
)
# What the matrix leaves out, each with its reason.  A combination that a later policy change makes unreachable FAILS test_coverage_matrix by name.
NOT_IN_MATRIX = (
    "the two-barrier 256 x 256 loop outside policy wgrad_p4=0: launch_wgrad_bf16_big takes it when cin % 64 != 0, but the 256 x 256 tile wants K % 256 == 0, and with "
    "1, 9 or 7 taps that implies cin % 64 == 0 (256 = 2^8, the tap counts are odd) -- the branch is dead under the default policy, wgrad_p4=0 is the only way in",
    "the split operand on a 128 x 64 tile: that tile is K <= 64, a pointwise conv of at most 64 input channels; no case splits so narrow an operand",
    "the split operand on the widening kernel (bf16 with split_c % 8 != 0): the engine's split operands are multiples of 64 channels",
    "the 128 x 64 tile on the two-buffer LDS-DMA kernel and the four-stage ring: K <= 64 reaches the LDS-DMA loaders only under wgrad_dma=2, which no leg combines "
    "with wgrad_stages=2 / 4 (the three-stage ring covers that tile's loader under wgrad_dma=2)",
    "bf16 storage on the f32 / x3 families and fp32 storage on the bf16 ones: the families ARE the storage types' kernels; both direct kernels are bf16 only",
    "the 256 x 256 tile with a caller-named workgroup count: mvf_conv2d_nhwc_wgrad_wgs never takes it (wgrad_impl)",
    "test_wgs_4096_runs_in_the_published_workspace in the forced legs: a 20000-pixel reference per child; the caller-named path is reached by the M = 2048 cases there",
)


def test_coverage_matrix(leg_dir):
    seen = set()
    for leg in LEGS:
        rc, tail, recs = _run_leg(leg, leg_dir)
        assert rc == 0, "leg %s: %s" % (leg, tail)
        seen |= {(r["family"], tuple(r["tile"]), r["dtype"], r["split"]) for r in recs if r["launches"]}
    missing = [k for k in MATRIX if k not in seen]
    assert not missing, "never reached (family, tile, storage type, split operand): %s" % missing
    extra = sorted(k for k in seen if k not in MATRIX)
    assert not extra, "reached but not in the written matrix: %s" % extra
