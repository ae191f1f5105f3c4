"""GPU: every epilogue entry point of the implicit-GEMM conv (csrc/conv_nhwc.hip) through the C ABI against the INDEPENDENT fp64 reference
tests/conv_epilogue_ref.py (proved against autograd in tests/test_conv_epilogue_ref_cpu.py), at the smallest shapes at which the kernels can still go
wrong, in both storage types -- in this process under the default launch policy, and again in one child process per forced policy so that every kernel
family conv_nhwc.hip instantiates runs every epilogue of its list.  After every call the host-side launch record (mvf_conv2d_last_launch) says which
kernel ran; the last test asserts the written family x epilogue x loader x storage matrix over the forced legs.

Bounds.  Stored tensors: helpers.rel_err < 2e-5 (fp32, the test_conv_gpu.py bound) / 6e-3 (bf16: one bf16 rounding of fp32 sums over bf16-rounded operands).
Sums: per PARTIAL (not per column total: this is what checks the channel-major layout and the parity-class order) against fp64 sums over the kernel's own
stored output, 1e-4 on signed sums, 1e-5 on sums of squares, as in the direct-kernel tests.  The two epilogues that store no z3 get their allowance from
the reference alone:
  mode 9  : the reference is evaluated twice more with z3 moved by +-1 storage ulp; twice the larger deviation is allowed on top of the stored-tensor
            bound (dgamma / dbeta are the fp64 sums of the same case, so the factor stays small): profiles/conv_epilogue_errors.txt has the numbers.
  mode 10 : sum gm does not depend on z3 (1e-4 against the reference).  sum gm * xhat does: the kernel's fp32 accumulator and the fp64 one round to
            DIFFERENT bf16 neighbours where the exact value lies within the fp32 accumulation error of a rounding boundary (a few elements in 1e4), and one
            such element moves its partial by |gm| * invstd * ulp(z3) -- more than 1e-4 of the largest partial.  So a partial may deviate by 1e-4 of the
            scale PLUS that amount summed over its UNDECIDED elements: those whose exact z3 lies within _acc_err() of a rounding boundary, found from the
            reference alone (fp32 storage rounds nothing away: no allowance there).  The allowance must stay below 1 % of the largest partial.
Gates taken from an input (epilogue 6): z is repaired on the CPU until no scale * z + shift lies within 1e-3 of zero, asserted before the launch."""
import collections
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import conv_epilogue_ref as R
from helpers import policy_env, policy_set, rel_err

pytestmark = pytest.mark.gpu

COVERAGE_ENV = "MVF_CONV_EPILOGUE_COVERAGE"       # a file: this module appends one JSON line per conv call (the forced legs' children; tooling)
ERRORS_ENV = "MVF_CONV_EPILOGUE_ERRORS"           # a file: one JSON line per measured error (tooling: profiles/conv_epilogue_errors.txt)
_coverage = []

Geo = collections.namedtuple("Geo", "n h w cin cout k stride pad dil ho wo split")


def _pw(n, h, w, cin, cout):
    return Geo(n, h, w, cin, cout, 1, 1, 0, 1, h, w, 0)


def _c3(n, h, w, cin, cout, k, s):
    p = k // 2
    return Geo(n, h, w, cin, cout, k, s, p, 1, (h + 2 * p - k) // s + 1, (w + 2 * p - k) // s + 1, 0)


def _dg(n, h, w, cin, cout, k, dil):
    """Data gradient of a k x k, stride `dil` conv with padding k // 2: h x w is that conv's INPUT map = the data gradient's output map (as in
    test_train_gpu.py); the gradient map read has cin channels, the output cout."""
    p = k // 2
    return Geo(n, (h + 2 * p - k) // dil + 1, (w + 2 * p - k) // dil + 1, cin, cout, k, 1, k - 1 - p, dil, h, w, 0)


def _sp(n, h, w, c, k):
    """The split operand of the dz3-free data gradient (train_engine.py dzfree_dgrad): the contraction runs over [x2 | x], x2 = gm [M][c], x = a_in [M][k]."""
    return Geo(n, h, w, c + k, k, 1, 1, 0, 1, h, w, c)


POINTWISE = [
    _pw(2, 9, 7, 64, 256),         # M = 126: one ragged tile; one bf16 chunk; Cout % 256 == 0
    _pw(3, 6, 6, 128, 96),         # ragged N tile; Cout % 64 != 0: the gate bytes are read from memory, not LDS
    _pw(1, 14, 14, 256, 1024),     # M = 196: the second 128-row partial is ragged, a 256-row tile holds two partials; many N tiles
    _pw(5, 5, 5, 32, 64),          # the 128 x 64 tile; cin is half a bf16 chunk
    _pw(3, 10, 10, 1024, 256),     # M = 300: the second 256-row tile has ONE live partial (the pidx * 128 < M guard); 16 bf16 chunks = the conv_big2 threshold
    _pw(2, 8, 8, 2048, 128),       # M = 128 exactly; 32 chunks: the two-buffer DMA loop is the default
]
CONV3 = [
    _c3(2, 7, 9, 128, 64, 3, 1),       # narrow tile, 18 chunks
    _c3(1, 14, 14, 192, 256, 3, 1),    # 27 chunks, an odd count
    _c3(2, 6, 6, 96, 256, 3, 1),       # cin % 64 != 0: a forced 256 x 256 tile must take the two-barrier loop, not the four-phase one
    _c3(2, 13, 11, 128, 128, 3, 2),    # stride 2, odd map
]
DGRAD = [
    _dg(2, 13, 11, 128, 64, 3, 2),     # strided 3x3: four parity classes with 4 / 2 / 2 / 1 taps
    _dg(3, 8, 8, 64, 128, 1, 2),       # three of the four parity classes have zero taps: launches with zero K chunks
    _dg(1, 12, 12, 256, 256, 3, 1),    # stride-1 3x3 with 256 output channels: the 256 x 256 tiles apply
    _dg(2, 9, 7, 256, 64, 1, 1),       # pointwise, narrow output
]
SPLIT = [_sp(2, 9, 7, 256, 64), _sp(3, 6, 6, 128, 96), _sp(1, 14, 14, 1024, 256)]
FORWARD = POINTWISE + CONV3
DTYPES = ["f32", "bf16"]
TOL = {"f32": 2e-5, "bf16": 6e-3}


def _gid(g):
    return "n%d_%dx%d_c%d_o%d_k%d_s%d_d%d%s" % (g.n, g.h, g.w, g.cin, g.cout, g.k, g.stride, g.dil, "_split%d" % g.split if g.split else "")


# ------------------------------------------------------------------------------------------------ operands (one set per shape and storage type, shared, never modified)
_ops_cache = {}


def _ops(g, dtype):
    key = (g, dtype)
    if key in _ops_cache:
        return _ops_cache[key]
    td = torch.float32 if dtype == "f32" else torch.bfloat16
    gen = torch.Generator().manual_seed(g.cin + g.cout)
    m = g.n * g.ho * g.wo
    o = {"m": m, "td": td}
    st = lambda t: t.to(td)                                                   # noqa: E731
    if g.split:
        c, k = g.split, g.cin - g.split
        o["x2"] = st(torch.randn(g.n, g.h, g.w, c, generator=gen))             # gm
        o["x"] = st(torch.randn(g.n, g.h, g.w, k, generator=gen))              # a_in: channels [c, c + k) at column (channel - c)
        x64 = torch.cat([o["x2"], o["x"]], dim=3).double().numpy()
    else:
        o["x"] = st(torch.randn(g.n, g.h, g.w, g.cin, generator=gen))
        x64 = o["x"].double().numpy()
    o["w"] = st(torch.randn(g.cout, g.k, g.k, g.cin, generator=gen) * (2.0 / (g.cin * g.k * g.k)) ** 0.5)
    o["res"] = st(torch.randn(m, g.cout, generator=gen))
    o["rbits"] = torch.randint(0, 16, (m, g.cout // 4), generator=gen, dtype=torch.uint8)
    o["gbits"] = torch.randint(0, 16, (m, g.cout // 4), generator=gen, dtype=torch.uint8)
    f = lambda t: t.float().contiguous()                                     # noqa: E731
    o["bias"] = f(torch.randn(g.cout, generator=gen) * 0.2)
    o["kshift"] = f(torch.randn(g.cout, generator=gen) * 0.1)
    o["mean"] = f(torch.randn(g.cout, generator=gen) * 0.1)
    o["invstd"] = f(torch.rand(g.cout, generator=gen) + 0.5)
    o["gamma"] = f(torch.rand(g.cout, generator=gen) + 0.5)
    sign = torch.where(torch.rand(g.cout, generator=gen) < 0.25, -1.0, 1.0)
    o["scale"] = f((torch.rand(g.cout, generator=gen) + 0.5) * sign)           # (a quarter of the channels with a negative BatchNorm weight)
    o["shift"] = f(torch.randn(g.cout, generator=gen) * 0.3)
    o["ap_scale"] = f(torch.rand(g.cout, generator=gen) + 0.5)
    o["ap_shift"] = f(torch.randn(g.cout, generator=gen) * 0.3)
    o["rscale"] = f(torch.rand(g.cout, generator=gen) + 0.5)
    o["rshift"] = f(torch.randn(g.cout, generator=gen) * 0.3)
    # z of the ReLU(BN(z)) the data gradient feeds: repaired until the gate scale * z + shift is decided in any arithmetic
    z = st(torch.randn(m, g.cout, generator=gen))
    for _ in range(4):
        t = o["scale"].double()[None, :] * z.double() + o["shift"].double()[None, :]
        bad = t.abs() < 2e-3
        if not bool(bad.any()):
            break
        target = torch.where(t >= 0, 0.05, -0.05)
        z = torch.where(bad, st(((target - o["shift"].double()[None, :]) / o["scale"].double()[None, :]).float()), z)
    o["z"] = z
    o["n64"] = {k_: v.double().numpy() for k_, v in o.items() if isinstance(v, torch.Tensor) and v.dtype != torch.uint8 and k_ not in ("x", "x2")}
    o["n64"]["x"] = x64
    o["n64"]["rbits"], o["n64"]["gbits"] = o["rbits"].numpy(), o["gbits"].numpy()
    o["geom"] = dict(stride=g.stride, pad=g.pad, in_dil=g.dil, ho=g.ho, wo=g.wo)
    o["acc"] = R.conv(x64, o["n64"]["w"], **o["geom"])                         # THE fp64 convolution of the stored operands, computed once
    o["runs"] = R.row_runs(g.n, g.ho, g.wo, g.dil)
    o["gpu"] = {k_: v.cuda() for k_, v in o.items() if isinstance(v, torch.Tensor)}
    _ops_cache[key] = o
    return o


# ------------------------------------------------------------------------------------------------ calls
def _P(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _desc(g, dtype, res_c0=0):
    from mvfnet_amd import _lib
    dt = _lib.MVF_F32 if dtype == "f32" else _lib.MVF_BF16
    if g.split:
        c, k = g.split, g.cin - g.split
        return _lib.ConvDesc(g.n, g.h, g.w, g.cin, g.cout, 1, 1, 1, 0, g.ho, g.wo, k, dt, 0, c, c, 0, res_c0, c)
    return _lib.ConvDesc(g.n, g.h, g.w, g.cin, g.cout, g.k, g.k, g.stride, g.pad, g.ho, g.wo, g.cin, dt, 0, 0, 0, g.dil if g.dil > 1 else 0, res_c0, 0)


class _Out(object):
    """Output buffers with a guard behind each: a row of NaN after the last output row, a row of 0xA5 after the last sign-bit row, NaN floats after the
    last partial; everything pre-filled (NaN / 0xA5), so an unwritten row or partial shows."""

    def __init__(self, g, dtype, m, rows):
        td = torch.float32 if dtype == "f32" else torch.bfloat16
        self.m, self.c, self.rows = m, g.cout, rows
        self.y = torch.full((m + 1, g.cout), float("nan"), dtype=td, device="cuda")
        self.bits = torch.full((m + 1, g.cout // 4), 0xA5, dtype=torch.uint8, device="cuda")
        self.part = torch.full((g.cout * rows * 2 + 64,), float("nan"), dtype=torch.float32, device="cuda")

    def stored(self, written=True):
        y = self.y.double().cpu().numpy()
        assert np.isnan(y[self.m]).all(), "the row past M was written"
        if written:
            assert np.isfinite(y[:self.m]).all(), "%d output elements were never written" % int((~np.isfinite(y[:self.m])).sum())
        else:
            assert np.isnan(y[:self.m]).all(), "an epilogue that stores nothing wrote the output"
        return y[:self.m]

    def sign_bits(self, written=True):
        b = self.bits.cpu().numpy()
        assert (b[self.m] == 0xA5).all(), "the sign-bit row past M was written"
        if written:
            assert (b[:self.m] < 16).all(), "sign-bit bytes were never written (or hold bits above the low four)"
        else:
            assert (b == 0xA5).all()
        return b[:self.m]

    def partials(self, written=True):
        p = self.part.double().cpu().numpy()
        n = self.c * self.rows * 2
        assert np.isnan(p[n:]).all(), "floats past the last partial were written"
        if written:
            assert np.isfinite(p[:n]).all(), "%d partial sums were never written" % int((~np.isfinite(p[:n])).sum())
        else:
            assert np.isnan(p[:n]).all()
        return p[:n].reshape(self.c, self.rows, 2)


def _record(entry, dtype, expect_launch=True):
    from mvfnet_amd import _lib
    info = _lib.ConvLaunchInfo()
    _lib.check(_lib.lib.mvf_conv2d_last_launch(C.byref(info)))
    rec = dict(entry=entry, dtype=dtype, family=_lib.CONV_FAMILIES[info.family], asked=info.epi_asked, run=info.epi_run, pw=info.pointwise,
               buffers=info.buffers, tile=[info.tile_m, info.tile_n], chunks=info.k_chunks, half_k=info.half_k, launches=info.launches)
    _coverage.append(rec)
    if os.environ.get(COVERAGE_ENV):
        with open(os.environ[COVERAGE_ENV], "a") as f_:
            f_.write(json.dumps(rec) + "\n")
    if expect_launch:
        assert info.launches >= 1 and info.family != 0
        assert info.dtype == (_lib.MVF_F32 if dtype == "f32" else _lib.MVF_BF16)
        assert info.epi_run in (0, info.epi_asked)
    return rec


def _note_error(entry, g, dtype, rec, what, value, bound):
    if os.environ.get(ERRORS_ENV):
        with open(os.environ[ERRORS_ENV], "a") as f_:
            f_.write(json.dumps(dict(entry=entry, shape=_gid(g), dtype=dtype, family=rec["family"], buffers=rec["buffers"], run=rec["run"], what=what,
                                     value=float(value), bound=float(bound))) + "\n")
    print("%s %s %s %s/%d epi %d->%d: %s = %.3g (bound %.3g)" % (entry, _gid(g), dtype, rec["family"], rec["buffers"], rec["asked"], rec["run"], what, value, bound))


def _check(entry, g, dtype, rec, what, got, ref, bound):
    e = rel_err(got, ref)
    _note_error(entry, g, dtype, rec, what, e, bound)
    assert e < bound, "%s %s %s on %s: %s deviates %.3g (bound %.3g)" % (entry, _gid(g), dtype, rec, what, e, bound)


def _check_sums(entry, g, dtype, rec, part, ref_part, second_bound=1e-5, second_allow=None):
    """Partial by partial: [..][0] a signed sum (1e-4), [..][1] a sum of squares (1e-5) or a signed sum (1e-4), relative to the largest partial."""
    assert part.shape == ref_part.shape
    _check(entry, g, dtype, rec, "partials[0]", part[:, :, 0], ref_part[:, :, 0], 1e-4)
    if second_allow is None:
        _check(entry, g, dtype, rec, "partials[1]", part[:, :, 1], ref_part[:, :, 1], second_bound)
    else:
        scale = np.abs(ref_part[:, :, 1]).max()
        excess = (np.abs(part[:, :, 1] - ref_part[:, :, 1]) - second_allow).max() / scale
        _note_error(entry, g, dtype, rec, "partials[1] against the reference z3, no allowance (figure only)", rel_err(part[:, :, 1], ref_part[:, :, 1]), 0.0)
        _note_error(entry, g, dtype, rec, "largest allowance of a partial / scale (figure only)", second_allow.max() / scale, 0.0)
        _note_error(entry, g, dtype, rec, "partials[1] beyond the undecided elements' allowance", max(excess, 0.0), second_bound)
        assert excess < second_bound, "%s %s %s on %s: partials[1] deviate %.3g of the scale beyond the allowance" % (entry, _gid(g), dtype, rec, excess)


def _lib_():
    from mvfnet_amd import _lib
    return _lib.lib, _lib.check


def _sync():
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ forward entry points
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("g", FORWARD, ids=_gid)
def test_fwd_stats(g, dtype):
    """z = the convolution rounded once; partials of (z_stored - shift) and its square per 128 rows, channel-major; y = NULL leaves the same partials."""
    lib, check = _lib_()
    o = _ops(g, dtype)
    G, n64 = o["gpu"], o["n64"]
    d = _desc(g, dtype)
    rows = lib.mvf_conv2d_stats_rows(C.byref(d))
    assert rows == R.stats_rows(g.n, g.ho, g.wo)
    out = _Out(g, dtype, o["m"], rows)
    # (the bf16 64-channel pointwise statistics-only pass has its own kernel with its own partial layout, csrc/pw_sums.hip: here the implicit GEMM is asked)
    with policy_set(pw_sums=0):
        check(lib.mvf_conv2d_nhwc_fwd_stats(C.byref(d), _P(G["x"]), None, _P(G["w"]), _P(out.y), _P(out.part), _P(G["kshift"]), None, 0, None))
        rec = _record("fwd_stats", dtype)
        out0 = _Out(g, dtype, o["m"], rows)
        check(lib.mvf_conv2d_nhwc_fwd_stats(C.byref(d), _P(G["x"]), None, _P(G["w"]), None, _P(out0.part), _P(G["kshift"]), None, 0, None))
        rec0 = _record("fwd_stats_nostore", dtype)
    _sync()
    assert (rec0["family"], rec0["run"], rec0["pw"], rec0["buffers"]) == (rec["family"], rec["run"], rec["pw"], rec["buffers"])
    z_ref, _ = R.fwd_stats(n64["x"], n64["w"], dtype, n64["kshift"], acc=o["acc"], **o["geom"])
    z = out.stored()
    _check("fwd_stats", g, dtype, rec, "z", z, z_ref, TOL[dtype])
    part = out.partials()
    k = n64["kshift"][None, :]
    _check_sums("fwd_stats", g, dtype, rec, part, R.partials(o["runs"], z - k, (z - k) ** 2))
    out0.stored(written=False)
    assert np.array_equal(out0.partials(), part), "the statistics-only pass (y = NULL) leaves other partials than the storing one"


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("g,variant", [(g_, v_) for g_ in FORWARD + DGRAD for v_ in ("plain", "res", "bias_relu", "bias_res_relu") if g_.dil == 1 or v_ == "plain"],
                         ids=lambda a_: a_ if isinstance(a_, str) else _gid(a_))
def test_fwd_ws(g, variant, dtype):
    """Plain (a data gradient: strided ones scatter their parity classes), + residual, and the two inference epilogues."""
    lib, check = _lib_()
    o = _ops(g, dtype)
    G, n64 = o["gpu"], o["n64"]
    d = _desc(g, dtype)
    bias, res, relu = "bias" in variant, "res" in variant, "relu" in variant
    d.relu = int(relu)
    out = _Out(g, dtype, o["m"], 1)
    check(lib.mvf_conv2d_nhwc_fwd_ws(C.byref(d), _P(G["x"]), None, _P(G["w"]), _P(G["bias"]) if bias else None, _P(G["res"]) if res else None, _P(out.y), None, 0, None))
    rec = _record("fwd_ws_" + variant, dtype)
    _sync()
    if g.dil > 1:
        assert rec["launches"] == g.dil * g.dil
    ref = R.fwd(n64["x"], n64["w"], dtype, n64["bias"] if bias else None, n64["res"] if res else None, relu, acc=o["acc"], **o["geom"])
    _check("fwd_ws_" + variant, g, dtype, rec, "y", out.stored(), ref, TOL[dtype])
    out.partials(written=False)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("res_c0", [0, 8, 64])
@pytest.mark.parametrize("entry", ["resmask", "resmask_nobits", "resmask_gate", "resmask_gate_bias", "resmask_gate_colsums"])
@pytest.mark.parametrize("g", FORWARD + DGRAD[2:], ids=_gid)
def test_fwd_resmask(g, entry, res_c0, dtype):
    """The residual is read for channels >= res_c0 only, bit j of byte k gates channel 4k + j; the output gate applies to channels >= res_c0 only; the
    column sums are those of what is stored."""
    lib, check = _lib_()
    o = _ops(g, dtype)
    G, n64 = o["gpu"], o["n64"]
    d = _desc(g, dtype, res_c0)
    rows = lib.mvf_conv2d_stats_rows(C.byref(d))
    out = _Out(g, dtype, o["m"], rows)
    rb = None if entry == "resmask_nobits" else G["rbits"]
    bias = G["bias"] if entry == "resmask_gate_bias" else None
    if entry in ("resmask", "resmask_nobits"):
        check(lib.mvf_conv2d_nhwc_fwd_resmask(C.byref(d), _P(G["x"]), None, _P(G["w"]), None, _P(G["res"]), _P(rb), _P(out.y), None, 0, None))
    elif entry in ("resmask_gate", "resmask_gate_bias"):
        check(lib.mvf_conv2d_nhwc_fwd_resmask_gate(C.byref(d), _P(G["x"]), None, _P(G["w"]), _P(bias), _P(G["res"]), _P(rb), _P(G["gbits"]), _P(out.y), None, 0, None))
    else:
        check(lib.mvf_conv2d_nhwc_fwd_resmask_gate_colsums(C.byref(d), _P(G["x"]), None, _P(G["w"]), _P(G["res"]), _P(rb), _P(G["gbits"]), _P(out.y), _P(out.part),
                                                           None, 0, None))
    rec = _record(entry, dtype)
    _sync()
    ref = R.fwd_resmask(n64["x"], n64["w"], dtype, n64["res"], None if rb is None else n64["rbits"], n64["gbits"] if "gate" in entry else None, res_c0,
                        n64["bias"] if bias is not None else None, acc=o["acc"], **o["geom"])
    y = out.stored()
    _check(entry, g, dtype, rec, "y", y, ref, TOL[dtype])
    if entry == "resmask_gate_colsums":
        _check_sums(entry, g, dtype, rec, out.partials(), R.partials(o["runs"], y, y * y))
    else:
        out.partials(written=False)
    if "gate" in entry:          # gated elements are exact zeros, below res_c0 nothing is gated
        gate = R.unpack_bits(n64["gbits"], g.cout) > 0
        hi = np.arange(g.cout)[None, :] >= res_c0
        assert (y[~gate & hi] == 0).all()


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("rbn", [False, True], ids=["identity", "downsample_bn"])
@pytest.mark.parametrize("g", FORWARD, ids=_gid)
def test_fwd_bnapply(g, rbn, dtype):
    """out = relu(scale * z3 + shift + res') on the ROUNDED z3, res' = res or rscale * res + rshift, and the sign bits."""
    lib, check = _lib_()
    o = _ops(g, dtype)
    G, n64 = o["gpu"], o["n64"]
    d = _desc(g, dtype)
    out = _Out(g, dtype, o["m"], 1)
    check(lib.mvf_conv2d_nhwc_fwd_bnapply(C.byref(d), _P(G["x"]), None, _P(G["w"]), _P(G["ap_scale"]), _P(G["ap_shift"]), _P(G["res"]), _P(G["rscale"]) if rbn else None,
                                          _P(G["rshift"]) if rbn else None, _P(out.y), _P(out.bits), None, 0, None))
    rec = _record("fwd_bnapply", dtype)
    _sync()
    ref = R.fwd_bnapply(n64["x"], n64["w"], dtype, n64["ap_scale"], n64["ap_shift"], n64["res"], n64["rscale"] if rbn else None, n64["rshift"] if rbn else None,
                        acc=o["acc"], **o["geom"])
    y, bits = out.stored(), out.sign_bits()
    _check("fwd_bnapply", g, dtype, rec, "out", y, ref["out"], TOL[dtype])
    # (a) the bits are those of the tensor stored beside them, exactly
    assert np.array_equal(bits, R.pack_bits(y > 0))
    # (b) ... and the reference's wherever the reference is decided (from the reference alone: one storage ulp of z3 either way, and fp32 evaluation)
    sc = np.abs(n64["ap_scale"])[None, :]
    margin = 1e-5 * (np.abs(n64["ap_scale"][None, :] * ref["z3"]) + np.abs(n64["ap_shift"])[None, :] + np.abs(ref["res"]))
    if dtype == "bf16":
        margin = margin + 2.0 * R.ulp(ref["z3"], dtype) * sc
    decided = np.abs(ref["t"]) > margin
    undecided = 1.0 - decided.mean()
    _note_error("fwd_bnapply", g, dtype, rec, "undecided sign bits (fraction)", undecided, 0.01)
    assert undecided <= 0.01
    got_pos = R.unpack_bits(bits, g.cout) > 0
    assert np.array_equal(got_pos[decided], (ref["t"] > 0)[decided]), "%d decided sign bits differ" % int((got_pos != (ref["t"] > 0))[decided].sum())
    assert 0.2 < (y > 0).mean() < 0.8                       # the ReLU and the bits are exercised on both sides
    out.partials(written=False)


def _acc_err(o):
    """How far a kernel's fp32 accumulator may lie from the exact convolution: the project's own bound for fp32 results, TOL["f32"] of the tensor's largest
    magnitude (tests/test_conv_gpu.py).  Used only to call an element's rounded z3 `undecided`; taken from the reference, not from a kernel."""
    return TOL["f32"] * float(np.abs(o["acc"]).max())


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("g", FORWARD, ids=_gid)
def test_fwd_bnbwd_sums_and_apply(g, dtype):
    """Modes 10 and 9 on the rounded recomputed z3: partials of gm and gm * xhat; dz3 from the fp64 dgamma / dbeta of the same case."""
    lib, check = _lib_()
    o = _ops(g, dtype)
    G, n64 = o["gpu"], o["n64"]
    d = _desc(g, dtype)
    rows = lib.mvf_conv2d_stats_rows(C.byref(d))
    args = (n64["x"], n64["w"], dtype, n64["res"], n64["rbits"], n64["mean"], n64["invstd"])
    ref = R.fwd_bnbwd(*args, acc=o["acc"], **o["geom"])
    dbeta, dgamma = ref["sums"][:, :, 0].sum(1), ref["sums"][:, :, 1].sum(1)
    dg, db = torch.from_numpy(dgamma).float().cuda(), torch.from_numpy(dbeta).float().cuda()
    dg64, db64 = dg.double().cpu().numpy(), db.double().cpu().numpy()
    ref = R.fwd_bnbwd(*args, gamma=n64["gamma"], dgamma=dg64, dbeta=db64, acc=o["acc"], **o["geom"])
    out10, out9 = _Out(g, dtype, o["m"], rows), _Out(g, dtype, o["m"], rows)
    with policy_set(pw_sums=0):                              # (as in test_fwd_stats: the implicit GEMM, not csrc/pw_sums.hip)
        check(lib.mvf_conv2d_nhwc_fwd_bnbwd_sums(C.byref(d), _P(G["x"]), None, _P(G["w"]), _P(G["res"]), _P(G["rbits"]), _P(G["mean"]), _P(G["invstd"]), _P(out10.part),
                                                 None, 0, None))
        rec10 = _record("fwd_bnbwd_sums", dtype)
    check(lib.mvf_conv2d_nhwc_fwd_bnbwd_apply(C.byref(d), _P(G["x"]), None, _P(G["w"]), _P(G["res"]), _P(G["rbits"]), _P(G["gamma"]), _P(G["mean"]), _P(G["invstd"]),
                                              _P(dg), _P(db), _P(out9.y), None, 0, None))
    rec9 = _record("fwd_bnbwd_apply", dtype)
    _sync()
    # mode 10: nothing stored; sum gm to 1e-4; sum gm * xhat to 1e-4 of the scale plus what the UNDECIDED roundings of z3 can move (module docstring)
    out10.stored(written=False)
    part = out10.partials()
    allow = None
    if dtype == "bf16":
        exact, z3 = o["acc"], ref["z3"]
        half = 0.5 * R.ulp(z3, dtype)
        und = (half - np.abs(exact - z3)) < _acc_err(o)                       # the exact value lies this close to the midpoint between two bf16 neighbours
        per_elem = np.where(und, np.abs(ref["gm"]) * n64["invstd"][None, :] * 2.0 * half, 0.0)
        allow = R.partials(o["runs"], per_elem, per_elem)[:, :, 0]
        # (the allowance stays a small part of what is compared: a wrong row, mean or gate moves a partial by far more)
        assert allow.max() < 0.01 * np.abs(ref["sums"][:, :, 1]).max(), allow.max() / np.abs(ref["sums"][:, :, 1]).max()
        _note_error("fwd_bnbwd_sums", g, dtype, rec10, "undecided z3 roundings (fraction, figure only)", und.mean(), 0.0)
    _check_sums("fwd_bnbwd_sums", g, dtype, rec10, part, ref["sums"], second_bound=1e-4, second_allow=allow)
    # mode 9: the stored-tensor bound + twice the larger deviation of the reference under z3 +- 1 storage ulp
    dev = max(rel_err(R.fwd_bnbwd(*args, gamma=n64["gamma"], dgamma=dg64, dbeta=db64, acc=o["acc"], z3_ulps=s_, **o["geom"])["dz"], ref["dz"]) for s_ in (1, -1))
    _note_error("fwd_bnbwd_apply", g, dtype, rec9, "dz deviation of the reference under z3 +- 1 ulp", dev, 0.0)
    _check("fwd_bnbwd_apply", g, dtype, rec9, "dz", out9.stored(), ref["dz"], TOL[dtype] + 2.0 * dev)
    out9.partials(written=False)


# ------------------------------------------------------------------------------------------------ data gradients with the BatchNorm-backward sums
def _dgrad_case(entry, g, dtype, split):
    lib, check = _lib_()
    o = _ops(g, dtype)
    G, n64 = o["gpu"], o["n64"]
    d = _desc(g, dtype)
    rows = lib.mvf_conv2d_stats_rows(C.byref(d))
    assert rows == R.stats_rows(g.n, g.ho, g.wo, g.dil)
    assert float(R.gate_margin(n64["z"], n64["scale"], n64["shift"]).min()) > 1e-3          # the gate is decided in any arithmetic
    out = _Out(g, dtype, o["m"], rows)
    if split:
        check(lib.mvf_conv2d_nhwc_dgrad_bnsums_split(C.byref(d), _P(G["x"]), _P(G["x2"]), _P(G["w"]), _P(G["bias"]), _P(out.y), _P(G["z"]), _P(G["mean"]), _P(G["invstd"]),
                                                     _P(G["scale"]), _P(G["shift"]), _P(out.part), None, 0, None))
    else:
        check(lib.mvf_conv2d_nhwc_dgrad_bnsums(C.byref(d), _P(G["x"]), _P(G["w"]), _P(out.y), _P(G["z"]), _P(G["mean"]), _P(G["invstd"]), _P(G["scale"]), _P(G["shift"]),
                                               _P(out.part), None, 0, None))
    rec = _record(entry, dtype)
    _sync()
    if g.dil > 1:
        assert rec["launches"] == g.dil * g.dil
    y_ref, _ = R.dgrad_bnsums(n64["x"], n64["w"], dtype, n64["z"], n64["mean"], n64["invstd"], n64["scale"], n64["shift"], n64["bias"] if split else None,
                              acc=o["acc"], **o["geom"])
    y = out.stored()
    _check(entry, g, dtype, rec, "y", y, y_ref, TOL[dtype])
    gm = y * ((n64["scale"][None, :] * n64["z"] + n64["shift"][None, :]) > 0)
    xhat = (n64["z"] - n64["mean"][None, :]) * n64["invstd"][None, :]
    _check_sums(entry, g, dtype, rec, out.partials(), R.partials(o["runs"], gm, gm * xhat), second_bound=1e-4)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("g", DGRAD + FORWARD, ids=_gid)
def test_dgrad_bnsums(g, dtype):
    """y = the transposed convolution, gm = y_stored * [scale * z + shift > 0], partials of gm and gm * xhat; in_dil = 2: the four parity classes' partial
    rows back to back (three of them without a single tap for the 1x1 case)."""
    _dgrad_case("dgrad_bnsums", g, dtype, False)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("g", SPLIT, ids=_gid)
def test_dgrad_bnsums_split(g, dtype):
    """The same over the split operand [x2 | x] with a bias (the engine's dz3-free data gradient, train_engine.py dzfree_dgrad)."""
    _dgrad_case("dgrad_bnsums_split", g, dtype, True)


def test_direct_kernels_report_themselves():
    """The three direct paths ahead of the implicit GEMM (their arithmetic has its own tests) leave their own launch record; a refused call leaves none."""
    from mvfnet_amd import _lib
    lib, check = _lib_()
    g = _pw(8, 16, 16, 64, 128)                            # (csrc/pw_sums.hip wants at least 16 partial rows: M >= 2048)
    o = _ops(g, "bf16")
    G = o["gpu"]
    d = _desc(g, "bf16")
    rows = lib.mvf_conv2d_stats_rows(C.byref(d))
    out = _Out(g, "bf16", o["m"], rows)
    check(lib.mvf_conv2d_nhwc_fwd_stats(C.byref(d), _P(G["x"]), None, _P(G["w"]), None, _P(out.part), _P(G["kshift"]), None, 0, None))
    assert _record("fwd_stats_nostore_direct", "bf16")["family"] == "pw_sums"
    # the BatchNorm-backward sums come with a plain data gradient only: with a ReLU asked for there is no epilogue that computes them -> refused, nothing launched
    d.relu = 1
    rc = lib.mvf_conv2d_nhwc_dgrad_bnsums(C.byref(d), _P(G["x"]), _P(G["w"]), _P(out.y), _P(G["z"]), _P(G["mean"]), _P(G["invstd"]), _P(G["scale"]), _P(G["shift"]),
                                          _P(out.part), None, 0, None)
    assert rc == -5 and _record("dgrad_bnsums_relu_refused", "bf16", expect_launch=False)["launches"] == 0          # MVF_EUNSUPPORTED
    d.relu = 0
    g3 = _c3(2, 8, 8, 64, 64, 3, 1)
    o3 = _ops(g3, "bf16")
    out3 = _Out(g3, "bf16", o3["m"], 1)
    d3 = _desc(g3, "bf16")
    check(lib.mvf_conv2d_nhwc_fwd_ws(C.byref(d3), _P(o3["gpu"]["x"]), None, _P(o3["gpu"]["w"]), None, None, _P(out3.y), None, 0, None))
    r3 = _record("fwd_ws_plain_direct", "bf16")
    assert (r3["family"], r3["asked"], r3["run"]) == ("c3x3_c64", 2, 2)
    _sync()
    _check("fwd_ws_plain_direct", g3, "bf16", r3, "y", out3.stored(), R.fwd(o3["n64"]["x"], o3["n64"]["w"], "bf16", acc=o3["acc"], **o3["geom"]), TOL["bf16"])
    n, h, w = 2, 32, 32                                    # the stem: 7 x 1 taps over the 32-"channel" view of the padded NHWC4 input, stride 2
    hp, wp_ = h + 6, (w + 6 + 2 + 1) // 2 * 2
    ho, wo = (h + 6 - 7) // 2 + 1, (w + 6 - 7) // 2 + 1
    xp = torch.zeros(n, hp, wp_, 4, device="cuda", dtype=torch.bfloat16)
    wst = torch.zeros(64, 7, 8, 4, device="cuda", dtype=torch.bfloat16)
    ys = torch.empty(n * ho * wo, 64, device="cuda", dtype=torch.bfloat16)
    ds = _lib.ConvDesc(n, hp, wp_, 32, 64, 7, 1, 2, 0, ho, wo, 4, 1, 1, 0, 0, 0, 0, 0)
    check(lib.mvf_conv2d_nhwc_fwd_ws(C.byref(ds), _P(xp), None, _P(wst), _P(G["bias"]), None, _P(ys), None, 0, None))
    rs = _record("stem_bias_relu_direct", "bf16")
    assert (rs["family"], rs["run"]) == ("stem_direct", 4)
    _sync()
    d.cout = 6                                             # refused before any launch
    assert lib.mvf_conv2d_nhwc_fwd_ws(C.byref(d), _P(G["x"]), None, _P(G["w"]), None, None, _P(out.y), None, 0, None) != 0
    info = _lib.ConvLaunchInfo()
    check(lib.mvf_conv2d_last_launch(C.byref(info)))
    assert info.launches == 0 and info.family == 0
    assert lib.mvf_conv2d_last_launch(None) == -1


# ------------------------------------------------------------------------------------------------ forced families
LEGS = {
    "register_staged_only": dict(conv_glds=0, conv_glds1=0, conv_big2=0),
    "register_staged_only_exact_fp32_mfma": dict(conv_glds=0, conv_glds1=0, conv_big2=0, f32_x3=0),
    "lds_dma_1buf_everywhere_sums_and_fp32_included": dict(conv_glds1=1000, conv_big2=0, f32_x3=0),
    "lds_dma_2buf_everywhere": dict(conv_glds=1, conv_glds_nb=2, conv_glds1=0, conv_big2=0, f32_x3=0),
    "tile_256x256_four_phase": dict(conv_big2=1, conv_big2_force=1),
    "tile_256x256_two_barrier": dict(conv_big2=1, conv_big2_force=1, conv_p4=0),
    "generic_epilogue_general_loader": dict(conv_epi=0),
    "specialised_epilogue_without_pointwise_loader": dict(conv_epi=1),
    "generic_epilogue_with_pointwise_loader": dict(conv_epi=2),
    "double_buffered_kernels": dict(conv_lowk=0, f32_x3=0),
}
_leg_results = {}


def _run_leg(leg, tmp_dir):
    """This file's in-process cases again in a fresh child process under the leg's policy (the policies are read once per process); memoised."""
    if leg not in _leg_results:
        cov = os.path.join(str(tmp_dir), "coverage_%s.jsonl" % leg)
        env = policy_env(**LEGS[leg])
        env[COVERAGE_ENV] = cov
        if env.get(ERRORS_ENV):
            env[ERRORS_ENV] = env[ERRORS_ENV] + "." + leg
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-m", "gpu", "-k", "not forced and not coverage_matrix",
                            "-p", "no:cacheprovider"], env=env, capture_output=True, text=True, timeout=600)
        recs = [json.loads(line) for line in open(cov)] if os.path.exists(cov) else []
        _leg_results[leg] = (r.returncode, r.stdout[-3000:] + r.stderr[-2000:], recs)
    return _leg_results[leg]


@pytest.fixture(scope="module")
def leg_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("conv_epilogue_legs")


@pytest.mark.parametrize("leg", list(LEGS))
def test_epilogues_under_forced_kernel_families(leg, leg_dir):
    rc, tail, recs = _run_leg(leg, leg_dir)
    assert rc == 0, tail
    assert recs


# Epilogues each launcher instantiates (csrc/conv_nhwc.hip with_epi<...>); 0 = the generic run-time epilogue every family has
EPI_T256 = [1, 2, 3, 4, 5, 6]
EPI_128 = [1, 2, 3, 4, 5, 6, 8, 9, 10, 12]
# (family, buffers, storage types, pointwise-loader settings, epilogues)
MATRIX = [
    ("reg", 1, ["bf16", "f32"], [0, 1], EPI_128 + [0]),          # (fp32: only with f32_x3=0)
    ("x3", 1, ["f32"], [0, 1], EPI_128 + [0]),
    ("lds_dma", 1, ["bf16", "f32"], [0, 1], EPI_128 + [0]),
    ("lds_dma", 2, ["bf16", "f32"], [0, 1], EPI_128 + [0]),
    ("t256_2b", 2, ["bf16"], [0], EPI_T256 + [0]),
    ("t256_p4", 2, ["bf16"], [0, 1], EPI_T256 + [0]),
    ("dbuf", 2, ["f32"], [0], [0]),
    ("dbuf_pf2", 2, ["bf16"], [0], [0]),
]
# What the matrix leaves out, each with its reason.  A combination that a later policy change makes unreachable FAILS test_coverage_matrix by name.
NOT_IN_MATRIX = (
    "fp32 on the 256 x 256 tiles: the four-phase loop is written for bf16 (launch_p4 refuses fp32) and launch_conv sends only bf16 launches to either 256 x 256 kernel",
    "epilogues 8 / 9 / 10 on the 256 x 256 tiles: launch_conv keeps the BatchNorm-apply / BatchNorm-backward-on-recompute launches off them (their with_epi lists end at 6)",
    "scattered parity classes on the 256 x 256 tiles: launch_conv requires contiguous output rows there (o_s <= 0)",
    "the pointwise loader on the two-barrier 256 x 256 kernel: conv_igemm_big2_kernel has no PW instance",
    "the half-K LDS-DMA variant (conv_igemm_glds_kernel<.., HALFK>): it only takes the stem's 7 x 1 view, whose arithmetic has its own tests (test_conv_gpu.py)",
    "fp32 on the register-staged family outside f32_x3=0, and the x3 family in bf16: x3 IS the fp32 storage type's register-staged kernel",
    "the double-buffered, stream-K, generic-shape and MVF-loader kernels beyond epilogue 0 / their one inference epilogue: they instantiate nothing else",
)


def _required():
    return [(fam, nb, dt, pw, e) for fam, nb, dts, pws, epis in MATRIX for dt in dts for pw in pws for e in epis]


def test_coverage_matrix(leg_dir):
    """Every kernel family conv_nhwc.hip instantiates was reached by the forced legs with every epilogue of its with_epi list, with both loaders and in both
    storage types where that instance exists; epilogue 12 reached the 256 x 256 tiles and ran there as the generic epilogue 0."""
    seen = set()
    asked12_on_t256 = set()
    for leg in LEGS:
        rc, tail, recs = _run_leg(leg, leg_dir)
        assert rc == 0, "leg %s: %s" % (leg, tail)
        for r in recs:
            seen.add((r["family"], r["buffers"], r["dtype"], r["pw"], r["run"]))
            if r["asked"] == 12 and r["family"] in ("t256_2b", "t256_p4"):
                assert r["run"] == 0
                asked12_on_t256.add(r["family"])
    missing = [k for k in _required() if k not in seen]
    assert not missing, "never reached (family, buffers, dtype, pointwise loader, epilogue run): %s" % missing
    assert asked12_on_t256 == {"t256_2b", "t256_p4"}
