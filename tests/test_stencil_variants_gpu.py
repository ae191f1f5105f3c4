"""GPU: every kernel and launch variant of the channels-last MVF stencil (mvf_nhwc_stencil, _gate, _gate_colsums, _stats) and of the tap gradients
(mvf_nhwc_tapgrad) -- csrc/mvf_nhwc.hip -- through the C ABI against the INDEPENDENT fp64 reference tests/stencil_ref.py (proved against the oracle in
tests/test_stencil_ref_cpu.py), at the smallest shapes that reach each branch, in both storage types: in this process under the default launch policy and
again in one child process per forced policy (the walk kernels, the tiled kernel on few-clip shapes, the (clip, band) tap-gradient kernel).  After every call
the host-side launch record (mvf_nhwc_stencil_last_launch / mvf_nhwc_tapgrad_last_launch) says which kernel ran; under the default policy each case asserts it.

Every call: `out`, the partial sums and the tap gradients are NaN before and must be written completely; `out` and the tap-gradient workspace (exactly
mvf_nhwc_tapgrad_workspace_bytes of NaN) are followed by a 4 KiB canary that must be unchanged; channels >= cs of a wider `out` keep their prefill bit for bit
(or equal x when x_c == out_c: the tail copy); where an output gate bit is 0 the output is +-0.  Operands are rounded to the storage type on the CPU and
the reference is evaluated on exactly those values.

Two operand classes.  `int`: x, dy in {-2..2}, taps in {-1, 0, 1}, addend in {-4..4}, K in {-2..2} -- every product and sum is an integer below 256
(outputs) or 2^24 (sums), exact in bf16 and fp32 in any order, so outputs, partial-row sums and tap gradients must EQUAL the reference.  `rnd`: normal data,
taps in [-1, 1], scale in [0.5, 1.5]; per element |got - ref| <= B with B = 32 * 2^-24 * A (fp32) or 2^-8 |ref| + 32 * 2^-24 * A (bf16: one rounding of the
stored value + fp32 error that crosses a rounding boundary), A = the reference expression on absolute values; 32 counts the roundings an element can see
(9 products, 8 adds, the BatchNorm fma, 4 hard-swish operations, the addend).  Sums against the fp64 sums of the values the kernel STORED:
L * 2^-24 * sum |terms|, L = the terms per channel one partial row covers, from the launch record.  Measured maxima: profiles/stencil_errors.txt."""
import collections
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import stencil_ref as R
from helpers import policy_env

pytestmark = pytest.mark.gpu

COVERAGE_ENV = "MVF_STENCIL_COVERAGE"     # a file: this module appends one JSON line per stencil / tap-gradient call (the forced legs' children)
ERRORS_ENV = "MVF_STENCIL_ERRORS"         # a file: one JSON line per measured error against its bound (tooling: profiles/stencil_errors.txt)
POLICY = os.environ.get("MVF_POLICY", "").lower().replace(" ", "")
# the plans asserted per case are those of the DEFAULT policy: a child of a forced leg (or a caller's own MVF_POLICY) checks the arithmetic only
DEFAULT_POLICY = not any(k in POLICY for k in ("stencil", "tapgrad"))
WALK_FORCED = "stencil_chunked=0" in POLICY           # no chunked kernel: a statistics launch outside the tiled kernel is MVF_EUNSUPPORTED
EINVAL, EWS, EUNSUPPORTED = -1, -3, -5
CANARY = 4096
U24 = 2.0 ** -24
_seen = []                                            # this process's own calls, for test_coverage_matrix

# clips of T frames (an int, or (fp32, bf16): the chunked kernel takes 4 / 8 frames per chunk) of h x w pixels; the slice is cs of x_c channels, out has
# out_c, the addend add_c; x_off / tap_off: the operand starts that many ELEMENTS / floats into its allocation
Geo = collections.namedtuple("Geo", "name clips T h w cs x_c out_c add_c mode share x_off tap_off")


def _g(name, clips, T, h, w, cs, x_c=0, out_c=0, add_c=0, mode=7, share=False, x_off=0, tap_off=0):
    out_c = out_c or cs
    return Geo(name, clips, T, h, w, cs, x_c or cs, out_c, add_c or out_c, mode, share, x_off, tap_off)


# what a variant passes: hs = scale / shift, add = an addend, bits = its gate bits, gate = the output gate, sums = column sums, stats = statistics (K or NULL)
VARIANTS = {
    "plain": {}, "hs": dict(hs=1), "flip": dict(flip=1), "add": dict(flip=1, add=1), "addbits": dict(add=1, bits=1), "hs_add": dict(hs=1, add=1),
    "gate": dict(flip=1, add=1, bits=1, gate=1), "gate_hs": dict(hs=1, gate=1), "colsums": dict(flip=1, add=1, bits=1, gate=1, sums=1),
    "colsums_noadd": dict(gate=1, sums=1), "stats_k": dict(stats=1, K=1), "stats_0": dict(stats=1),
}
CATEGORY = {"plain": "plain", "gate": "flip+addend+gate", "colsums": "colsums", "stats_k": "stats", "stats_0": "stats"}
ALL = ["plain", "hs", "flip", "add", "addbits", "hs_add", "gate", "gate_hs", "colsums", "colsums_noadd", "stats_k", "stats_0"]

# (geometry, variants)
WALK1 = [
    (_g("cs3_c6", 2, 4, 3, 4, 3, 6, 6), ["plain", "hs", "flip", "add"]),                                   # x_c == out_c: the tail copy
    (_g("cs6_c10", 2, 3, 2, 5, 6, 10, 6, 7), ["plain", "hs", "add"]),                                        # pitches % 4 != 0
    (_g("cs8_xoff1", 1, 5, 3, 3, 8, 8, 8, x_off=1), ["plain", "flip"]),                                      # a 4-channel shape, x misaligned by one element
    (_g("cs6_bits", 2, 4, 3, 4, 6, 10, 8, 8), ["addbits"]),                                                  # gate bits read at c0 & 3 != 0
    (_g("cs5_t1_th", 3, 1, 4, 1, 5, 7, 5, mode=3), ["plain", "flip"]),
]
WALK4 = [
    (_g("cs8_tapoff", 2, 5, 3, 4, 8, 12, 8, 12, tap_off=1), ["plain", "hs", "flip", "add", "addbits", "gate", "gate_hs"]),
    (_g("cs12_tapoff_th", 1, 4, 5, 3, 12, 12, 20, mode=3, tap_off=1), ["plain", "gate"]),
]
CHUNKED = [
    (_g("t1_cs4", 2, (1, 1), 3, 4, 4, 8, 4), ["plain", "flip", "stats_k"]),                                  # wide -> compact
    (_g("1x7_cs12", 2, (4, 3), 1, 7, 12, 16, 12), ["plain", "gate", "stats_k", "colsums"]),                  # cg = 3 under cgp = 4: one idle lane
    (_g("5x1_cs12", 1, (5, 8), 5, 1, 12, 12, 20), ["flip", "gate", "colsums", "hs"]),                        # compact -> wide (the backward)
    (_g("1x1_cs4", 2, (6, 12), 1, 1, 4), ["plain", "stats_0", "gate"]),
    (_g("1x3_cs1028", 1, (4, 8), 1, 3, 1028), ["plain", "gate", "stats_k", "colsums"]),                      # grid_y = 2
    (_g("9x11_cs256", 2, (5, 3), 9, 11, 256, 264, 264, 260), ALL),                                           # 25 bands per clip; wide -> wide: the tail copy
    (_g("4x5_cs8_t", 2, (4, 8), 4, 5, 8, 8, 12, mode=1), ["plain", "flip", "stats_k", "gate"]),              # mode T: w_h, w_w NULL
    (_g("4x5_cs8_th", 2, (6, 12), 4, 5, 8, 16, 8, mode=3), ["plain", "hs", "gate", "colsums"]),              # mode TH: w_w NULL
    (_g("3x3_cs8_wide", 2, (4, 8), 3, 3, 8, 16, 12, 20), ["plain", "gate", "colsums"]),                      # wide -> wide with three different pitches: no tail copy
    (_g("5x5_cs16_share", 2, (5, 3), 5, 5, 16, share=True), ["plain", "flip", "colsums", "stats_0"]),       # one tap pointer three times
]
# bf16 shapes on which the tiled kernel's plan exists under the default policy (>= 150 workgroups, a tile of >= 8 KiB)
LDS = [
    (_g("c75_t4_4x4_cs128", 75, 4, 4, 4, 128, 136, 128, 132), ALL),                                          # CW = 64, two channel slabs; wide -> compact
    (_g("c50_t8_4x4_cs96", 50, 8, 4, 4, 96, 96, 104), ["flip", "gate", "colsums", "plain"]),                 # CW = 32; compact -> wide
    (_g("c50_t4_6x8_cs48_th", 50, 4, 6, 8, 48, 56, 56, mode=3), ["plain", "stats_k", "gate", "hs"]),         # CW = 16; wide -> wide: the tail copy
    (_g("c75_t16_2x2_cs128_share", 75, 16, 2, 2, 128, share=True), ["plain", "colsums", "stats_0", "gate"]),
]
# ... many tiny clips of 16 / 32 / 64 channels: their tiles are smaller than the 8 KiB the statistics' reduction reuses, or make fewer than 150 workgroups, so
# the plan refuses them (tile_plan = 0) and they stay on the chunked kernel
LDS_TINY = [
    (_g("c150_t4_4x4_cs16", 150, 4, 4, 4, 16), ["plain", "gate", "stats_k", "colsums"]),
    (_g("c75_t4_4x4_cs64", 75, 4, 4, 4, 64), ["plain", "gate", "stats_k", "colsums"]),
    (_g("c40_t8_4x4_cs32", 40, 8, 4, 4, 32), ["plain", "colsums"]),
    (_g("c10_t16_4x4_cs16", 10, 16, 4, 4, 16), ["plain", "stats_0"]),
]
# few clips, several bands: chunked under the default policy, tiled under stencil_lds_minwg=1
FEWCLIP = [
    (_g("c2_t4_9x5_cs64", 2, 4, 9, 5, 64, 72, 64), ["plain", "hs", "gate", "colsums", "stats_k"]),           # H = 9: bands of 5 and 4 rows
    (_g("c1_t16_14x14_cs64", 1, 16, 14, 14, 64), ["plain", "gate", "stats_0", "colsums"]),                   # 64 channels do not fit: 32-channel tiles of 2 rows
    (_g("c3_t8_9x3_cs32_th", 3, 8, 9, 3, 32, 40, 40, mode=3), ["flip", "colsums", "stats_k"]),
]
DTYPES = ["f32", "bf16"]
CLASSES = ["int", "rnd"]


def _params(lst, dtypes=DTYPES):
    out = []
    for g, variants in lst:
        for v in variants:
            for dt in dtypes:
                for cls in CLASSES:
                    if cls == "int" and VARIANTS[v].get("hs"):
                        continue                                      # (the exact class has no scale / shift)
                    out.append(pytest.param(g, v, dt, cls, id="%s-%s-%s-%s" % (g.name, v, dt, cls)))
    return out


# ------------------------------------------------------------------------------------------------ operands (one set per shape, storage type and class, shared, never modified)
_ops_cache = {}
_ref_cache = {}


def _tdt(dtype):
    return torch.float32 if dtype == "f32" else torch.bfloat16


def _T(g, dtype):
    return g.T if isinstance(g.T, int) else g.T[0 if dtype == "f32" else 1]


def _dev(t, off=0):
    """t on the device, `off` elements into a larger allocation -> (keep-alive, address)"""
    buf = torch.zeros(t.numel() + 16, dtype=t.dtype, device="cuda")
    buf[off:off + t.numel()] = t.flatten().cuda()
    return buf, buf.data_ptr() + off * t.element_size()


def _ops(g, dtype, cls):
    key = (g, dtype, cls)
    if key in _ops_cache:
        return _ops_cache[key]
    T = _T(g, dtype)
    m = g.clips * T * g.h * g.w
    gen = torch.Generator().manual_seed(sum(v for v in g[1:] if isinstance(v, int)) * 2 + T + (cls == "int"))
    td = _tdt(dtype)
    o = dict(T=T, m=m, desc=R.Desc(g.clips * T, g.h, g.w, T, g.cs, g.mode))
    if cls == "int":
        rnd = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=gen).float()      # noqa: E731
        o["x"], o["dy"], o["add"] = rnd(-2, 2, m, g.x_c).to(td), rnd(-2, 2, m, g.out_c).to(td), rnd(-4, 4, m, g.add_c).to(td)
        taps = [rnd(-1, 1, g.cs, 3) for _ in range(3)]
        o["K"] = rnd(-2, 2, g.cs)
    else:
        o["x"], o["dy"], o["add"] = (torch.randn(m, c_, generator=gen).to(td) for c_ in (g.x_c, g.out_c, g.add_c))      # (every column of a pitch holds data)
        taps = [torch.rand(g.cs, 3, generator=gen) * 2 - 1 for _ in range(3)]
        o["K"] = torch.randn(g.cs, generator=gen)
        o["scale"], o["shift"] = torch.rand(g.cs, generator=gen) + 0.5, torch.randn(g.cs, generator=gen) * 0.5
    if g.share:
        taps = [taps[0]] * 3
    o["taps"] = taps
    o["abits"] = torch.randint(0, 256, (m, g.add_c // 4), generator=gen, dtype=torch.uint8) if g.add_c % 4 == 0 else None
    o["gbits"] = torch.randint(0, 256, (m, g.out_c // 4), generator=gen, dtype=torch.uint8) if g.out_c % 4 == 0 else None
    d = {}
    d["x"] = _dev(o["x"], g.x_off)
    d["add"] = _dev(o["add"])
    d["wt"] = _dev(taps[0], g.tap_off)
    d["wh"] = d["wt"] if g.share else _dev(taps[1], g.tap_off)
    d["ww"] = d["wt"] if g.share else _dev(taps[2], g.tap_off)
    for k in ("K", "scale", "shift", "abits", "gbits"):
        if o.get(k) is not None:
            d[k] = _dev(o[k])
    o["dev"] = d
    _ops_cache[key] = o
    return o


def _np(t):
    return None if t is None else t.double().numpy() if t.is_floating_point() else t.numpy()


def _ref(g, dtype, cls, variant):
    key = (g, dtype, cls, variant)
    if key not in _ref_cache:
        o, v = _ops(g, dtype, cls), VARIANTS[variant]
        wt, wh, ww = (_np(t) for t in o["taps"])
        _ref_cache[key] = R.stencil(_np(o["x"]), o["desc"], wt, wh if g.mode & 2 else None, ww if g.mode & 4 else None, flip=v.get("flip", 0),
                                    scale=_np(o["scale"]) if v.get("hs") else None, shift=_np(o["shift"]) if v.get("hs") else None,
                                    addend=_np(o["add"]) if v.get("add") else None, addend_c=g.add_c, addend_bits=_np(o["abits"]) if v.get("bits") else None,
                                    out_gate_bits=_np(o["gbits"]) if v.get("gate") else None)
    return _ref_cache[key]


# ------------------------------------------------------------------------------------------------ the calls
def _nan_buffer(nelem, td):
    """nelem elements of NaN followed by a canary -> (raw bytes, the elements)"""
    nbytes = nelem * torch.empty(0, dtype=td).element_size()
    raw = torch.empty(nbytes + CANARY, dtype=torch.uint8, device="cuda")
    raw[nbytes:] = 0xA5
    view = raw[:nbytes].view(td)
    view.fill_(float("nan"))
    return raw, view


def _canary_ok(raw):
    return bool((raw[-CANARY:] == 0xA5).all())


def _P(addr):
    return C.c_void_p(addr)


def _mvf_desc(g, dtype, T):
    from mvfnet_amd import _lib
    return _lib.MvfDesc(g.clips * T, g.x_c, g.h, g.w, T, g.cs, g.mode, _lib.MVF_NHWC, _lib.MVF_F32 if dtype == "f32" else _lib.MVF_BF16)


def _log(env, rec):
    if os.environ.get(env):
        with open(os.environ[env], "a") as f_:
            f_.write(json.dumps(rec) + "\n")


def _stencil_record(g, dtype, cls, variant):
    from mvfnet_amd import _lib
    info = _lib.StencilLaunchInfo()
    _lib.check(_lib.lib.mvf_nhwc_stencil_last_launch(C.byref(info)))
    rec = {k: getattr(info, k) for k, _ in info._fields_}
    rec.update(kind="stencil", kernel=_lib.STENCIL_KERNELS[info.kernel], case=g.name, variant=variant, category=CATEGORY.get(variant, "other"), dtype=dtype, cls=cls,
               rec_dtype=info.dtype)
    _seen.append(rec)
    _log(COVERAGE_ENV, rec)
    return rec


def _measure(what, g, dtype, cls, variant, kernel, err, bound):
    """assert err <= bound element-wise; the largest fraction of the bound goes to the errors file"""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    nz = bound > 0
    ratio = float((err[nz] / bound[nz]).max()) if nz.any() else 0.0
    _log(ERRORS_ENV, dict(what=what, case=g.name, dtype=dtype, cls=cls, variant=variant, kernel=kernel, ratio=ratio, max_err=float(err.max()) if err.size else 0.0,
                          policy=POLICY))
    bad = err > bound
    assert not bad.any(), "%s %s %s %s %s on %s: %d of %d elements beyond their bound, worst %.3g x the bound (first at %s: error %.3g, bound %.3g)" % (
        what, g.name, variant, dtype, cls, kernel, int(bad.sum()), bad.size, float((err[bad] / np.maximum(bound[bad], 1e-300)).max()), np.argwhere(bad)[0].tolist(),
        float(err[bad][0]), float(bound[bad][0]))


def _tile_plan(g, dtype, T):
    from mvfnet_amd import _lib
    rb, cw = C.c_int(0), C.c_int(0)
    on = _lib.lib.mvf_nhwc_stencil_tile_plan(C.byref(_mvf_desc(g, dtype, T)), g.x_c, g.out_c, C.byref(rb), C.byref(cw))
    return on, rb.value, cw.value


def _run_stencil(g, variant, dtype, cls, expect, expect_rc=0, x_off=None):
    """One stencil call of `variant` with every check of the module's docstring.  expect: the kernel the default policy takes ("tiled?" = what the plan query says)."""
    from mvfnet_amd import _lib
    lib = _lib.lib
    o, v = _ops(g, dtype, cls), VARIANTS[variant]
    T, m, dev, td = o["T"], o["m"], o["dev"], _tdt(dtype)
    d = _mvf_desc(g, dtype, T)
    raw_out, out = _nan_buffer(m * g.out_c, td)
    prefill = out.clone()
    nul = _P(0)
    x_moved = None if x_off is None else _dev(o["x"], x_off)           # (kept alive until the call has finished)
    x = _P(dev["x"][1] if x_moved is None else x_moved[1])
    wt, wh, ww = _P(dev["wt"][1]), (_P(dev["wh"][1]) if g.mode & 2 else nul), (_P(dev["ww"][1]) if g.mode & 4 else nul)
    scale, shift = (_P(dev["scale"][1]), _P(dev["shift"][1])) if v.get("hs") else (nul, nul)
    add = _P(dev["add"][1]) if v.get("add") else nul
    abits = _P(dev["abits"][1]) if v.get("bits") else nul
    gbits = _P(dev["gbits"][1]) if v.get("gate") else nul
    flip = v.get("flip", 0)
    want_sums = v.get("sums") or v.get("stats")
    rows = lib.mvf_nhwc_stencil_stats_rows(C.byref(d), g.x_c, g.out_c) if want_sums else 0
    raw_part, part = _nan_buffer(max(g.cs * rows * 2, 1), torch.float32)
    if v.get("sums"):
        rc = lib.mvf_nhwc_stencil_gate_colsums(C.byref(d), x, g.x_c, _P(out.data_ptr()), g.out_c, wt, wh, ww, flip, add, g.add_c, abits, gbits, _P(part.data_ptr()), None)
    elif v.get("stats"):
        rc = lib.mvf_nhwc_stencil_stats(C.byref(d), x, g.x_c, _P(out.data_ptr()), g.out_c, wt, wh, ww, _P(part.data_ptr()), _P(dev["K"][1]) if v.get("K") else nul, None)
    elif v.get("gate"):
        rc = lib.mvf_nhwc_stencil_gate(C.byref(d), x, g.x_c, _P(out.data_ptr()), g.out_c, wt, wh, ww, scale, shift, flip, add, g.add_c, abits, gbits, None)
    else:
        rc = lib.mvf_nhwc_stencil(C.byref(d), x, g.x_c, _P(out.data_ptr()), g.out_c, wt, wh, ww, scale, shift, flip, add, g.add_c, abits, None)
    rec = _stencil_record(g, dtype, cls, variant)
    torch.cuda.synchronize()
    assert _canary_ok(raw_out) and _canary_ok(raw_part), "written past the end of out / the partial sums"
    if expect_rc == 0 and WALK_FORCED and want_sums and rc == EUNSUPPORTED:
        expect_rc = EUNSUPPORTED                                    # (no chunked kernel under this policy)
    if expect_rc:
        assert rc == expect_rc, (rc, lib.mvf_last_error())
        assert rec["launches"] == 0 and rec["kernel"] == "none", rec
        assert bool(torch.isnan(out).all()) and bool(torch.isnan(part).all()), "a refused call wrote its outputs"
        return rec
    assert rc == 0, lib.mvf_last_error()
    tail_copy = g.x_c == g.out_c and g.out_c > g.cs
    # ---- the record
    assert rec["launches"] == (2 if tail_copy else 1) and rec["kernel"] != "none", rec
    assert rec["rec_dtype"] == (_lib.MVF_F32 if dtype == "f32" else _lib.MVF_BF16)
    flags = (_lib.STENCIL_FLIP if flip else 0) | (_lib.STENCIL_HSWISH if v.get("hs") else 0) | (_lib.STENCIL_ADDEND if v.get("add") else 0) | \
            (_lib.STENCIL_ADDEND_BITS if v.get("bits") else 0) | (_lib.STENCIL_OUT_GATE if v.get("gate") else 0) | (_lib.STENCIL_STATS if want_sums else 0) | \
            (_lib.STENCIL_TAIL_COPY if tail_copy else 0)
    assert rec["flags"] == flags, (rec, flags)
    assert rec["partial_rows"] == rows and rec["grid_x"] == g.clips * rec["bands"] and rec["grid_x"] > 0 and rec["grid_y"] > 0, (rec, rows)
    if DEFAULT_POLICY:
        if expect == "tiled?":
            on, rb, cw = _tile_plan(g, dtype, T)
            expect = "lds" if on and dtype == "bf16" else "chunked"
        assert rec["kernel"] == expect, (rec, expect)
    if rec["kernel"] == "lds":
        on, rb, cw = _tile_plan(g, dtype, T)
        assert on == 1 and (rec["rows_per_band"], rec["chan_per_wg"]) == (rb, cw) and rec["frames_per_chunk"] == 0, (rec, rb, cw)
        assert rec["bands"] == -(-g.h // rb) and rec["pixels_per_wg"] == rb * g.w and rec["grid_y"] == g.cs // cw, rec
    else:
        assert rec["frames_per_chunk"] == ((4 if dtype == "f32" else 8) if rec["kernel"] == "chunked" else 0) and rec["rows_per_band"] == rec["chan_per_wg"] == 0, rec
        assert rec["bands"] == -(-(g.h * g.w) // rec["pixels_per_wg"]), rec
    # ---- the output
    got_t = out.view(m, g.out_c).cpu()
    got = got_t[:, :g.cs].double().numpy()
    assert np.isfinite(got).all(), "%d of %d output elements were not written" % (int((~np.isfinite(got)).sum()), got.size)
    ref, A = _ref(g, dtype, cls, variant)
    if g.out_c > g.cs:
        it = torch.int32 if dtype == "f32" else torch.int16
        if tail_copy:
            assert torch.equal(got_t[:, g.cs:].contiguous().view(it), o["x"][:, g.cs:].contiguous().view(it)), "x_c == out_c: channels >= cs of out are not those of x"
        else:
            assert torch.equal(got_t[:, g.cs:].contiguous().view(it), prefill.view(m, g.out_c).cpu()[:, g.cs:].contiguous().view(it)), "channels >= cs of out were written"
    if v.get("gate"):
        off = R.unpack_bits(_np(o["gbits"]), g.cs) == 0
        assert off.any() and (got[off] == 0).all(), "an output whose gate bit is 0 is not zero"
    if cls == "int":
        assert np.abs(ref).max() < 256 and (ref == np.round(ref)).all()
        _measure("y", g, dtype, cls, variant, rec["kernel"], np.abs(got - ref), np.zeros_like(ref))
    else:
        B = 32 * U24 * A + (2.0 ** -8 * np.abs(ref) if dtype == "bf16" else 0.0)
        _measure("y", g, dtype, cls, variant, rec["kernel"], np.abs(got - ref), B)
    # ---- the partial sums, against the fp64 sums of what was stored
    if want_sums:
        p = part.view(g.cs, rows, 2).double().cpu().numpy()
        assert np.isfinite(p).all(), "%d of %d partial sums were not written" % (int((~np.isfinite(p)).sum()), p.size)
        K = _np(o["K"]) if v.get("K") else None
        s1, s2 = R.stats(got, K)
        a1 = np.abs(got - (0.0 if K is None else K)).sum(axis=0)
        what = "colsums" if v.get("sums") else "stats"
        if cls == "int":
            assert a1.max() < 2 ** 24 and s2.max() < 2 ** 24
            bound1 = bound2 = np.zeros(g.cs)
        else:
            L = T * rec["pixels_per_wg"]
            bound1, bound2 = L * U24 * a1, L * U24 * s2
        _measure(what + "_sum", g, dtype, cls, variant, rec["kernel"], np.abs(p[:, :, 0].sum(axis=1) - s1), bound1)
        _measure(what + "_sumsq", g, dtype, cls, variant, rec["kernel"], np.abs(p[:, :, 1].sum(axis=1) - s2), bound2)
    return rec


# ------------------------------------------------------------------------------------------------ stencil cases
@pytest.mark.parametrize("g,variant,dtype,cls", _params(WALK1))
def test_walk1_shapes(g, variant, dtype, cls):
    """mvf_nhwc_apply<T, 1>: slices or pitches that are no multiple of 4, a misaligned x."""
    _run_stencil(g, variant, dtype, cls, "walk1")


@pytest.mark.parametrize("dtype", DTYPES)
def test_walk1_refuses_the_output_gate_and_the_statistics(dtype):
    _run_stencil(WALK1[3][0], "gate_hs", dtype, "rnd", "walk1", expect_rc=EUNSUPPORTED)                  # (out_c = 8 has gate bytes; x_c = 10 keeps the walk)
    _run_stencil(WALK1[0][0], "stats_0", dtype, "rnd", "walk1", expect_rc=EUNSUPPORTED)
    _run_stencil(WALK1[2][0], "colsums_noadd", dtype, "int", "walk1", expect_rc=EUNSUPPORTED)        # (cs = 8, x off by one element)


@pytest.mark.parametrize("g,variant,dtype,cls", _params(WALK4))
def test_walk4_shapes(g, variant, dtype, cls):
    """mvf_nhwc_apply<T, 4> in this process: tap pointers 4 bytes into their allocation are not 16-byte aligned."""
    _run_stencil(g, variant, dtype, cls, "walk4")


@pytest.mark.parametrize("dtype", DTYPES)
def test_walk4_refuses_the_statistics(dtype):
    _run_stencil(WALK4[0][0], "stats_k", dtype, "int", "walk4", expect_rc=EUNSUPPORTED)
    _run_stencil(WALK4[0][0], "colsums", dtype, "int", "walk4", expect_rc=EUNSUPPORTED)


@pytest.mark.parametrize("g,variant,dtype,cls", _params(CHUNKED))
def test_chunked_shapes(g, variant, dtype, cls):
    """mvf_nhwc_apply_chunked<float, 4> / <bf16_t, 8>: T below, at and above a chunk, idle channel lanes, two channel slabs, many bands."""
    _run_stencil(g, variant, dtype, cls, "chunked")


@pytest.mark.parametrize("g,variant,dtype,cls", _params(LDS, ["bf16"]))
def test_lds_shapes(g, variant, dtype, cls):
    """mvf_nhwc_apply_lds<T, 64 | 32 | 16> under the default policy: the record names the tile mvf_nhwc_stencil_tile_plan promises."""
    if DEFAULT_POLICY:
        assert _tile_plan(g, dtype, _T(g, dtype))[0] == 1
    _run_stencil(g, variant, dtype, cls, "lds")


@pytest.mark.parametrize("g,variant,dtype,cls", _params(LDS_TINY, ["bf16"]))
def test_lds_tiny_clip_shapes(g, variant, dtype, cls):
    _run_stencil(g, variant, dtype, cls, "tiled?")


@pytest.mark.parametrize("g,variant,dtype,cls", _params(FEWCLIP))
def test_fewclip_shapes(g, variant, dtype, cls):
    _run_stencil(g, variant, dtype, cls, "tiled?")


def test_refusals():
    g = LDS[0][0]
    # a statistics launch on a tiled shape names the tiled kernel's partial rows: x 8 bytes into its allocation cannot take that kernel
    if DEFAULT_POLICY:
        _run_stencil(g, "stats_k", "bf16", "int", "lds", expect_rc=EINVAL, x_off=4)
        _run_stencil(g, "colsums", "bf16", "int", "lds", expect_rc=EINVAL, x_off=4)
    # ... without partial rows the same operands run, on the chunked kernel
    rec = _run_stencil(g, "plain", "bf16", "int", "chunked", x_off=4)
    assert not DEFAULT_POLICY or rec["kernel"] == "chunked"
    gc = CHUNKED[1][0]
    _run_stencil(gc._replace(add_c=8), "add", "f32", "int", "chunked", expect_rc=EINVAL)            # addend pitch < cs = 12
    from mvfnet_amd import _lib
    o = _ops(gc, "f32", "int")
    d = _mvf_desc(gc, "f32", o["T"])
    raw, out = _nan_buffer(o["m"] * gc.out_c, torch.float32)
    dev = o["dev"]
    rc = _lib.lib.mvf_nhwc_stencil(C.byref(d), _P(dev["x"][1]), gc.x_c, _P(out.data_ptr()), gc.out_c, _P(dev["wt"][1]), _P(dev["wh"][1]), _P(dev["ww"][1]), None, None, 0,
                                   None, 0, _P(dev["abits"][1]), None)                              # bits without an addend
    rec = _stencil_record(gc, "f32", "int", "refused")
    torch.cuda.synchronize()
    assert rc == EINVAL and rec["launches"] == 0 and rec["kernel"] == "none" and bool(torch.isnan(out).all())
    assert _lib.lib.mvf_nhwc_stencil_last_launch(None) == -1 and _lib.lib.mvf_nhwc_tapgrad_last_launch(None) == -1


# ------------------------------------------------------------------------------------------------ tap gradients
# name clips T h w cs x_c dy_c mode, which of dw_h / dw_w are passed, the row kernel's block count under the default policy (0: not asserted)
Tap = collections.namedtuple("Tap", "name clips T h w cs x_c dy_c mode nulls nblk")
TAPS = [
    Tap("1x1_t1_cs4", 1, 1, 1, 1, 4, 4, 4, 7, False, 1),                      # one row: fewer rows than row lanes
    Tap("1x7_t4_cs8", 2, 4, 1, 7, 8, 16, 8, 7, False, 1),                     # x_c = c > cs, dy compact
    Tap("5x7_t4_cs256", 2, 4, 5, 7, 256, 256, 256, 7, False, 18),             # 280 rows in blocks of 16: boundaries inside frames and clips
    Tap("14x14_t5_cs12", 1, 5, 14, 14, 12, 16, 20, 7, False, 4),              # both wide; cs / 4 = 3 is no power of two
    Tap("1x3_t8_cs1028", 1, 8, 1, 3, 1028, 1028, 1028, 7, False, 6),          # 257 channel groups: grid_y = 2
    Tap("5x7_t5_cs8_t", 2, 5, 5, 7, 8, 8, 8, 1, False, 0),                    # mode T: dw_h, dw_w are written as zeros
    Tap("5x7_t8_cs8_nulls", 2, 8, 5, 7, 8, 12, 8, 7, True, 0),                # dw_h / dw_w NULL
    Tap("5x7_t4_cs12_th", 2, 4, 5, 7, 12, 12, 16, 3, False, 0),
    Tap("14x14_t4_cs256", 1, 4, 14, 14, 256, 256, 256, 7, False, 0),          # H * W larger than one band of the (clip, band) kernel
]
_tap_cache = {}


def _tap_ops(t, dtype, cls):
    key = (t, dtype, cls)
    if key not in _tap_cache:
        m = t.clips * t.T * t.h * t.w
        gen = torch.Generator().manual_seed(sum(v for v in t[1:] if isinstance(v, int)) + (cls == "int"))
        if cls == "int":
            x, dy = (torch.randint(-2, 3, (m, c_), generator=gen).float().to(_tdt(dtype)) for c_ in (t.x_c, t.dy_c))
        else:
            x, dy = (torch.randn(m, c_, generator=gen).to(_tdt(dtype)) for c_ in (t.x_c, t.dy_c))
        desc = R.Desc(t.clips * t.T, t.h, t.w, t.T, t.cs, t.mode)
        ref = R.tapgrad(_np(x), _np(dy), desc)
        absref = R.tapgrad(np.abs(_np(x)), np.abs(_np(dy)), R.Desc(t.clips * t.T, t.h, t.w, t.T, t.cs, 7))
        _tap_cache[key] = dict(m=m, x=x, dy=dy, ref=ref, absref=absref, dev=(_dev(x), _dev(dy)))
    return _tap_cache[key]


def _run_tapgrad(t, dtype, cls, ws_short=0, expect_rc=0):
    from mvfnet_amd import _lib
    lib = _lib.lib
    o = _tap_ops(t, dtype, cls)
    d = _lib.MvfDesc(t.clips * t.T, t.x_c, t.h, t.w, t.T, t.cs, t.mode, _lib.MVF_NHWC, _lib.MVF_F32 if dtype == "f32" else _lib.MVF_BF16)
    nbytes = lib.mvf_nhwc_tapgrad_workspace_bytes(C.byref(d))
    assert nbytes > 0 and nbytes % 256 == 0
    raw_ws, ws = _nan_buffer(nbytes // 4, torch.float32)
    raw_dw, dw = _nan_buffer(3 * t.cs * 3, torch.float32)
    dw = dw.view(3, t.cs, 3)
    rc = lib.mvf_nhwc_tapgrad(C.byref(d), _P(o["dev"][0][1]), t.x_c, _P(o["dev"][1][1]), t.dy_c, _P(dw[0].data_ptr()), _P(0 if t.nulls else dw[1].data_ptr()),
                              _P(0 if t.nulls else dw[2].data_ptr()), _P(ws.data_ptr()), nbytes - ws_short, None)
    info = _lib.TapgradLaunchInfo()
    _lib.check(lib.mvf_nhwc_tapgrad_last_launch(C.byref(info)))
    rec = {k: getattr(info, k) for k, _ in info._fields_}
    rec.update(kind="tapgrad", kernel=_lib.TAPGRAD_KERNELS[info.kernel], case=t.name, dtype=dtype, cls=cls, rec_dtype=info.dtype)
    _seen.append(rec)
    _log(COVERAGE_ENV, rec)
    torch.cuda.synchronize()
    assert _canary_ok(raw_ws), "the workspace was written past mvf_nhwc_tapgrad_workspace_bytes"
    assert _canary_ok(raw_dw)
    got = dw.double().cpu().numpy()
    if expect_rc:
        assert rc == expect_rc, (rc, lib.mvf_last_error())
        assert rec["launches"] == 0 and rec["kernel"] == "none", rec
        assert np.isnan(got).all(), "a refused call wrote the tap gradients"
        return rec
    assert rc == 0, lib.mvf_last_error()
    assert rec["launches"] == 2 and rec["rec_dtype"] == d.dtype and rec["nblk"] > 0, rec
    if DEFAULT_POLICY:
        assert rec["kernel"] == "rows", rec
        assert rec["nblk"] == -(-o["m"] // rec["rows_per_blk"]) and (not t.nblk or rec["nblk"] == t.nblk), rec
    cg = t.cs // 4
    assert rec["grid_y"] == -(-cg // rec["cgp"]) and rec["cgp"] == min(256, 1 << (cg - 1).bit_length()), rec
    L = rec["rows_per_blk"] * (t.T if rec["kernel"] == "bands" else 1)
    if t.nulls:
        assert np.isnan(got[1:]).all(), "dw_h / dw_w were NULL"
    for i, name in enumerate(("dw_t", "dw_h", "dw_w")):
        if i and t.nulls:
            continue
        assert np.isfinite(got[i]).all(), "%d of %d elements of %s were not written" % (int((~np.isfinite(got[i])).sum()), got[i].size, name)
        if i and not t.mode & (2 if i == 1 else 4):
            assert not got[i].any(), "%s of an absent view is not zero" % name
        if cls == "int":
            assert o["absref"][i].max() < 2 ** 24
            bound = np.zeros_like(o["ref"][i])
        else:
            bound = L * U24 * o["absref"][i]
        g_ = Geo(t.name, *([0] * 12))
        _measure(name, g_, dtype, cls, "tapgrad", rec["kernel"], np.abs(got[i] - o["ref"][i]), bound)
    return rec


@pytest.mark.parametrize("cls", CLASSES)
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("t", TAPS, ids=lambda t: t.name)
def test_tapgrad(t, dtype, cls):
    _run_tapgrad(t, dtype, cls)


def test_tapgrad_workspace_one_byte_short_is_refused():
    _run_tapgrad(TAPS[2], "bf16", "int", ws_short=1, expect_rc=EWS)


# ------------------------------------------------------------------------------------------------ forced legs
def _kernels(recs, **match):
    return {r["kernel"] for r in recs if r["launches"] and all(r.get(k_) == v_ for k_, v_ in match.items())}


def _of(recs, case):
    return [r for r in recs if r["launches"] and r["case"] == case]


# leg -> (policy, the cases its switch changes (-k), check(records) that the forced policy reached the kernels it names)
LEGS = {
    "stencil_lds=0": (dict(stencil_lds=0), "test_lds_shapes", lambda rs: _kernels(rs) == {"chunked"}),
    "stencil_lds=1,stencil_lds_minwg=1": (dict(stencil_lds=1, stencil_lds_minwg=1), "test_fewclip_shapes and bf16",
                                           lambda rs: _kernels(rs) == {"lds"} and
                                           {(r["rows_per_band"], r["bands"]) for r in _of(rs, "c2_t4_9x5_cs64") if r["dtype"] == "bf16"} == {(5, 2)} and
                                           {(r["rows_per_band"], r["chan_per_wg"]) for r in _of(rs, "c1_t16_14x14_cs64") if r["dtype"] == "bf16"} == {(2, 32)}),
    "stencil_chunked=0,stencil_lds=0": (dict(stencil_chunked=0, stencil_lds=0), "test_chunked_shapes or test_lds_shapes or test_fewclip_shapes or test_walk4_shapes",
                                        lambda rs: _kernels(rs) == {"walk4"}),
    # the walk in place of the chunked kernel, the tiled kernel left on: its statistics and column sums do not need the chunked kernel (such a launch used to run
    # the tiled kernel and then return MVF_EUNSUPPORTED)
    "stencil_chunked=0": (dict(stencil_chunked=0), "test_lds_shapes", lambda rs: _kernels(rs) == {"lds"} and all(r["launches"] for r in rs)),
    "tapgrad_rows=0": (dict(tapgrad_rows=0), "test_tapgrad and not workspace",
                       lambda rs: _kernels(rs) == {"bands"} and {r["nblk"] for r in _of(rs, "14x14_t4_cs256")} == {7} and {r["nblk"] for r in _of(rs, "5x7_t4_cs256")} == {4}),
}
_leg_results = {}


def _run_leg(leg, tmp_dir):
    """The cases the leg's switch changes again in a fresh child process under that policy (the switches are read once per process); memoised."""
    if leg not in _leg_results:
        cov = os.path.join(str(tmp_dir), "coverage_%d.jsonl" % list(LEGS).index(leg))
        env = policy_env(**LEGS[leg][0])
        env[COVERAGE_ENV] = cov
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-x", "-q", "-m", "gpu", "-k", LEGS[leg][1], "-p", "no:cacheprovider"], env=env,
                           capture_output=True, text=True, timeout=300)
        recs = [json.loads(line) for line in open(cov)] if os.path.exists(cov) else []
        _leg_results[leg] = (r.returncode, r.stdout[-3000:] + r.stderr[-2000:], recs)
    return _leg_results[leg]


@pytest.fixture(scope="module")
def leg_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("stencil_legs")


@pytest.mark.parametrize("leg", list(LEGS))
def test_kernels_under_forced_policies(leg, leg_dir):
    rc, tail, recs = _run_leg(leg, leg_dir)
    assert rc == 0, tail
    assert recs
    assert LEGS[leg][2](recs), "policy %s did not reach the kernels it names: %s" % (leg, sorted({(r["kernel"], r["case"], r["dtype"], r.get("rows_per_band", 0),
                                                                                                r.get("chan_per_wg", 0), r.get("bands", 0), r.get("nblk", 0)) for r in recs}))


FOUR = ("plain", "flip+addend+gate", "stats", "colsums")
MATRIX = ([("stencil", "walk1", dt, "plain") for dt in DTYPES] +
          [("stencil", "walk4", dt, c_) for dt in DTYPES for c_ in FOUR[:2]] +
          [("stencil", "chunked", dt, c_) for dt in DTYPES for c_ in FOUR] +
          [("stencil", "lds", "bf16", c_) for c_ in FOUR] +
          [("tapgrad", k_, dt, "") for k_ in ("rows", "bands") for dt in DTYPES])
# What the matrix leaves out: the output gate and the partial sums on walk1, the partial sums on walk4 (refused: MVF_EUNSUPPORTED, asserted above); fp32 on the
# tiled kernel (it is bf16 only).


def test_coverage_matrix(leg_dir):
    """Every stencil kernel x storage type it supports x {plain, flip + addend + gate, statistics, column sums} and both tap-gradient kernels x both storage
    types were reached, by this process's own cases (the whole module must have run) or by a forced leg's child."""
    recs = list(_seen)
    for leg in LEGS:
        rc, tail, r_ = _run_leg(leg, leg_dir)
        assert rc == 0, "leg %s: %s" % (leg, tail)
        recs += r_
    seen = {(r["kind"], r["kernel"], r["dtype"], r.get("category", "")) for r in recs if r["launches"]}
    missing = [k for k in MATRIX if k not in seen]
    assert not missing, "never reached (kernel, storage type, variant): %s" % missing
