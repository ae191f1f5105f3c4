"""CPU: the C-ABI library loads and exports every symbol include/mvfnet_hip.h declares (no compute calls)."""
import ctypes

import pytest


def test_library_loads_and_exports_declared_symbols():
    from mvfnet_amd import _lib
    names = _lib.declared_symbols()
    assert "mvf_fwd_infer" in names and "mvf_bwd" in names
    for n in names:
        assert hasattr(_lib.lib, n), "libmvfnet_hip.so does not export %s" % n
    assert _lib.lib.mvf_abi_version() == 2        # [r5] 2: mvf_conv_desc_t.x_c0


def test_queries_names_every_entry_point_that_launches_nothing():
    """_lib.QUERIES is what a launch plan never holds (launch_plan.RecordingLib): mvf_plan_run reads every callee's return value as a status, so every declared
    function that returns anything else must be in it; it is no weaker than the name rule it replaces (four suffixes, two names), it holds the host-side launch
    records that rule missed, and it names nothing the header does not declare."""
    from mvfnet_amd import _lib
    names = _lib.declared_symbols()
    no_status = [n for n in names if getattr(_lib.lib, n).restype is not ctypes.c_int]
    assert no_status and not [n for n in no_status if n not in _lib.QUERIES], [n for n in no_status if n not in _lib.QUERIES]
    old_rule = [n for n in names if n.endswith(("_bytes", "_rows", "_splits", "_plan")) or n in ("mvf_last_error", "mvf_abi_version")]
    assert len(old_rule) >= 18 and not [n for n in old_rule if n not in _lib.QUERIES], [n for n in old_rule if n not in _lib.QUERIES]
    assert "mvf_conv2d_last_launch" in _lib.QUERIES and "mvf_bn_last_launch" in _lib.QUERIES
    assert isinstance(_lib.QUERIES, frozenset) and not sorted(_lib.QUERIES - set(names)), sorted(_lib.QUERIES - set(names))


def test_recording_lib_passes_queries_through_and_refuses_what_returns_no_status():
    """launch_plan.RecordingLib without a GPU: a query is handed out as the library's own function and leaves the recorder alone; an entry point outside
    _lib.QUERIES is wrapped, and one that does not return a status marks the step as unsupported (no plan is built from it)."""
    from mvfnet_amd import _lib, launch_plan

    class FakeLib(object):
        mvf_bn_workspace_bytes = _lib.lib.mvf_bn_workspace_bytes
        mvf_bn_bwd_finalize = _lib.lib.mvf_bn_bwd_finalize
        mvf_new_count = ctypes.CFUNCTYPE(ctypes.c_size_t)(lambda: 3)

    rec = launch_plan.Recorder()
    lib = launch_plan.RecordingLib(rec, FakeLib)
    assert lib.mvf_bn_workspace_bytes is FakeLib.mvf_bn_workspace_bytes and lib.mvf_bn_workspace_bytes(8, 8) > 0
    assert lib.mvf_bn_bwd_finalize is not FakeLib.mvf_bn_bwd_finalize and rec.unsupported is None and rec.ops == []
    assert lib.mvf_bn_bwd_finalize(None, 0, 8, None, None, None) == -1 and [op[2] for op in rec.ops] == ["mvf_bn_bwd_finalize"] and rec.unsupported is None
    assert lib.mvf_new_count is not FakeLib.mvf_new_count and "mvf_new_count" in rec.unsupported


def test_argument_validation_needs_no_gpu():
    from mvfnet_amd import _lib
    d = _lib.MvfDesc(10, 16, 4, 4, 4, 4, 7, 0, 0)
    assert _lib.lib.mvf_fwd_infer(ctypes.byref(d), None, None, None, None, None, None, None, None) == -2
    assert b"multiple of n_segment" in _lib.lib.mvf_last_error()
    assert _lib.lib.mvf_fwd_train_workspace_bytes(ctypes.byref(d)) == 0
    d = _lib.MvfDesc(8, 16, 4, 4, 4, 4, 7, 0, 0)
    assert _lib.lib.mvf_fwd_train_workspace_bytes(ctypes.byref(d)) > 0
    assert _lib.lib.mvf_fwd_infer(ctypes.byref(d), None, None, None, None, None, None, None, None) == -1   # NULL x


def test_product_modules_refuse_cpu_tensors():
    import torch
    import torch.nn as nn
    from mvfnet_amd.modules import MVF
    m = MVF(nn.Conv2d(32, 16, 1, bias=False), 4, 32, 0.125)
    assert sorted(m.state_dict()) == sorted(
        ["net.weight", "shift_conv.weight", "h_conv.weight", "w_conv.weight", "bn.weight", "bn.bias",
         "bn.running_mean", "bn.running_var", "bn.num_batches_tracked"])
    assert tuple(m.shift_conv.weight.shape) == (4, 1, 3, 1, 1)
    assert tuple(m.h_conv.weight.shape) == (4, 1, 1, 3, 1)
    assert tuple(m.w_conv.weight.shape) == (4, 1, 1, 1, 3)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.randn(8, 32, 5, 5))


def test_stencil_partial_row_plan_follows_the_kernel_choice():
    """[r5] mvf_nhwc_stencil_stats_rows names the partial rows of the launch that WILL run (no launch, no GPU): the LDS-tiled bf16 kernel
    (clips x bands of rows) where its plan exists and makes >= 150 workgroups, the register-chunked kernel's (clips x pixel bands) otherwise."""
    import os
    if "stencil_lds" in os.environ.get("MVF_POLICY", ""):
        pytest.skip("the plan switches are set in the environment")
    from mvfnet_amd import _lib
    L = _lib
    rows = lambda nt, t, hw, c, cs, dt: L.lib.mvf_nhwc_stencil_stats_rows(ctypes.byref(L.MvfDesc(nt, c, hw, hw, t, cs, 7, L.MVF_NHWC, dt)), c, cs)  # noqa: E731
    assert rows(256, 8, 14, 1024, 128, L.MVF_BF16) == 32 * 7          # layer3 at 32 clips: 64 channels x 2 rows x 8 frames in 57 KB -> 448 workgroups
    assert rows(256, 16, 14, 1024, 128, L.MVF_BF16) == 16 * 7         # C4: 32 channels x 2 rows x 16 frames
    assert rows(256, 8, 7, 2048, 256, L.MVF_BF16) == 32 * 4           # layer4: whole planes would make 128 workgroups -> the halved budget, 2-row bands
    assert rows(96, 8, 14, 1024, 128, L.MVF_BF16) == 12 * 7           # 12 clips: 168 workgroups, still tiled
    assert rows(32, 8, 14, 1024, 128, L.MVF_BF16) == 4 * 25           # 4 clips: 56 workgroups -> the chunked kernel (8 pixels per workgroup)
    assert rows(256, 8, 14, 1024, 128, L.MVF_F32) == 32 * 25          # fp32: chunked


def test_plan_run_generic_call_marshals_integers_and_floats_in_order():
    """[r6] mvf_plan_run (csrc/launch_plan.hip) calls a recorded entry point as int (*)(uint64 x NI, float x NF): on x86-64 System V the two argument classes are
    assigned independently, so a prototype that INTERLEAVES them (the library's own entry points do: pointers, sizes, an eps, a stream) receives each argument where
    it expects it.  Checked here with host callbacks in place of the library's entry points -- no GPU, no launch: every integer word (64-bit pointers, 32-bit ints in
    the low half of their slot), every float, more integers than registers (the stack), and the stop-at-first-failure contract with the failing op's index."""
    import ctypes as C
    from mvfnet_amd import _lib
    seen = []
    proto_a = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_float, C.c_longlong, C.c_float, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float)

    def fa(p, n, eps, big, mom, q, a, b, c, d, s):
        seen.append(("a", p, n, round(eps, 6), big, round(mom, 6), q, a, b, c, d, round(s, 6)))
        return 0
    proto_b = C.CFUNCTYPE(C.c_int, C.c_int)

    def fb(code):
        seen.append(("b", code))
        return code
    cba, cbb = proto_a(fa), proto_b(fb)
    ops = (_lib.PlanOp * 4)()
    words = (C.c_ulonglong * 16)(0x7F00DEADBEE0, 12, 1 << 40, 0x7F00CAFEF000, 1, 2, 3, 4,   # op 0: 8 integer-class words (two past the six registers)
                                 0,                                                              # op 1
                                 0xFFFFFFFF00000000 | 5,                                         # op 2: an int argument reads the LOW half of its slot -> 5 -> failure code
                                 0)                                                              # op 3 (never reached)
    floats = (C.c_float * 4)(1e-5, 0.9, 2.5, 0.0)
    for i, (fn, ni, nf, w0, f0) in enumerate(((cba, 8, 3, 0, 0), (cbb, 1, 0, 8, 3), (cbb, 1, 0, 9, 3), (cbb, 1, 0, 10, 3))):
        ops[i].kind, ops[i].n_int, ops[i].n_flt, ops[i].fn, ops[i].word0, ops[i].float0 = 0, ni, nf, C.cast(fn, C.c_void_p).value, w0, f0
    failed = C.c_int(-1)
    rc = _lib.lib.mvf_plan_run(ops, 4, words, floats, C.byref(failed))
    assert rc == 5 and failed.value == 2
    assert seen == [("a", 0x7F00DEADBEE0, 12, 1e-5, 1 << 40, 0.9, 0x7F00CAFEF000, 1, 2, 3, 4, 2.5), ("b", 0), ("b", 5)]
    # a malformed record is refused before anything is called
    ops[0].n_int = 41
    assert _lib.lib.mvf_plan_run(ops, 1, words, floats, C.byref(failed)) == -1 and failed.value == 0          # MVF_EINVAL
    assert b"bad call record" in _lib.lib.mvf_last_error()


def test_head_and_optimizer_argument_failures_return_before_any_launch():
    """The head's and the optimizer's entry points check their arguments before the first launch (csrc/head.hip, csrc/optim.hip): the codes come back on
    a machine without a GPU, from host addresses that are never read."""
    import ctypes as C
    from mvfnet_amd import _lib
    lib = _lib.lib
    host = (C.c_float * 64)()
    a = C.cast(host, C.c_void_p)
    EINVAL, ESHAPE, EWS = -1, -2, -3
    ws_bytes = lib.mvf_sgd_workspace_bytes(1)
    assert ws_bytes > 4
    assert lib.mvf_sgd_nesterov_step(a, a, a, 0, 1.0, 40.0, 0.015, 0.9, 1e-4, 1, a, a, ws_bytes, None) == EINVAL
    assert b"sgd_nesterov_step" in lib.mvf_last_error()
    assert lib.mvf_sgd_nesterov_step(a, a, a, 1, 1.0, 40.0, 0.015, 0.9, 1e-4, 1, a, a, ws_bytes - 1, None) == EWS
    assert b"workspace too small" in lib.mvf_last_error()
    assert lib.mvf_sgd_nesterov_step(a, a, a, 1, 1.0, 40.0, 0.015, 0.9, 1e-4, 1, a, None, ws_bytes, None) == EWS
    assert lib.mvf_sgd_step_segments(a, a, a, 1, 1.0, 40.0, 0.015, 0.9, 1e-4, 1, 1, a, 0, a, a, ws_bytes, None) == EINVAL
    assert b"sgd_step_segments" in lib.mvf_last_error()
    assert lib.mvf_sgd_step_segments(a, a, a, 1, 1.0, 40.0, 0.015, 0.9, 1e-4, 1, 1, a, 1, a, a, ws_bytes - 1, None) == EWS
    assert lib.mvf_head_train_bwd(a, a, a, None, 1, 1, 1, 6, 1, a, a, a, a, 0, None) == ESHAPE
    assert b"multiple of 4" in lib.mvf_last_error()
    assert lib.mvf_head_pool_fc(a, 1, 1, 1, 6, a, a, 1, a, a, 0, None) == ESHAPE
    assert b"multiple of 4" in lib.mvf_last_error()


def test_every_head_form_refuses_bad_score_arguments_before_any_launch():
    """The four fused forward forms of csrc/head.hip share one argument check, mvf_head_train_bwd has its counterpart: a storage type that is neither fp32 nor
    bf16, more frames than a grid holds, more channels than the LDS feature buffer and a NULL pooled come back with the same code from every form.  The addresses
    are host memory that is never read, and this machine has no GPU: a call that reached a launch would return MVF_EHIP, so each code shows the refusal came first."""
    import ctypes as C
    from mvfnet_amd import _lib
    lib = _lib.lib
    host = (C.c_float * 64)()
    a = C.cast(host, C.c_void_p)
    EINVAL, ESHAPE, EUNSUPPORTED = -1, -2, -5
    prm = _lib.FocalParams(gamma_pos=2.0, gamma_neg=2.0, margin=0.0, alpha=0.25, target_threshold=float("nan"), sum_classes=0)
    forms = {"head_train_fwd": (lib.mvf_head_train_fwd, ()), "head_train_fwd_soft": (lib.mvf_head_train_fwd_soft, ()),
             "head_train_fwd_bce": (lib.mvf_head_train_fwd_bce, (None, C.c_float(float("nan")), 0)), "head_train_fwd_focal": (lib.mvf_head_train_fwd_focal, (None, prm))}
    for who, (fn, mid) in forms.items():
        def call(clips=2, t=4, c=8, pooled=a, dtype=0):
            return fn(a, clips, t, 9, c, a, a, 10, a, None, *mid, pooled, a, a, a, a, dtype, None)
        for rc_want, word, kw in ((EINVAL, b"dtype 2", dict(dtype=2)), (ESHAPE, b"exceed the grid", dict(clips=65536, t=1)),
                                  (EUNSUPPORTED, b"c=40961 does not fit", dict(c=40961)), (EINVAL, b"NULL", dict(pooled=None))):
            assert call(**kw) == rc_want, (who, kw, lib.mvf_last_error())
            err = lib.mvf_last_error()
            assert err.startswith(who.encode() + b":") and word in err, (who, kw, err)
        assert call(clips=0) == EINVAL and b"bad argument" in lib.mvf_last_error()
    bwd = lambda clips=2, t=4, dtype=0: lib.mvf_head_train_bwd(a, a, a, None, clips, t, 9, 8, 10, a, a, a, a, dtype, None)  # noqa: E731
    assert bwd(dtype=2) == EINVAL and b"head_train_bwd: dtype 2" in lib.mvf_last_error()
    assert bwd(clips=16384, t=4) == ESHAPE and b"exceed the grid" in lib.mvf_last_error()
    assert bwd(clips=65536, t=1) == ESHAPE


def test_refused_weight_gradient_calls_leave_an_empty_launch_record():
    """mvf_conv2d_wgrad_last_launch is a host-side record: a call refused before its first launch -- checked here from host addresses that are never read -- leaves
    launches = 0 and family NONE, also after the caller-named entry point refuses its workgroup count."""
    import ctypes as C
    from mvfnet_amd import _lib
    lib = _lib.lib
    host = (C.c_float * 64)()
    a = C.cast(host, C.c_void_p)
    info = _lib.WgradLaunchInfo()
    assert C.sizeof(info) == 12 * 4 and len(_lib.WGRAD_FAMILIES) == 12
    d = _lib.ConvDesc(2, 4, 4, 64, 64, 1, 1, 1, 0, 4, 4, 64, _lib.MVF_BF16, 0, 0, 0, 0, 0, 0)
    nb = lib.mvf_conv2d_wgrad_workspace_bytes(C.byref(d))
    assert nb > 0
    for rc_want, call in ((-3, lambda: lib.mvf_conv2d_nhwc_wgrad(C.byref(d), a, a, None, 1, 64, 1, 64, a, a, nb - 1, None)),
                          (-1, lambda: lib.mvf_conv2d_nhwc_wgrad(C.byref(d), a, a, None, 1, 64, 2, 64, a, a, nb, None)),
                          (-1, lambda: lib.mvf_conv2d_nhwc_wgrad_wgs(C.byref(d), a, a, None, 1, 64, 1, 64, a, a, nb, 7, None)),
                          (-1, lambda: lib.mvf_conv2d_nhwc_wgrad_wgs(C.byref(d), a, a, None, 1, 64, 1, 64, a, a, nb, 4097, None))):
        info.family, info.launches = 99, 99
        assert call() == rc_want
        assert lib.mvf_conv2d_wgrad_last_launch(C.byref(info)) == 0
        assert (info.family, info.launches, info.nsplit) == (0, 0, 0)
    assert lib.mvf_conv2d_wgrad_last_launch(None) == -1


def test_refused_stencil_calls_leave_an_empty_launch_record():
    """mvf_nhwc_stencil_last_launch is a host-side record: a stencil call refused before its first launch -- checked here from host addresses that are never
    read -- leaves launches = 0 and kernel NONE, on each entry point of the family; a plan query does not touch the record."""
    import ctypes as C
    from mvfnet_amd import _lib
    lib = _lib.lib
    host = (C.c_float * 64)()
    a = C.cast(host, C.c_void_p)
    b = C.c_void_p(a.value + 64)
    info = _lib.StencilLaunchInfo()
    assert C.sizeof(info) == 12 * 4 and len(_lib.STENCIL_KERNELS) == 5
    d = _lib.MvfDesc(8, 16, 4, 4, 4, 8, 7, _lib.MVF_NHWC, _lib.MVF_BF16)
    d3 = _lib.MvfDesc(8, 6, 4, 4, 4, 3, 7, _lib.MVF_NHWC, _lib.MVF_F32)
    EINVAL, EUNSUPPORTED = -1, -5
    for rc_want, call in ((EINVAL, lambda: lib.mvf_nhwc_stencil(C.byref(d), a, 16, a, 16, a, a, a, None, None, 0, None, 0, None, None)),           # x == out
                          (EINVAL, lambda: lib.mvf_nhwc_stencil(C.byref(d), a, 16, b, 8, a, a, a, None, None, 0, a, 4, None, None)),              # addend pitch < cs
                          (EINVAL, lambda: lib.mvf_nhwc_stencil(C.byref(d), a, 16, b, 8, a, a, a, None, None, 1, None, 0, a, None)),              # bits without an addend
                          (EINVAL, lambda: lib.mvf_nhwc_stencil_gate(C.byref(d), a, 16, b, 8, a, a, a, None, None, 1, None, 0, None, None, None)),  # no gate bits
                          (EUNSUPPORTED, lambda: lib.mvf_nhwc_stencil_gate(C.byref(d3), a, 6, b, 6, a, a, a, None, None, 0, None, 0, None, a, None)),  # gate on cs = 3
                          (EINVAL, lambda: lib.mvf_nhwc_stencil_gate_colsums(C.byref(d), a, 16, b, 8, a, a, a, 1, None, 0, None, a, None, None)),   # no sums_part
                          (EINVAL, lambda: lib.mvf_nhwc_stencil_stats(C.byref(d), a, 4, b, 8, a, a, a, a, None, None)),                           # x pitch < cs
                          (EUNSUPPORTED, lambda: lib.mvf_nhwc_stencil_stats(C.byref(d3), a, 6, b, 6, a, a, a, a, None, None))):                   # statistics on cs = 3
        info.kernel, info.launches, info.grid_x = 99, 99, 99
        assert call() == rc_want, lib.mvf_last_error()
        assert lib.mvf_nhwc_stencil_last_launch(C.byref(info)) == 0
        assert (info.kernel, info.launches, info.grid_x, info.flags) == (0, 0, 0, 0)
    assert lib.mvf_nhwc_stencil_stats_rows(C.byref(d), 16, 8) > 0
    assert lib.mvf_nhwc_stencil_last_launch(C.byref(info)) == 0 and (info.kernel, info.launches) == (0, 0)
    assert lib.mvf_nhwc_stencil_last_launch(None) == -1


def test_refused_tap_gradient_calls_leave_an_empty_launch_record():
    """mvf_nhwc_tapgrad_last_launch: the same for the tap gradients -- a workspace one byte short (MVF_EWS), a NULL workspace, cs % 4 != 0."""
    import ctypes as C
    from mvfnet_amd import _lib
    lib = _lib.lib
    host = (C.c_float * 64)()
    a = C.cast(host, C.c_void_p)
    info = _lib.TapgradLaunchInfo()
    assert C.sizeof(info) == 7 * 4 and len(_lib.TAPGRAD_KERNELS) == 3
    d = _lib.MvfDesc(8, 16, 4, 4, 4, 8, 7, _lib.MVF_NHWC, _lib.MVF_F32)
    d6 = _lib.MvfDesc(8, 16, 4, 4, 4, 6, 7, _lib.MVF_NHWC, _lib.MVF_F32)
    nb = lib.mvf_nhwc_tapgrad_workspace_bytes(C.byref(d))
    assert nb > 0 and nb % 256 == 0 and lib.mvf_nhwc_tapgrad_workspace_bytes(C.byref(d6)) == 0
    for rc_want, call in ((-3, lambda: lib.mvf_nhwc_tapgrad(C.byref(d), a, 16, a, 8, a, a, a, a, nb - 1, None)),
                          (-3, lambda: lib.mvf_nhwc_tapgrad(C.byref(d), a, 16, a, 8, a, a, a, None, nb, None)),
                          (-1, lambda: lib.mvf_nhwc_tapgrad(C.byref(d6), a, 16, a, 8, a, a, a, a, nb, None)),
                          (-1, lambda: lib.mvf_nhwc_tapgrad(C.byref(d), a, 18, a, 8, a, a, a, a, nb, None))):
        info.kernel, info.launches, info.nblk = 99, 99, 99
        assert call() == rc_want, lib.mvf_last_error()
        assert lib.mvf_nhwc_tapgrad_last_launch(C.byref(info)) == 0
        assert (info.kernel, info.launches, info.nblk) == (0, 0, 0)
    assert lib.mvf_nhwc_tapgrad_last_launch(None) == -1


@pytest.mark.cpu
def test_refused_batchnorm_and_pool_calls_leave_a_record_that_says_so():
    """mvf_bn_last_launch is a host-side record: every BatchNorm / max-pool entry point of csrc/train_ops.hip starts a new one, so a call refused before its first
    launch -- checked here from host addresses that are never read -- names the entry point and reports no launch, no lane width and no kernel form."""
    import ctypes as C
    from mvfnet_amd import _lib
    lib = _lib.lib
    host = (C.c_float * 64)()
    a = C.cast(host, C.c_void_p)
    f = lambda v: C.c_float(v)  # noqa: E731
    info = _lib.BnLaunchInfo()
    assert C.sizeof(info) == 13 * 4 and len(_lib.BN_ENTRIES) == 14 and len(_lib.BN_FINALIZE_FORMS) == 4 and len(_lib.POOL_FORMS) == 6
    EINVAL, EWS, EUNSUPPORTED = -1, -3, -5
    nb = lib.mvf_bn_workspace_bytes(8, 8)
    assert nb > 0 and nb % 256 == 0 and lib.mvf_bn_workspace_bytes(8, 6) == 0
    E = {v: k for k, v in _lib.BN_ENTRIES.items()}
    calls = (
        ("train_stats", -1, EINVAL, lambda: lib.mvf_bn_train_stats(a, 8, 6, a, a, f(1e-5), f(0.1), a, a, a, a, a, a, a, nb, 0, None)),                 # c % 4
        ("train_stats", -1, EWS, lambda: lib.mvf_bn_train_stats(a, 8, 8, a, a, f(1e-5), f(0.1), a, a, a, a, a, a, a, nb - 1, 0, None)),               # one byte short
        ("train_finalize", -1, EINVAL, lambda: lib.mvf_bn_train_finalize(a, 0, 8, 8, a, a, f(1e-5), f(0.1), a, a, a, a, a, a, None)),                 # no partial rows
        ("apply", -1, EINVAL, lambda: lib.mvf_bn_apply_bits(a, 8, 8, a, a, a, a, None, 1, a, a, 0, None)),                                              # rscale without rshift
        ("apply", -1, EINVAL, lambda: lib.mvf_bn_apply(a, 8, 6, a, a, None, None, None, 1, a, 1, None)),
        ("apply_colmeans", -1, EINVAL, lambda: lib.mvf_bn_apply_colmeans(a, 8, 12, a, a, 1, a, a, a, nb, 1, None)),                                   # c % 8
        ("bwd_reduce", 1, EINVAL, lambda: lib.mvf_bn_bwd_reduce(a, 8, a, None, 8, 8, a, a, a, a, 1, None, a, a, a, nb, 0, None)),                    # mode 1 without ymask
        ("bwd_reduce", 2, EINVAL, lambda: lib.mvf_bn_bwd_reduce(a, 8, a, None, 8, 8, a, a, None, None, 2, None, a, a, a, nb, 0, None)),              # mode 2 without scale
        ("bwd_reduce", 0, EINVAL, lambda: lib.mvf_bn_bwd_reduce(a, 4, a, None, 8, 8, a, a, a, a, 0, None, a, a, a, nb, 0, None)),                    # g_pitch < c
        ("bwd_reduce", 0, EWS, lambda: lib.mvf_bn_bwd_reduce(a, 8, a, None, 8, 8, a, a, a, a, 0, None, a, a, a, nb - 1, 0, None)),
        ("bwd_finalize", -1, EINVAL, lambda: lib.mvf_bn_bwd_finalize(a, 0, 8, a, a, None)),
        ("bwd_apply", 4, EINVAL, lambda: lib.mvf_bn_bwd_apply(a, 8, a, 8, 8, a, a, a, a, a, a, a, 4, a, 0, None)),                                    # bits need _masked
        ("bwd_apply", 4, EINVAL, lambda: lib.mvf_bn_bwd_apply_masked(a, 8, a, None, 8, 8, a, a, a, a, a, a, a, 4, a, 0, None)),
        ("bwd_pair", 4, EWS, lambda: lib.mvf_bn_bwd_pair(a, 8, a, a, a, 8, 8, a, a, a, a, a, a, a, a, a, a, a, a, a, 2 * nb - 1, 0, None)),
        ("pool_fwd", -1, EINVAL, lambda: lib.mvf_maxpool_bn_relu_fwd(a, 1, 4, 4, 6, a, a, a, a, 0, None)),
        ("pool_bwd", -1, EINVAL, lambda: lib.mvf_maxpool_bn_relu_bwd(a, a, 1, 4, 4, 8, None, 0, None)),
        ("pool_bwd_sums", 2, EUNSUPPORTED, lambda: lib.mvf_maxpool_bn_relu_bwd_sums(a, a, 1, 4, 4, 12, a, a, a, a, a, a, a, 0, None)),                # 256 % (c / 4)
        ("pool_bwd_apply", 2, EUNSUPPORTED, lambda: lib.mvf_maxpool_bn_relu_bwd_apply(a, a, 1, 4, 4, 12, a, a, a, a, a, a, a, a, a, 0, None)),
    )
    for entry, mode, rc_want, call in calls:
        for k, _ in info._fields_:
            setattr(info, k, 99)
        assert call() == rc_want, (entry, lib.mvf_last_error())
        assert lib.mvf_bn_last_launch(C.byref(info)) == 0
        assert (info.entry, info.mask_mode) == (E[entry], mode), (entry, info.entry, info.mask_mode)
        assert (info.launches, info.vn, info.cqb, info.rows, info.gx, info.gy, info.specialised, info.finalize, info.part_rows, info.pool) == (0,) * 10, entry
    assert lib.mvf_bn_workspace_bytes(8, 8) == nb and lib.mvf_maxpool_bwd_sums_rows(2, 9) == 3           # plan queries leave the record alone
    assert lib.mvf_bn_last_launch(C.byref(info)) == 0 and info.entry == E["pool_bwd_apply"]
    assert lib.mvf_bn_last_launch(None) == -1


@pytest.mark.cpu
def test_dzfree_and_gram_glue_entry_points_refuse_before_any_launch():
    """The four entry points of csrc/bn_dzfree.hip check their arguments before the launch: every code below comes back on a machine without a GPU (a call that
    reached the launch would return MVF_EHIP), from host addresses that are never read.  `a` is 64-byte aligned; the misaligned rows move one operand off it."""
    import ctypes as C
    from mvfnet_amd import _lib
    lib = _lib.lib
    host = (C.c_char * 4096)()
    base = (C.addressof(host) + 63) // 64 * 64
    a = C.c_void_p(base)
    off = lambda n: C.c_void_p(base + n)  # noqa: E731
    EINVAL, ESHAPE, EUNSUPPORTED = -1, -2, -5
    BF16, F32 = _lib.MVF_BF16, _lib.MVF_F32

    def prep(c=256, k=32, m=37, dtype=BF16, ptrs=None, w_out=a):
        p = [a] * 7 if ptrs is None else ptrs                        # w_packed_dgrad, gamma, mean, invstd, dgamma, dbeta, bias_out
        return lib.mvf_bn_bwd_dzfree_prep(p[0], c, k, p[1], p[2], p[3], p[4], p[5], m, w_out, p[6], dtype, None)

    def wgrad(c=32, k=64, m=37, dtype=BF16, gram=a):
        return lib.mvf_bn_bwd_dzfree_wgrad(a, a, gram, a, a, a, a, a, a, m, c, k, dtype, None)

    def sums(c=8, k=4, q=a, w=a, part_lo=a, rows_lo=2, c_split=4, part_hi=a, rows_hi=2):
        return lib.mvf_bn_bwd_dzfree_sums(q, w, c, k, a, a, part_lo, rows_lo, c_split, part_hi, rows_hi, a, a, BF16, None)

    def gram(c=32, k=32, m=37, dtype=BF16, a_mean=a):
        return lib.mvf_bn_train_stats_gram(a, a_mean, a, m, c, k, a, a, C.c_float(1e-5), C.c_float(0.1), a, a, a, a, a, a, dtype, None)

    rows = [("prep", EINVAL, lambda i=i: prep(ptrs=[None if j == i else a for j in range(7)])) for i in range(7)]        # a NULL among the nine pointers ...
    rows += [
        ("prep", EINVAL, lambda: prep(w_out=None)),                                                                      # ... (w_out; bias_out is ptrs[6])
        ("prep", EINVAL, lambda: prep(m=0)),
        ("prep", EUNSUPPORTED, lambda: prep(dtype=F32)),
        ("prep", ESHAPE, lambda: prep(c=96)),
        ("prep", ESHAPE, lambda: prep(c=192)),                                                                           # a multiple of 64, not of 256
        ("prep", ESHAPE, lambda: prep(c=4352)),                                                                          # 17 x 256: past the 64 KiB of LDS
        ("prep", ESHAPE, lambda: prep(k=48)),
        ("prep", EINVAL, lambda: prep(w_out=off(8))),
        ("wgrad", ESHAPE, lambda: wgrad(k=32)),
        ("wgrad", ESHAPE, lambda: wgrad(c=48)),
        ("wgrad", EINVAL, lambda: wgrad(gram=off(4))),
        ("wgrad", EUNSUPPORTED, lambda: wgrad(dtype=F32)),
        ("sums", ESHAPE, lambda: sums(k=6)),
        ("sums", ESHAPE, lambda: sums(c_split=-1)),
        ("sums", ESHAPE, lambda: sums(c_split=9)),
        ("sums", EINVAL, lambda: sums(part_lo=None)),
        ("sums", EINVAL, lambda: sums(rows_lo=0)),
        ("sums", EINVAL, lambda: sums(part_hi=None)),
        ("sums", EINVAL, lambda: sums(q=off(4))),
        ("sums", EINVAL, lambda: sums(w=off(2))),
        ("stats_gram", ESHAPE, lambda: gram(c=48)),
        ("stats_gram", ESHAPE, lambda: gram(k=48)),
        ("stats_gram", EINVAL, lambda: gram(a_mean=off(4))),
        ("stats_gram", EUNSUPPORTED, lambda: gram(dtype=F32)),
    ]
    for who, rc_want, call in rows:
        rc = call()
        err = lib.mvf_last_error()
        assert rc == rc_want, (who, rc, rc_want, err)
        assert who.encode() in err, (who, err)
