"""GPU: averaged weights (EMA) -- mvf_ema_update / mvf_ema_swap (csrc/ema.hip), the _ema twins of the fused optimizer steps (csrc/optim.hip) and the
engine / runner / checkpoint layers above them (TrainEngine.enable_ema, averaged_weights, Runner(ema=...), checkpoint.averaged_state_dict).

The arithmetic is pinned: e' = fmaf(m, p' - e, e) in fp32 once per optimizer step, e' = p' itself at m = 1.  Against an fp64 restatement every update makes
two roundings (the difference and the fma), each at most 2^-24 relative to max(|p|, |e|), and earlier error contracts by 1 - m: after K updates
max|e_gpu - e_ref| <= K * 2^-23 * max(max|p|, max|e|) (BOUND below; an fp32 numpy emulation sits at a quarter of it)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from helpers import library_names
from mvfnet_amd import synth

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23
PAD = 8
SIZES = [1, 3, 4, 5, 255, 1024, 1025, 65543]
OFFSETS = (4, 5, 6, 7)          # the allocations are 256-byte aligned: an offset of 4 + o elements puts the view o elements past a 16-byte boundary
MOMENTA = (1.0, 0.5, 2e-4)
BEYOND_ONE_SWEEP = 4 * (2 * 2048 * 256 + 300) + 3      # more 16-byte vectors than 2 x (ema.hip's kMaxBlocks = 2048 workgroups x 256 threads), + remainder + scalar ends


def _lib():
    from mvfnet_amd import _lib as L
    return L.lib


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _values(n, seed):
    return np.random.RandomState(seed).standard_normal(n).astype(np.float32)


def _guarded(values, off, fill):
    host = np.full(off + values.size + PAD, fill, np.float32)
    host[off:off + values.size] = values
    return host


# ------------------------------------------------------------------------------------------------ 1. mvf_ema_update
def _check_update(lib, n, e_off, p_off, m, K=3):
    what = "n=%d offsets (%d, %d) m=%g" % (n, e_off, p_off, m)
    e0 = _values(n, 100 + n)
    host_e = _guarded(e0, e_off, 7.25)
    ema = torch.from_numpy(host_e).cuda()
    ref = e0.astype(np.float64)
    scale = float(np.abs(e0).max())
    m64 = float(np.float32(m))
    for k in range(K):
        p = _values(n, 1000 * (k + 1) + n)
        host_p = _guarded(p, p_off, -3.5)
        par = torch.from_numpy(host_p).cuda()
        assert lib.mvf_ema_update(ema.data_ptr() + 4 * e_off, par.data_ptr() + 4 * p_off, n, m, None) == 0, lib.mvf_last_error()
        torch.cuda.synchronize()
        ref = ref + m64 * (p.astype(np.float64) - ref)
        scale = max(scale, float(np.abs(p).max()))
        out = ema.cpu().numpy()
        assert np.array_equal(_bits(par.cpu().numpy()), _bits(host_p)), "params were written, " + what
        assert np.array_equal(_bits(out[:e_off]), _bits(host_e[:e_off])) and np.array_equal(_bits(out[e_off + n:]), _bits(host_e[e_off + n:])), "guards, " + what
        err = float(np.abs(out[e_off:e_off + n].astype(np.float64) - ref).max())
        assert err <= (k + 1) * ULP * scale, (what, k, err, (k + 1) * ULP * scale)
        if m == 1.0:
            assert np.array_equal(_bits(out[e_off:e_off + n]), _bits(p)), "m = 1 is a copy, " + what
    # ema bit-equal to params on entry: an exact fixed point for any m
    cur = ema.cpu().numpy()
    par = torch.from_numpy(_guarded(cur[e_off:e_off + n], p_off, -3.5)).cuda()
    assert lib.mvf_ema_update(ema.data_ptr() + 4 * e_off, par.data_ptr() + 4 * p_off, n, m, None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(_bits(ema.cpu().numpy()), _bits(cur)), "fixed point, " + what


@pytest.mark.parametrize("n", SIZES)
def test_ema_update_vs_fp64_at_every_offset(n):
    lib = _lib()
    for e_off in OFFSETS:
        for p_off in OFFSETS:
            for m in MOMENTA:
                _check_update(lib, n, e_off, p_off, m)


# ------------------------------------------------------------------------------------------------ 2. beyond one sweep of the grid
def test_ema_update_and_swap_beyond_one_sweep_of_the_grid():
    """The two-vectors-in-flight loop iterates, then its one-vector remainder and the scalar ends, in one launch."""
    lib = _lib()
    for o0, o1 in ((4, 4), (5, 6)):
        _check_update(lib, BEYOND_ONE_SWEEP, o0, o1, 0.5, K=1)
        _check_swap(lib, BEYOND_ONE_SWEEP, o0, o1)


# ------------------------------------------------------------------------------------------------ 3. mvf_ema_swap
def _check_swap(lib, n, a_off, b_off):
    what = "n=%d offsets (%d, %d)" % (n, a_off, b_off)
    host_a, host_b = _guarded(_values(n, 300 + n), a_off, 7.25), _guarded(_values(n, 400 + n), b_off, -3.5)
    a, b = torch.from_numpy(host_a).cuda(), torch.from_numpy(host_b).cuda()
    want_a, want_b = host_a.copy(), host_b.copy()
    want_a[a_off:a_off + n], want_b[b_off:b_off + n] = host_b[b_off:b_off + n], host_a[a_off:a_off + n]
    assert lib.mvf_ema_swap(a.data_ptr() + 4 * a_off, b.data_ptr() + 4 * b_off, n, None) == 0, lib.mvf_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(_bits(a.cpu().numpy()), _bits(want_a)) and np.array_equal(_bits(b.cpu().numpy()), _bits(want_b)), what
    assert lib.mvf_ema_swap(a.data_ptr() + 4 * a_off, b.data_ptr() + 4 * b_off, n, None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(_bits(a.cpu().numpy()), _bits(host_a)) and np.array_equal(_bits(b.cpu().numpy()), _bits(host_b)), "second swap, " + what


@pytest.mark.parametrize("n", SIZES)
def test_ema_swap_exchanges_bit_for_bit_at_every_offset(n):
    lib = _lib()
    for a_off in OFFSETS:
        for b_off in OFFSETS:
            _check_swap(lib, n, a_off, b_off)


# ------------------------------------------------------------------------------------------------ 4. argument checks
def test_ema_entry_points_argument_checks():
    lib = _lib()
    err = lib.mvf_last_error
    for f in (lib.mvf_ema_update, lib.mvf_ema_swap, lib.mvf_sgd_nesterov_step_ema, lib.mvf_sgd_step_segments_ema):
        assert f.restype is C.c_int
    buf = torch.full((64,), 2.0, device="cuda")
    p = buf.data_ptr()
    assert lib.mvf_ema_update(None, None, 0, 0.5, None) == 0 and lib.mvf_ema_swap(None, None, 0, None) == 0        # n = 0: nothing to do, nothing launched
    assert lib.mvf_ema_update(p, p + 32, 0, 0.5, None) == 0 and lib.mvf_ema_swap(p, p + 32, 0, None) == 0
    for a, b in ((None, p), (p, None), (None, None)):
        assert lib.mvf_ema_update(a, b, 4, 0.5, None) != 0 and b"NULL" in err()
        assert lib.mvf_ema_swap(a, b, 4, None) != 0 and b"NULL" in err()
    assert lib.mvf_ema_update(p, p + 32, -1, 0.5, None) != 0 and b"negative" in err()
    assert lib.mvf_ema_swap(p, p + 32, -1, None) != 0 and b"negative" in err()
    assert lib.mvf_ema_update(p, p + 16, 8, 0.5, None) != 0 and b"overlap" in err()
    assert lib.mvf_ema_swap(p, p + 16, 8, None) != 0 and b"overlap" in err()
    assert lib.mvf_ema_swap(p, p, 8, None) != 0 and b"overlap" in err()
    assert lib.mvf_ema_update(p + 2, p + 32, 4, 0.5, None) != 0 and b"aligned" in err()
    for m in (-0.25, 1.5, float("nan"), float("inf")):
        assert lib.mvf_ema_update(p, p + 32, 8, m, None) != 0 and b"momentum" in err(), m
    # the _ema optimizer steps: params / grads / momentum / ema of 8 elements each, 8 apart
    norm = torch.zeros(2, device="cuda")
    ws = torch.empty(lib.mvf_sgd_workspace_bytes(8), dtype=torch.uint8, device="cuda")
    tab = torch.from_numpy(np.array([(0, 1.0, 1.0)], dtype=SEG_DTYPE).view(np.uint8)).cuda()

    def flat(ema, m):
        return lib.mvf_sgd_nesterov_step_ema(p, p + 32, p + 64, 8, 1.0, 40.0, 0.01, 0.9, 1e-4, 1, ema, m, norm.data_ptr(), ws.data_ptr(), ws.numel(), None)

    def segs(ema, m):
        return lib.mvf_sgd_step_segments_ema(p, p + 32, p + 64, 8, 1.0, 40.0, 0.01, 0.9, 1e-4, 1, 1, tab.data_ptr(), 1, ema, m, norm.data_ptr(), ws.data_ptr(),
                                             ws.numel(), None)
    for step in (flat, segs):
        assert step(None, 0.5) != 0 and b"NULL ema" in err()
        assert step(p + 96 + 2, 0.5) != 0 and b"aligned" in err()
        for other, name in ((0, b"params"), (32, b"grads"), (64, b"momentum_buf")):
            assert step(p + other + 16, 0.5) != 0 and b"overlap" in err() and name in err(), name
        for m in (-0.25, 1.5, float("nan")):
            assert step(p + 96, m) != 0 and b"ema_momentum" in err(), m
    torch.cuda.synchronize()
    assert bool((buf == 2.0).all()) and bool((norm == 0.0).all())


# ------------------------------------------------------------------------------------------------ 5. fused equals unfused
LR, MOM, WD, MAX_NORM = 0.01, 0.9, 1e-4, 40.0
SEG_DTYPE = np.dtype([("first", "<i8"), ("lr_mult", "<f4"), ("decay_mult", "<f4")])      # mvf_sgd_segment_t
SEG_N = 262144 + 3
# the eight-segment table of test_head_optimizer_gpu.py: starts inside and on the edges of a workgroup's 256-element run, two excluded segments (lr_mult < 0)
SEGMENTS = ((0, 1.0, 1.0), (7, 2.0, 0.0), (256, -1.0, 0.0), (257, 1.0, 0.0), (1000, 0.5, 0.5), (1001, -1.0, 1.0), (70000, 1.0, 1.0), (262146, 2.0, 0.0))


def _fused_vs_unfused(n, segs=None, nesterov=1):
    """Three steps (clipping / not clipping / max_norm = 0; ema momentum 1, 0.5, 2e-4): the _ema step on one set of buffers, the plain step + mvf_ema_update on
    copies.  Views one element into their allocations (4-byte aligned only, as the engine's flat_*[off:])."""
    lib = _lib()
    gen = torch.Generator().manual_seed(n + 7 * nesterov)
    P = lambda t: t.data_ptr()       # noqa: E731

    def view(t):
        full = torch.full((n + 2,), -123.25, device="cuda")
        full[1:n + 1] = t.cuda()
        return full, full[1:n + 1]
    p0, e0 = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    (pf, pa), (bf, ba), (ef, ea) = view(p0), view(torch.full((n,), 7.0)), view(e0)
    (pg, pb), (bg, bb), (eg, eb) = view(p0), view(torch.full((n,), 7.0)), view(e0)
    norm_a, norm_b = torch.full((2,), float("nan"), device="cuda"), torch.full((2,), float("nan"), device="cuda")
    ws = torch.empty(lib.mvf_sgd_workspace_bytes(n), dtype=torch.uint8, device="cuda")
    tab, excl = None, torch.zeros(n, dtype=torch.bool)
    if segs is not None:
        tab = torch.from_numpy(np.array(list(segs), dtype=SEG_DTYPE).view(np.uint8)).cuda()
        firsts = [s[0] for s in segs] + [n]
        excl = torch.from_numpy(np.repeat(np.array([s[1] < 0 for s in segs]), np.diff(firsts)))
    excl = excl.cuda()
    for step, m in enumerate(MOMENTA):
        g = torch.randn(n, generator=gen)
        g[excl.cpu()] = 0.0
        g = g * ((10.0 if step == 1 else 100.0) / float(g.double().norm()))          # norm 100 / 10 / 100 against max_norm 40 / 40 / 0
        g[excl.cpu()] = 1e30                                                          # would make the norm infinite if it entered it
        gf, gv = view(g)
        max_norm, first = (0.0 if step == 2 else MAX_NORM), int(step == 0)
        e_before = ea.clone()
        if segs is None:
            ra = lib.mvf_sgd_nesterov_step_ema(P(pa), P(gv), P(ba), n, 1.0, max_norm, LR, MOM, WD, first, P(ea), m, P(norm_a), P(ws), ws.numel(), None)
            rb = lib.mvf_sgd_nesterov_step(P(pb), P(gv), P(bb), n, 1.0, max_norm, LR, MOM, WD, first, P(norm_b), P(ws), ws.numel(), None)
        else:
            ra = lib.mvf_sgd_step_segments_ema(P(pa), P(gv), P(ba), n, 1.0, max_norm, LR, MOM, WD, first, nesterov, P(tab), len(segs), P(ea), m, P(norm_a), P(ws),
                                               ws.numel(), None)
            rb = lib.mvf_sgd_step_segments(P(pb), P(gv), P(bb), n, 1.0, max_norm, LR, MOM, WD, first, nesterov, P(tab), len(segs), P(norm_b), P(ws), ws.numel(), None)
        assert ra == 0 and rb == 0, lib.mvf_last_error()
        assert lib.mvf_ema_update(P(eb), P(pb), n, m, None) == 0, lib.mvf_last_error()
        torch.cuda.synchronize()
        coef = float(norm_a[1])
        assert (coef < 0.5) if step == 0 else (coef == 1.0), (step, coef)
        bits = lambda t: t.view(torch.int32)       # noqa: E731
        assert torch.equal(bits(norm_a), bits(norm_b)), step
        assert torch.equal(bits(pf), bits(pg)) and torch.equal(bits(bf), bits(bg)), step          # whole allocations: the guards too
        assert not torch.equal(pa, p0.cuda())
        if bool(excl.any()):
            assert torch.equal(bits(ea[excl]), bits(e_before[excl])), step                        # excluded segments: the average keeps its bits
            eb[excl] = e_before[excl]                                                               # (the unfused update knows no segments)
        assert torch.equal(bits(ef), bits(eg)), step
        assert not torch.equal(ea[~excl], e_before[~excl])
        if m == 1.0:
            assert torch.equal(bits(ea[~excl]), bits(pa[~excl]))
        assert bool((gf[0] == -123.25) & (gf[-1] == -123.25))


@pytest.mark.parametrize("n", [1, 255, 5000, 262147, 1048579], ids=lambda n: "n%d" % n)
def test_sgd_nesterov_step_ema_equals_the_plain_step_then_ema_update(n):
    """n above 1048576 iterates the update kernel's own grid-stride loop (grid_for caps it at 4096 x 256 threads)."""
    _fused_vs_unfused(n)


@pytest.mark.parametrize("nesterov", [0, 1], ids=["plain_momentum", "nesterov"])
def test_sgd_step_segments_ema_equals_the_plain_step_then_ema_update(nesterov):
    _fused_vs_unfused(SEG_N, segs=SEGMENTS, nesterov=nesterov)


# ------------------------------------------------------------------------------------------------ engines
def _model(dropout=0.0, **backbone):
    import mvfnet_amd
    cfg = mvfnet_amd.mvfnet_config(50, 4, dropout_ratio=dropout)
    cfg["backbone"].update(backbone)
    m = mvfnet_amd.build_recognizer(cfg, None, dict(average_clips=None))
    sd = m.state_dict()
    vals = synth.synth_state_dict({"r50/" + k: tuple(v.shape) for k, v in sd.items()})
    m.load_state_dict({k: torch.from_numpy(vals["r50/" + k]) for k in sd}, strict=True)
    return m.cuda().train()


def _batch(seed, clips=2):
    return (torch.from_numpy(synth.synth_clip_batch(clips, 4, 64, 64, seed=seed)).cuda(), torch.from_numpy(synth.synth_labels(clips, seed=seed)).cuda())


def _same_training_state(ma, ea, mb, eb):
    return (torch.equal(ea.flat_params, eb.flat_params) and torch.equal(ea.flat_mom, eb.flat_mom)
            and all(torch.equal(a, b) for a, b in zip(ma.buffers(), mb.buffers())))


class _Recurrence(object):
    """The host-side fp64 recurrence on the parameter snapshots read back from the device."""

    def __init__(self, eng, momentum, warmup):
        from mvfnet_amd.ema import momentum_at
        self.at = lambda t: float(np.float32(momentum_at(momentum, warmup, t)))
        self.ref = eng.flat_params.cpu().numpy().astype(np.float64)
        self.scale, self.t = float(np.abs(self.ref).max()), 0

    def step(self, eng):
        """-> (max |flat_ema - reference|, the bound) after one more update"""
        p = eng.flat_params.cpu().numpy().astype(np.float64)
        self.ref += self.at(self.t) * (p - self.ref)
        self.t += 1
        self.scale = max(self.scale, float(np.abs(p).max()))
        return float(np.abs(eng.flat_ema.cpu().numpy().astype(np.float64) - self.ref).max()), self.t * ULP * self.scale


_RUNS = {}


def _twin_run(dtype):
    """Engine A with the average on (momentum 0.25, two warm-up steps: m = 1, 1/2, 0.25, 0.25), engine B without, same weights, same batches.  Four
    train_steps (two eager, two recorded: a launch plan is live afterwards), then A scores a batch inside averaged_weights(), then a fifth step on both."""
    if dtype in _RUNS:
        return _RUNS[dtype]
    import mvfnet_amd
    from mvfnet_amd import checkpoint
    ma, mb = _model(), _model()
    ea, eb = ma.train_engine(dtype=dtype), mb.train_engine(dtype=dtype)
    assert eb.flat_ema is None and ea.flat_ema is None
    ea.enable_ema(momentum=0.25, warmup_steps=2)
    r = dict(init_equal=torch.equal(ea.flat_ema, ea.flat_params), updates0=ea.ema_updates, same=[], err=[], moved=[])
    rec = _Recurrence(ea, 0.25, 2)
    for i in range(4):
        imgs, labels = _batch(30 + i)
        before = ea.flat_ema.clone()
        la, lb = ea.train_step(imgs.clone(), labels.clone(), lr=0.01), eb.train_step(imgs.clone(), labels.clone(), lr=0.01)
        torch.cuda.synchronize()
        r["same"].append(_same_training_state(ma, ea, mb, eb) and torch.equal(la, lb))
        r["err"].append(rec.step(ea))
        r["moved"].append(not torch.equal(before, ea.flat_ema))
        if i == 0:
            r["first_is_copy"] = torch.equal(ea.flat_ema.view(torch.int32), ea.flat_params.view(torch.int32))
    r["updates4"], r["steps4"] = ea.ema_updates, ea.steps
    r["views"] = all(torch.equal(ea.ema_of(p), ea.flat_ema[ea.grad_of(p).storage_offset():][:p.numel()].view(p.shape)) for p in ma.parameters())
    r["ema_differs"] = not torch.equal(ea.flat_ema, ea.flat_params)
    r["plan_live"] = any(st["plan"] is not None for st in ea._plans.values())
    # ---- averaged_weights()
    imgs, labels = _batch(40)
    p_before, e_before = ea.flat_params.clone(), ea.flat_ema.clone()
    ckpt = dict(state_dict=checkpoint.weights_to_cpu(ma.state_dict()), ema=ea.ema_state_dict())
    with ea.averaged_weights():
        r["inside_params_are_ema"] = torch.equal(ea.flat_params, e_before) and torch.equal(ea.flat_ema, p_before)
        sd_inside = {k: v.detach().cpu().clone() for k, v in ma.state_dict().items()}
        ma.eval()
        r["scores_inside"] = ma(return_loss=False, img_group=imgs)
        ma.train()
        raised = []
        for call in (lambda: ea.train_step(imgs, labels), lambda: ea.accumulate_step(imgs, labels), lambda: ea.step(), lambda: ea.averaged_weights().__enter__(),
                     lambda: ea.reset_ema()):
            try:
                call()
                raised.append(False)
            except RuntimeError:
                raised.append(True)
        r["raised"] = raised
    torch.cuda.synchronize()
    r["restored"] = torch.equal(ea.flat_params.view(torch.int32), p_before.view(torch.int32)) and torch.equal(ea.flat_ema.view(torch.int32), e_before.view(torch.int32))
    ma.eval()
    r["scores_live"] = ma(return_loss=False, img_group=imgs)
    ma.train()
    avg = checkpoint.averaged_state_dict(ckpt)
    r["state_dict_inside_is_averaged"] = all(torch.equal(sd_inside[k], avg[k]) for k in avg) and set(avg) == set(sd_inside)
    fresh = mvfnet_amd.build_recognizer(mvfnet_amd.mvfnet_config(50, 4, dropout_ratio=0.0), None, dict(average_clips=None))
    fresh.load_state_dict(avg, strict=True)
    r["scores_fresh"] = fresh.cuda().eval()(return_loss=False, img_group=imgs)
    del fresh
    imgs, labels = _batch(34)
    la, lb = ea.train_step(imgs.clone(), labels.clone(), lr=0.01), eb.train_step(imgs.clone(), labels.clone(), lr=0.01)
    torch.cuda.synchronize()
    r["same_after_block"] = _same_training_state(ma, ea, mb, eb) and torch.equal(la, lb)
    r["err5"] = rec.step(ea)
    r["b_never_enabled"] = eb.flat_ema is None and eb.ema_updates == 0
    _RUNS[dtype] = r
    return r


DTYPES = pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])


# ------------------------------------------------------------------------------------------------ 6. train_step
@DTYPES
def test_train_steps_keep_the_average_and_do_not_perturb_training(dtype):
    r = _twin_run(dtype)
    assert r["init_equal"] and r["updates0"] == 0
    assert r["same"] == [True] * 4                       # parameters, momentum, BatchNorm buffers and loss: bit-identical to the engine without the average
    for i, (err, bound) in enumerate(r["err"] + [r["err5"]]):
        print("step %d: max |flat_ema - fp64 recurrence| = %.3e (bound %.3e)" % (i + 1, err, bound))
    assert all(err <= bound for err, bound in r["err"] + [r["err5"]]), r["err"]
    assert r["first_is_copy"]                            # m = 1: the average after the first step IS the parameters
    assert r["moved"] == [True] * 4 and r["ema_differs"]
    assert r["updates4"] == 4 and r["steps4"] == 4 and r["views"] and r["b_never_enabled"]


# ------------------------------------------------------------------------------------------------ 9. averaged_weights()
def test_averaged_weights_block_scores_the_average_and_restores_every_bit():
    r = _twin_run(torch.bfloat16)
    assert r["plan_live"]                                # the step after the block replays a launch plan
    assert r["inside_params_are_ema"] and r["state_dict_inside_is_averaged"]
    assert np.array_equal(_bits(r["scores_inside"]), _bits(r["scores_fresh"]))          # the model loaded with averaged_state_dict
    assert not np.array_equal(r["scores_inside"], r["scores_live"])
    assert r["raised"] == [True] * 5                     # train_step, accumulate_step, step, nested entry, reset_ema
    assert r["restored"]
    assert r["same_after_block"]                         # loss, parameters, momentum, buffers equal the twin's that never entered the block


# ------------------------------------------------------------------------------------------------ 7. accumulation
@DTYPES
def test_accumulated_steps_move_the_average_once_per_optimizer_step(dtype):
    ma, mb = _model(), _model()
    ea, eb = ma.train_engine(dtype=dtype), mb.train_engine(dtype=dtype)
    ea.enable_ema(momentum=0.25, warmup_steps=2)
    rec = _Recurrence(ea, 0.25, 2)
    for group in range(2):
        before = ea.flat_ema.clone()
        for i in range(3):
            imgs, labels = _batch(50 + 3 * group + i)
            ea.accumulate_step(imgs.clone(), labels.clone())
            eb.accumulate_step(imgs.clone(), labels.clone())
            assert torch.equal(ea.flat_ema.view(torch.int32), before.view(torch.int32)) and ea.ema_updates == group          # untouched between micro-steps
        ea.apply_accumulated(lr=0.01)
        eb.apply_accumulated(lr=0.01)
        torch.cuda.synchronize()
        assert _same_training_state(ma, ea, mb, eb)
        assert not torch.equal(ea.flat_ema, before) and ea.ema_updates == group + 1
        err, bound = rec.step(ea)
        print("optimizer step %d: max |flat_ema - fp64 recurrence| = %.3e (bound %.3e)" % (group + 1, err, bound))
        assert err <= bound
        if group == 0:
            assert torch.equal(ea.flat_ema.view(torch.int32), ea.flat_params.view(torch.int32))
    assert ea.ema_updates == 2 and ea.steps == 2 and eb.flat_ema is None


# ------------------------------------------------------------------------------------------------ 8. frozen parts
@pytest.mark.parametrize("backbone", [dict(frozen_stages=1), dict(norm_eval=True, norm_frozen=True)], ids=["frozen_prefix", "norm_frozen_scattered"])
def test_average_of_untrained_parameters_stays_bit_equal_to_them(backbone):
    m = _model(**backbone)
    frozen = [n for n, p in m.named_parameters() if not p.requires_grad]
    assert frozen and len(frozen) < len(list(m.parameters()))
    eng = m.train_engine(max_norm=5.0)
    eng.enable_ema(momentum=0.25)
    p0 = {n: p.detach().clone() for n, p in m.named_parameters()}
    for i in range(2):
        eng.train_step(*_batch(60 + i))
    torch.cuda.synchronize()
    assert eng._scattered_frozen == ("norm_frozen" in backbone) and eng.ema_updates == 2
    for n, p in m.named_parameters():
        e = eng.ema_of(p)
        if p.requires_grad:
            assert not torch.equal(p, p0[n]) and not torch.equal(e, p), n
        else:
            assert torch.equal(e.view(torch.int32), p.view(torch.int32)) and torch.equal(p, p0[n]), n


# ------------------------------------------------------------------------------------------------ 10. never enabled
NEW_ENTRY_POINTS = {"mvf_sgd_nesterov_step_ema", "mvf_sgd_step_segments_ema", "mvf_ema_update", "mvf_ema_swap"}


def test_an_engine_that_never_enables_the_average_calls_only_the_plain_entry_points():
    m = _model()
    eng = m.train_engine()
    imgs, labels = _batch(70)
    seen = {}
    for form, nesterov in (("flat", True), ("segments", False)):
        eng.nesterov = nesterov
        eng.forward(imgs, labels)
        eng.backward()
        with library_names(eng) as names:
            eng.step()
        seen[form] = names
    torch.cuda.synchronize()
    assert eng.flat_ema is None and eng.ema_updates == 0
    assert [n for n in seen["flat"] if "sgd" in n and "workspace" not in n] == ["mvf_sgd_nesterov_step"]
    assert [n for n in seen["segments"] if "sgd" in n and "workspace" not in n] == ["mvf_sgd_step_segments"]
    assert not NEW_ENTRY_POINTS & set(seen["flat"] + seen["segments"])
    # and with the average on, the same two paths take the _ema twins
    eng.enable_ema(momentum=0.25)
    for form, nesterov, want in (("flat", True, "mvf_sgd_nesterov_step_ema"), ("segments", False, "mvf_sgd_step_segments_ema")):
        eng.nesterov = nesterov
        eng.forward(imgs, labels)
        eng.backward()
        with library_names(eng) as names:
            eng.step()
        assert [n for n in names if "sgd" in n and "workspace" not in n] == [want]
    assert eng.ema_updates == 2


# ------------------------------------------------------------------------------------------------ the other two ways into the optimizer
def test_engine_sgd_and_the_fp16_hook_move_the_average_too():
    """EngineSGD.step (build_optimizer's object) and Fp16OptimizerHook.after_train_iter end in _apply_sgd like train_step and apply_accumulated."""
    from mvfnet_amd.dist import Fp16OptimizerHook
    from mvfnet_amd.runner import build_optimizer
    m = _model()
    hook = Fp16OptimizerHook(grad_clip=dict(max_norm=40.0, norm_type=2), distributed=False)
    hook.before_run(m)
    opt = build_optimizer(m, dict(type="SGD", lr=0.01, momentum=0.9, weight_decay=1e-4, nesterov=True))
    eng = opt.engine
    assert eng is m.train_engine() and eng.tdtype == torch.bfloat16
    eng.enable_ema(momentum=0.25, warmup_steps=1)
    imgs, labels = _batch(80)
    hook.after_train_iter(m, opt, m(imgs, labels)["loss_cls"])
    torch.cuda.synchronize()
    assert eng.ema_updates == 1 and torch.equal(eng.flat_ema, eng.flat_params)          # m = 1
    eng.forward(imgs, labels)
    eng.backward()
    opt.step()
    torch.cuda.synchronize()
    assert eng.ema_updates == 2 and not torch.equal(eng.flat_ema, eng.flat_params)


# ------------------------------------------------------------------------------------------------ 11. checkpoints
def test_checkpoint_round_trip_carries_the_average(tmp_path):
    import mvfnet_amd
    from mvfnet_amd.checkpoint import averaged_state_dict, load_checkpoint
    from mvfnet_amd.runner import Runner
    ema = dict(momentum=0.25, warmup_steps=3)
    log = []
    m = _model()
    run = Runner(m, work_dir=str(tmp_path), lr=0.01, ema=ema, logger=log.append)
    eng = run.engine
    for i in range(2):
        eng.train_step(*_batch(90 + i), lr=0.01)
    path = run.save_checkpoint()
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    assert sorted(ckpt) == ["ema", "meta", "optimizer", "state_dict"]
    assert ckpt["ema"]["updates"] == 2 and ckpt["ema"]["momentum"] == 0.25 and ckpt["ema"]["warmup_steps"] == 3
    assert list(ckpt["ema"]["state_dict"]) == [n for n, _ in m.named_parameters()]
    assert all(torch.equal(ckpt["state_dict"][n], p.detach().cpu()) for n, p in m.named_parameters())          # state_dict stays the live weights
    m2 = _model()
    with torch.no_grad():
        for p in m2.parameters():
            p.add_(1.0)
    run2 = Runner(m2, work_dir=str(tmp_path), lr=0.01, ema=ema, logger=log.append)
    run2.resume(path)
    eng2 = run2.engine
    assert eng2.ema_updates == eng.ema_updates == 2
    assert torch.equal(eng2.flat_ema.view(torch.int32), eng.flat_ema.view(torch.int32)) and torch.equal(eng2.flat_params, eng.flat_params)
    assert not torch.equal(eng2.flat_ema, eng2.flat_params)
    imgs, labels = _batch(92)
    eng.train_step(imgs.clone(), labels.clone(), lr=0.01)
    eng2.train_step(imgs.clone(), labels.clone(), lr=0.01)
    torch.cuda.synchronize()
    assert eng.ema_updates == eng2.ema_updates == 3
    assert torch.equal(eng2.flat_ema.view(torch.int32), eng.flat_ema.view(torch.int32))
    # the file loads through the plain loader into a model that keeps no average
    m3 = mvfnet_amd.build_recognizer(mvfnet_amd.mvfnet_config(50, 4, dropout_ratio=0.0), None, dict(average_clips=None))
    info = load_checkpoint(m3, path, strict=True)
    assert "ema" in info and all(torch.equal(a, b) for a, b in zip(m3.state_dict().values(), ckpt["state_dict"].values()))
    avg = averaged_state_dict(ckpt)
    assert all(torch.equal(avg[n], ckpt["ema"]["state_dict"][n]) for n in ckpt["ema"]["state_dict"])
    assert torch.equal(avg["backbone.bn1.running_mean"], ckpt["state_dict"]["backbone.bn1.running_mean"])
    # a checkpoint without the entry: the average starts over from the loaded weights, and one line says so
    del ckpt["ema"]
    bare = os.path.join(str(tmp_path), "bare.pth")
    torch.save(ckpt, bare)
    assert not any("averaged" in line for line in log)
    run2.resume(bare)
    assert eng2.ema_updates == 0 and torch.equal(eng2.flat_ema, eng2.flat_params)
    assert sum("averaged" in line and "bare.pth" in line for line in log) == 1
