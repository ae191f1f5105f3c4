"""The fused clip + Adam / AdamW step (mvf_adamw_step; csrc/optim.hip norm_finalize / adamw_kernel) through the C ABI against the fp64 restatement
in adamw_numpy.py, and the engine / runner / checkpoint layers above it (TrainEngine(optimizer='adamw'), build_optimizer(type='AdamW'), Runner.resume).

Settings: lr 1e-3, betas (0.9, 0.999), eps 1e-8, weight_decay 0.05, max_norm 40 (adamw_numpy's constants).  Gradients follow test_head_optimizer_gpu.sgd_grads:
the scaled norm is 100, 10, 100 over three steps against max_norm 40, 40, 0, so only step 0 clips; moments and the device step counter carry over.

Bounds.  Norm and clip coefficient: the SGD test's (NORM_BOUND = 1e-5; |coef - ref| <= 2e-5 ref).  params / exp_avg / exp_avg_sq, each as max abs error over max
abs reference: 10 x the figure the same update in fp32 numpy (adamw_numpy.adamw_ref(ft=np.float32), every scalar rounded once from double) reaches against fp64
for that case -- ADAMW_FP32 below, measured on the CPU with `python tests/adamw_numpy.py`: 1.7e-8 ... 2.7e-7, so every bound is under 3e-6.  A case the table does
not list (segment tables, the guard's and the engine's cases) takes the table's row of the same n / grad_scale / decoupled, else the worst row."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adamw_numpy as A  # noqa: E402
from helpers import library_names  # noqa: E402
from mvfnet_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu

P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
NORM_BOUND = 1e-5
SEG_DTYPE = np.dtype([("first", "<i8"), ("lr_mult", "<f4"), ("decay_mult", "<f4")])      # mvf_sgd_segment_t
SEG_N = 262144 + 3
SEGMENTS = ((0, 1.0, 1.0), (7, 2.0, 0.0), (256, -1.0, 0.0), (257, 1.0, 0.0), (1000, 0.5, 0.5), (1001, -1.0, 1.0), (70000, 1.0, 1.0), (262146, 2.0, 0.0))
# (n, grad_scale, decoupled) -> worst fp32-numpy-vs-fp64 figure over the three steps: (params, exp_avg, exp_avg_sq)
ADAMW_FP32 = {
    (1, 1.0, 0): (1.323e-07, 4.774e-08, 5.671e-08), (1, 1.0, 1): (8.215e-08, 1.726e-08, 3.723e-08),
    (1, 0.125, 0): (5.860e-08, 1.819e-08, 5.552e-08), (1, 0.125, 1): (7.679e-08, 4.087e-08, 3.723e-08),
    (255, 1.0, 0): (6.832e-08, 9.861e-08, 1.425e-07), (255, 1.0, 1): (1.144e-07, 9.862e-08, 2.179e-07),
    (255, 0.125, 0): (1.054e-07, 9.642e-08, 2.519e-07), (255, 0.125, 1): (1.022e-07, 9.910e-08, 1.907e-07),
    (257, 1.0, 0): (7.443e-08, 8.113e-08, 1.076e-07), (257, 1.0, 1): (1.389e-07, 9.252e-08, 1.343e-07),
    (257, 0.125, 0): (6.440e-08, 1.003e-07, 1.304e-07), (257, 0.125, 1): (1.058e-07, 9.961e-08, 1.959e-07),
    (5000, 1.0, 0): (8.176e-08, 1.138e-07, 2.105e-07), (5000, 1.0, 1): (1.306e-07, 1.002e-07, 2.717e-07),
    (5000, 0.125, 0): (6.860e-08, 9.455e-08, 1.712e-07), (5000, 0.125, 1): (1.204e-07, 1.136e-07, 1.758e-07),
    (262147, 1.0, 0): (6.299e-08, 1.273e-07, 1.727e-07), (262147, 1.0, 1): (1.506e-07, 1.233e-07, 2.222e-07),
    (262147, 0.125, 0): (8.113e-08, 1.265e-07, 2.025e-07), (262147, 0.125, 1): (2.105e-07, 1.118e-07, 2.381e-07),
    (1048581, 1.0, 1): (1.911e-07, 1.461e-07, 2.009e-07),
}
WORST = tuple(max(v[k] for v in ADAMW_FP32.values()) for k in range(3))


def bounds(n=None, gs=None, decoupled=None):
    return tuple(10.0 * f for f in ADAMW_FP32.get((n, gs, decoupled), WORST))


def _lib():
    from mvfnet_amd import _lib as L
    return L


def _bits(t):
    return t.view(torch.int32)


class Ops(object):
    """Device operands of one mvf_adamw_step call sequence: views at `offset` into buffers filled with a guard value."""
    FILL = -123.25

    def __init__(self, n, p0, offset=0, segs=None, ema=False, guard=False, decoupled=1):
        self.L = _lib()
        self.n, self.offset, self.decoupled = n, offset, decoupled
        self.full = {}
        for name, v in (("p", p0), ("g", np.zeros(n)), ("m", np.zeros(n)), ("v", np.zeros(n))) + ((("e", p0),) if ema else ()):
            full = torch.full((n + 2 * offset,), self.FILL, device="cuda")
            full[offset:offset + n] = torch.from_numpy(np.asarray(v, dtype=np.float32)).cuda()
            self.full[name] = full
        view = lambda k: self.full[k][offset:offset + n] if k in self.full else None  # noqa: E731
        self.p, self.g, self.m, self.v, self.e = (view(k) for k in "pgmve")
        self.norm = torch.full((2,), float("nan"), device="cuda")
        self.ws = torch.empty(self.L.lib.mvf_adamw_workspace_bytes(n), dtype=torch.uint8, device="cuda")
        self.count = torch.zeros(1, dtype=torch.int64, device="cuda")
        self.guard = torch.zeros(4, dtype=torch.int32, device="cuda") if guard else None
        self.tab = torch.from_numpy(np.array(list(segs), dtype=SEG_DTYPE).view(np.uint8)).cuda() if segs is not None else None
        self.nseg = len(segs) if segs is not None else 0
        self.hyper = self.L.AdamwHyper(A.LR, A.BETAS[0], A.BETAS[1], A.EPS, A.WD, decoupled)

    def step(self, g, gs, max_norm, ema_m=0.25, use_ema=True):
        self.g.copy_(torch.from_numpy(np.asarray(g, dtype=np.float32)).cuda())
        e = self.e if use_ema else None
        self.L.check(self.L.lib.mvf_adamw_step(P(self.p), P(self.g), P(self.m), P(self.v), self.n, gs, max_norm, C.byref(self.hyper), P(self.tab), self.nseg,
                                               P(e), ema_m, P(self.guard), P(self.count), P(self.norm), P(self.ws), self.ws.numel(), None), "adamw_step")
        torch.cuda.synchronize()

    def untouched_outside(self):
        o, n = self.offset, self.n
        return all(bool((f[:o] == self.FILL).all()) and bool((f[o + n:] == self.FILL).all()) for f in self.full.values())

    def state(self):
        torch.cuda.synchronize()
        return [_bits(t).clone() for t in (self.p, self.m, self.v, self.e, self.norm) if t is not None]


def _close(got, ref, bound, what):
    e = A.rel(got, ref)
    print("%s: %.3e (bound %.3e)" % (what, e, bound))
    assert np.isfinite(np.asarray(got)).all() and e < bound, (what, e, bound)


def run_steps(n, gs, decoupled, segs=None, offset=0, excluded_fill=None):
    """Three steps against the fp64 reference, which keeps its own fp64 state; returns the operands."""
    p0, m0, v0, grads = A.case_inputs(n, gs, decoupled)
    tab = segs if segs is not None else ((0, 1.0, 1.0),)
    excl = np.repeat(np.array([s[1] < 0 for s in tab]), np.diff([s[0] for s in tab] + [n]))
    bp, bm, bv = bounds(n, gs, decoupled)
    ops = Ops(n, p0, offset=offset, segs=segs, decoupled=decoupled)
    p_ref, m_ref, v_ref = p0.astype(np.float64), m0.astype(np.float64), v0.astype(np.float64)
    p_start = ops.p.clone()
    for step, g in enumerate(grads):
        if excluded_fill is not None:           # excluded elements outside the norm: finite norm = 100 or 10 over the rest
            keep = np.where(excl, np.float32(0), g)
            g = (keep * ((10.0 if step == 1 else 100.0) / (gs * np.sqrt((keep.astype(np.float64) ** 2).sum())))).astype(np.float32)
            g[excl] = np.resize(np.array(excluded_fill, dtype=np.float32), int(excl.sum()))
        max_norm = 0.0 if step == 2 else A.MAX_NORM
        p_ref, m_ref, v_ref, n_ref, c_ref = A.adamw_ref(p_ref, m_ref, v_ref, g, gs, max_norm, step + 1, decoupled, tab)
        assert (c_ref < 0.5) if step == 0 else (c_ref == 1.0), (step, c_ref)          # the reference clips in step 0 only
        ops.step(g, gs, max_norm)
        nrm, coef = float(ops.norm[0]), float(ops.norm[1])
        print("step %d: norm %.3g" % (step, abs(nrm - n_ref) / n_ref))
        assert np.isfinite(nrm) and abs(nrm - n_ref) < NORM_BOUND * n_ref, (step, nrm, n_ref)
        assert abs(coef - c_ref) <= 2e-5 * c_ref, (step, coef, c_ref)
        t = ~excl
        _close(ops.p.cpu().numpy()[t], p_ref[t], bp, "step %d params" % step)
        _close(ops.m.cpu().numpy()[t], m_ref[t], bm, "step %d exp_avg" % step)
        _close(ops.v.cpu().numpy()[t], v_ref[t], bv, "step %d exp_avg_sq" % step)
        assert int(ops.count) == step + 1
        if excl.any():                          # excluded segments: parameters and both moments bit-unchanged
            e = torch.from_numpy(excl).cuda()
            assert torch.equal(_bits(ops.p[e]), _bits(p_start[e])) and not bool(_bits(ops.m[e]).any()) and not bool(_bits(ops.v[e]).any()), step
        if offset:
            assert ops.untouched_outside(), step
    return ops


# ------------------------------------------------------------------------------------------------ 1. against fp64
@pytest.mark.parametrize("decoupled", [0, 1], ids=["adam", "adamw"])
@pytest.mark.parametrize("gs", [1.0, 0.125])
@pytest.mark.parametrize("n", [1, 255, 257, 5000, 262144 + 3], ids=lambda n: "n%d" % n)
def test_adamw_step_vs_fp64(n, gs, decoupled):
    """Flat form, three steps (clipping / not clipping / max_norm = 0); 262147 iterates the norm kernels' grid-stride loop (1024 workgroups x 256); 1, 255 and
    257 are the one-workgroup edges.  *applied_steps reads 1, 2, 3."""
    run_steps(n, gs, decoupled)


def test_adamw_step_vs_fp64_beyond_one_sweep_of_the_update_grid():
    """n = 1048576 + 5: the update kernel's grid-stride loop iterates (4096 workgroups x 256)."""
    run_steps(1048576 + 5, 1.0, 1)


# ------------------------------------------------------------------------------------------------ 2. offset views
@pytest.mark.parametrize("n", [257, 5000])
def test_adamw_step_on_offset_views_leaves_the_neighbours_alone(n):
    """The engine calls the step on views of its flat buffers (flat_params[off:]): 4-byte aligned only.  Same bounds; the elements before and after all four
    arrays keep their bits."""
    run_steps(n, 0.125, 1, offset=1)


# ------------------------------------------------------------------------------------------------ 3. segments
@pytest.mark.parametrize("fill", [(1e30,), (float("nan"), float("inf"), -float("inf"))], ids=["excluded_1e30", "excluded_nan_inf"])
@pytest.mark.parametrize("decoupled", [0, 1], ids=["adam", "adamw"])
def test_adamw_step_segments_vs_fp64(decoupled, fill):
    """Eight segments whose starts are no multiples of 256, mixed multipliers, two excluded segments whose gradients would make the norm infinite or NaN if they
    entered it: the norm stays finite, the trained elements are within test 1's bounds, the excluded ones keep their bits."""
    run_steps(SEG_N, 0.125, decoupled, segs=SEGMENTS, excluded_fill=fill)


@pytest.mark.parametrize("decoupled", [0, 1], ids=["adam", "adamw"])
def test_adamw_one_segment_table_equals_the_flat_form_bit_for_bit(decoupled):
    a = run_steps(SEG_N, 0.125, decoupled)
    b = run_steps(SEG_N, 0.125, decoupled, segs=((0, 1.0, 1.0),))
    assert all(torch.equal(x, y) for x, y in zip(a.state(), b.state()))


# ------------------------------------------------------------------------------------------------ 4. average
@pytest.mark.parametrize("segs", [None, SEGMENTS], ids=["flat", "segments"])
@pytest.mark.parametrize("n", [257, SEG_N], ids=lambda n: "n%d" % n)
def test_adamw_step_with_the_average_equals_the_plain_step_then_ema_update(n, segs):
    """ema != NULL against the plain step followed by mvf_ema_update (per trained segment in the segment form): params, exp_avg, exp_avg_sq, ema and norm_out
    bit-equal over three steps with momenta 1, 0.5, 2e-4."""
    if segs is not None and n < SEG_N:
        segs = tuple(s for s in segs if s[0] < n)
    p0, _, _, grads = A.case_inputs(n, 0.125, 1)
    fused, plain = Ops(n, p0, segs=segs, ema=True), Ops(n, p0, segs=segs, ema=True)
    L = fused.L
    tab = segs if segs is not None else ((0, 1.0, 1.0),)
    firsts = [s[0] for s in tab] + [n]
    for step, (g, mom) in enumerate(zip(grads, (1.0, 0.5, 2e-4))):
        fused.step(g, 0.125, A.MAX_NORM, ema_m=mom)
        plain.step(g, 0.125, A.MAX_NORM, use_ema=False)
        for k, s in enumerate(tab):
            if s[1] >= 0:
                a, b = firsts[k], firsts[k + 1]
                L.check(L.lib.mvf_ema_update(P(plain.e[a:b]), P(plain.p[a:b]), b - a, mom, None), "ema_update")
        assert all(torch.equal(x, y) for x, y in zip(fused.state(), plain.state())), step
        assert int(fused.count) == int(plain.count) == step + 1
    assert not torch.equal(fused.e, fused.p)


# ------------------------------------------------------------------------------------------------ 5. guard
@pytest.mark.parametrize("bad", [float("nan"), 3e19], ids=["nan", "overflowing_sum_of_squares"])
def test_adamw_guard_skips_the_step_and_the_step_count(bad):
    """Good, bad, good at n = 5000: the bad step (one NaN element / one 3e19 element, whose square leaves fp32) leaves params, both moments and the average
    bit-unchanged, the guard reads {1, 1, 1, 2} and *applied_steps stays 1; after the third step everything matches an fp64 reference that never saw the bad
    step and bias-corrects with t = 2, within test 1's bounds -- the count lives on the device.  Only good steps: bit-equal to guard == NULL."""
    n, gs = 5000, 1.0
    p0, m0, v0, grads = A.case_inputs(n, gs, 1)
    bp, bm, bv = bounds(n, gs, 1)
    ops = Ops(n, p0, ema=True, guard=True)
    ref = [p0.astype(np.float64), m0.astype(np.float64), v0.astype(np.float64)]
    ops.step(grads[0], gs, A.MAX_NORM)
    ref = list(A.adamw_ref(ref[0], ref[1], ref[2], grads[0], gs, A.MAX_NORM, 1)[:3])
    after1 = ops.state()[:4]
    assert ops.guard.tolist() == [0, 0, 0, 1] and int(ops.count) == 1
    g_bad = grads[1].copy()
    g_bad[n // 2] = bad
    ops.step(g_bad, gs, A.MAX_NORM)
    assert not bool(torch.isfinite(ops.norm[0]))
    assert all(torch.equal(x, y) for x, y in zip(ops.state()[:4], after1))
    assert ops.guard.tolist() == [1, 1, 1, 2] and int(ops.count) == 1
    ops.step(grads[2], gs, 0.0)
    ref = list(A.adamw_ref(ref[0], ref[1], ref[2], grads[2], gs, 0.0, 2)[:3])
    assert ops.guard.tolist() == [0, 1, 0, 3] and int(ops.count) == 2
    _close(ops.p.cpu().numpy(), ref[0], bp, "params")
    _close(ops.m.cpu().numpy(), ref[1], bm, "exp_avg")
    _close(ops.v.cpu().numpy(), ref[2], bv, "exp_avg_sq")
    # the wrong count would show: the same third step corrected with t = 3 is far outside the bound
    wrong = A.adamw_ref(*A.adamw_ref(p0.astype(np.float64), m0.astype(np.float64), v0.astype(np.float64), grads[0], gs, A.MAX_NORM, 1)[:3], grads[2], gs, 0.0, 3)
    assert A.rel(wrong[0], ref[0]) > 10 * bp
    # good steps only: guard on == guard off, bit for bit
    a, b = Ops(n, p0, ema=True, guard=True), Ops(n, p0, ema=True, guard=False)
    for step, g in enumerate(grads):
        a.step(g, gs, A.MAX_NORM)
        b.step(g, gs, A.MAX_NORM)
        assert all(torch.equal(x, y) for x, y in zip(a.state(), b.state())), step
    assert a.guard.tolist() == [0, 0, 0, 3] and int(a.count) == int(b.count) == 3


# ================================================================================================ engine level
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


PARAMWISE = dict(bias_lr_mult=2.0, bias_decay_mult=0.0, norm_decay_mult=0.0)
OPT = dict(type="AdamW", lr=A.LR, betas=A.BETAS, eps=A.EPS, weight_decay=A.WD, paramwise_options=PARAMWISE)


def _optimizer(m, dtype=None, max_norm=5.0, cfg=OPT):
    from mvfnet_amd.runner import build_optimizer
    opt = build_optimizer(m, cfg, dtype=dtype)
    opt.engine.max_norm = max_norm
    return opt, opt.engine


class TorchTwin(object):
    """torch.optim.AdamW (foreach=False) + clip_grad_norm_ on fp64 CPU copies of the model's parameters, with the param groups build_optimizer's paramwise
    options describe; fed with the engine's own flat gradient."""

    def __init__(self, m, eng, max_norm, decoupled=True):
        from mvfnet_amd.runner import paramwise_multipliers
        self.m, self.eng, self.max_norm = m, eng, max_norm
        mult = paramwise_multipliers(m, PARAMWISE)
        self.named = [(n, p) for n, p in m.named_parameters()]
        self.copies = [torch.nn.Parameter(p.detach().cpu().double(), requires_grad=p.requires_grad) for _, p in self.named]
        groups = [dict(params=[c], lr=A.LR * mult.get(p, (1.0, 1.0))[0], weight_decay=A.WD * mult.get(p, (1.0, 1.0))[1]) for (_, p), c in zip(self.named, self.copies)]
        cls = torch.optim.AdamW if decoupled else torch.optim.Adam
        self.opt = cls(groups, lr=A.LR, betas=A.BETAS, eps=A.EPS, weight_decay=A.WD, foreach=False)

    def step(self, flat_grads, scale=1.0):
        for (_, p), c in zip(self.named, self.copies):
            c.grad = None
            if p.requires_grad:
                v = self.eng.grad_of(p)
                first = v.storage_offset()
                c.grad = flat_grads[first:first + p.numel()].view(p.shape).detach().cpu().double() * scale
        torch.nn.utils.clip_grad_norm_([c for c in self.copies if c.requires_grad], self.max_norm)
        self.opt.step()

    def compare(self, bound, what):
        """Trained parameters: max abs error over max abs reference, over the whole flat vector; untrained ones: bit-equal to their start."""
        got = torch.cat([p.detach().cpu().double().reshape(-1) for (_, p), c in zip(self.named, self.copies) if p.requires_grad])
        ref = torch.cat([c.detach().reshape(-1) for (_, p), c in zip(self.named, self.copies) if p.requires_grad])
        _close(got.numpy(), ref.numpy(), bound, what)
        for (n, p), c in zip(self.named, self.copies):
            if not p.requires_grad:
                assert torch.equal(p.detach().cpu(), c.detach().float()), n

    def resync(self):
        """Start the next step from the engine's parameters (the comparison is per step: 'fp64 copies of the parameters before the step')."""
        with torch.no_grad():
            for (_, p), c in zip(self.named, self.copies):
                c.copy_(p.detach().cpu().double())


# ------------------------------------------------------------------------------------------------ 7. train_step
@pytest.mark.parametrize("dtype,backbone", [(torch.float32, dict()), (torch.bfloat16, dict()), (torch.float32, dict(norm_eval=True, norm_frozen=True)),
                                            (torch.float32, dict(frozen_stages=1))], ids=["f32", "bf16", "f32_norm_frozen_scattered", "f32_frozen_prefix"])
def test_train_steps_under_adamw_vs_torch_adamw_on_the_engines_gradients(dtype, backbone):
    """Three train_steps with paramwise options and max_norm = 5; after each, torch.optim.AdamW + clip_grad_norm_ on fp64 copies of the parameters before the
    step, fed with flat_grads, against the parameters after it.  The gradients are the engine's own, so the bound is the kernel's (the worst row of ADAMW_FP32
    x 10) for either storage type.  The moments are torch's fp64 ones carried across the steps.  norm_frozen gives scattered exclusions (the segment table's
    lr_mult < 0), frozen_stages = 1 a prefix that is cut off; the untrained parameters stay bit-equal."""
    m = _model(**backbone)
    opt, eng = _optimizer(m, dtype=dtype)
    assert eng.optimizer == "adamw" and eng.flat_var is not None
    twin = TorchTwin(m, eng, 5.0)
    for i in range(3):
        eng.train_step(*_batch(200 + i), lr=A.LR)
        torch.cuda.synchronize()
        twin.step(eng.flat_grads)
        twin.compare(bounds()[0], "step %d parameters" % i)
        twin.resync()
    assert eng.applied_steps() == 3 and eng.steps == 3
    assert eng._scattered_frozen == ("norm_frozen" in backbone)


# ------------------------------------------------------------------------------------------------ 8. accumulation
def test_accumulated_micro_steps_make_one_adamw_step_on_their_mean_gradient():
    m = _model()
    opt, eng = _optimizer(m)
    twin = TorchTwin(m, eng, 5.0)
    for group in range(2):
        for i in range(2):
            eng.accumulate_step(*_batch(210 + 2 * group + i))
            assert not bool(eng.flat_var.any()) or group == 1
        before = (eng.flat_mom.clone(), eng.flat_var.clone())
        eng.apply_accumulated(lr=A.LR)
        torch.cuda.synchronize()
        assert eng.applied_steps() == group + 1
        assert not torch.equal(before[0], eng.flat_mom) and not torch.equal(before[1], eng.flat_var)
        twin.step(eng.flat_acc, scale=0.5)
        twin.compare(bounds()[0], "optimizer step %d parameters" % group)
        twin.resync()


# ------------------------------------------------------------------------------------------------ 9. twin engines, with and without the average
def test_adamw_training_is_bit_identical_with_and_without_the_average():
    ma, mb = _model(), _model()
    (_, ea), (_, eb) = _optimizer(ma), _optimizer(mb)
    ea.enable_ema(momentum=0.25, warmup_steps=2)
    L = _lib()
    sep = ea.flat_ema.clone()          # the separate-launch average, moved by mvf_ema_update after each of B's steps
    from mvfnet_amd.ema import momentum_at
    for i in range(3):
        imgs, labels = _batch(220 + i)
        la, lb = ea.train_step(imgs.clone(), labels.clone(), lr=A.LR), eb.train_step(imgs.clone(), labels.clone(), lr=A.LR)
        for first, k, trained in _runs(mb, eb):
            if trained:
                L.check(L.lib.mvf_ema_update(P(sep[first:first + k]), P(eb.flat_params[first:first + k]), k, momentum_at(0.25, 2, i), None), "ema_update")
        torch.cuda.synchronize()
        assert torch.equal(la, lb) and torch.equal(ea.flat_params, eb.flat_params) and torch.equal(ea.flat_mom, eb.flat_mom) and torch.equal(ea.flat_var, eb.flat_var), i
        assert all(torch.equal(a, b) for a, b in zip(ma.buffers(), mb.buffers())), i
        assert torch.equal(_bits(ea.flat_ema), _bits(sep)), i
    assert eb.flat_ema is None and ea.ema_updates == 3 and not torch.equal(ea.flat_ema, ea.flat_params)


def _runs(m, eng):
    """(first, length, trained) per parameter in the flat layout."""
    return [(eng.grad_of(p).storage_offset(), p.numel(), p.requires_grad) for p in m.parameters()]


# ------------------------------------------------------------------------------------------------ 10. step guard
def test_a_poisoned_batch_is_skipped_under_adamw_and_the_run_continues():
    m = _model()
    opt, eng = _optimizer(m)
    eng.enable_ema(momentum=0.25)
    eng.enable_step_guard()

    def state():
        torch.cuda.synchronize()
        return [_bits(t.detach()).clone() if t.is_floating_point() else t.detach().clone() for t in [eng.flat_params, eng.flat_mom, eng.flat_var, eng.flat_ema] + list(m.buffers())]

    eng.train_step(*_batch(230), lr=A.LR)
    after1 = state()
    imgs, labels = _batch(231)
    imgs[0, 1, 2, 17, 29] = float("nan")
    eng.train_step(imgs, labels, lr=A.LR)
    assert all(torch.equal(a, b) for a, b in zip(state(), after1))          # parameters, both moments, the average, BatchNorm statistics, num_batches_tracked
    assert eng.guard_state() == dict(skipped_last=True, skipped=1, consecutive=1, steps=2) and eng.applied_steps() == 1
    loss = eng.train_step(*_batch(232), lr=A.LR)
    after3 = state()
    assert bool(torch.isfinite(loss).all()) and not torch.equal(after3[0], after1[0]) and all(bool(torch.isfinite(t.view(torch.float32)).all()) for t in after3[:4])
    assert eng.guard_state() == dict(skipped_last=False, skipped=1, consecutive=0, steps=3) and eng.applied_steps() == 2


# ------------------------------------------------------------------------------------------------ 11. checkpoint and resume
def test_checkpoint_resume_takes_the_next_adamw_step_bit_identically(tmp_path):
    from mvfnet_amd.runner import Runner
    m = _model()
    opt, eng = _optimizer(m)
    run = Runner(m, work_dir=str(tmp_path), max_norm=5.0, optimizer=opt, logger=None, warmup=None)
    for i in range(2):
        eng.train_step(*_batch(240 + i), lr=A.LR)
    path = run.save_checkpoint()
    m2 = _model()
    with torch.no_grad():
        for p in m2.parameters():
            p.add_(1.0)
    opt2, eng2 = _optimizer(m2)
    run2 = Runner(m2, work_dir=str(tmp_path), max_norm=5.0, optimizer=opt2, logger=None, warmup=None)
    run2.resume(path)
    assert eng2.applied_steps() == 2 and torch.equal(eng2.flat_mom, eng.flat_mom) and torch.equal(eng2.flat_var, eng.flat_var)
    imgs, labels = _batch(242)
    la, lb = eng.train_step(imgs.clone(), labels.clone(), lr=A.LR), eng2.train_step(imgs.clone(), labels.clone(), lr=A.LR)
    torch.cuda.synchronize()
    assert torch.equal(la, lb)
    for a, b in ((eng.flat_params, eng2.flat_params), (eng.flat_mom, eng2.flat_mom), (eng.flat_var, eng2.flat_var)):
        assert torch.equal(_bits(a), _bits(b))
    assert eng2.applied_steps() == 3
    # torch.optim.AdamW accepts the saved entry with the group structure it expects under paramwise options: one group per parameter
    saved = torch.load(path, map_location="cpu", weights_only=False)["optimizer"]
    params = [torch.nn.Parameter(torch.zeros(p.shape)) for p in m.parameters()]
    topt = torch.optim.AdamW([dict(params=[q]) for q in params], lr=A.LR)
    topt.load_state_dict(saved)
    assert len(saved["param_groups"]) == len(params) and saved["param_groups"][0]["decoupled_weight_decay"] is True
    ckpt_m, ckpt_v = {}, {}
    for q, p in zip(params, m.parameters()):
        st = topt.state[q]
        assert float(st["step"]) == 2.0 and st["step"].dtype == torch.float32
        ckpt_m[id(p)], ckpt_v[id(p)] = st["exp_avg"], st["exp_avg_sq"]
    assert eng2.applied_steps() == 3          # (read above; the saved moments are those after two steps: compare with a third engine loaded from the file)
    m3 = _model()
    opt3, eng3 = _optimizer(m3)
    opt3.load_state_dict(saved)
    for p3, p in zip(m3.parameters(), m.parameters()):
        first = eng3.grad_of(p3).storage_offset()
        assert torch.equal(eng3.flat_mom[first:first + p.numel()].view(p.shape).cpu(), ckpt_m[id(p)])
        assert torch.equal(eng3.flat_var[first:first + p.numel()].view(p.shape).cpu(), ckpt_v[id(p)])
    assert eng3.applied_steps() == 2
    bias = [g for g, (n, _) in zip(saved["param_groups"], m.named_parameters()) if n.endswith("new_fc.bias")][0]
    assert bias["lr"] == A.LR * 2.0 and bias["weight_decay"] == 0.0 and bias["initial_lr"] == A.LR * 2.0


# ------------------------------------------------------------------------------------------------ 12. plain SGD engine is unchanged
def test_a_plain_sgd_engine_makes_no_adamw_call_and_allocates_no_second_moment():
    m = _model()
    eng = m.train_engine()
    with library_names(eng) as names:
        eng.train_step(*_batch(250))
        eng.accumulate_step(*_batch(251))
        eng.apply_accumulated()
    torch.cuda.synchronize()
    assert eng.optimizer == "sgd" and eng.flat_var is None and eng._adam is None
    assert not [n for n in names if "adamw" in n]
    assert [n for n in names if "sgd" in n and "workspace" not in n] == ["mvf_sgd_nesterov_step"] * 2
    # ... and the switch is refused once the engine has stepped
    with pytest.raises(RuntimeError):
        eng.optimizer = "adamw"
    # selected before the first step, the same paths reach mvf_adamw_step
    m2 = _model()
    eng2 = m2.train_engine()
    eng2.optimizer = "adam"
    with library_names(eng2) as names:
        eng2.train_step(*_batch(250))
    torch.cuda.synchronize()
    assert [n for n in names if ("sgd" in n or "adamw" in n) and "workspace" not in n] == ["mvf_adamw_step"]
    assert eng2.optimizer == "adam" and eng2.flat_var is not None and eng2.applied_steps() == 1


# ------------------------------------------------------------------------------------------------ the config route: train_network with AdamW + a cosine schedule
def test_train_network_runs_an_adamw_config_with_a_cosine_schedule_and_resumes(tmp_path):
    """An mmaction-style fine-tuning config through train_network: optimizer type AdamW with paramwise options, lr_config policy 'cosine' by iteration; the
    logged rates are the closed form over max_iters = total_epochs x len(loader), which the runner learns in run(); resume_from continues the count."""
    import math
    import re
    from mvfnet_amd.runner import Config, train_network
    batches = [dict(img_group=torch.from_numpy(synth.synth_clip_batch(2, 4, 64, 64, seed=260 + i)), label=torch.from_numpy(synth.synth_labels(2, seed=260 + i)))
               for i in range(3)]
    cfg = Config(optimizer=dict(OPT), optimizer_config=dict(grad_clip=dict(max_norm=5.0, norm_type=2)),
                 lr_config=dict(policy="cosine", min_lr_ratio=0.1, by_epoch=False, warmup=None),
                 checkpoint_config=dict(interval=2), log_config=dict(interval=1), total_epochs=2, work_dir=str(tmp_path),
                 data=dict(videos_per_gpu=2, workers_per_gpu=0), resume_from=None, load_from=None)
    logs = []
    m = _model()
    run = train_network(m, batches, cfg, logger=logs.append)
    eng = run.engine
    assert run.epoch == 2 and run.iter == 6 and run.max_epochs == 2 and run.max_iters == 6
    assert eng.optimizer == "adamw" and eng.param_options and eng.max_norm == 5.0 and eng.applied_steps() == 6
    want = [1e-4 + 0.5 * 9e-4 * (1 + math.cos(math.pi * k / 6)) for k in range(6)]
    got = [float(re.search(r" lr ([0-9.]+) ", line).group(1)) for line in logs]
    assert len(got) == 6 and all(abs(a - b) <= 0.5e-5 + 1e-12 for a, b in zip(got, want)), (got, want)
    assert abs(run.current_lr() - 1e-4) < 1e-15                     # progress = max_progress: the target
    ck = torch.load(str(tmp_path / "latest.pth"), weights_only=False)
    assert set(ck["optimizer"]["state"][0]) == {"step", "exp_avg", "exp_avg_sq"} and float(ck["optimizer"]["state"][0]["step"]) == 6.0
    m2 = _model()
    run2 = train_network(m2, batches, Config(dict(cfg, resume_from=str(tmp_path / "latest.pth"), total_epochs=3)), logger=logs.append)
    assert run2.epoch == 3 and run2.iter == 9 and run2.max_iters == 9 and run2.engine.applied_steps() == 9
    assert bool(torch.isfinite(run2.engine.flat_params).all())
    with pytest.raises(NotImplementedError):
        train_network(m2, batches, Config(dict(cfg, lr_config=dict(policy="cyclic"))), logger=logs.append)          # refused before anything is built
