"""The fused clip + LAMB step (mvf_lamb_step; csrc/optim.hip lamb_moments / lamb_ratio / lamb_apply kernels) through the C ABI against the fp64 restatement in
lamb_numpy.py, and the engine / runner / checkpoint layers above it (TrainEngine(optimizer='lamb'), build_optimizer(type='Lamb'), trust_ratios()).

Settings: lr 5e-3, betas (0.9, 0.999), eps 1e-6, weight_decay 0.02, max_norm 40 (lamb_numpy's constants).  Gradients follow test_adamw_gpu: the scaled norm is
100, 10, 100 over three steps against max_norm 40, 40, 0, so only step 0 clips; moments and the device step counter carry over.

Bounds.  Norm and clip coefficient: the SGD test's (NORM_BOUND = 1e-5; |coef - ref| <= 2e-5 ref).  params / exp_avg / exp_avg_sq / ratios, each as max abs error
over max abs reference: 10 x the figure the same update in fp32 numpy (lamb_numpy.lamb_ref(ft=np.float32), every scalar rounded once from double, the norms
fp64 sums) reaches against fp64 for that case -- LAMB_FP32 below, measured on the CPU with `python tests/lamb_numpy.py`.  The margin is test_adamw_gpu's: it
covers fma contraction and the order of the reductions, and nothing else should differ.  A case the table does not list (the exact cases, the closed form, the
guard's) takes the table's row of the same n / grad_scale, else the worst row.  Where a ratio is exactly 1 or 0 by the rules it is compared exactly."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lamb_numpy as A  # noqa: E402
from helpers import library_names  # noqa: E402
from mvfnet_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu

P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
NORM_BOUND = 1e-5
SEG_DTYPE = np.dtype([("first", "<i8"), ("lr_mult", "<f4"), ("decay_mult", "<f4")])      # mvf_sgd_segment_t
SEG_N, SEGMENTS = A.SEG_N, A.SEGMENTS
ONE = ((0, 1.0, 1.0),)
# (n | name, grad_scale) -> worst fp32-numpy-vs-fp64 figure over the three steps: (params, exp_avg, exp_avg_sq, ratios)
LAMB_FP32 = {
    (1, 1.0): (3.395e-08, 4.087e-08, 3.723e-08, 6.070e-08), (1, 0.125): (2.574e-08, 4.087e-08, 3.723e-08, 1.053e-07),
    (255, 1.0): (6.463e-08, 7.671e-08, 1.158e-07, 7.506e-08), (255, 0.125): (7.899e-08, 9.164e-08, 1.602e-07, 6.208e-08),
    (257, 1.0): (7.515e-08, 7.851e-08, 1.867e-07, 8.839e-08), (257, 0.125): (1.155e-07, 8.807e-08, 1.606e-07, 7.191e-08),
    (5000, 1.0): (8.622e-08, 1.040e-07, 1.757e-07, 1.067e-07), (5000, 0.125): (7.836e-08, 9.057e-08, 1.714e-07, 9.632e-08),
    (262147, 1.0): (9.349e-08, 1.027e-07, 2.095e-07, 7.641e-08), (262147, 0.125): (8.213e-08, 1.000e-07, 2.290e-07, 5.088e-08),
    ("table", 0.125): (1.195e-07, 1.094e-07, 2.619e-07, 7.019e-08), ("table_always_adapt", 0.125): (1.195e-07, 1.094e-07, 2.619e-07, 7.292e-08),
}
WORST = tuple(max(v[k] for v in LAMB_FP32.values()) for k in range(4))


def bounds(n=None, gs=None):
    return tuple(10.0 * f for f in LAMB_FP32.get((n, gs), WORST))


def _lib():
    from mvfnet_amd import _lib as L
    return L


def _bits(t):
    return t.view(torch.int32)


class Ops(object):
    """Device operands of one mvf_lamb_step call sequence: views at `offset` into buffers filled with a guard value."""
    FILL = -123.25

    def __init__(self, n, p0, offset=0, segs=ONE, ema=False, guard=False, m0=None, v0=None, **hyper):
        self.L = _lib()
        self.n, self.offset, self.segs = n, offset, tuple(segs)
        self.full = {}
        zeros = np.zeros(n)
        for name, v in (("p", p0), ("g", zeros), ("m", zeros if m0 is None else m0), ("v", zeros if v0 is None else v0)) + ((("e", p0),) if ema else ()):
            full = torch.full((n + 2 * offset,), self.FILL, device="cuda")
            full[offset:offset + n] = torch.from_numpy(np.asarray(v, dtype=np.float32)).cuda()
            self.full[name] = full
        view = lambda k: self.full[k][offset:offset + n] if k in self.full else None  # noqa: E731
        self.p, self.g, self.m, self.v, self.e = (view(k) for k in "pgmve")
        self.nseg = len(self.segs)
        self.norm = torch.full((2,), float("nan"), device="cuda")
        self.ratio = torch.full((self.nseg + 2,), self.FILL, device="cuda")          # (the two words behind the nseg ratios must keep the fill value)
        self.ws = torch.empty(self.L.lib.mvf_lamb_workspace_bytes(n, self.nseg), dtype=torch.uint8, device="cuda")
        self.count = torch.zeros(1, dtype=torch.int64, device="cuda")
        self.guard = torch.zeros(4, dtype=torch.int32, device="cuda") if guard else None
        self.tab = torch.from_numpy(np.array(list(self.segs), dtype=SEG_DTYPE).view(np.uint8)).cuda()
        hp = dict(lr=A.LR, betas=A.BETAS, eps=A.EPS, wd=A.WD, trust_clip=0, always_adapt=0)
        hp.update(hyper)
        self.hp = hp
        self.hyper = self.L.LambHyper(hp["lr"], hp["betas"][0], hp["betas"][1], hp["eps"], hp["wd"], hp["trust_clip"], hp["always_adapt"])

    def call(self, gs, max_norm, ema_m=0.25, use_ema=True, **over):
        """The raw status code of one call; `over` replaces arguments by name (the refusal test)."""
        e = self.e if use_ema else None
        a = dict(params=P(self.p), grads=P(self.g), exp_avg=P(self.m), exp_avg_sq=P(self.v), n=self.n, gs=gs, max_norm=max_norm, hyper=C.byref(self.hyper),
                 segments=P(self.tab), nseg=self.nseg, ema=P(e), ema_m=ema_m, guard=P(self.guard), count=P(self.count), norm=P(self.norm), ratio=P(self.ratio),
                 ws=P(self.ws), ws_bytes=self.ws.numel())
        a.update(over)
        return self.L.lib.mvf_lamb_step(a["params"], a["grads"], a["exp_avg"], a["exp_avg_sq"], a["n"], a["gs"], a["max_norm"], a["hyper"], a["segments"], a["nseg"],
                                        a["ema"], a["ema_m"], a["guard"], a["count"], a["norm"], a["ratio"], a["ws"], a["ws_bytes"], None)

    def step(self, g, gs, max_norm, ema_m=0.25, use_ema=True):
        self.g.copy_(torch.from_numpy(np.asarray(g, dtype=np.float32)).cuda())
        self.L.check(self.call(gs, max_norm, ema_m, use_ema), "lamb_step")
        torch.cuda.synchronize()

    def ratios(self):
        assert bool((self.ratio[self.nseg:] == self.FILL).all())
        return self.ratio[:self.nseg].cpu().numpy()

    def untouched_outside(self):
        o, n = self.offset, self.n
        return all(bool((f[:o] == self.FILL).all()) and bool((f[o + n:] == self.FILL).all()) for f in self.full.values())

    def state(self):
        torch.cuda.synchronize()
        return [_bits(t).clone() for t in (self.p, self.m, self.v, self.e, self.norm, self.ratio) if t is not None]


def _close(got, ref, bound, what):
    e = A.rel(got, ref)
    print("%s: %.3e (bound %.3e)" % (what, e, bound))
    assert np.isfinite(np.asarray(got)).all() and e < bound, (what, e, bound)


def _check_ratios(got, ref, segs, hp, bound, what):
    """Exact where the rules fix the ratio (excluded: 0; no decay and no always_adapt: 1), bounded elsewhere."""
    free = []
    for k, s in enumerate(segs):
        if s[1] < 0:
            assert got[k] == 0.0 and ref[k] == 0.0, (what, k, got[k])
        elif hp["wd"] * s[2] == 0 and not hp["always_adapt"]:
            assert got[k] == 1.0 and ref[k] == 1.0, (what, k, got[k])
        else:
            free.append(k)
    _close(got[free], ref[free], bound, what)
    if hp["trust_clip"]:
        assert (got <= 1.0).all(), what


def run_steps(n, gs, segs=None, offset=0, excluded_fill=None, key=None, **hyper):
    """Three steps against the fp64 reference, which keeps its own fp64 state; returns the operands."""
    p0, m0, v0, grads = A.case_inputs(n, gs, segs)
    tab = segs if segs is not None else ONE
    excl = np.repeat(np.array([s[1] < 0 for s in tab]), A.seg_lens(n, tab))
    bp, bm, bv, br = bounds(key if key is not None else n, gs)
    ops = Ops(n, p0, offset=offset, segs=tab, **hyper)
    kw = {k: v for k, v in ops.hp.items() if k != "betas"}
    p_ref, m_ref, v_ref = p0.astype(np.float64), m0.astype(np.float64), v0.astype(np.float64)
    p_start = ops.p.clone()
    for step, g in enumerate(grads):
        if excluded_fill is not None:           # the excluded elements' gradient stays outside the norm, whatever it holds
            g = g.copy()
            g[excl] = np.resize(np.array(excluded_fill, dtype=np.float32), int(excl.sum()))
        max_norm = 0.0 if step == 2 else A.MAX_NORM
        p_ref, m_ref, v_ref, r_ref, n_ref, c_ref = A.lamb_ref(p_ref, m_ref, v_ref, g, gs, max_norm, step + 1, tab, betas=ops.hp["betas"], **kw)
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
        _check_ratios(ops.ratios(), r_ref, tab, ops.hp, br, "step %d ratios" % step)
        assert int(ops.count) == step + 1
        if excl.any():                          # excluded segments: parameters and both moments bit-unchanged
            e = torch.from_numpy(excl).cuda()
            assert torch.equal(_bits(ops.p[e]), _bits(p_start[e])) and not bool(_bits(ops.m[e]).any()) and not bool(_bits(ops.v[e]).any()), step
        if offset:
            assert ops.untouched_outside(), step
    return ops


# ------------------------------------------------------------------------------------------------ 1. flat sizes against fp64
@pytest.mark.parametrize("gs", [1.0, 0.125])
@pytest.mark.parametrize("n", [1, 255, 257, 5000, 262144 + 3], ids=lambda n: "n%d" % n)
def test_lamb_step_vs_fp64(n, gs):
    """One segment, three steps (clipping / not clipping / max_norm = 0).  1, 255 and 257 are the one-workgroup edges (below 8 elements everything is ragged),
    5000 is two chunks with a ragged tail, 262147 is 65 chunks: the ratio wavefront's loop over the slots iterates.  *applied_steps reads 1, 2, 3."""
    run_steps(n, gs)


# ------------------------------------------------------------------------------------------------ 2. the per-parameter table
@pytest.mark.parametrize("always_adapt", [0, 1])
def test_lamb_step_table_vs_fp64(always_adapt):
    """Nine segments over n = 262147: boundaries at odd offsets (7, 257, 1001), a one-element segment, two excluded segments whose gradient is NaN / inf (it
    stays outside the norm), decay_mult = 0 segments (ratio exactly 1 unless always_adapt), a segment over 47 chunks, six segments inside chunk 0."""
    run_steps(SEG_N, 0.125, segs=SEGMENTS, excluded_fill=(float("nan"), float("inf"), -float("inf")), always_adapt=always_adapt,
              key="table_always_adapt" if always_adapt else "table")


@pytest.mark.parametrize("offset", [1, 3])
def test_lamb_step_table_on_offset_views_leaves_the_neighbours_alone(offset):
    """The same table with every operand view 4 / 12 bytes past a 16-byte boundary (the dwordx4 body starts behind a ragged head in every intersection) inside
    fill-valued buffers: same bounds, nothing outside the views changes, excluded segments keep their bits."""
    run_steps(SEG_N, 0.125, segs=SEGMENTS, offset=offset, excluded_fill=(float("nan"),), key="table")


def test_the_table_norm_equals_the_adam_segment_forms_bit_for_bit():
    """The clip norm over the per-parameter table comes from a kernel of its own (a binary search per element is too slow for ~200 segments); its partial sums
    are those of the segment form of mvf_adamw_step: norm_out bit-equal on the same gradient, NaN in the excluded segments included."""
    import adamw_numpy as W
    L = _lib()
    p0, _, _, grads = A.case_inputs(SEG_N, 0.125, SEGMENTS)
    excl = np.repeat(np.array([s[1] < 0 for s in SEGMENTS]), A.seg_lens(SEG_N, SEGMENTS))
    g = grads[1].copy()
    g[excl] = np.nan
    ops = Ops(SEG_N, p0, segs=SEGMENTS)
    ops.step(g, 0.125, A.MAX_NORM)
    dev = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32)).cuda()  # noqa: E731
    p, gg, m, v = dev(p0), dev(g), torch.zeros(SEG_N, device="cuda"), torch.zeros(SEG_N, device="cuda")
    norm, count = torch.zeros(2, device="cuda"), torch.zeros(1, dtype=torch.int64, device="cuda")
    ws = torch.empty(L.lib.mvf_adamw_workspace_bytes(SEG_N), dtype=torch.uint8, device="cuda")
    h = L.AdamwHyper(W.LR, W.BETAS[0], W.BETAS[1], W.EPS, W.WD, 1)
    L.check(L.lib.mvf_adamw_step(P(p), P(gg), P(m), P(v), SEG_N, 0.125, A.MAX_NORM, C.byref(h), P(ops.tab), ops.nseg, None, 0.0, None, P(count), P(norm), P(ws),
                                 ws.numel(), None), "adamw_step")
    torch.cuda.synchronize()
    assert bool(torch.isfinite(norm).all()) and torch.equal(_bits(norm), _bits(ops.norm))


# ------------------------------------------------------------------------------------------------ 3. exact cases
EXACT_SEGS = ((0, 1.0, 1.0), (1000, 1.0, 1.0), (3000, 1.0, 1.0))


def _exact_inputs():
    p0, m0, v0, grads = A.case_inputs(5000, 1.0, EXACT_SEGS)
    p0 = p0.copy()
    p0[:1000] = 0.0            # wn = 0 under wd != 0: ratio exactly 1
    p0[1000:3000] *= 3.0       # |u| ~ 1 in the first step, so wn / un ~ 3: a ratio trust_clip has to cap
    return p0, grads[0]


@pytest.mark.parametrize("trust_clip", [0, 1])
def test_zero_parameters_give_ratio_one_and_trust_clip_caps_a_ratio_above_one(trust_clip):
    p0, g = _exact_inputs()
    ops = Ops(5000, p0, segs=EXACT_SEGS, trust_clip=trust_clip)
    ops.step(g, 1.0, A.MAX_NORM)
    z = np.zeros(5000)
    free = A.lamb_ref(p0.astype(np.float64), z, z, g, 1.0, A.MAX_NORM, 1, EXACT_SEGS)
    ref = A.lamb_ref(p0.astype(np.float64), z, z, g, 1.0, A.MAX_NORM, 1, EXACT_SEGS, trust_clip=trust_clip)
    assert free[3][0] == 1.0 and free[3][1] > 2.0 and free[3][2] < 2.0          # what the reference shows without the cap
    got = ops.ratios()
    bp, _, _, br = bounds(5000, 1.0)
    assert got[0] == 1.0
    if trust_clip:
        assert got[1] == 1.0 and ref[3][1] == 1.0 and (got <= 1.0).all()
    else:
        assert got[1] > 2.0
    _close(got, ref[3], br, "ratios")
    _close(ops.p.cpu().numpy(), ref[0], bp, "params")


def test_zero_update_gives_ratio_one_and_leaves_the_parameters_bit_equal():
    """always_adapt = 1, weight_decay = 0, zero gradient and zero moments: u = 0, un = 0, ratio exactly 1, p' = p - step * 0 = p."""
    p0, _, _, _ = A.case_inputs(5000, 1.0, EXACT_SEGS)
    ops = Ops(5000, p0, segs=EXACT_SEGS, wd=0.0, always_adapt=1)
    before = _bits(ops.p).clone()
    ops.step(np.zeros(5000), 1.0, A.MAX_NORM)
    assert (ops.ratios() == 1.0).all() and torch.equal(_bits(ops.p), before) and int(ops.count) == 1
    assert not bool(_bits(ops.m).any()) and not bool(_bits(ops.v).any()) and float(ops.norm[0]) == 0.0 and float(ops.norm[1]) == 1.0


# ------------------------------------------------------------------------------------------------ 4. closed form
def test_first_step_with_unit_gradients_matches_the_closed_form():
    """First step, wd = 0, always_adapt, |g| = 1, no clip: m' / (1 - b1) = g and v' / (1 - b2) = 1 up to rounding, so u = sign(g) / (1 + eps),
    r_k = wn_k / (sqrt(n_k) / (1 + eps)) and p' = p - lr_k r_k sign(g) / (1 + eps)."""
    n, segs = 5000, ((0, 1.0, 1.0), (7, 2.0, 0.0), (1001, 1.0, 1.0))
    p0, _, _, grads = A.case_inputs(n, 1.0, segs)
    g = np.sign(grads[0]).astype(np.float32)
    ops = Ops(n, p0, segs=segs, wd=0.0, always_adapt=1)
    ops.step(g, 1.0, 0.0)
    u = 1.0 / (1.0 + A.EPS)
    firsts = [s[0] for s in segs] + [n]
    r = np.array([np.sqrt((p0[a:b].astype(np.float64) ** 2).sum()) / (np.sqrt(b - a) * u) for a, b in zip(firsts[:-1], firsts[1:])])
    step = np.repeat(A.LR * np.array([s[1] for s in segs]) * r, A.seg_lens(n, segs))
    bp, _, _, br = bounds(n, 1.0)
    _close(ops.ratios(), r, br, "ratios")
    _close(ops.p.cpu().numpy(), p0.astype(np.float64) - step * g.astype(np.float64) * u, bp, "params")
    assert abs(float(ops.norm[0]) - np.sqrt(n)) < NORM_BOUND * np.sqrt(n) and float(ops.norm[1]) == 1.0


# ------------------------------------------------------------------------------------------------ 5. average
@pytest.mark.parametrize("n", [257, SEG_N], ids=lambda n: "n%d" % n)
def test_lamb_step_with_the_average_equals_the_plain_step_then_ema_update(n):
    """ema != NULL against the plain step followed by mvf_ema_update per trained segment: params, exp_avg, exp_avg_sq, ema, norm_out and ratio_out bit-equal
    over three steps with momenta 1, 0.5, 2e-4."""
    segs = tuple(s for s in SEGMENTS if s[0] < n)
    p0, _, _, grads = A.case_inputs(n, 0.125, segs)
    fused, plain = Ops(n, p0, segs=segs, ema=True), Ops(n, p0, segs=segs, ema=True)
    L = fused.L
    firsts = [s[0] for s in segs] + [n]
    for step, (g, mom) in enumerate(zip(grads, (1.0, 0.5, 2e-4))):
        fused.step(g, 0.125, A.MAX_NORM, ema_m=mom)
        plain.step(g, 0.125, A.MAX_NORM, use_ema=False)
        for k, s in enumerate(segs):
            if s[1] >= 0:
                a, b = firsts[k], firsts[k + 1]
                L.check(L.lib.mvf_ema_update(P(plain.e[a:b]), P(plain.p[a:b]), b - a, mom, None), "ema_update")
        assert all(torch.equal(x, y) for x, y in zip(fused.state(), plain.state())), step
        assert int(fused.count) == int(plain.count) == step + 1
    assert not torch.equal(fused.e, fused.p)


# ------------------------------------------------------------------------------------------------ 6. guard
def test_lamb_guard_skips_the_step_and_the_step_count():
    """Good, bad, good on the table (n = 262147): a NaN in one trained gradient leaves params, both moments, the average, the ratios and *applied_steps
    bit-unchanged with guard = {1, 1, 1, 2}; after the third step everything matches an fp64 reference that never saw the bad step and bias-corrects with
    t = 2.  Only good steps: bit-equal to guard == NULL."""
    n, gs, segs = SEG_N, 0.125, SEGMENTS
    p0, m0, v0, grads = A.case_inputs(n, gs, segs)
    t = np.repeat(np.array([s[1] >= 0 for s in segs]), A.seg_lens(n, segs))
    bp, bm, bv, br = bounds("table", gs)
    ops = Ops(n, p0, segs=segs, ema=True, guard=True)
    ref = [p0.astype(np.float64), m0.astype(np.float64), v0.astype(np.float64)]
    ops.step(grads[0], gs, A.MAX_NORM)
    ref = list(A.lamb_ref(ref[0], ref[1], ref[2], grads[0], gs, A.MAX_NORM, 1, segs)[:3])
    after1 = ops.state()
    assert ops.guard.tolist() == [0, 0, 0, 1] and int(ops.count) == 1
    g_bad = grads[1].copy()
    g_bad[70000 + 12345] = float("nan")
    ops.step(g_bad, gs, A.MAX_NORM)
    assert not bool(torch.isfinite(ops.norm[0]))
    now = ops.state()
    assert all(torch.equal(x, y) for x, y in zip(now[:4] + now[5:], after1[:4] + after1[5:]))          # (all but norm_out, which holds the honest NaN)
    assert ops.guard.tolist() == [1, 1, 1, 2] and int(ops.count) == 1
    ops.step(grads[2], gs, 0.0)
    out = A.lamb_ref(ref[0], ref[1], ref[2], grads[2], gs, 0.0, 2, segs)
    assert ops.guard.tolist() == [0, 1, 0, 3] and int(ops.count) == 2
    _close(ops.p.cpu().numpy()[t], out[0][t], bp, "params")
    _close(ops.m.cpu().numpy()[t], out[1][t], bm, "exp_avg")
    _close(ops.v.cpu().numpy()[t], out[2][t], bv, "exp_avg_sq")
    _check_ratios(ops.ratios(), out[3], segs, ops.hp, br, "ratios")
    wrong = A.lamb_ref(ref[0], ref[1], ref[2], grads[2], gs, 0.0, 3, segs)          # the wrong count would show
    assert A.rel(wrong[0][t], out[0][t]) > 10 * bp
    a, b = Ops(n, p0, segs=segs, ema=True, guard=True), Ops(n, p0, segs=segs, ema=True, guard=False)
    for step, g in enumerate(grads):
        a.step(g, gs, A.MAX_NORM)
        b.step(g, gs, A.MAX_NORM)
        assert all(torch.equal(x, y) for x, y in zip(a.state(), b.state())), step
    assert a.guard.tolist() == [0, 0, 0, 3] and int(a.count) == int(b.count) == 3


# ------------------------------------------------------------------------------------------------ 7. repeatability
def test_two_runs_from_the_same_state_are_bit_identical():
    p0, _, _, grads = A.case_inputs(SEG_N, 0.125, SEGMENTS)
    a, b = Ops(SEG_N, p0, segs=SEGMENTS, ema=True), Ops(SEG_N, p0, segs=SEGMENTS, ema=True)
    for step, g in enumerate(grads):
        a.step(g, 0.125, A.MAX_NORM)
        b.step(g, 0.125, A.MAX_NORM)
        assert all(torch.equal(x, y) for x, y in zip(a.state(), b.state())), step


# ------------------------------------------------------------------------------------------------ 8. refusals
def test_refused_calls_launch_nothing():
    """Every MVF_EINVAL / MVF_EWS refusal returns its code and leaves params, both moments, the average, norm_out, ratio_out, the guard and the counter alone."""
    n = 5000
    p0, _, _, grads = A.case_inputs(n, 1.0, EXACT_SEGS)
    ops = Ops(n, p0, segs=EXACT_SEGS, ema=True, guard=True)
    ops.g.copy_(torch.from_numpy(grads[0]).cuda())
    before = ops.state()
    L = ops.L
    EINVAL, EWS = -1, -3
    H = lambda **kw: C.byref(L.LambHyper(*[kw.get(k, d) for k, d in (("lr", A.LR), ("b1", 0.9), ("b2", 0.999), ("eps", A.EPS), ("wd", A.WD), ("tc", 0), ("aa", 0))]))  # noqa: E731
    off = lambda t, k: C.c_void_p(t.data_ptr() + k)  # noqa: E731
    cases = [(EINVAL, dict(params=None)), (EINVAL, dict(grads=None)), (EINVAL, dict(exp_avg=None)), (EINVAL, dict(exp_avg_sq=None)), (EINVAL, dict(norm=None)),
             (EINVAL, dict(ratio=None)), (EINVAL, dict(hyper=None)), (EINVAL, dict(count=None)), (EINVAL, dict(segments=None)), (EINVAL, dict(n=0)),
             (EINVAL, dict(nseg=0)), (EINVAL, dict(n=2, nseg=3)),
             (EINVAL, dict(params=off(ops.p, 2))), (EINVAL, dict(ratio=off(ops.ratio, 1))), (EINVAL, dict(count=off(ops.g, 4))), (EINVAL, dict(ws=off(ops.ws, 4))),
             (EINVAL, dict(segments=off(ops.tab, 4))),
             (EINVAL, dict(exp_avg=P(ops.p))), (EINVAL, dict(ratio=P(ops.norm))), (EINVAL, dict(ratio=P(ops.m))), (EINVAL, dict(ema=P(ops.v))),
             (EINVAL, dict(ratio=P(ops.ws))), (EINVAL, dict(guard=P(ops.ratio))),
             (EINVAL, dict(hyper=H(b1=1.0))), (EINVAL, dict(hyper=H(b2=-0.1))), (EINVAL, dict(hyper=H(eps=0.0))), (EINVAL, dict(hyper=H(lr=-1.0))),
             (EINVAL, dict(hyper=H(wd=-1.0))), (EINVAL, dict(hyper=H(lr=float("nan")))), (EINVAL, dict(hyper=H(tc=2))), (EINVAL, dict(hyper=H(aa=-1))),
             (EINVAL, dict(ema_m=1.5)), (EINVAL, dict(ema_m=float("nan"))),
             (EWS, dict(ws=None)), (EWS, dict(ws_bytes=ops.ws.numel() - 1))]
    for want, over in cases:
        assert ops.call(1.0, A.MAX_NORM, **over) == want, (over, L.lib.mvf_last_error())
        assert b"lamb_step" in L.lib.mvf_last_error()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(ops.state(), before))
    assert int(ops.count) == 0 and ops.guard.tolist() == [0, 0, 0, 0] and bool(torch.isnan(ops.norm).all())
    assert L.lib.mvf_lamb_workspace_bytes(0, 1) == 0 and L.lib.mvf_lamb_workspace_bytes(2, 3) == 0
    ops.step(grads[0], 1.0, A.MAX_NORM)          # ... and the same operands are accepted as they are
    assert int(ops.count) == 1


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


OPT = dict(type="Lamb", lr=A.LR, betas=A.BETAS, eps=A.EPS, weight_decay=A.WD, paramwise_options=dict(bias_lr_mult=2.0, bias_decay_mult=0.0, norm_decay_mult=0.0))


def _optimizer(m, max_norm=5.0):
    from mvfnet_amd.runner import EngineLamb, build_optimizer
    opt = build_optimizer(m, OPT)
    assert type(opt) is EngineLamb
    opt.engine.max_norm = max_norm
    return opt, opt.engine


def test_engine_trains_under_lamb_and_resumes_bit_identically():
    """build_optimizer(type='Lamb') with norm_decay_mult = 0: two train_steps; trust_ratios() has one finite entry per parameter, exactly 1 for every BatchNorm
    parameter (and the head's bias: bias_decay_mult = 0), positive and not all 1 elsewhere.  The state dict of the second step, loaded into a second engine
    whose parameters were copied over, gives a bit-identical third step."""
    import re
    m = _model()
    opt, eng = _optimizer(m)
    assert eng.optimizer == "lamb" and eng.flat_var is not None and eng.eps == A.EPS and eng.trust_ratios() == {}
    before = eng.flat_params.clone()
    for i in range(2):
        eng.train_step(*_batch(300 + i), lr=A.LR)
    ratios = eng.trust_ratios()
    names = [n for n, _ in m.named_parameters()]
    assert sorted(ratios) == sorted(names) and all(np.isfinite(v) and v > 0 for v in ratios.values())
    no_decay = [n for n in names if re.search(r"(bn|gn)(\d+)?.(weight|bias)", n) or n.endswith(".bias")]
    assert len(no_decay) > 50 and all(ratios[n] == 1.0 for n in no_decay)
    assert sum(1 for n in names if n not in no_decay and ratios[n] != 1.0) > 30
    assert eng.applied_steps() == 2 and eng.steps == 2 and not torch.equal(before, eng.flat_params) and bool(torch.isfinite(eng.flat_params).all())
    sd = opt.state_dict()
    assert sd["param_groups"][0]["lamb"] is True and set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"} and float(sd["state"][0]["step"]) == 2.0
    m2 = _model()
    opt2, eng2 = _optimizer(m2)
    m2.load_state_dict(m.state_dict())
    opt2.load_state_dict(sd)
    assert eng2.applied_steps() == 2 and torch.equal(eng2.flat_mom, eng.flat_mom) and torch.equal(eng2.flat_var, eng.flat_var)
    assert torch.equal(_bits(eng2.flat_params), _bits(eng.flat_params))
    imgs, labels = _batch(302)
    la, lb = eng.train_step(imgs.clone(), labels.clone(), lr=A.LR), eng2.train_step(imgs.clone(), labels.clone(), lr=A.LR)
    torch.cuda.synchronize()
    assert torch.equal(la, lb)
    for a, b in ((eng.flat_params, eng2.flat_params), (eng.flat_mom, eng2.flat_mom), (eng.flat_var, eng2.flat_var)):
        assert torch.equal(_bits(a), _bits(b))
    assert eng2.applied_steps() == 3 and eng.trust_ratios() == eng2.trust_ratios()
    # a state another optimizer kind wrote is refused
    from mvfnet_amd.checkpoint import adamw_state_dict
    with pytest.raises(ValueError):
        opt2.load_state_dict(adamw_state_dict(2, [None] * len(names), [None] * len(names), A.LR))


def test_an_engine_left_on_sgd_has_no_lamb_buffers_and_makes_no_lamb_call():
    m = _model()
    eng = m.train_engine()
    with library_names(eng) as names:
        eng.train_step(*_batch(310))
    torch.cuda.synchronize()
    assert eng.optimizer == "sgd" and eng.flat_var is None and eng._adam is None and eng.trust_clip is None
    assert not [n for n in names if "lamb" in n]
    with pytest.raises(RuntimeError):
        eng.trust_ratios()
    with pytest.raises(RuntimeError):
        eng.optimizer = "lamb"          # refused once the engine has stepped
    # selected before the first step, the same path reaches mvf_lamb_step
    m2 = _model()
    eng2 = m2.train_engine()
    eng2.set_optimizer("lamb", trust_clip=True)
    with library_names(eng2) as names:
        eng2.train_step(*_batch(310))
    torch.cuda.synchronize()
    assert [n for n in names if ("sgd" in n or "adamw" in n or "lamb" in n) and "workspace" not in n] == ["mvf_lamb_step"]
    assert eng2.optimizer == "lamb" and eng2.eps == 1e-6 and eng2.trust_clip is True and eng2.applied_steps() == 1
    assert all(0 < v <= 1.0 for v in eng2.trust_ratios().values())
