"""CPU: the numpy restatement of the LAMB step (lamb_numpy.lamb_ref, the text of include/mvfnet_hip.h) against an independent plain-torch restatement of timm's
Lamb.step written per tensor with torch.norm; the checkpoint helpers; build_optimizer's refusals; the argument checks of mvf_lamb_step (no launch)."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lamb_numpy as A  # noqa: E402


def timm_lamb_step(params, grads, state, t, lr, betas, eps, wd, max_grad_norm, trust_clip, always_adapt, clip_eps=0.0):
    """timm/optim/lamb.py Lamb.step for one param group (bias_correction and grad_averaging on), fp64 tensors, one tensor at a time.  clip_eps = 0 is timm's
    clip, grad / max(1, norm / max_grad_norm); clip_eps = 1e-6 is clip_grad_norm_'s, which the project puts in front: grad / max(1, (norm + 1e-6) / max_norm)."""
    one = torch.tensor(1.0, dtype=torch.float64)
    global_grad_norm = torch.sqrt(sum(g.pow(2).sum() for g in grads))
    clip = torch.where(global_grad_norm > max_grad_norm, (global_grad_norm + clip_eps) / max_grad_norm, one) if max_grad_norm is not None else one
    beta1, beta2 = betas
    beta3 = 1 - beta1
    bias_correction1, bias_correction2 = 1 - beta1 ** t, 1 - beta2 ** t
    ratios = []
    for p, g, st in zip(params, grads, state):
        grad = g / clip
        st["exp_avg"].mul_(beta1).add_(grad, alpha=beta3)
        st["exp_avg_sq"].mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
        denom = (st["exp_avg_sq"].sqrt() / math.sqrt(bias_correction2)).add_(eps)
        update = (st["exp_avg"] / bias_correction1).div_(denom)
        if wd != 0:
            update.add_(p, alpha=wd)
        ratio = one
        if wd != 0 or always_adapt:
            w_norm, g_norm = torch.norm(p, 2.0), torch.norm(update, 2.0)
            ratio = torch.where(w_norm > 0, torch.where(g_norm > 0, w_norm / g_norm, one), one)
            if trust_clip:
                ratio = torch.minimum(ratio, one)
            update.mul_(ratio)
        ratios.append(float(ratio))
        p.add_(update, alpha=-lr)
    return ratios


@pytest.mark.parametrize("trust_clip", [0, 1])
@pytest.mark.parametrize("wd", [0.0, 0.02])
@pytest.mark.parametrize("sizes", [(300,), (7, 250, 43)], ids=["one_tensor", "three_tensors"])
def test_lamb_ref_follows_timms_step(sizes, wd, trust_clip):
    """Three steps, fp64 on both sides, always_adapt on where wd = 0 (so the ratio is exercised) and off otherwise; the middle tensor is scaled by 3 so that
    trust_clip has a ratio to cap.  The clip is the project's (clip_eps = 1e-6); with timm's own the clipped step's gradient differs by 1e-6 / norm = 1e-8
    relative, and the moments carry that on: checked at 1e-7 on a second pair of states."""
    n = sum(sizes)
    firsts = np.concatenate([[0], np.cumsum(sizes)])
    segs = tuple((int(f), 1.0, 1.0) for f in firsts[:-1])
    always_adapt = int(wd == 0.0)
    p0, m0, v0, grads = A.case_inputs(n, 1.0, segs)
    p0 = p0.astype(np.float64)
    if len(sizes) > 1:
        p0[firsts[1]:firsts[2]] *= 3.0
    tp = [torch.from_numpy(p0[a:b].copy()) for a, b in zip(firsts[:-1], firsts[1:])]
    st = [dict(exp_avg=torch.zeros_like(x), exp_avg_sq=torch.zeros_like(x)) for x in tp]
    tp0, st0 = [x.clone() for x in tp], [dict(exp_avg=torch.zeros_like(x), exp_avg_sq=torch.zeros_like(x)) for x in tp]          # under timm's own clip
    p, m, v = p0, m0.astype(np.float64), v0.astype(np.float64)
    capped = False
    for step, g in enumerate(grads):
        mx = 0.0 if step == 2 else A.MAX_NORM
        p, m, v, r, norm, coef = A.lamb_ref(p, m, v, g, 1.0, mx, step + 1, segs, wd=wd, trust_clip=trust_clip, always_adapt=always_adapt)
        tg = [torch.from_numpy(g[a:b].astype(np.float64)) for a, b in zip(firsts[:-1], firsts[1:])]
        tr = timm_lamb_step(tp, tg, st, step + 1, A.LR, A.BETAS, A.EPS, wd, mx if mx > 0 else None, trust_clip, always_adapt, clip_eps=1e-6)
        tr0 = timm_lamb_step(tp0, tg, st0, step + 1, A.LR, A.BETAS, A.EPS, wd, mx if mx > 0 else None, trust_clip, always_adapt)
        assert (coef < 0.5) if step == 0 else (coef == 1.0)
        assert A.rel(p, torch.cat(tp0).numpy()) < 1e-7 and A.rel(r, tr0) < 1e-7
        tol = 1e-12
        assert A.rel(p, torch.cat(tp).numpy()) < tol and A.rel(r, tr) < tol
        assert A.rel(m, torch.cat([s["exp_avg"] for s in st]).numpy()) < tol and A.rel(v, torch.cat([s["exp_avg_sq"] for s in st]).numpy()) < tol
        capped = capped or (trust_clip and any(x == 1.0 for x in r))
        assert not trust_clip or max(r) <= 1.0
    assert capped or not trust_clip or len(sizes) == 1


def test_lamb_ref_rules_for_excluded_and_non_adapting_segments():
    n, segs = 40, ((0, 1.0, 1.0), (10, -1.0, 1.0), (20, 2.0, 0.0), (30, 1.0, 1.0))
    p0, m0, v0, grads = A.case_inputs(n, 1.0, segs)
    p0 = p0.astype(np.float64)
    p0[30:] = 0.0
    g = grads[0].copy()
    g[10:20] = np.nan
    p, m, v, r, norm, coef = A.lamb_ref(p0, m0, v0, g, 1.0, A.MAX_NORM, 1, segs)
    assert np.isfinite(norm) and abs(norm - 100.0) < 1e-3
    assert r[1] == 0.0 and r[2] == 1.0 and r[3] == 1.0 and r[0] != 1.0
    assert np.array_equal(p[10:20], p0[10:20]) and not m[10:20].any() and not v[10:20].any()
    assert np.isfinite(p).all() and not np.array_equal(p[30:], p0[30:])


def test_fp32_figures_are_finite_and_small():
    for n, gs, segs in ((1, 1.0, None), (257, 0.125, None), (5000, 1.0, None), (5000, 0.125, tuple(s for s in A.SEGMENTS if s[0] < 5000))):
        fig = A.fp32_figures(n, gs, segs)
        assert len(fig) == 4 and np.isfinite(fig).all() and all(0.0 <= f < 1e-6 for f in fig), (n, gs, fig)


def test_lamb_state_dict_round_trip_and_foreign_states():
    from mvfnet_amd.checkpoint import adamw_state_dict, lamb_moments, lamb_state_dict, sgd_state_dict
    ms = [torch.ones(3), None, torch.full((2,), 2.0)]
    vs = [torch.zeros(3), None, torch.ones(2)]
    out = lamb_state_dict(4, ms, vs, 5e-3, (0.9, 0.99), 1e-6, 0.02, trust_clip=True, always_adapt=False, initial_lr=1e-2)
    g = out["param_groups"][0]
    assert len(out["param_groups"]) == 1 and g["lamb"] is True and g["trust_clip"] is True and g["always_adapt"] is False and g["params"] == [0, 1, 2]
    assert (g["lr"], g["initial_lr"], g["betas"], g["eps"], g["weight_decay"]) == (5e-3, 1e-2, (0.9, 0.99), 1e-6, 0.02)
    assert sorted(out["state"]) == [0, 2] and set(out["state"][0]) == {"step", "exp_avg", "exp_avg_sq"} and out["state"][0]["step"].dtype == torch.float32
    step, ms2, vs2, group = lamb_moments(out, 3)
    assert step == 4 and ms2[1] is None and vs2[1] is None and torch.equal(ms2[2], ms[2]) and torch.equal(vs2[0], vs[0]) and group["trust_clip"] is True
    per = lamb_state_dict(1, ms, vs, 5e-3, weight_decay=0.02, multipliers=[(1.0, 1.0), (2.0, 0.0), (1.0, 0.5)])
    assert [q["params"] for q in per["param_groups"]] == [[0], [1], [2]] and per["param_groups"][1]["lr"] == 1e-2 and per["param_groups"][1]["weight_decay"] == 0.0
    assert all(q["lamb"] for q in per["param_groups"]) and lamb_moments(per, 3)[0] == 1
    assert lamb_moments(lamb_state_dict(0, [None] * 3, [None] * 3, 5e-3), 3)[0] == 0
    with pytest.raises(ValueError):
        lamb_moments(out, 4)                                                           # another parameter count
    with pytest.raises(ValueError):
        lamb_moments(adamw_state_dict(4, ms, vs, 1e-3), 3)                             # AdamW's: the groups lack lamb=True
    with pytest.raises(ValueError):
        lamb_moments(sgd_state_dict([torch.zeros(3)] * 3, 0.1, 0.9, 1e-4), 3)          # SGD's: no moments
    with pytest.raises(ValueError):
        lamb_moments(dict(momentum_buffer=torch.zeros(3)), 3)                          # not an optimizer state_dict


def test_build_optimizer_refusals_for_lamb():
    import mvfnet_amd
    from mvfnet_amd.runner import EngineLamb, build_optimizer
    m = mvfnet_amd.build_recognizer(mvfnet_amd.mvfnet_config(50, 4), None, dict(average_clips=None))
    with pytest.raises(NotImplementedError):
        build_optimizer(m, dict(type="Lamb", lr=5e-3, grad_averaging=False))
    with pytest.raises(NotImplementedError):
        build_optimizer(m, dict(type="Lamb", lr=5e-3, bias_correction=False))
    with pytest.raises(TypeError):
        build_optimizer(m, dict(type="Lamb", lr=5e-3, momentum=0.9))                 # an unknown key
    with pytest.raises(TypeError):
        build_optimizer(m, dict(type="Lamb", lr=5e-3, decoupled_decay=True))
    for name in ("LAMB", "lamb"):                                                      # type names are case-sensitive: timm's class is Lamb
        with pytest.raises(NotImplementedError):
            build_optimizer(m, dict(type=name, lr=5e-3))
    with pytest.raises(ValueError):                                                    # a decay multiplier without an explicit weight_decay, as for SGD
        build_optimizer(m, dict(type="Lamb", lr=5e-3, paramwise_options=dict(norm_decay_mult=0.0)))
    with pytest.raises(NotImplementedError, match="train engine"):
        build_optimizer(torch.nn.Linear(4, 4), dict(type="Lamb", lr=5e-3))            # a model without a train engine
    assert getattr(m, "_train_engine", None) is None                                   # nothing was built on the way to those refusals
    assert EngineLamb.zero_grad is not None and hasattr(EngineLamb, "state_dict") and hasattr(EngineLamb, "load_state_dict")


def test_lamb_step_argument_failures_return_before_any_launch():
    """The codes come back on a machine without a GPU, from host addresses that are never read; LambHyper matches mvf_lamb_hyper_t (5 doubles, 2 ints)."""
    from mvfnet_amd import _lib
    lib = _lib.lib
    assert C.sizeof(_lib.LambHyper) == 48 and "mvf_lamb_step" in _lib.declared_symbols() and "mvf_lamb_workspace_bytes" in _lib.declared_symbols()
    host = (C.c_float * 4096)()
    at = lambda k: C.c_void_p(C.addressof(host) + 256 * k)  # noqa: E731
    h = _lib.LambHyper(5e-3, 0.9, 0.999, 1e-6, 0.02, 0, 0)
    EINVAL, EWS = -1, -3
    nb = lib.mvf_lamb_workspace_bytes(8, 2)
    assert nb == lib.mvf_adamw_workspace_bytes(8) + (1 + 2) * 16 and lib.mvf_lamb_workspace_bytes(8, 9) == 0 and lib.mvf_lamb_workspace_bytes(0, 1) == 0
    assert lib.mvf_lamb_workspace_bytes(4097, 1) == nb - 16 + 16          # two chunks, one segment
    ok = lambda **kw: [kw.get(k, d) for k, d in (("p", at(0)), ("g", at(1)), ("m", at(2)), ("v", at(3)), ("n", 8), ("gs", 1.0), ("mx", 40.0), ("h", C.byref(h)),  # noqa: E731
                                                 ("seg", at(4)), ("nseg", 2), ("ema", None), ("em", 0.0), ("guard", None), ("cnt", at(5)), ("norm", at(6)),
                                                 ("ratio", at(7)), ("ws", at(8)), ("wsb", nb), ("st", None))]
    assert lib.mvf_lamb_step(*ok(wsb=nb - 1)) == EWS and b"workspace too small" in lib.mvf_last_error()
    assert lib.mvf_lamb_step(*ok(ws=None)) == EWS
    for bad in (dict(seg=None), dict(ratio=None), dict(nseg=9), dict(nseg=0), dict(n=0), dict(h=None), dict(cnt=None), dict(ratio=at(6)), dict(ema=at(0), em=0.5),
                dict(ema=at(9), em=2.0), dict(h=C.byref(_lib.LambHyper(5e-3, 0.9, 0.999, 1e-6, 0.02, 2, 0))),
                dict(h=C.byref(_lib.LambHyper(5e-3, 0.9, 0.999, 1e-6, 0.02, 0, 3))), dict(h=C.byref(_lib.LambHyper(5e-3, 1.0, 0.999, 1e-6, 0.02, 0, 0))),
                dict(h=C.byref(_lib.LambHyper(5e-3, 0.9, 0.999, 0.0, 0.02, 0, 0)))):
        assert lib.mvf_lamb_step(*ok(**bad)) == EINVAL, (bad, lib.mvf_last_error())
        assert b"lamb_step" in lib.mvf_last_error()
