"""What the fused Adam / AdamW step and the cosine / poly learning-rate policies promise without a GPU: mvf_adamw_step refuses bad arguments before any launch
(host addresses that are never read, as in test_abi_cpu.py), the schedules match closed-form values written out by hand, and the state-dict helpers of
checkpoint.py round-trip through a real torch.optim.AdamW."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import adamw_numpy as A  # noqa: E402

EINVAL, EWS = -1, -3


# ------------------------------------------------------------------------------------------------ 6. argument checks
class _Arena(object):
    """Host memory laid out like a valid call with n = 8: every operand in its own 64-byte slot of an 8-byte aligned arena, a workspace of its own."""

    def __init__(self, L):
        self.L = L
        self.mem = (C.c_double * 128)()                   # 1024 bytes, zero
        self.ws = (C.c_double * 1024)()                   # 8192 bytes >= mvf_adamw_workspace_bytes(8)
        self.seg = (L.SgdSegment * 1)(L.SgdSegment(0, 1.0, 1.0))
        b = C.addressof(self.mem)
        self.at = dict(params=b, grads=b + 64, exp_avg=b + 128, exp_avg_sq=b + 192, ema=b + 256, guard=b + 320, steps=b + 384, norm=b + 448)
        self.hyper = L.AdamwHyper(A.LR, A.BETAS[0], A.BETAS[1], A.EPS, A.WD, 1)

    def call(self, hyper="own", **over):
        a = dict(self.at, n=8, segments=None, nseg=0, ema=None, ema_m=0.0, guard=None, ws=C.addressof(self.ws), ws_bytes=C.sizeof(self.ws))
        a.update(over)
        h = C.byref(self.hyper) if hyper == "own" else hyper
        return self.L.lib.mvf_adamw_step(a["params"], a["grads"], a["exp_avg"], a["exp_avg_sq"], a["n"], 1.0, 40.0, h, a["segments"], a["nseg"], a["ema"],
                                         a["ema_m"], a["guard"], a["steps"], a["norm"], a["ws"], a["ws_bytes"], None)

    def untouched(self):
        return not any(self.mem) and not any(self.ws)


def test_adamw_step_refuses_bad_arguments_before_any_launch():
    from mvfnet_amd import _lib as L
    ar = _Arena(L)
    at = ar.at
    assert L.lib.mvf_adamw_workspace_bytes(8) <= C.sizeof(ar.ws) and L.lib.mvf_adamw_workspace_bytes(8) >= 1024 * 4 + 16
    cases = {
        # the checks of the guarded SGD entry point
        "NULL params": dict(params=None), "NULL grads": dict(grads=None), "NULL exp_avg": dict(exp_avg=None), "NULL exp_avg_sq": dict(exp_avg_sq=None),
        "NULL norm_out": dict(norm=None), "n = 0": dict(n=0), "n < 0": dict(n=-3), "segments with nseg = 0": dict(segments=C.addressof(ar.seg), nseg=0),
        "misaligned ema": dict(ema=at["ema"] + 2), "ema over params": dict(ema=at["params"] + 4), "ema over grads": dict(ema=at["grads"]),
        "ema_momentum > 1": dict(ema=at["ema"], ema_m=1.5), "ema_momentum < 0": dict(ema=at["ema"], ema_m=-0.1), "ema_momentum NaN": dict(ema=at["ema"], ema_m=float("nan")),
        "misaligned guard": dict(guard=at["guard"] + 2), "guard over params": dict(guard=at["params"] + 16), "guard over norm_out": dict(guard=at["norm"] - 12),
        "guard over the workspace": dict(guard=C.addressof(ar.ws) + 64), "guard over the segment table": dict(guard=C.addressof(ar.seg), segments=C.addressof(ar.seg), nseg=1),
        # applied_steps
        "NULL applied_steps": dict(steps=None), "misaligned applied_steps": dict(steps=at["steps"] + 4), "applied_steps over params": dict(steps=at["params"] + 8),
        "applied_steps over grads": dict(steps=at["grads"]), "applied_steps over exp_avg": dict(steps=at["exp_avg"] + 24), "applied_steps over exp_avg_sq": dict(steps=at["exp_avg_sq"]),
        "applied_steps over ema": dict(ema=at["ema"], steps=at["ema"] + 8), "applied_steps over guard": dict(guard=at["guard"], steps=at["guard"] + 8),
        "applied_steps over norm_out": dict(steps=at["norm"]), "applied_steps over the workspace": dict(steps=C.addressof(ar.ws) + 4096),
        # the moments
        "exp_avg over params": dict(exp_avg=at["params"]), "exp_avg over grads": dict(exp_avg=at["grads"] + 4), "exp_avg_sq over params": dict(exp_avg_sq=at["params"] + 28),
        "exp_avg_sq over exp_avg": dict(exp_avg_sq=at["exp_avg"] + 4), "exp_avg over ema": dict(ema=at["ema"], exp_avg=at["ema"]), "exp_avg_sq over norm_out": dict(exp_avg_sq=at["norm"] - 28),
        "exp_avg over the workspace": dict(exp_avg=C.addressof(ar.ws)), "exp_avg_sq over guard": dict(guard=at["guard"], exp_avg_sq=at["guard"] + 4),
        "misaligned workspace": dict(ws=C.addressof(ar.ws) + 4),
    }
    for what, over in cases.items():
        assert ar.call(**over) == EINVAL, what
        assert L.lib.mvf_last_error(), what
        assert ar.untouched(), what
    assert ar.call(hyper=None) == EINVAL and b"hyper" in L.lib.mvf_last_error()
    nan = float("nan")
    good = (A.LR, A.BETAS[0], A.BETAS[1], A.EPS, A.WD, 1)
    for field, values in (("lr", (-1e-3, nan)), ("beta1", (1.0, -0.1, 1.5, nan)), ("beta2", (1.0, -1e-9, nan)), ("eps", (0.0, -1e-8, nan)),
                          ("weight_decay", (-0.05, nan)), ("decoupled", (2, -1))):
        for v in values:
            h = L.AdamwHyper(*good)
            setattr(h, field, v)
            assert ar.call(hyper=C.byref(h)) == EINVAL, (field, v)
            assert ar.untouched(), (field, v)
    for what, over in {"NULL workspace": dict(ws=None), "short workspace": dict(ws_bytes=L.lib.mvf_adamw_workspace_bytes(8) - 1), "no workspace bytes": dict(ws_bytes=0)}.items():
        assert ar.call(**over) == EWS, what
        assert ar.untouched(), what


# ------------------------------------------------------------------------------------------------ 13. learning-rate policies
def test_cosine_lr_matches_closed_form_values():
    from mvfnet_amd.runner import cosine_lr
    # base 0.1, target 0.001, ten epochs: target + 0.5 * 0.099 * (1 + cos(pi * e / 10))
    for kw in (dict(min_lr=0.001), dict(min_lr_ratio=0.01)):
        assert abs(cosine_lr(0.1, 0, 0, max_epochs=10, **kw) - 0.1) < 1e-15
        assert abs(cosine_lr(0.1, 5, 1234, max_epochs=10, **kw) - 0.0505) < 1e-15          # cos(pi / 2) = 0: the midpoint of base and target
        assert abs(cosine_lr(0.1, 10, 9999, max_epochs=10, **kw) - 0.001) < 1e-15          # progress = max_progress: the target
        assert abs(cosine_lr(0.1, 2, 7, max_epochs=8, **kw) - (0.001 + 0.0495 * (1 + math.sqrt(0.5)))) < 1e-15          # cos(pi / 4)
    # by iteration: the epoch does not enter
    assert abs(cosine_lr(0.1, 3, 0, max_iters=100, min_lr=0.001, by_epoch=False) - 0.1) < 1e-15
    assert abs(cosine_lr(0.1, 3, 50, max_iters=100, min_lr=0.001, by_epoch=False) - 0.0505) < 1e-15
    assert abs(cosine_lr(0.1, 3, 100, max_iters=100, min_lr=0.001, by_epoch=False) - 0.001) < 1e-15
    # linear warm-up on top, as step_lr applies it: lr * (1 - (1 - it / iters) * (1 - ratio)); it = 5 of 10 at ratio 0.1 -> x 0.55
    assert abs(cosine_lr(0.1, 0, 5, max_epochs=10, min_lr=0.001, warmup="linear", warmup_iters=10, warmup_ratio=0.1) - 0.055) < 1e-15
    assert abs(cosine_lr(0.1, 5, 5, max_epochs=10, min_lr=0.001, warmup="linear", warmup_iters=10, warmup_ratio=0.1) - 0.0505 * 0.55) < 1e-15
    assert abs(cosine_lr(0.1, 5, 10, max_epochs=10, min_lr=0.001, warmup="linear", warmup_iters=10, warmup_ratio=0.1) - 0.0505) < 1e-15          # warm-up over
    assert abs(cosine_lr(0.1, 0, 5, max_iters=100, min_lr=0.001, by_epoch=False, warmup="linear", warmup_iters=10, warmup_ratio=0.1)
               - 0.55 * (0.001 + 0.0495 * (1 + math.cos(math.pi * 0.05)))) < 1e-15
    assert abs(cosine_lr(0.1, 0, 5, max_epochs=10, min_lr=0.001, warmup="constant", warmup_iters=10, warmup_ratio=0.25) - 0.025) < 1e-15
    with pytest.raises(ValueError):
        cosine_lr(0.1, 0, 0, max_epochs=10)                                   # neither min_lr nor min_lr_ratio
    with pytest.raises(ValueError):
        cosine_lr(0.1, 0, 0, max_epochs=10, min_lr=0.0, min_lr_ratio=0.1)     # both
    with pytest.raises(ValueError):
        cosine_lr(0.1, 0, 0, min_lr=0.0)                                      # max_epochs unknown
    with pytest.raises(NotImplementedError):
        cosine_lr(0.1, 0, 3, max_epochs=10, min_lr=0.0, warmup="cosine", warmup_iters=10)


def test_poly_lr_matches_closed_form_values():
    from mvfnet_amd.runner import poly_lr
    # (0.1 - 0.01) * (1 - e / 10) ** 2 + 0.01
    assert abs(poly_lr(0.1, 0, 0, max_epochs=10, power=2.0, min_lr=0.01) - 0.1) < 1e-15
    assert abs(poly_lr(0.1, 5, 77, max_epochs=10, power=2.0, min_lr=0.01) - 0.0325) < 1e-15
    assert abs(poly_lr(0.1, 10, 77, max_epochs=10, power=2.0, min_lr=0.01) - 0.01) < 1e-15          # the target at the end
    # defaults: power 1, min_lr 0 -> a straight line to zero
    assert abs(poly_lr(0.1, 5, 0, max_epochs=10) - 0.05) < 1e-15 and poly_lr(0.1, 10, 0, max_epochs=10) == 0.0
    # by iteration, power 0.9 (the segmentation recipes' value): 0.1 * 0.5 ** 0.9
    assert abs(poly_lr(0.1, 9, 50, max_iters=100, power=0.9, by_epoch=False) - 0.1 * 0.5 ** 0.9) < 1e-15
    assert abs(poly_lr(0.1, 9, 100, max_iters=100, power=0.9, min_lr=1e-4, by_epoch=False) - 1e-4) < 1e-15
    # linear warm-up on top: it = 5 of 10 at ratio 0.1 -> x 0.55
    assert abs(poly_lr(0.1, 5, 5, max_epochs=10, power=2.0, min_lr=0.01, warmup="linear", warmup_iters=10, warmup_ratio=0.1) - 0.0325 * 0.55) < 1e-15
    assert abs(poly_lr(0.1, 0, 2, max_iters=100, by_epoch=False, warmup="exp", warmup_iters=4, warmup_ratio=0.25) - 0.1 * 0.98 * 0.25 ** 0.5) < 1e-15


def test_lr_policy_settings_are_checked_and_step_is_unchanged():
    from mvfnet_amd.runner import check_lr_policy, step_lr
    assert check_lr_policy(None) is None and check_lr_policy(dict(policy="step", step=[90, 130])) is None and check_lr_policy(dict()) is None
    assert check_lr_policy(dict(policy="cosine", min_lr=0.0)) == dict(policy="cosine", by_epoch=True, min_lr=0.0, min_lr_ratio=None)
    assert check_lr_policy(dict(policy="CosineAnnealing", min_lr_ratio=0.01, by_epoch=False)) == dict(policy="cosine", by_epoch=False, min_lr=None, min_lr_ratio=0.01)
    assert check_lr_policy(dict(policy="poly", power=0.9)) == dict(policy="poly", by_epoch=True, power=0.9, min_lr=0.0)
    with pytest.raises(ValueError):
        check_lr_policy(dict(policy="cosine"))
    for unknown in ("cyclic", "exp", "OneCycle", 3):
        with pytest.raises(NotImplementedError):
            check_lr_policy(dict(policy=unknown))
    # the 'step' results for the arguments the existing tests and the shipped config use
    assert abs(step_lr(0.015, 0, 0) - 0.015 * 0.01) < 1e-15 and abs(step_lr(0.015, 0, 25070) - 0.015) < 1e-15
    assert abs(step_lr(0.015, 95, 30000) - 0.0015) < 1e-15 and abs(step_lr(0.015, 130, 30000) - 0.00015) < 1e-15
    assert abs(step_lr(0.1, 0, 5, warmup="constant", warmup_iters=10, warmup_ratio=0.25) - 0.025) < 1e-12
    assert abs(step_lr(0.1, 0, 5, warmup="exp", warmup_iters=10, warmup_ratio=0.25) - 0.1 * 0.25 ** 0.5) < 1e-12
    assert step_lr(0.1, 0, 3, warmup=None, warmup_iters=10) == 0.1


# ------------------------------------------------------------------------------------------------ 14. state-dict helpers
class _Three(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.fc = torch.nn.Linear(3, 2)
        self.scale = torch.nn.Parameter(torch.ones(2))

    def forward(self, x):
        return (self.fc(x) * self.scale).sum()


def _stepped(seed, steps, groups=False, **kw):
    torch.manual_seed(seed)
    m = _Three()
    params = list(m.parameters())
    opt = torch.optim.AdamW([dict(params=[p]) for p in params] if groups else params, lr=A.LR, betas=A.BETAS, eps=A.EPS, weight_decay=A.WD, **kw)
    for i in range(steps):
        opt.zero_grad()
        m(torch.full((4, 3), 1.0 + i)).backward()
        opt.step()
    return m, opt


@pytest.mark.parametrize("groups", [False, True], ids=["one_group", "group_per_parameter"])
def test_adamw_state_dict_helpers_round_trip_through_torch_adamw(groups):
    from mvfnet_amd.checkpoint import adamw_moments, adamw_state_dict
    m, opt = _stepped(0, 2, groups)
    sd = opt.state_dict()
    step, ms, vs, group = adamw_moments(sd, 3)
    assert step == 2 and len(ms) == len(vs) == 3 and group["betas"] == A.BETAS and group["decoupled_weight_decay"] is True
    assert all(torch.equal(a, sd["state"][i]["exp_avg"]) and torch.equal(b, sd["state"][i]["exp_avg_sq"]) for i, (a, b) in enumerate(zip(ms, vs)))
    mult = [(1.0, 1.0), (2.0, 0.0), (1.0, 0.0)] if groups else None
    # (clones: torch's state_dict() hands out the live state tensors and load_state_dict keeps what it is given)
    out = adamw_state_dict(step, [t.clone() for t in ms], [t.clone() for t in vs], A.LR, A.BETAS, A.EPS, A.WD, True, multipliers=mult, initial_lr=0.5)
    assert len(out["param_groups"]) == (3 if groups else 1)
    assert set(sd["param_groups"][0]) <= set(out["param_groups"][0])                       # every key torch.optim.AdamW writes, + initial_lr
    assert out["param_groups"][0]["initial_lr"] == 0.5 and [g["params"] for g in out["param_groups"]] == [g["params"] for g in sd["param_groups"]]
    if groups:
        assert out["param_groups"][1]["lr"] == A.LR * 2.0 and out["param_groups"][1]["weight_decay"] == 0.0 and out["param_groups"][1]["initial_lr"] == 1.0
    st = out["state"][0]["step"]
    assert st.dtype == torch.float32 and st.shape == () and float(st) == 2.0
    # a fresh torch.optim.AdamW takes it and continues exactly as the original does
    m2, opt2 = _stepped(0, 0, groups)
    m2.load_state_dict(m.state_dict())
    if groups:
        for g in out["param_groups"]:          # (the multipliers above are this test's own: the twin keeps torch's uniform groups)
            g.update(lr=A.LR, weight_decay=A.WD)
    opt2.load_state_dict(out)
    for mod, o in ((m, opt), (m2, opt2)):
        o.zero_grad()
        mod(torch.full((4, 3), 3.0)).backward()
        o.step()
    assert all(torch.equal(a, b) for a, b in zip(m.parameters(), m2.parameters()))
    assert all(float(opt2.state[p]["step"]) == 3.0 for p in m2.parameters())


def test_adamw_state_dict_helpers_handle_unstepped_parameters_and_refuse_what_is_not_built():
    from mvfnet_amd.checkpoint import adamw_moments, adamw_state_dict
    out = adamw_state_dict(4, [torch.zeros(2, 3), None, torch.ones(2)], [torch.zeros(2, 3), None, torch.ones(2)], 1e-3, decoupled=False)
    assert sorted(out["state"]) == [0, 2] and out["param_groups"][0]["decoupled_weight_decay"] is False and out["param_groups"][0]["initial_lr"] == 1e-3
    step, ms, vs, _ = adamw_moments(out, 3)
    assert step == 4 and ms[1] is None and vs[1] is None and torch.equal(vs[2], torch.ones(2))
    assert adamw_moments(adamw_state_dict(0, [None] * 3, [None] * 3, 1e-3), 3)[0] == 0
    with pytest.raises(ValueError):
        adamw_moments(out, 4)                                      # another parameter count
    with pytest.raises(ValueError):
        adamw_moments(dict(momentum_buffer=torch.zeros(3)), 3)      # not a torch optimizer state_dict
    out["state"][2]["step"] = torch.tensor(5.0)
    with pytest.raises(ValueError):
        adamw_moments(out, 3)                                      # the fused optimizer keeps ONE step count
    _, opt = _stepped(1, 1, amsgrad=True)
    with pytest.raises(NotImplementedError):
        adamw_moments(opt.state_dict(), 3)
    from mvfnet_amd.checkpoint import sgd_state_dict
    with pytest.raises(ValueError):
        adamw_moments(sgd_state_dict([torch.zeros(3)] * 3, 0.1, 0.9, 1e-4), 3)          # an SGD state: no exp_avg


def test_build_optimizer_refuses_amsgrad_maximize_and_unknown_types():
    import mvfnet_amd
    from mvfnet_amd.runner import build_optimizer
    m = mvfnet_amd.build_recognizer(mvfnet_amd.mvfnet_config(50, 4), None, dict(average_clips=None))
    for kind in ("AdamW", "Adam"):
        with pytest.raises(NotImplementedError):
            build_optimizer(m, dict(type=kind, lr=1e-3, amsgrad=True))
        with pytest.raises(NotImplementedError):
            build_optimizer(m, dict(type=kind, lr=1e-3, maximize=True))
    with pytest.raises(NotImplementedError):
        build_optimizer(m, dict(type="LAMB", lr=1e-3))
    with pytest.raises(ValueError):                 # a decay multiplier without an explicit weight_decay, as for SGD
        build_optimizer(m, dict(type="AdamW", lr=1e-3, paramwise_options=dict(norm_decay_mult=0.0)))
    assert getattr(m, "_train_engine", None) is None          # nothing was built on the way to those refusals
    assert np.isfinite(A.fp32_figures(257, 0.125, 1)).all()
