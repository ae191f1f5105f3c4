"""CPU: the focal / asymmetric sigmoid losses -- everything that needs no device: the fp64 restatement of mvf_focal_loss (focal_numpy.py) against torch
autograd of the defining formula in float64, against bce_numpy at gamma = 0, and against torchvision's focal formula and the asymmetric paper's formula
(both restated here; timm's and mmaction2's sources were not at hand: parity with them is claimed from the papers); class_balanced_weights; the head's
loss_cls parsing and every refusal; the ctypes declarations and the entry points' argument failures (from host addresses that are never read); the plan
key of an engine with and without the loss."""
import ctypes as C
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bce_numpy as bn
import focal_numpy as fn

EPS = np.finfo(np.float64).eps
ULPS = 16 * EPS                 # "a few fp64 ulps" of the largest value: both sides form the same products, pow / exp / log1p may differ in the last bit
# the gradient against autograd: each side chains up to 16 roundings per element (exp, 1 + e, the quotient, log1p, the max's sum, two pows, gamma *, four
# products, the two-term sum, a *, t *, c *), and autograd's chain rule adds its own per node: 2 x 16 ulps.  (Against a 40-digit evaluation of the header's
# gradient the restatement is within 5.3e-16 of the largest value and autograd within 3.2e-15, on the 5 x 400 focal case with soft targets.)
GRAD_ULPS = 32 * EPS
# the published formulas form 1 - sigmoid(s): an absolute error of one ulp of 1 where the restatement has a relative one.  It enters (1 - p_t)^gamma * ce
# with gamma <= 4 and ce <= 15 (|s| <= 15): 4 * 15 * 1.1e-16 = 6.7e-15 absolute, against a largest value >= 1
PUBLISHED = 64 * EPS
# (gamma+, gamma-, margin, alpha): BCE, focal, asymmetric, asymmetric without the positive exponent, margin alone, everything at once with a fractional gamma
SETTINGS = [(0.0, 0.0, 0.0, None), (2.0, 2.0, 0.0, 0.25), (1.0, 4.0, 0.05, None), (0.0, 4.0, 0.05, None), (0.0, 0.0, 0.05, None), (3.0, 1.5, 0.2, 0.75)]
IDS = ["bce", "focal", "asl", "asl_g0", "margin", "all"]


def _inputs(clips, classes, seed=0, limit=None):
    gen = np.random.default_rng(clips * 1009 + classes + seed)
    s = (gen.standard_normal((clips, classes)) * 6).astype(np.float32)
    if limit is None:
        flat = s.reshape(-1)
        planted = np.array([0.0, 40.0, -40.0, 100.0, -100.0], dtype=np.float32)
        flat[:min(flat.size, 5)] = planted[:min(flat.size, 5)]
    else:
        s = np.clip(s, -limit, limit)
    soft = (gen.random((clips, classes)) ** 3).astype(np.float32)
    soft[gen.random((clips, classes)) < 0.2] = 1.0
    hard = (gen.random((clips, classes)) < 0.3).astype(np.float32)
    cw = (gen.random(classes) * 4 + 0.25).astype(np.float32)
    return s, soft, hard, cw


def _rel(got, ref):
    return float(np.abs(np.asarray(got) - np.asarray(ref)).max()) / max(float(np.abs(ref).max()), 1e-300)


def _defining(s, t, gp, gn, m, alpha, cw):
    """The element loss as the header defines it, in torch float64, for autograd."""
    m = float(np.float32(m))
    p, pn = torch.sigmoid(s), torch.sigmoid(-s)
    logp = F.logsigmoid(s)
    lpos = -(pn ** float(np.float32(gp))) * logp if gp else -logp
    on = p > m
    pm = torch.where(on, p - m, torch.zeros_like(p))
    log1m = torch.where(on, F.logsigmoid(-s) if m == 0 else torch.log(pn + m), torch.zeros_like(p))
    lneg = -(pm ** float(np.float32(gn))) * log1m if gn else -log1m
    ap, an = (1.0, 1.0) if alpha is None else (float(np.float32(alpha)), 1.0 - float(np.float32(alpha)))
    el = ap * t * lpos + an * (1.0 - t) * lneg
    return el * cw if cw is not None else el


# ------------------------------------------------------------------------------------------------ the restatement against torch autograd, float64
@pytest.mark.parametrize("sum_classes", [False, True], ids=["mean", "sum"])
@pytest.mark.parametrize("weighted", [False, True], ids=["cw0", "cw1"])
@pytest.mark.parametrize("kind", ["hard", "soft", "thr"])
@pytest.mark.parametrize("setting", SETTINGS, ids=IDS)
def test_restatement_equals_autograd_in_float64(setting, kind, weighted, sum_classes):
    gp, gn, m, alpha = setting
    for clips, classes in ((1, 1), (3, 65), (5, 400)):
        s, soft, hard, cw = _inputs(clips, classes)
        t, thr = (hard, None) if kind == "hard" else (soft, None) if kind == "soft" else (soft, 0.3)
        td = torch.from_numpy((t > np.float32(0.3)).astype(np.float64) if thr is not None else t.astype(np.float64))
        sd = torch.from_numpy(s.astype(np.float64)).requires_grad_(True)
        el = _defining(sd, td, gp, gn, m, alpha, torch.from_numpy(cw.astype(np.float64)) if weighted else None)
        part = el.sum(dim=1) if sum_classes else el.mean(dim=1)
        loss = part.mean()
        loss.backward()
        out = fn.focal_loss(s, t, gp, gn, m, alpha, cw if weighted else None, thr, sum_classes, raw=True)
        e_part, e_loss, e_grad = _rel(out["loss_part"], part.detach().numpy()), _rel(np.float64(out["loss"]), loss.item()), _rel(out["dscores"], sd.grad.numpy())
        print("%dx%d loss_part %.3g loss %.3g grad %.3g (bound %.3g)" % (clips, classes, e_part, e_loss, e_grad, ULPS))
        assert np.isfinite(out["dscores"]).all() and np.isfinite(out["loss_part"]).all()
        assert e_part <= ULPS and e_loss <= ULPS and e_grad <= GRAD_ULPS


@pytest.mark.parametrize("sum_classes", [False, True], ids=["mean", "sum"])
def test_restatement_is_bce_without_focusing(sum_classes):
    for clips, classes in ((1, 1), (7, 10), (3, 400)):
        s, soft, hard, _ = _inputs(clips, classes)
        for t, thr in ((soft, None), (hard, None), (soft, 0.5)):
            a = fn.focal_loss(s, t, target_threshold=thr, sum_classes=sum_classes, raw=True)
            b = bn.bce_loss(s, t, None, thr, sum_classes, raw=True)
            assert all(_rel(a[k], b[k]) <= ULPS for k in a), {k: _rel(a[k], b[k]) for k in a}


@pytest.mark.parametrize("gamma,alpha", [(2.0, 0.25), (2.0, None), (1.0, 0.5), (4.0, 0.9), (0.0, 0.25)])
def test_restatement_equals_the_torchvision_formula_on_hard_targets(gamma, alpha):
    """torchvision.ops.sigmoid_focal_loss, restated: ce * (1 - p_t)^gamma * alpha_t."""
    s, _, hard, _ = _inputs(6, 157, limit=15.0)
    sd, td = torch.from_numpy(s.astype(np.float64)), torch.from_numpy(hard.astype(np.float64))
    p = torch.sigmoid(sd)
    ce = F.binary_cross_entropy_with_logits(sd, td, reduction="none")
    p_t = p * td + (1 - p) * (1 - td)
    ref = ce * (1 - p_t) ** gamma
    if alpha is not None:
        a32 = float(np.float32(alpha))                                          # the setting travels as a float
        ref = (a32 * td + (1 - a32) * (1 - td)) * ref
    got, _ = fn.focal_elements(s, hard, gamma, gamma, 0.0, alpha)
    print("rel %.3g (bound %.3g)" % (_rel(got, ref.numpy()), PUBLISHED))
    assert _rel(got, ref.numpy()) <= PUBLISHED


@pytest.mark.parametrize("gp,gn,clip", [(1.0, 4.0, 0.05), (0.0, 4.0, 0.05), (1.0, 4.0, 0.0), (2.0, 1.0, 0.3)])
def test_restatement_equals_the_asymmetric_papers_formula_on_hard_targets(gp, gn, clip):
    """Ridnik et al., "Asymmetric Loss For Multi-Label Classification", as its published implementation forms it (probability shifting, one-sided gammas, clamp
    at 1e-8, which is inactive for |s| <= 15)."""
    s, _, hard, _ = _inputs(6, 157, limit=15.0)
    x, y = torch.from_numpy(s.astype(np.float64)), torch.from_numpy(hard.astype(np.float64))
    xs_pos = torch.sigmoid(x)
    xs_neg = 1 - xs_pos
    if clip > 0:
        xs_neg = (xs_neg + float(np.float32(clip))).clamp(max=1)
    loss = y * torch.log(xs_pos.clamp(min=1e-8)) + (1 - y) * torch.log(xs_neg.clamp(min=1e-8))
    pt = xs_pos * y + xs_neg * (1 - y)
    ref = -(loss * torch.pow(1 - pt, gp * y + gn * (1 - y)))
    got, _ = fn.focal_elements(s, hard, gp, gn, clip, None)
    # without the shift the published form takes log(1 - sigmoid(s)): the absolute ulp of 1 - p is a relative eps / (1 - p) <= eps * e^15 of the logarithm's
    # argument, i.e. that much absolute error in a loss whose largest value is >= 1
    bound = PUBLISHED if clip > 0 else EPS * np.exp(15.0)
    print("rel %.3g (bound %.3g)" % (_rel(got, ref.numpy()), bound))
    assert _rel(got, ref.numpy()) <= bound


def test_restatement_exact_cases():
    one, zero = np.ones((1, 1), dtype=np.float32), np.zeros((1, 1), dtype=np.float32)
    out = fn.focal_loss(zero, one, 2.0, 2.0, raw=True)
    assert out["loss"] == 0.25 * np.log(2.0) and np.isclose(out["dscores"][0, 0], 0.25 * (2 * 0.5 * -np.log(2.0) - 0.5), rtol=1e-15)
    out = fn.focal_loss(zero, zero, 1.0, 4.0, 0.5, raw=True)                  # p = 0.5 is not above the margin
    assert out["loss"] == 0.0 and out["dscores"][0, 0] == 0.0
    out = fn.focal_loss(np.full((1, 1), -100.0, dtype=np.float32), one, raw=True)
    assert out["loss"] == 100.0
    # linear in the target: a soft target's loss is the mix of the two hard ones
    s, soft, _, cw = _inputs(3, 40)
    for gp, gn, m, alpha in SETTINGS:
        l1, g1 = fn.focal_elements(s, np.ones_like(s), gp, gn, m, alpha, cw)
        l0, g0 = fn.focal_elements(s, np.zeros_like(s), gp, gn, m, alpha, cw)
        l, g = fn.focal_elements(s, soft, gp, gn, m, alpha, cw)
        t = soft.astype(np.float64)
        assert _rel(l, t * l1 + (1 - t) * l0) <= ULPS and _rel(g, t * g1 + (1 - t) * g0) <= ULPS
    # finite for every finite score, NaN where the score or the class weight is not
    big = np.array([[3e38, -3e38, 800.0, -800.0]], dtype=np.float32)
    for gp, gn, m, alpha in SETTINGS:
        for t in (0.0, 1.0, 0.3):
            out = fn.focal_loss(big, np.full_like(big, t), gp, gn, m, alpha, raw=True)
            assert np.isfinite(out["loss_part"]).all() and np.isfinite(out["dscores"]).all(), (gp, gn, m, alpha, t)
    s[1, 3] = np.nan
    out = fn.focal_loss(s, soft, 1.0, 4.0, 0.05, raw=True)
    assert np.isnan(out["loss_part"][1]) and np.isnan(out["dscores"][1, 3]) and np.isfinite(out["loss_part"][[0, 2]]).all()


# ------------------------------------------------------------------------------------------------ class-balanced weights
def test_class_balanced_weights():
    from mvfnet_amd.heads import class_balanced_weights
    n = [1, 3, 10, 100, 1000, 100000]
    w = class_balanced_weights(n, 0.9999)
    assert w.dtype == np.float64 and w.shape == (6,) and abs(w.sum() - 6.0) <= 1e-12 and (np.diff(w) < 0).all()        # rarer classes weigh more
    raw = (1 - 0.9999) / (1 - 0.9999 ** np.asarray(n, dtype=np.float64))
    assert np.allclose(w, raw * 6 / raw.sum(), rtol=1e-14)
    assert np.array_equal(class_balanced_weights(n, 0.0), np.ones(6)) and np.array_equal(class_balanced_weights(n, 0), np.ones(6))
    assert np.allclose(class_balanced_weights([7, 7, 7], 0.99), 1.0, rtol=1e-15)
    assert np.array_equal(class_balanced_weights(np.array([2, 5]), 0.9), class_balanced_weights([2, 5], 0.9))
    for bad in ([], [0, 1], [1, -2], [1.5, 2], [True, 2], 5, None):
        with pytest.raises(ValueError, match="samples_per_cls"):
            class_balanced_weights(bad, 0.9)
    for bad in (1.0, -0.1, 2, float("nan"), "0.9", True, None):
        with pytest.raises(ValueError, match="beta"):
            class_balanced_weights([1, 2], bad)


# ------------------------------------------------------------------------------------------------ configuration and refusals
def _head(**kw):
    from mvfnet_amd.heads.tsn_clshead import TSNClsHead
    return TSNClsHead(in_channels=8, num_classes=5, **kw)


def _struct(prm):
    return (prm.gamma_pos, prm.gamma_neg, prm.margin, prm.alpha, prm.target_threshold, prm.sum_classes)


def test_loss_cls_parsing_of_the_focal_family():
    from mvfnet_amd.heads import class_balanced_weights
    assert _head().focal_settings("cpu") is None and _head(loss_cls=dict(type="BCELossWithLogits")).focal_settings("cpu") is None
    h = _head(loss_cls=dict(type="SigmoidFocalLoss"))
    assert h.loss_cls == dict(kind="focal", type="SigmoidFocalLoss", gamma_pos=2.0, gamma_neg=2.0, margin=0.0, alpha=0.25, class_weight=None,
                              target_threshold=None, sum_classes=False)
    assert h.bce_settings("cpu") is None
    cw, prm = h.focal_settings("cpu")
    assert cw is None and _struct(prm)[:4] == (2.0, 2.0, 0.0, 0.25) and np.isnan(prm.target_threshold) and prm.sum_classes == 0
    assert h.focal_settings("cpu")[1] is prm                     # one struct for the head's life: a plan records its address
    h = _head(loss_cls=dict(type="SigmoidFocalLoss", gamma=0, alpha=None, class_weight=[1, 2, 3, 4, 0.5], target_threshold=0.25, sum_classes=True))
    cw, prm = h.focal_settings("cpu")
    assert cw.dtype == torch.float32 and cw.tolist() == [1.0, 2.0, 3.0, 4.0, 0.5] and _struct(prm) == (0.0, 0.0, 0.0, -1.0, 0.25, 1)
    assert h.focal_settings("cpu")[0] is cw                      # uploaded once
    h = _head(loss_cls=dict(type="AsymmetricLossMultiLabel"))
    assert (h.loss_cls["gamma_pos"], h.loss_cls["gamma_neg"], h.loss_cls["margin"], h.loss_cls["alpha"]) == (1.0, 4.0, 0.05, None)
    assert _struct(h.focal_settings("cpu")[1])[:4] == (1.0, 4.0, float(np.float32(0.05)), -1.0)
    h = _head(loss_cls=dict(type="AsymmetricLossMultiLabel", gamma_neg=2, gamma_pos=0, clip=None, class_weight=np.ones(5), sum_classes=True))
    assert (h.loss_cls["gamma_pos"], h.loss_cls["gamma_neg"], h.loss_cls["margin"], h.loss_cls["class_weight"]) == (0.0, 2.0, 0.0, (1.0,) * 5)
    n = [10, 100, 1000, 10, 1]
    h = _head(loss_cls=dict(type="CBFocalLoss", samples_per_cls=n))
    assert h.loss_cls["class_weight"] == tuple(class_balanced_weights(n, 0.9999)) and h.loss_cls["alpha"] is None and h.loss_cls["gamma_pos"] == 2.0
    h = _head(loss_cls=dict(type="CBFocalLoss", samples_per_cls=n, beta=0.0, gamma=1.5, alpha=0.5, sum_classes=True))
    assert h.loss_cls["class_weight"] == (1.0,) * 5 and (h.loss_cls["gamma_neg"], h.loss_cls["alpha"], h.loss_cls["sum_classes"]) == (1.5, 0.5, True)
    # the names the BCE head's tests pin as "not built" stay so, and the list of what is built grows
    for kind in ("FocalLoss", "AsymmetricLoss", "NLLLoss", None):
        with pytest.raises(NotImplementedError, match="not built .*SigmoidFocalLoss, CBFocalLoss, AsymmetricLossMultiLabel"):
            _head(loss_cls=dict(type=kind))


def test_loss_cls_refusals_of_the_focal_family():
    for kind, key in (("SigmoidFocalLoss", "gamma"), ("CBFocalLoss", "gamma"), ("AsymmetricLossMultiLabel", "gamma_pos"), ("AsymmetricLossMultiLabel", "gamma_neg")):
        extra = dict(samples_per_cls=[1] * 5) if kind == "CBFocalLoss" else {}
        for bad in (0.5, -1, 17, float("nan"), float("inf"), "2", True, None):
            with pytest.raises(ValueError, match=key):
                _head(loss_cls=dict(type=kind, **{key: bad}, **extra))
    for bad in (-0.1, 1.5, float("nan"), "0.25", True):
        with pytest.raises(ValueError, match="alpha"):
            _head(loss_cls=dict(type="SigmoidFocalLoss", alpha=bad))
    for bad in (-0.05, 1.0, float("nan"), "0.05", True):
        with pytest.raises(ValueError, match="clip"):
            _head(loss_cls=dict(type="AsymmetricLossMultiLabel", clip=bad))
    for kind in ("SigmoidFocalLoss", "AsymmetricLossMultiLabel"):
        for n in (4, 6, 0):
            with pytest.raises(ValueError, match="class_weight holds %d entries for num_classes=5" % n):
                _head(loss_cls=dict(type=kind, class_weight=[1.0] * n))
        with pytest.raises(ValueError, match="class_weight"):
            _head(loss_cls=dict(type=kind, class_weight=2.0))
        for bad in (float("inf"), float("nan"), "0.2", True):
            with pytest.raises(ValueError, match="target_threshold"):
                _head(loss_cls=dict(type=kind, target_threshold=bad))
        for bad in (1, "yes", None):
            with pytest.raises(ValueError, match="sum_classes"):
                _head(loss_cls=dict(type=kind, sum_classes=bad))
        with pytest.raises(ValueError, match="%s: unknown key 'pos_weight'" % kind):
            _head(loss_cls=dict(type=kind, pos_weight=[1.0] * 5))
    with pytest.raises(ValueError, match="unknown key 'clip'"):
        _head(loss_cls=dict(type="SigmoidFocalLoss", clip=0.05))
    with pytest.raises(ValueError, match="unknown key 'gamma'"):
        _head(loss_cls=dict(type="AsymmetricLossMultiLabel", gamma=2.0))
    with pytest.raises(ValueError, match="unknown key 'class_weight', 'target_threshold'"):
        _head(loss_cls=dict(type="CBFocalLoss", samples_per_cls=[1] * 5, class_weight=[1.0] * 5, target_threshold=0.5))
    with pytest.raises(ValueError, match="needs samples_per_cls"):
        _head(loss_cls=dict(type="CBFocalLoss"))
    with pytest.raises(ValueError, match="samples_per_cls holds 4 entries for num_classes=5"):
        _head(loss_cls=dict(type="CBFocalLoss", samples_per_cls=[1] * 4))
    with pytest.raises(ValueError, match="CBFocalLoss: .*samples_per_cls"):
        _head(loss_cls=dict(type="CBFocalLoss", samples_per_cls=[1, 2, 0, 4, 5]))
    with pytest.raises(ValueError, match="CBFocalLoss: .*beta"):
        _head(loss_cls=dict(type="CBFocalLoss", samples_per_cls=[1] * 5, beta=1.0))


def test_the_recognizer_takes_the_focal_loss_from_its_config():
    import mvfnet_amd
    cfg = mvfnet_amd.mvfnet_config(50, 4, num_classes=10)
    cfg["cls_head"]["loss_cls"] = dict(type="AsymmetricLossMultiLabel", clip=0.1)
    m = mvfnet_amd.build_recognizer(cfg, None, dict(average_clips="sigmoid"))
    assert m.cls_head.loss_cls["margin"] == 0.1 and m.cls_head.loss_cls["kind"] == "focal"
    plain = mvfnet_amd.build_recognizer(mvfnet_amd.mvfnet_config(50, 4, num_classes=10), None, dict(average_clips=None))
    assert sorted(plain.state_dict()) == sorted(m.state_dict())               # the loss adds no parameter and no buffer


# ------------------------------------------------------------------------------------------------ the C ABI
def test_header_declarations_and_argument_failures():
    from mvfnet_amd import _lib
    lib = _lib.lib
    declared = _lib.declared_symbols()
    for name in ("mvf_focal_loss", "mvf_head_train_fwd_focal"):
        assert name in declared and hasattr(lib, name) and getattr(lib, name).restype is C.c_int and getattr(lib, name).argtypes is not None
    assert lib.mvf_abi_version() == 2              # additions only
    assert C.sizeof(_lib.FocalParams) == 32        # five floats, three ints
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    nan, inf = float("nan"), float("inf")

    def prm(gp=2.0, gn=2.0, m=0.0, alpha=-1.0, thr=nan, sc=0):
        return _lib.FocalParams(gamma_pos=gp, gamma_neg=gn, margin=m, alpha=alpha, target_threshold=thr, sum_classes=sc)
    bad_prm = [dict(gp=0.5), dict(gp=-1.0), dict(gp=16.5), dict(gp=nan), dict(gp=inf), dict(gn=0.999), dict(gn=17.0), dict(gn=nan), dict(m=-0.01), dict(m=1.0),
               dict(m=nan), dict(alpha=nan), dict(alpha=1.5), dict(alpha=inf), dict(thr=inf), dict(thr=-inf), dict(sc=2), dict(sc=-1)]

    def call(s=p, t=p, n=2, k=3, cw=None, q=None, dsc=p, part=p, loss=p, null_prm=False):
        return lib.mvf_focal_loss(s, t, n, k, cw, None if null_prm else (q or prm()), dsc, part, loss, None)
    for kw in [dict(s=None), dict(t=None), dict(part=None), dict(loss=None), dict(null_prm=True), dict(n=0), dict(n=-2), dict(k=0), dict(k=-1)] + \
            [dict(q=prm(**b)) for b in bad_prm]:
        assert call(**kw) == -1, kw                # MVF_EINVAL
        assert b"focal_loss" in lib.mvf_last_error()

    def head(feat=p, n=2, t=4, hw=1, c=8, w=p, k=3, tg=p, q=None, pooled=p, scores=p, dsc=p, part=p, loss=p, dtype=0, null_prm=False):
        return lib.mvf_head_train_fwd_focal(feat, n, t, hw, c, w, None, k, tg, None, None, None if null_prm else (q or prm()), pooled, scores, dsc, part, loss,
                                            dtype, None)
    for kw in [dict(feat=None), dict(w=None), dict(tg=None), dict(pooled=None), dict(scores=None), dict(dsc=None), dict(part=None), dict(loss=None),
               dict(null_prm=True), dict(n=0), dict(t=0), dict(hw=0), dict(c=0), dict(k=0), dict(dtype=2)] + [dict(q=prm(**b)) for b in bad_prm]:
        assert head(**kw) == -1, kw
        assert b"head_train_fwd_focal" in lib.mvf_last_error()
    assert all(v == 0.0 for v in buf)


# ------------------------------------------------------------------------------------------------ the engine's plan key and label kinds, without a device
def _bare_engine(monkeypatch, focal=None):
    """A TrainEngine that never ran __init__ (which needs a device): only what _plan_key and _step_tensors read."""
    from mvfnet_amd.train_engine import TrainEngine
    eng = object.__new__(TrainEngine)
    eng.num_classes, eng.keep_io, eng.input_pipeline, eng._nbt_mods = 5, False, None, []
    eng.erasing = eng.distill = eng.blending = eng.randaug = None
    eng.label_smooth_eps, eng.dropout, eng.bce, eng.focal = 0.0, 0.5, None, focal
    eng.model = torch.nn.Linear(2, 2)
    eng._ddp_active = lambda: False
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a: types.SimpleNamespace(cuda_stream=0))
    return eng


def test_the_plan_key_holds_the_loss_only_when_set(monkeypatch):
    eng = _bare_engine(monkeypatch)
    eng.use_plan = True
    imgs, labels = torch.zeros(2, 4, 3, 8, 8), torch.zeros(2, 1, dtype=torch.int64)
    key = eng._plan_key(imgs, labels)
    assert len(key) == 12 and key[-3:] == (False, 0.0, False)                 # the key of the default loss is what it was
    h = _head(loss_cls=dict(type="SigmoidFocalLoss", class_weight=[1.0] * 5))
    eng.focal = h.focal_settings("cpu")
    with_focal = eng._plan_key(imgs, labels)
    assert with_focal[:-1] == key and with_focal[-1] == ("focal", eng.focal[0].data_ptr(), C.addressof(eng.focal[1]), "2.0", "2.0", "0.0", "0.25", "nan", 0)
    assert with_focal == eng._plan_key(imgs, labels)                           # a NaN threshold does not make the key unequal to itself
    other = _head(loss_cls=dict(type="AsymmetricLossMultiLabel", sum_classes=True)).focal_settings("cpu")
    eng.focal = other
    assert eng._plan_key(imgs, labels)[-1] == ("focal", 0, C.addressof(other[1]), "1.0", "4.0", repr(float(np.float32(0.05))), "-1.0", "nan", 1)


def test_label_kinds_under_the_focal_head_and_the_blending_refusal(monkeypatch):
    eng = _bare_engine(monkeypatch, focal=_head(loss_cls=dict(type="SigmoidFocalLoss")).focal_settings("cpu"))
    imgs = torch.zeros(2, 4, 3, 8, 8)
    hot = torch.tensor([[1, 0, 1, 0, 0], [0, 0, 0, 0, 1]])
    assert eng._soft_labels(imgs, hot.float()) and eng._soft_labels(imgs, hot.bool()) and eng._soft_labels(imgs, hot.to(torch.uint8))
    assert not eng._soft_labels(imgs, torch.zeros(2, 1, dtype=torch.int64)) and not eng._soft_labels(imgs, hot)        # int64: class indices
    assert eng._uses_soft_head(torch.zeros(2, dtype=torch.int64))           # the head always takes the target-matrix path
    for blending, eps in ((object(), 0.0), (None, 0.1)):
        eng.blending, eng.label_smooth_eps = blending, eps
        for lab in (hot.float(), hot.bool()):
            with pytest.raises(ValueError, match="soft .* labels are taken as they are"):
                eng._step_tensors(imgs, lab)
