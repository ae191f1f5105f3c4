"""CPU: the binary cross-entropy head -- everything that needs no device: the fp64 restatement of mvf_bce_loss (bce_numpy.py) against torch's own
binary_cross_entropy_with_logits in float64, values and autograd gradient; the head's loss_cls parsing and every refusal; average_clips='sigmoid' in the
configuration; the header / ctypes declarations and the entry points' argument failures (from host addresses that are never read); the plan key of an
engine with the default loss."""
import ctypes as C
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import bce_numpy as bn

ULPS = 16 * np.finfo(np.float64).eps            # "a few fp64 ulps": the two sides order (1 - t) * s + lw * softplus(-s) alike, exp / log1p may differ in the last bit


# ------------------------------------------------------------------------------------------------ the restatement against torch, float64
@pytest.mark.parametrize("sum_classes", [False, True], ids=["mean", "sum"])
@pytest.mark.parametrize("with_weight", [False, True], ids=["pw0", "pw1"])
@pytest.mark.parametrize("clips,classes,scale,thr", [(1, 1, 1.0, None), (7, 10, 1.0, None), (3, 257, 40.0, 0.2), (7, 400, 1.0, 0.5), (2, 1000, 200.0, None),
                                                      (5, 400, 40.0, 0.0)])
def test_restatement_equals_torch_in_float64(clips, classes, scale, thr, with_weight, sum_classes):
    gen = torch.Generator().manual_seed(clips * 1009 + classes)
    s = (torch.randn(clips, classes, generator=gen) * scale).float()
    t = torch.rand(clips, classes, generator=gen).float() ** 3
    pw = (torch.rand(classes, generator=gen) * 4 + 0.25).float() if with_weight else None
    sd = s.double().requires_grad_(True)
    td = (t > np.float32(thr)).double() if thr is not None else t.double()
    el = F.binary_cross_entropy_with_logits(sd, td, pos_weight=pw.double() if with_weight else None, reduction="none")
    part = el.sum(dim=1) if sum_classes else el.mean(dim=1)
    loss = part.mean()
    loss.backward()
    out = bn.bce_loss(s.numpy(), t.numpy(), pw.numpy() if with_weight else None, thr, sum_classes, raw=True)
    rel = lambda got, ref: float(np.abs(got - ref).max()) / max(float(np.abs(ref).max()), 1e-300)  # noqa: E731
    e_part, e_loss, e_grad = rel(out["loss_part"], part.detach().numpy()), rel(np.float64(out["loss"]), loss.item()), rel(out["dscores"], sd.grad.numpy())
    print("loss_part %.3g loss %.3g grad %.3g (bound %.3g)" % (e_part, e_loss, e_grad, ULPS))
    assert e_part <= ULPS and e_loss <= ULPS and e_grad <= ULPS


def test_restatement_exact_cases():
    z = np.zeros((3, 5), dtype=np.float32)
    for t in (0.0, 1.0):
        out = bn.bce_loss(z, np.full((3, 5), t, dtype=np.float32), raw=True)
        assert np.array_equal(out["loss_part"], np.full(3, np.log(2.0))) and out["loss"] == np.log(2.0)
    out = bn.bce_loss(z, np.ones((3, 5), dtype=np.float32), sum_classes=True, raw=True)
    assert np.allclose(out["loss_part"], 5 * np.log(2.0), rtol=1e-15)
    # the threshold turns soft targets into hard ones; NaN = off
    s = np.random.default_rng(0).standard_normal((2, 6)).astype(np.float32)
    t = np.array([[0.0, 0.1, 0.2, 0.3, 0.9, 1.0]] * 2, dtype=np.float32)
    a, b = bn.bce_loss(s, t, target_threshold=0.2), bn.bce_loss(s, (t > np.float32(0.2)).astype(np.float32))
    assert all(np.array_equal(a[k], b[k]) for k in a)
    c, d = bn.bce_loss(s, t, target_threshold=float("nan")), bn.bce_loss(s, t)
    assert all(np.array_equal(c[k], d[k]) for k in c) and not np.array_equal(a["loss"], c["loss"])
    # |s| = 200: finite, and the gradient keeps the tail a float32 exp would lose
    big = np.array([[200.0, -200.0]], dtype=np.float32)
    out = bn.bce_loss(big, np.array([[1.0, 0.0]], dtype=np.float32), raw=True)
    assert np.isfinite(out["loss_part"]).all() and (out["loss_part"] > 0).all() and out["dscores"][0, 0] < 0      # (-1.4e-87 / 2: t = 1, s = 200)
    assert np.allclose(bn.average_clip_sigmoid(np.array([[0.0, 800.0, -800.0]])), [[0.5, 1.0, 0.0]])


# ------------------------------------------------------------------------------------------------ configuration and refusals
def _head(**kw):
    from mvfnet_amd.heads.tsn_clshead import TSNClsHead
    return TSNClsHead(in_channels=8, num_classes=5, **kw)


def test_loss_cls_parsing():
    from mvfnet_amd.heads.tsn_clshead import check_loss_cls
    assert _head().loss_cls is None and _head(loss_cls=None).loss_cls is None and _head(loss_cls=dict(type="CrossEntropyLoss")).loss_cls is None
    assert _head().bce_settings("cpu") is None
    h = _head(loss_cls=dict(type="BCELossWithLogits"))
    assert h.loss_cls == dict(pos_weight=None, target_threshold=None, sum_classes=False)
    pw, thr, sc = h.bce_settings("cpu")
    assert pw is None and np.isnan(thr) and sc == 0
    h = _head(loss_cls=dict(type="BCELossWithLogits", pos_weight=[1, 2, 3, 4, 0.5], target_threshold=0.2, sum_classes=True))
    assert h.loss_cls == dict(pos_weight=(1.0, 2.0, 3.0, 4.0, 0.5), target_threshold=0.2, sum_classes=True)
    pw, thr, sc = h.bce_settings("cpu")
    assert pw.dtype == torch.float32 and pw.tolist() == [1.0, 2.0, 3.0, 4.0, 0.5] and (thr, sc) == (0.2, 1)
    assert h.bce_settings("cpu")[0] is pw                       # uploaded once: a persistent buffer
    assert check_loss_cls(dict(type="BCELossWithLogits", pos_weight=np.ones(5, dtype=np.float32)), 5)["pos_weight"] == (1.0,) * 5
    for kind in ("FocalLoss", "AsymmetricLoss", "NLLLoss", None):
        with pytest.raises(NotImplementedError, match="not built"):
            _head(loss_cls=dict(type=kind))
    for n in (4, 6, 0):
        with pytest.raises(ValueError, match="pos_weight holds %d entries for num_classes=5" % n):
            _head(loss_cls=dict(type="BCELossWithLogits", pos_weight=[1.0] * n))
    with pytest.raises(ValueError, match="pos_weight"):
        _head(loss_cls=dict(type="BCELossWithLogits", pos_weight=2.0))
    for bad in (float("inf"), float("-inf"), float("nan"), "0.2", True):
        with pytest.raises(ValueError, match="target_threshold"):
            _head(loss_cls=dict(type="BCELossWithLogits", target_threshold=bad))
    for bad in (1, "yes", None):
        with pytest.raises(ValueError, match="sum_classes"):
            _head(loss_cls=dict(type="BCELossWithLogits", sum_classes=bad))
    with pytest.raises(ValueError, match="unknown key 'reduction'"):
        _head(loss_cls=dict(type="BCELossWithLogits", reduction="sum"))
    with pytest.raises(ValueError, match="takes no options"):
        _head(loss_cls=dict(type="CrossEntropyLoss", class_weight=[1.0]))
    with pytest.raises(ValueError, match="'type'"):
        _head(loss_cls=dict(pos_weight=None))


def test_the_recognizer_takes_the_loss_from_its_config_and_sigmoid_averaging():
    import mvfnet_amd
    from mvfnet_amd.engine import HeadEngine
    cfg = mvfnet_amd.mvfnet_config(50, 4, num_classes=10)
    cfg["cls_head"]["loss_cls"] = dict(type="BCELossWithLogits", target_threshold=0.2)
    m = mvfnet_amd.build_recognizer(cfg, None, dict(average_clips="sigmoid"))
    assert m.cls_head.loss_cls == dict(pos_weight=None, target_threshold=0.2, sum_classes=False) and m.test_cfg["average_clips"] == "sigmoid"
    plain = mvfnet_amd.build_recognizer(mvfnet_amd.mvfnet_config(50, 4, num_classes=10), None, dict(average_clips=None))
    assert plain.cls_head.loss_cls is None and sorted(plain.state_dict()) == sorted(m.state_dict())       # the loss adds no parameter and no buffer
    # 'sigmoid' is a kind of its own, not a widened `kind` of mvf_average_clip; anything else is refused as before
    assert "sigmoid" not in HeadEngine.KINDS and sorted(k for k in HeadEngine.KINDS if k) == ["prob", "score"]
    eng = HeadEngine(torch.nn.Linear(4, 3), "cpu")
    with pytest.raises(ValueError, match="softmax is not supported"):
        eng.average(torch.zeros(2, 3), "softmax")
    assert eng.average(torch.zeros(2, 3), None).shape == (2, 3)


# ------------------------------------------------------------------------------------------------ the C ABI
def test_header_declarations_and_argument_failures():
    from mvfnet_amd import _lib
    lib = _lib.lib
    declared = _lib.declared_symbols()
    for name in ("mvf_bce_loss", "mvf_head_train_fwd_bce", "mvf_average_clip_sigmoid"):
        assert name in declared and hasattr(lib, name) and getattr(lib, name).restype is C.c_int and getattr(lib, name).argtypes is not None
    assert lib.mvf_abi_version() == 2              # additions only
    buf = (C.c_float * 64)()
    p = C.cast(buf, C.c_void_p)
    nan, inf = float("nan"), float("inf")

    def call(s=p, t=p, n=2, k=3, pw=None, thr=nan, sc=0, dsc=p, part=p, loss=p):
        return lib.mvf_bce_loss(s, t, n, k, pw, C.c_float(thr), sc, dsc, part, loss, None)
    cases = [dict(s=None), dict(t=None), dict(part=None), dict(loss=None), dict(n=0), dict(n=-2), dict(k=0), dict(k=-1), dict(thr=inf), dict(thr=-inf), dict(sc=2),
             dict(sc=-1)]
    for kw in cases:
        assert call(**kw) == -1, kw                # MVF_EINVAL
        assert b"bce_loss" in lib.mvf_last_error()

    def head(feat=p, n=2, t=4, hw=1, c=8, w=p, k=3, tg=p, thr=nan, sc=0, pooled=p, scores=p, dsc=p, part=p, loss=p, dtype=0):
        return lib.mvf_head_train_fwd_bce(feat, n, t, hw, c, w, None, k, tg, None, None, C.c_float(thr), sc, pooled, scores, dsc, part, loss, dtype, None)
    for kw in [dict(feat=None), dict(w=None), dict(tg=None), dict(pooled=None), dict(scores=None), dict(dsc=None), dict(part=None), dict(loss=None), dict(n=0),
               dict(t=0), dict(hw=0), dict(c=0), dict(k=0), dict(thr=inf), dict(sc=3), dict(dtype=2)]:
        assert head(**kw) == -1, kw
        assert b"head_train_fwd_bce" in lib.mvf_last_error()
    for kw in [dict(s=None), dict(o=None), dict(n=0), dict(k=0)]:
        a = dict(s=p, n=2, k=3, o=p)
        a.update(kw)
        assert lib.mvf_average_clip_sigmoid(a["s"], a["n"], a["k"], a["o"], None) == -1, kw
    # mvf_average_clip's own check is what it was: kind 3 is not 'sigmoid'
    assert lib.mvf_average_clip(p, 2, 3, 3, p, None) == -1
    assert all(v == 0.0 for v in buf)


# ------------------------------------------------------------------------------------------------ the engine's plan key and refusals, without a device
def _bare_engine(monkeypatch, bce=None):
    """A TrainEngine that never ran __init__ (which needs a device): only what _plan_key and _step_tensors read."""
    from mvfnet_amd.train_engine import TrainEngine
    eng = object.__new__(TrainEngine)
    eng.num_classes, eng.keep_io, eng.input_pipeline, eng._nbt_mods = 5, False, None, []
    eng.erasing = eng.distill = eng.blending = eng.randaug = None
    eng.label_smooth_eps, eng.dropout, eng.bce = 0.0, 0.5, bce
    eng.model = torch.nn.Linear(2, 2)
    eng._ddp_active = lambda: False
    monkeypatch.setattr(torch.cuda, "current_stream", lambda *a: types.SimpleNamespace(cuda_stream=0))
    return eng


def test_the_default_heads_plan_key_is_unchanged(monkeypatch):
    eng = _bare_engine(monkeypatch)
    eng.use_plan = True
    imgs, labels = torch.zeros(2, 4, 3, 8, 8), torch.zeros(2, 1, dtype=torch.int64)
    key = eng._plan_key(imgs, labels)
    # shapes, dtype, device, stream, ddp, dropout, requires_grad, switches, blending, eps, soft labels -- and nothing behind them
    assert len(key) == 12 and key[-3:] == (False, 0.0, False) and not any(isinstance(k, tuple) and k[:1] == ("bce",) for k in key)
    pw = torch.ones(5)
    eng.bce = (pw, float("nan"), 0)
    with_bce = eng._plan_key(imgs, labels)
    assert with_bce[:-1] == key and with_bce[-1] == ("bce", pw.data_ptr(), "nan", 0)
    assert with_bce == eng._plan_key(imgs, labels)              # a NaN threshold does not make the key unequal to itself
    eng.bce = (None, 0.2, 1)
    assert eng._plan_key(imgs, labels)[-1] == ("bce", 0, "0.2", 1)


def test_label_kinds_under_bce_and_the_blending_refusal(monkeypatch):
    eng = _bare_engine(monkeypatch, bce=(None, float("nan"), 0))
    imgs = torch.zeros(2, 4, 3, 8, 8)
    hot = torch.tensor([[1, 0, 1, 0, 0], [0, 0, 0, 0, 1]])
    assert eng._soft_labels(imgs, hot.float()) and eng._soft_labels(imgs, hot.bool()) and eng._soft_labels(imgs, hot.to(torch.uint8))
    assert not eng._soft_labels(imgs, torch.zeros(2, 1, dtype=torch.int64)) and not eng._soft_labels(imgs, hot)        # int64: class indices
    assert eng._uses_soft_head(torch.zeros(2, dtype=torch.int64))           # under BCE the head always takes the target-matrix path
    for blending, eps in ((object(), 0.0), (None, 0.1)):
        eng.blending, eng.label_smooth_eps = blending, eps
        for lab in (hot.float(), hot.bool()):
            with pytest.raises(ValueError, match="soft .* labels are taken as they are"):
                eng._step_tensors(imgs, lab)
    # without the BCE head a bool / uint8 matrix is no label matrix, as before
    plain = _bare_engine(monkeypatch)
    assert not plain._soft_labels(imgs, hot.bool()) and plain._soft_labels(imgs, hot.float()) and not plain._uses_soft_head(torch.zeros(2, dtype=torch.int64))
