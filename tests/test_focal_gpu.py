"""GPU: the focal / asymmetric sigmoid losses -- mvf_focal_loss / mvf_head_train_fwd_focal (csrc/focal.hip, csrc/head.hip) against the fp64 restatement in
focal_numpy.py, and the train engine with a focal head: multi-hot labels, integer labels through mvf_soft_targets (smoothing, Mixup), launch plans,
distillation behind it, and the plans of the default and the BCE head.

Bounds are the suite's own for the head's loss and gradient (test_head_optimizer_gpu.py: LOSS_BOUND for loss_part / loss, HEAD_BOUND for dscores): the
kernels compute in fp64 and round once, so they owe nothing more than the fp32 head in front of them.

End-to-end shapes: ResNet-50, T = 4, 2 clips of 32 x 32, 10 classes, synthetic weights."""
import ctypes as C

import numpy as np
import pytest
import torch

import blend_numpy as BN
import distill_numpy as dn
import focal_numpy as fn
from helpers import rel_err
from mvfnet_amd import synth
from test_head_optimizer_gpu import HEAD_BOUND, HEAD_CASES, LOSS_BOUND, close, head_inputs

pytestmark = pytest.mark.gpu

P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)  # noqa: E731
F32, BF16 = torch.float32, torch.bfloat16
NAN = float("nan")
CLASSES = 10
# (gamma+, gamma-, margin, alpha; None = off): BCE, focal, asymmetric, asymmetric without the positive exponent, the margin alone, everything at once
SETTINGS = [(0.0, 0.0, 0.0, None), (2.0, 2.0, 0.0, 0.25), (1.0, 4.0, 0.05, None), (0.0, 4.0, 0.05, None), (0.0, 0.0, 0.05, None), (3.0, 1.5, 0.2, 0.75)]
IDS = ["bce", "focal", "asl", "asl_g0", "margin", "all"]


def _lib():
    from mvfnet_amd import _lib as L
    return L.lib, L.check


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _prm(gp=0.0, gn=0.0, m=0.0, alpha=None, thr=NAN, sum_classes=0):
    from mvfnet_amd._lib import FocalParams
    return FocalParams(gamma_pos=gp, gamma_neg=gn, margin=m, alpha=-1.0 if alpha is None else alpha, target_threshold=thr, sum_classes=sum_classes)


# ------------------------------------------------------------------------------------------------ 1. the kernel against fp64
def _kernel(s, t, prm, cw=None, with_dscores=True):
    """One mvf_focal_loss call on copies of the host arrays; every output starts as NaN.  -> rc, dict of host arrays."""
    lib, _ = _lib()
    dev = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda() if v is not None else None  # noqa: E731
    s_d, t_d, cw_d = dev(s), dev(t), dev(cw)
    dsc_d, part_d, loss_d = torch.full(s.shape, NAN, device="cuda"), torch.full((s.shape[0],), NAN, device="cuda"), torch.full((1,), NAN, device="cuda")
    rc = lib.mvf_focal_loss(P(s_d), P(t_d), s.shape[0], s.shape[1], P(cw_d), prm, P(dsc_d) if with_dscores else None, P(part_d), P(loss_d), _stream())
    torch.cuda.synchronize()
    return rc, dict(dscores=dsc_d.cpu().numpy(), loss_part=part_d.cpu().numpy(), loss=loss_d.cpu().numpy())


def _inputs(clips, classes, seed=0):
    """Scores 6 * N(0, 1) with 0, +-40, +-100 planted; soft targets (most small, a fifth exactly 1), hard targets, a class weight."""
    gen = np.random.default_rng((clips * 1009 + classes) * 31 + seed)
    s = (gen.standard_normal((clips, classes)) * 6).astype(np.float32)
    flat, planted = s.reshape(-1), np.array([0.0, 40.0, -40.0, 100.0, -100.0], dtype=np.float32)
    at = gen.permutation(flat.size)[:5]
    flat[at] = planted[:at.size]
    soft = (gen.random((clips, classes)) ** 3).astype(np.float32)
    soft[gen.random((clips, classes)) < 0.2] = 1.0
    hard = (gen.random((clips, classes)) < 0.3).astype(np.float32)
    cw = (gen.random(classes) * 4 + 0.25).astype(np.float32)
    return s, soft, hard, cw


@pytest.mark.parametrize("setting", SETTINGS, ids=IDS)
def test_kernel_vs_fp64(setting):
    """1 / 5 / 64 / 65 / 157 / 400 classes: below a wavefront, exactly one, one lane into the second, and 400: some of the 256 threads take a second element;
    1 / 3 / 12 clips.  Hard, soft and thresholded targets, the class weight on and off, both reductions.
    Worst errors observed on an MI355X over the whole grid -- the fp32 rounding of the outputs, nothing else: loss_part 5.7e-8, loss 9.3e-8 (bound 1e-5),
    dscores 5.7e-8 (bound 5e-5); each run prints its own."""
    gp, gn, m, alpha = setting
    worst = dict(loss_part=0.0, loss=0.0, dscores=0.0)
    for clips in (1, 3, 12):
        for classes in (1, 5, 64, 65, 157, 400):
            s, soft, hard, cw = _inputs(clips, classes)
            for t, thr in ((hard, NAN), (soft, NAN), (soft, 0.3)):
                for weight in (None, cw):
                    for sum_classes in (0, 1):
                        rc, got = _kernel(s, t, _prm(gp, gn, m, alpha, thr, sum_classes), weight)
                        assert rc == 0
                        ref = fn.focal_loss(s, t, gp, gn, m, alpha, weight, thr, bool(sum_classes), raw=True)
                        what = "clips=%d classes=%d cw=%s thr=%g sum=%d " % (clips, classes, weight is not None, thr, sum_classes)
                        close(got["loss_part"], ref["loss_part"], LOSS_BOUND, what + "loss_part")
                        close(got["loss"], np.array([ref["loss"]]), LOSS_BOUND, what + "loss")
                        close(got["dscores"], ref["dscores"], HEAD_BOUND, what + "dscores")
                        for k in worst:
                            worst[k] = max(worst[k], rel_err(got[k], np.asarray(ref[k]).reshape(got[k].shape)))
    print("setting %s worst rel_err: loss_part %.3g loss %.3g (bound %g), dscores %.3g (bound %g)" %
          (setting, worst["loss_part"], worst["loss"], LOSS_BOUND, worst["dscores"], HEAD_BOUND))


def test_kernel_exact_cases():
    one, zero = np.ones((1, 1), dtype=np.float32), np.zeros((1, 1), dtype=np.float32)
    # s = 0, t = 1, gamma = 2: 0.25 ln 2, gradient 0.25 * (2 * 0.5 * -ln 2 - 0.5)
    rc, got = _kernel(zero, one, _prm(2.0, 2.0))
    assert rc == 0 and got["loss"][0] == np.float32(0.25 * np.log(2.0)) and got["loss_part"][0] == got["loss"][0]
    assert got["dscores"][0, 0] == np.float32(0.25 * (-np.log(2.0) - 0.5))
    # p = 0.5 is not above the margin 0.5: loss and gradient exactly 0
    rc, got = _kernel(zero, zero, _prm(1.0, 4.0, 0.5))
    assert rc == 0 and got["loss"][0] == 0.0 and got["loss_part"][0] == 0.0 and got["dscores"][0, 0] == 0.0
    rc, got = _kernel(np.full((1, 1), -100.0, dtype=np.float32), one, _prm())
    assert rc == 0 and got["loss"][0] == 100.0
    # one class, any score: the restatement's bits (one element, no sum to reorder)
    s, soft, hard, cw = _inputs(12, 1)
    rc, got = _kernel(s, soft, _prm(1.0, 4.0, 0.05), cw)
    ref = fn.focal_loss(s, soft, 1.0, 4.0, 0.05, None, cw)
    assert rc == 0 and np.array_equal(got["loss_part"], ref["loss_part"]) and np.array_equal(got["dscores"], ref["dscores"])
    # two runs: identical bits; dscores == NULL: the same loss_part and loss
    s, soft, hard, cw = _inputs(12, 400)
    prm = _prm(3.0, 1.5, 0.2, 0.75, 0.3, 1)
    rc, a = _kernel(s, soft, prm, cw)
    rc2, b = _kernel(s, soft, prm, cw)
    assert rc == 0 and rc2 == 0 and all(np.array_equal(a[k], b[k]) for k in a) and np.isfinite(a["dscores"]).all()
    rc, bare = _kernel(s, soft, prm, cw, with_dscores=False)
    assert rc == 0 and np.array_equal(bare["loss_part"], a["loss_part"]) and np.array_equal(bare["loss"], a["loss"]) and np.isnan(bare["dscores"]).all()
    # the threshold on equals hard targets handed in
    rc, hd = _kernel(s, (soft > np.float32(0.3)).astype(np.float32), _prm(3.0, 1.5, 0.2, 0.75, NAN, 1), cw)
    assert rc == 0 and all(np.array_equal(a[k], hd[k]) for k in a)
    # without focusing it is mvf_bce_loss (another order of the same terms: the suite's bound, not bits)
    lib, _ = _lib()
    s_d, t_d = torch.from_numpy(s).cuda(), torch.from_numpy(soft).cuda()
    dsc, part, loss = torch.empty_like(s_d), torch.empty(12, device="cuda"), torch.empty(1, device="cuda")
    assert lib.mvf_bce_loss(P(s_d), P(t_d), 12, 400, None, C.c_float(NAN), 0, P(dsc), P(part), P(loss), _stream()) == 0
    rc, plain = _kernel(s, soft, _prm())
    close(plain["loss_part"], part.cpu().numpy(), LOSS_BOUND, "bce loss_part")
    close(plain["dscores"], dsc.cpu().numpy(), HEAD_BOUND, "bce dscores")
    # finite scores at the end of the fp32 range stay finite
    big = np.array([[3e38, -3e38, 800.0, -800.0]], dtype=np.float32)
    for gp, gn, m, alpha in SETTINGS:
        for t in (0.0, 1.0):
            rc, got = _kernel(big, np.full_like(big, t), _prm(gp, gn, m, alpha))
            assert rc == 0 and np.isfinite(got["loss_part"]).all() and np.isfinite(got["dscores"]).all()


def test_kernel_refusals_touch_nothing_and_nan_propagates():
    lib, _ = _lib()
    inf = float("inf")
    clips, classes = 3, 10
    t = {k: torch.full(shape, NAN, device="cuda") for k, shape in (("s", (clips, classes)), ("t", (clips, classes)), ("dsc", (clips, classes)), ("part", (clips,)),
                                                                    ("loss", (1,)))}

    def call(s="s", tg="t", n=clips, k=classes, prm=None, dsc="dsc", part="part", loss="loss", null_prm=False):
        p = lambda name: P(t[name]) if name else None  # noqa: E731
        return lib.mvf_focal_loss(p(s), p(tg), n, k, None, None if null_prm else (prm or _prm(2.0, 2.0)), p(dsc), p(part), p(loss), _stream())
    cases = [dict(s=None), dict(tg=None), dict(part=None), dict(loss=None), dict(null_prm=True), dict(n=0), dict(n=-2), dict(k=0), dict(k=-1)]
    cases += [dict(prm=_prm(**kw)) for kw in (dict(gp=0.5), dict(gp=17.0), dict(gp=NAN), dict(gn=-1.0), dict(gn=0.99), dict(gn=inf), dict(m=-0.1), dict(m=1.0), dict(m=NAN),
                                              dict(alpha=NAN), dict(alpha=1.01), dict(thr=inf), dict(thr=-inf), dict(sum_classes=2), dict(sum_classes=-1))]
    for kw in cases:
        assert call(**kw) == -1, (kw, lib.mvf_last_error())                  # MVF_EINVAL
        assert b"focal_loss" in lib.mvf_last_error()
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(v).all()) for v in t.values())
    # the ends of the accepted ranges are accepted
    s, soft, hard, cw = _inputs(3, 10)
    for kw in (dict(gp=1.0, gn=16.0), dict(gp=16.0, gn=1.0), dict(m=0.999), dict(alpha=0.0), dict(alpha=1.0)):
        assert _kernel(s, soft, _prm(**kw))[0] == 0, kw
    # a NaN score reaches its clip's loss_part, its own gradient element and the loss, and no other clip -- for either target, with and without exponents
    for prm in (_prm(), _prm(2.0, 2.0, 0.0, 0.25), _prm(1.0, 4.0, 0.05), _prm(0.0, 4.0, 0.05)):
        for tg in (soft, hard, np.zeros_like(soft), np.ones_like(soft)):
            s2 = s.copy()
            s2[1, 3] = NAN
            rc, got = _kernel(s2, tg, prm, cw)
            assert rc == 0 and np.isnan(got["loss_part"][1]) and np.isnan(got["dscores"][1, 3]) and np.isnan(got["loss"][0])
            assert np.isfinite(got["loss_part"][[0, 2]]).all() and np.isfinite(got["dscores"][[0, 2]]).all()
            assert np.isfinite(np.delete(got["dscores"][1], 3)).all()
    # a non-finite class_weight entry reaches every clip
    for bad in (NAN, inf, -inf):
        cw2 = cw.copy()
        cw2[4] = bad
        for tg in (soft, np.zeros_like(soft)):
            rc, got = _kernel(s, tg, _prm(1.0, 4.0, 0.05), cw2)
            assert rc == 0 and np.isnan(got["loss_part"]).all() and np.isnan(got["loss"][0])


# ------------------------------------------------------------------------------------------------ 2. the head call
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_head_train_fwd_focal_equals_soft_head_then_focal_loss(dtype):
    """pooled / scores are mvf_head_train_fwd_soft's bits (the same two launches); dscores / loss_part / loss are mvf_focal_loss's bits on those scores."""
    lib, check = _lib()
    inp = head_inputs(HEAD_CASES["k174_per7_c260"], dtype, 0.5)
    clips, T, hw, c, classes = inp["case"]
    dev, dt = "cuda", 0 if dtype == F32 else 1
    fg, wg, bg, mg = inp["feat"].to(dev, dtype).contiguous(), inp["w"].to(dev), inp["b"].to(dev), inp["mask"].to(dev)
    gen = torch.Generator().manual_seed(5)
    tg = (torch.rand(clips, classes, generator=gen) < 0.1).float().to(dev)
    cw = (torch.rand(classes, generator=gen) * 3 + 0.5).to(dev)
    prm = _prm(1.0, 4.0, 0.05, None, 0.5, 1)

    def outs():
        return [torch.full(s_, NAN, device=dev) for s_ in ((clips * T, c), (clips, classes), (clips, classes), (clips,), (1,))]
    a, b, k = outs(), outs(), outs()
    check(lib.mvf_head_train_fwd_soft(P(fg), clips, T, hw, c, P(wg), P(bg), classes, P(tg), P(mg), *[P(v) for v in a], dt, None), "head_train_fwd_soft")
    check(lib.mvf_head_train_fwd_focal(P(fg), clips, T, hw, c, P(wg), P(bg), classes, P(tg), P(mg), P(cw), prm, *[P(v) for v in b], dt, None),
          "head_train_fwd_focal")
    check(lib.mvf_focal_loss(P(b[1]), P(tg), clips, classes, P(cw), prm, P(k[2]), P(k[3]), P(k[4]), None), "focal_loss")
    torch.cuda.synchronize()
    assert torch.isfinite(b[0]).all() and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert all(torch.isfinite(b[i]).all() and torch.equal(b[i], k[i]) for i in (2, 3, 4))
    assert not torch.equal(a[4], b[4])                                      # another loss than the soft-target cross-entropy
    ref = fn.focal_loss(b[1].cpu().numpy(), tg.cpu().numpy(), 1.0, 4.0, 0.05, None, cw.cpu().numpy(), 0.5, True, raw=True)
    close(b[4].cpu().numpy(), np.array([ref["loss"]]), LOSS_BOUND, "loss")
    close(b[2].cpu().numpy(), ref["dscores"], HEAD_BOUND, "dscores")
    # a refusal of the loss's settings enqueues nothing: pooled and scores stay untouched
    c2 = outs()
    assert lib.mvf_head_train_fwd_focal(P(fg), clips, T, hw, c, P(wg), P(bg), classes, P(tg), P(mg), P(cw), _prm(0.5, 4.0), *[P(v) for v in c2], dt, None) == -1
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(v).all()) for v in c2)


# ------------------------------------------------------------------------------------------------ 3. the train engine
_VALS = {}
CW = tuple(float(v) for v in np.linspace(0.5, 3.0, CLASSES).astype(np.float32))
FOCAL = dict(type="SigmoidFocalLoss", gamma=2.0, alpha=0.25, class_weight=CW)
ASL = dict(type="AsymmetricLossMultiLabel", class_weight=CW)
FOCAL_KW = dict(gamma_pos=2.0, gamma_neg=2.0, margin=0.0, alpha=0.25, class_weight=CW)
ASL_KW = dict(gamma_pos=1.0, gamma_neg=4.0, margin=0.05, alpha=None, class_weight=CW)


def _model(seed=0, dropout=0.0, loss_cls=None, train_cfg=None):
    import mvfnet_amd
    cfg = mvfnet_amd.mvfnet_config(50, 4, num_classes=CLASSES, dropout_ratio=dropout)
    if loss_cls is not None:
        cfg["cls_head"]["loss_cls"] = loss_cls
    m = mvfnet_amd.build_recognizer(cfg, train_cfg, dict(average_clips=None))
    sd = m.state_dict()
    if seed not in _VALS:
        _VALS[seed] = synth.synth_state_dict({"r50/" + k: tuple(v.shape) for k, v in sd.items()}, seed=seed)
    m.load_state_dict({k: torch.from_numpy(_VALS[seed]["r50/" + k]) for k in sd})
    return m.cuda()


def _engine(dtype, loss_cls=FOCAL, use_plan=False, dropout=0.0):
    m = _model(0, dropout, loss_cls).train()
    eng = m.train_engine(dtype=dtype)
    eng.use_plan = use_plan
    return m, eng


def _clips(b=2, seed=3):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    imgs = torch.randn(b, 4, 3, 32, 32, device="cuda", generator=gen)
    hot = torch.rand(b, CLASSES, device="cuda", generator=gen) < 0.3
    hot[:, 1] = True
    return imgs, hot, torch.randint(0, CLASSES, (b, 1), device="cuda", generator=gen)


def _check_focal(saved, loss, targets, kw, **more):
    ref = fn.focal_loss(saved["scores"], targets, raw=True, **kw, **more)
    close(np.array([loss]), np.array([ref["loss"]]), LOSS_BOUND, "loss")
    close(saved["dscores"], ref["dscores"], HEAD_BOUND, "dscores")
    return ref


@pytest.mark.parametrize("loss_cls,kw", [(FOCAL, FOCAL_KW), (ASL, ASL_KW)], ids=["focal", "asl"])
def test_engine_step_from_multi_hot_labels(loss_cls, kw):
    imgs, hot, _ = _clips()
    m, eng = _engine(BF16, loss_cls)
    assert eng.bce is None and eng.focal is not None and eng.focal[0].tolist() == list(CW) and eng.focal[1] is m.cls_head.focal_settings(eng.device)[1]
    loss = eng.forward(imgs, hot.float())
    saved = {k: eng.saved[k].cpu().numpy().copy() for k in ("scores", "dscores")}
    eng.backward()
    torch.cuda.synchronize()
    assert torch.isfinite(eng.flat_grads).all() and eng.flat_grads.abs().max() > 0
    _check_focal(saved, float(loss), hot.float().cpu().numpy(), kw)
    # the model API takes the bool matrix, uint8 through the engine alone, the head's own loss() serves the eval path: the same loss bits
    m2 = _model(0, 0.0, loss_cls).train()
    m2.train_engine(dtype=BF16)
    out = m2(imgs, hot)["loss_cls"]
    m3, eng3 = _engine(BF16, loss_cls)
    l3 = eng3.forward(imgs, hot.to(torch.uint8))
    eng3.backward()
    eager = m2.cls_head.loss(torch.from_numpy(saved["scores"]).cuda(), hot)["loss_cls"]
    torch.cuda.synchronize()
    assert float(out) == float(loss) and float(l3) == float(loss) and float(eager) == float(loss)
    assert "soft_targets" not in [k[0] for k in eng._bufs]                  # a caller's matrix is taken as it is


def test_cb_focal_loss_is_the_focal_loss_with_the_derived_weight():
    from mvfnet_amd.heads import class_balanced_weights
    n = [3, 10, 10000, 500, 1, 70, 70, 2000, 5, 40]
    imgs, hot, _ = _clips()
    m, eng = _engine(F32, dict(type="CBFocalLoss", samples_per_cls=n, beta=0.999, gamma=1.0))
    w = class_balanced_weights(n, 0.999)
    assert np.array_equal(eng.focal[0].cpu().numpy(), w.astype(np.float32))
    loss = eng.forward(imgs, hot.float())
    saved = {k: eng.saved[k].cpu().numpy().copy() for k in ("scores", "dscores")}
    eng.backward()
    torch.cuda.synchronize()
    _check_focal(saved, float(loss), hot.float().cpu().numpy(), dict(gamma_pos=1.0, gamma_neg=1.0, class_weight=w.astype(np.float32)))


def test_replayed_focal_plan_equals_eager_steps_bit_for_bit():
    gen = torch.Generator(device="cuda").manual_seed(13)
    imgs = [torch.randn(2, 4, 3, 32, 32, device="cuda", generator=gen) for _ in range(2)]
    hots = [(torch.rand(2, CLASSES, device="cuda", generator=gen) < 0.4).to(torch.uint8) for _ in range(3)]
    out = {}
    for use_plan in (True, False):
        torch.manual_seed(7)
        m, eng = _engine(BF16, ASL, use_plan=use_plan, dropout=0.5)
        losses = [eng.train_step(imgs[i % 2].clone(), hots[i % 3].clone(), lr=0.01).clone() for i in range(7)]
        torch.cuda.synchronize()
        out[use_plan] = (eng, torch.cat(losses), eng.flat_params.clone())
    eng_p = out[True][0]
    st = list(eng_p._plans.values())
    assert len(st) == 1 and st[0]["plan"] is not None and st[0]["tries"] == 2, [(s_["eager"], s_["tries"]) for s_ in st]
    plan = st[0]["plan"]
    assert "mvf_head_train_fwd_focal" in plan.names and not any(n in plan.names for n in ("mvf_head_train_fwd_bce", "mvf_head_train_fwd_soft", "mvf_soft_targets"))
    assert any(v is eng_p.focal[1] for v in plan.keep)                     # the plan keeps the struct whose address it recorded
    key = [k for k in list(eng_p._plans)[0] if isinstance(k, tuple) and k[:1] == ("focal",)]
    assert len(key) == 1 and key[0][2] == C.addressof(eng_p.focal[1])
    assert len(plan.slots["labels"]) == 1 and not getattr(out[False][0], "_plans", None)
    assert torch.isfinite(out[True][1]).all() and len(set(out[True][1].tolist())) > 3
    assert torch.equal(out[True][1], out[False][1]) and torch.equal(out[True][2], out[False][2])


def test_integer_labels_smoothing_and_mixup_go_through_soft_targets():
    from mvfnet_amd.blending import MixupBlending
    imgs, _, labels = _clips(3)
    m, eng = _engine(BF16, dict(FOCAL, target_threshold=0.2))
    eng.blending, eng.label_smooth_eps = MixupBlending(alpha=0.8, seed=5), 0.1
    loss = eng.forward(imgs, labels)
    saved = {k: eng.saved[k].cpu().numpy().copy() for k in ("scores", "dscores")}
    rows, wts = (v.cpu().numpy() for v in eng._blend_table)
    targets = eng._bufs[("soft_targets", (3, CLASSES), F32)].cpu().numpy().copy()
    eng.backward()
    torch.cuda.synchronize()
    want = BN.soft_targets_ref(labels.cpu().numpy(), rows, wts, CLASSES, 0.1, np.float64)
    assert np.abs(targets - want).max() <= 2.0 ** -22 and 0 < (targets > 0.2).sum() < targets.size
    _check_focal(saved, float(loss), targets, FOCAL_KW, target_threshold=0.2)
    # soft (unthresholded) Mixup targets: the loss is linear in them
    m2, eng2 = _engine(BF16, ASL)
    eng2.blending, eng2.label_smooth_eps = MixupBlending(alpha=0.8, seed=5), 0.1
    loss2 = eng2.forward(imgs, labels)
    saved2 = {k: eng2.saved[k].cpu().numpy().copy() for k in ("scores", "dscores")}
    targets2 = eng2._bufs[("soft_targets", (3, CLASSES), F32)].cpu().numpy().copy()
    eng2.backward()
    torch.cuda.synchronize()
    assert np.array_equal(targets2, targets) and torch.isfinite(eng2.flat_grads).all()
    _check_focal(saved2, float(loss2), targets2, ASL_KW)
    # a caller's matrix with blending or smoothing stays refused
    with pytest.raises(ValueError, match="taken as they are"):
        eng.forward(imgs, torch.zeros(3, CLASSES, device="cuda"))


def test_distillation_composes_behind_the_focal_head():
    from mvfnet_amd.distill import KnowledgeDistillation
    imgs, hot, _ = _clips()
    teacher = _model(seed=1).eval()
    T, alpha = 4.0, 0.5
    m, eng = _engine(BF16, ASL)
    eng.distill = KnowledgeDistillation(teacher, temperature=T, alpha=alpha)
    loss = eng.forward(imgs, hot.float())
    saved = {k: eng.saved[k].cpu().numpy().copy() for k in ("scores", "dscores", "teacher_scores")}
    eng.backward()
    torch.cuda.synchronize()
    terms = eng.distill_terms()
    fl = fn.focal_loss(saved["scores"], hot.float().cpu().numpy(), raw=True, **ASL_KW)
    ref = dn.distill_loss(saved["scores"], saved["teacher_scores"], T, alpha, fl["dscores"], fl["loss_part"], raw=True)
    close(np.array([float(loss)]), np.array([ref["loss"]]), LOSS_BOUND, "loss")
    close(saved["dscores"], ref["dscores"], HEAD_BOUND, "dscores")
    close(np.array([terms["loss_ce"], terms["loss_kd"]]), ref["terms"], LOSS_BOUND, "terms")
    close(np.array([terms["loss_ce"]]), np.array([fl["loss"]]), LOSS_BOUND, "loss_ce is the asymmetric term")
    assert ref["terms"][1] > 0.0 and torch.isfinite(eng.flat_grads).all()


def test_the_default_and_the_bce_loss_record_the_plans_they_always_did():
    """The default head's plan holds mvf_head_train_fwd, the BCE head's mvf_head_train_fwd_bce, neither any of the new entry points or a 'focal' entry in its
    key; the focal head swaps that one call for mvf_head_train_fwd_focal (multi-hot labels: the same op count) and adds mvf_soft_targets for integer labels."""
    imgs, hot, labels = _clips()
    new = ("mvf_head_train_fwd_focal", "mvf_focal_loss")
    m, eng = _engine(BF16, loss_cls=None, use_plan=True)
    assert eng.bce is None and eng.focal is None
    for _ in range(5):
        eng.train_step(imgs, labels)
    plain = [s["plan"] for s in eng._plans.values()]
    assert len(plain) == 1 and plain[0] is not None
    names = list(plain[0].names)
    assert names.count("mvf_head_train_fwd") == 1 and not any(n in names for n in new + ("mvf_head_train_fwd_bce", "mvf_soft_targets", "mvf_head_train_fwd_soft"))
    assert all(len(key) == 12 for key in eng._plans)                        # the key of the default loss ends with the soft-label flag, as it did
    mb, engb = _engine(BF16, dict(type="BCELossWithLogits", pos_weight=CW), use_plan=True)
    assert engb.focal is None
    for _ in range(5):
        engb.train_step(imgs, hot.float())
    bce = [s["plan"] for s in engb._plans.values()]
    assert len(bce) == 1 and bce[0] is not None and bce[0].n_ops == plain[0].n_ops
    assert list(bce[0].names) == ["mvf_head_train_fwd_bce" if n == "mvf_head_train_fwd" else n for n in names]
    assert all(len(key) == 13 and key[-1][0] == "bce" for key in engb._plans)
    mf, engf = _engine(BF16, FOCAL, use_plan=True)
    for _ in range(5):
        engf.train_step(imgs, hot.float())
    for _ in range(5):
        engf.train_step(imgs, labels)
    torch.cuda.synchronize()
    plans = sorted((s["plan"] for s in engf._plans.values()), key=lambda p: p.n_ops)
    assert len(plans) == 2 and all(p is not None for p in plans)
    print("plan ops: default %d, bce %d, focal multi-hot %d, focal integer labels %d" % (plain[0].n_ops, bce[0].n_ops, plans[0].n_ops, plans[1].n_ops))
    assert [p.n_ops for p in plans] == [plain[0].n_ops, plain[0].n_ops + 1]
    swapped = ["mvf_head_train_fwd_focal" if n == "mvf_head_train_fwd" else n for n in names]
    assert list(plans[0].names) == swapped and [n for n in plans[1].names if n != "mvf_soft_targets"] == swapped
    assert all(len(key) == 13 and key[-1][0] == "focal" for key in engf._plans) and torch.isfinite(engf.flat_params).all()
