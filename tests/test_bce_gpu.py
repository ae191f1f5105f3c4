"""GPU: the binary cross-entropy head -- mvf_bce_loss / mvf_head_train_fwd_bce (csrc/bce.hip, csrc/head.hip) and mvf_average_clip_sigmoid
(csrc/head.hip) against the fp64 restatement in bce_numpy.py, and the train engine with a BCE head: multi-hot labels, integer labels through
mvf_soft_targets (smoothing, Mixup), launch plans, distillation behind it, and the default head's plan.

Bounds are the suite's own for the head's loss and gradient (test_head_optimizer_gpu.py: LOSS_BOUND for loss_part / loss, HEAD_BOUND for dscores,
INFER_BOUND for the averaged scores): the kernels compute in fp64 and round once, so they owe nothing more than the fp32 head in front of them.

End-to-end shapes: ResNet-50, T = 4, 2 clips of 32 x 32, 10 classes, synthetic weights."""
import ctypes as C

import numpy as np
import pytest
import torch

import bce_numpy as bn
import blend_numpy as BN
import distill_numpy as dn
from helpers import rel_err
from mvfnet_amd import synth
from test_head_optimizer_gpu import HEAD_BOUND, HEAD_CASES, INFER_BOUND, LOSS_BOUND, close, head_inputs

pytestmark = pytest.mark.gpu

P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)  # noqa: E731
F32, BF16 = torch.float32, torch.bfloat16
NAN = float("nan")
CLASSES = 10


def _lib():
    from mvfnet_amd import _lib as L
    return L.lib, L.check


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------------------------------------ 1. the kernel against fp64
def _kernel(s, t, pw=None, thr=NAN, sum_classes=0, with_dscores=True):
    """One mvf_bce_loss call on copies of the host arrays; every output starts as NaN.  -> rc, dict of host arrays."""
    lib, _ = _lib()
    dev = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda() if v is not None else None  # noqa: E731
    s_d, t_d, pw_d = dev(s), dev(t), dev(pw)
    dsc_d, part_d, loss_d = torch.full(s.shape, NAN, device="cuda"), torch.full((s.shape[0],), NAN, device="cuda"), torch.full((1,), NAN, device="cuda")
    rc = lib.mvf_bce_loss(P(s_d), P(t_d), s.shape[0], s.shape[1], P(pw_d), C.c_float(thr), sum_classes, P(dsc_d) if with_dscores else None, P(part_d), P(loss_d),
                          _stream())
    torch.cuda.synchronize()
    return rc, dict(dscores=dsc_d.cpu().numpy(), loss_part=part_d.cpu().numpy(), loss=loss_d.cpu().numpy())


def _inputs(clips, classes, scale, seed=0):
    gen = np.random.default_rng((clips * 1009 + classes) * 31 + int(scale) + seed)
    s = (gen.standard_normal((clips, classes)) * scale).astype(np.float32)
    t = (gen.random((clips, classes)) ** 3).astype(np.float32)               # soft targets in [0, 1), most of them small
    t[gen.random((clips, classes)) < 0.2] = 1.0                              # and hard positives among them
    pw = (gen.random(classes) * 4 + 0.25).astype(np.float32)
    return s, t, pw


@pytest.mark.parametrize("classes", [1, 10, 257, 400, 1000])
def test_kernel_vs_fp64(classes):
    """257 / 400 / 1000 classes: one thread of the 256 takes a second element, some do, all take three or four; 7 clips: the mean's lanes are not all
    used.  At scale 200 exp(-|s|) underflows in fp32 and not in fp64.  pos_weight on and off, the threshold on and off, both reductions.
    Worst errors observed on an MI355X over the whole grid -- the fp32 rounding of the outputs, nothing else: loss_part 5.7e-8, loss 6.5e-8 (bound 1e-5),
    dscores 5.8e-8 (bound 5e-5); each run prints its own."""
    worst = dict(loss_part=0.0, loss=0.0, dscores=0.0)
    for clips in (1, 7):
        for scale in (1, 40, 200):
            s, t, pw = _inputs(clips, classes, scale)
            for weight in (None, pw):
                for thr in (NAN, 0.3):
                    for sum_classes in (0, 1):
                        rc, got = _kernel(s, t, weight, thr, sum_classes)
                        assert rc == 0
                        ref = bn.bce_loss(s, t, weight, thr, bool(sum_classes), raw=True)
                        what = "clips=%d classes=%d scale=%g pw=%s thr=%g sum=%d " % (clips, classes, scale, weight is not None, thr, sum_classes)
                        close(got["loss_part"], ref["loss_part"], LOSS_BOUND, what + "loss_part")
                        close(got["loss"], np.array([ref["loss"]]), LOSS_BOUND, what + "loss")
                        close(got["dscores"], ref["dscores"], HEAD_BOUND, what + "dscores")
                        for k in worst:
                            worst[k] = max(worst[k], rel_err(got[k], np.asarray(ref[k]).reshape(got[k].shape)))
    print("classes=%d worst rel_err: loss_part %.3g loss %.3g (bound %g), dscores %.3g (bound %g)" %
          (classes, worst["loss_part"], worst["loss"], LOSS_BOUND, worst["dscores"], HEAD_BOUND))


def test_kernel_exact_cases():
    log2 = np.float32(np.log(2.0))
    for classes in (1, 257):
        z = np.zeros((7, classes), dtype=np.float32)
        for t in (0.0, 1.0):
            rc, got = _kernel(z, np.full_like(z, t))
            assert rc == 0 and (got["loss_part"] == log2).all() and got["loss"][0] == log2
            assert np.array_equal(got["dscores"], np.full_like(z, np.float32((0.5 - t) / (7.0 * classes))))
    # one class, any score: the restatement's bits (one element, no sum to reorder)
    s, t, pw = _inputs(7, 1, 40)
    rc, got = _kernel(s, t, pw, NAN, 0)
    ref = bn.bce_loss(s, t, pw)
    assert rc == 0 and np.array_equal(got["loss_part"], ref["loss_part"]) and np.array_equal(got["dscores"], ref["dscores"])
    # two runs: identical bits; dscores == NULL: the same loss_part and loss
    s, t, pw = _inputs(7, 1000, 40)
    rc, a = _kernel(s, t, pw, 0.3, 1)
    rc2, b = _kernel(s, t, pw, 0.3, 1)
    assert rc == 0 and rc2 == 0 and all(np.array_equal(a[k], b[k]) for k in a) and np.isfinite(a["dscores"]).all()
    rc, bare = _kernel(s, t, pw, 0.3, 1, with_dscores=False)
    assert rc == 0 and np.array_equal(bare["loss_part"], a["loss_part"]) and np.array_equal(bare["loss"], a["loss"]) and np.isnan(bare["dscores"]).all()
    # the threshold on equals hard targets handed in; sum_classes = classes x the mean over the classes
    rc, hard = _kernel(s, (t > np.float32(0.3)).astype(np.float32), pw, NAN, 1)
    assert rc == 0 and all(np.array_equal(a[k], hard[k]) for k in a)
    rc, mean = _kernel(s, t, pw, 0.3, 0)
    close(a["loss"], mean["loss"].astype(np.float64) * 1000, LOSS_BOUND, "sum against mean")


def test_kernel_refusals_touch_nothing_and_nan_propagates():
    lib, _ = _lib()
    inf = float("inf")
    clips, classes = 3, 10
    t = {k: torch.full(shape, NAN, device="cuda") for k, shape in (("s", (clips, classes)), ("t", (clips, classes)), ("dsc", (clips, classes)), ("part", (clips,)),
                                                                    ("loss", (1,)))}

    def call(s="s", tg="t", n=clips, k=classes, thr=NAN, sc=0, dsc="dsc", part="part", loss="loss"):
        p = lambda name: P(t[name]) if name else None  # noqa: E731
        return lib.mvf_bce_loss(p(s), p(tg), n, k, None, C.c_float(thr), sc, p(dsc), p(part), p(loss), _stream())
    cases = [dict(s=None), dict(tg=None), dict(part=None), dict(loss=None), dict(n=0), dict(n=-2), dict(k=0), dict(k=-1), dict(thr=inf), dict(thr=-inf),
             dict(sc=2), dict(sc=-1)]
    for kw in cases:
        assert call(**kw) == -1, (kw, lib.mvf_last_error())                  # MVF_EINVAL
        assert b"bce_loss" in lib.mvf_last_error()
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(v).all()) for v in t.values())
    # a NaN score reaches its clip's loss_part, its own gradient element and the loss, and no other clip; a non-finite pos_weight entry reaches every clip
    s, tg, pw = _inputs(3, 10, 1)
    s[1, 3] = NAN
    rc, got = _kernel(s, tg, pw)
    assert rc == 0 and np.isnan(got["loss_part"][1]) and np.isnan(got["dscores"][1, 3]) and np.isnan(got["loss"][0])
    assert np.isfinite(got["loss_part"][[0, 2]]).all() and np.isfinite(got["dscores"][[0, 2]]).all()
    s, tg, pw = _inputs(3, 10, 1)
    tg[:, 4] = 1.0
    for bad in (NAN, inf):
        pw[4] = bad
        rc, got = _kernel(s, tg, pw)
        assert rc == 0 and not np.isfinite(got["loss_part"]).any() and not np.isfinite(got["loss"][0])


# ------------------------------------------------------------------------------------------------ 2. the head call
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_head_train_fwd_bce_equals_soft_head_then_bce_loss(dtype):
    """pooled / scores are mvf_head_train_fwd_soft's bits (the same two launches); dscores / loss_part / loss are mvf_bce_loss's bits on those scores."""
    lib, check = _lib()
    inp = head_inputs(HEAD_CASES["k174_per7_c260"], dtype, 0.5)
    clips, T, hw, c, classes = inp["case"]
    dev, dt = "cuda", 0 if dtype == F32 else 1
    fg, wg, bg, mg = inp["feat"].to(dev, dtype).contiguous(), inp["w"].to(dev), inp["b"].to(dev), inp["mask"].to(dev)
    gen = torch.Generator().manual_seed(5)
    tg = (torch.rand(clips, classes, generator=gen) < 0.1).float().to(dev)
    pw = (torch.rand(classes, generator=gen) * 3 + 0.5).to(dev)

    def outs():
        return [torch.full(s_, NAN, device=dev) for s_ in ((clips * T, c), (clips, classes), (clips, classes), (clips,), (1,))]
    a, b, k = outs(), outs(), outs()
    check(lib.mvf_head_train_fwd_soft(P(fg), clips, T, hw, c, P(wg), P(bg), classes, P(tg), P(mg), *[P(v) for v in a], dt, None), "head_train_fwd_soft")
    check(lib.mvf_head_train_fwd_bce(P(fg), clips, T, hw, c, P(wg), P(bg), classes, P(tg), P(mg), P(pw), C.c_float(0.5), 1, *[P(v) for v in b], dt, None),
          "head_train_fwd_bce")
    check(lib.mvf_bce_loss(P(b[1]), P(tg), clips, classes, P(pw), C.c_float(0.5), 1, P(k[2]), P(k[3]), P(k[4]), None), "bce_loss")
    torch.cuda.synchronize()
    assert torch.isfinite(b[0]).all() and torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert all(torch.isfinite(b[i]).all() and torch.equal(b[i], k[i]) for i in (2, 3, 4))
    assert not torch.equal(a[4], b[4])                                      # another loss than the soft-target cross-entropy
    ref = bn.bce_loss(b[1].cpu().numpy(), tg.cpu().numpy(), pw.cpu().numpy(), 0.5, True, raw=True)
    close(b[4].cpu().numpy(), np.array([ref["loss"]]), LOSS_BOUND, "loss")
    close(b[2].cpu().numpy(), ref["dscores"], HEAD_BOUND, "dscores")


@pytest.mark.parametrize("clips,classes", [(1, 1), (3, 257), (10, 400), (64, 157)])
def test_average_clip_sigmoid_vs_fp64(clips, classes):
    lib, check = _lib()
    gen = np.random.default_rng(clips * 1009 + classes)
    s = (gen.standard_normal((clips, classes)) * 40).astype(np.float32)
    s.flat[::7] *= 20                                                       # |s| up to thousands: exp must not overflow for either sign
    s_d, out = torch.from_numpy(s).cuda(), torch.full((1, classes), NAN, device="cuda")
    check(lib.mvf_average_clip_sigmoid(P(s_d), clips, classes, P(out), _stream()), "average_clip_sigmoid")
    torch.cuda.synchronize()
    close(out.cpu().numpy(), bn.average_clip_sigmoid(s), INFER_BOUND, "sigmoid average")
    from mvfnet_amd.engine import HeadEngine
    eng = HeadEngine(torch.nn.Linear(4, classes).cuda(), torch.device("cuda"))
    assert torch.equal(eng.average(s_d, "sigmoid"), out)


# ------------------------------------------------------------------------------------------------ 3. the train engine
_VALS = {}
PW = tuple(float(v) for v in np.linspace(0.5, 3.0, CLASSES).astype(np.float32))


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


BCE = dict(type="BCELossWithLogits", pos_weight=PW)


def _engine(dtype, loss_cls=BCE, use_plan=False, dropout=0.0):
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


def _check_bce(saved, loss, targets, **kw):
    ref = bn.bce_loss(saved["scores"], targets, PW, raw=True, **kw)
    close(np.array([loss]), np.array([ref["loss"]]), LOSS_BOUND, "loss")
    close(saved["dscores"], ref["dscores"], HEAD_BOUND, "dscores")
    return ref


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_engine_step_from_multi_hot_labels(dtype):
    imgs, hot, _ = _clips()
    m, eng = _engine(dtype)
    assert eng.bce is not None and eng.bce[0].tolist() == list(PW) and np.isnan(eng.bce[1]) and eng.bce[2] == 0
    loss = eng.forward(imgs, hot.float())
    saved = {k: eng.saved[k].cpu().numpy().copy() for k in ("scores", "dscores")}
    eng.backward()
    torch.cuda.synchronize()
    assert torch.isfinite(eng.flat_grads).all() and eng.flat_grads.abs().max() > 0
    _check_bce(saved, float(loss), hot.float().cpu().numpy())
    # the model API takes the bool matrix, uint8 through the engine alone: the same loss bits (no dropout: nothing is drawn)
    m2 = _model(0, 0.0, BCE).train()
    m2.train_engine(dtype=dtype)
    out = m2(imgs, hot)["loss_cls"]
    m3, eng3 = _engine(dtype)
    l3 = eng3.forward(imgs, hot.to(torch.uint8))
    eng3.backward()
    eager = m2.cls_head.loss(torch.from_numpy(saved["scores"]).cuda(), hot)["loss_cls"]
    torch.cuda.synchronize()
    assert float(out) == float(loss) and float(l3) == float(loss) and float(eager) == float(loss)
    assert "soft_targets" not in [k[0] for k in eng._bufs]                  # a caller's matrix is taken as it is


def test_replayed_bce_plan_equals_eager_steps_bit_for_bit():
    gen = torch.Generator(device="cuda").manual_seed(13)
    imgs = [torch.randn(2, 4, 3, 32, 32, device="cuda", generator=gen) for _ in range(2)]
    hots = [(torch.rand(2, CLASSES, device="cuda", generator=gen) < 0.4).to(torch.uint8) for _ in range(3)]
    out = {}
    for use_plan in (True, False):
        torch.manual_seed(7)
        m, eng = _engine(BF16, use_plan=use_plan, dropout=0.5)
        losses = [eng.train_step(imgs[i % 2].clone(), hots[i % 3].clone(), lr=0.01).clone() for i in range(7)]
        torch.cuda.synchronize()
        out[use_plan] = (eng, torch.cat(losses), eng.flat_params.clone())
    eng_p = out[True][0]
    st = list(eng_p._plans.values())
    assert len(st) == 1 and st[0]["plan"] is not None and st[0]["tries"] == 2, [(s_["eager"], s_["tries"]) for s_ in st]
    plan = st[0]["plan"]
    assert "mvf_head_train_fwd_bce" in plan.names and "mvf_head_train_fwd_soft" not in plan.names and "mvf_soft_targets" not in plan.names
    assert len(plan.slots["labels"]) == 1 and not getattr(out[False][0], "_plans", None)
    assert torch.isfinite(out[True][1]).all() and len(set(out[True][1].tolist())) > 3
    assert torch.equal(out[True][1], out[False][1]) and torch.equal(out[True][2], out[False][2])


def test_integer_labels_smoothing_and_mixup_go_through_soft_targets():
    from mvfnet_amd.blending import MixupBlending
    imgs, _, labels = _clips(3)
    m, eng = _engine(BF16, dict(BCE, target_threshold=0.2))
    eng.blending, eng.label_smooth_eps = MixupBlending(alpha=0.8, seed=5), 0.1
    loss = eng.forward(imgs, labels)
    saved = {k: eng.saved[k].cpu().numpy().copy() for k in ("scores", "dscores")}
    rows, wts = (v.cpu().numpy() for v in eng._blend_table)
    targets = eng._bufs[("soft_targets", (3, CLASSES), F32)].cpu().numpy().copy()
    eng.backward()
    torch.cuda.synchronize()
    want = BN.soft_targets_ref(labels.cpu().numpy(), rows, wts, CLASSES, 0.1, np.float64)
    assert np.abs(targets - want).max() <= 2.0 ** -22 and 0 < (targets > 0.2).sum() < targets.size
    _check_bce(saved, float(loss), targets, target_threshold=0.2)
    # a caller's matrix with blending or smoothing stays refused
    with pytest.raises(ValueError, match="taken as they are"):
        eng.forward(imgs, torch.zeros(3, CLASSES, device="cuda"))


def test_distillation_composes_behind_the_bce_head():
    from mvfnet_amd.distill import KnowledgeDistillation
    imgs, hot, _ = _clips()
    teacher = _model(seed=1).eval()
    T, alpha = 4.0, 0.5
    m, eng = _engine(BF16)
    eng.distill = KnowledgeDistillation(teacher, temperature=T, alpha=alpha)
    loss = eng.forward(imgs, hot.float())
    saved = {k: eng.saved[k].cpu().numpy().copy() for k in ("scores", "dscores", "teacher_scores")}
    eng.backward()
    torch.cuda.synchronize()
    terms = eng.distill_terms()
    bce = bn.bce_loss(saved["scores"], hot.float().cpu().numpy(), PW, raw=True)
    ref = dn.distill_loss(saved["scores"], saved["teacher_scores"], T, alpha, bce["dscores"], bce["loss_part"], raw=True)
    close(np.array([float(loss)]), np.array([ref["loss"]]), LOSS_BOUND, "loss")
    close(saved["dscores"], ref["dscores"], HEAD_BOUND, "dscores")
    close(np.array([terms["loss_ce"], terms["loss_kd"]]), ref["terms"], LOSS_BOUND, "terms")
    close(np.array([terms["loss_ce"]]), np.array([bce["loss"]]), LOSS_BOUND, "loss_ce is the BCE term")
    assert ref["terms"][1] > 0.0 and torch.isfinite(eng.flat_grads).all()


def test_the_default_loss_records_the_plan_it_always_did():
    """An engine whose head uses the default loss launches what it did: its plan holds mvf_head_train_fwd and none of the new entry points.  The BCE head
    swaps that one call for mvf_head_train_fwd_bce (multi-hot labels: the same op count) and adds mvf_soft_targets for integer labels (one more)."""
    imgs, hot, labels = _clips()
    m, eng = _engine(BF16, loss_cls=None, use_plan=True)
    assert eng.bce is None
    for _ in range(5):
        eng.train_step(imgs, labels)
    plain = [s["plan"] for s in eng._plans.values()]
    assert len(plain) == 1 and plain[0] is not None
    names = list(plain[0].names)
    assert names.count("mvf_head_train_fwd") == 1 and not any(n in names for n in ("mvf_head_train_fwd_bce", "mvf_bce_loss", "mvf_soft_targets", "mvf_head_train_fwd_soft"))
    assert not any(isinstance(k, tuple) and k[:1] == ("bce",) for key in eng._plans for k in key)
    mb, engb = _engine(BF16, use_plan=True)
    for _ in range(5):
        engb.train_step(imgs, hot.float())
    for _ in range(5):
        engb.train_step(imgs, labels)
    torch.cuda.synchronize()
    plans = sorted((s["plan"] for s in engb._plans.values()), key=lambda p: p.n_ops)
    assert len(plans) == 2 and all(p is not None for p in plans)
    print("plan ops: default %d, bce multi-hot %d, bce integer labels %d" % (plain[0].n_ops, plans[0].n_ops, plans[1].n_ops))
    assert [p.n_ops for p in plans] == [plain[0].n_ops, plain[0].n_ops + 1]
    swapped = ["mvf_head_train_fwd_bce" if n == "mvf_head_train_fwd" else n for n in names]
    assert list(plans[0].names) == swapped and [n for n in plans[1].names if n != "mvf_soft_targets"] == swapped
    assert torch.isfinite(engb.flat_params).all()
