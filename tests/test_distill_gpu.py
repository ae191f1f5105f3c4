"""Knowledge distillation on the device: mvf_distill_loss against its fp64 restatement (distill_numpy.py), BackboneEngine.forward_stem, and the train engine
with a teacher -- what the teacher sees, what the loss and its gradient are, that the teacher and the student's stores stay what they were, launch plans,
accumulation, the non-finite guard and precise BatchNorm.

Shapes are tests/test_launch_plan_gpu.py's: 1-3 clips x 4 frames x 64^2, ResNet-50, synthetic weights; the teacher is a second ResNet-50 from another synth
seed.  Bounds are the suite's own for the head's loss and gradient (test_head_optimizer_gpu.py: LOSS_BOUND for loss_part / loss / terms, HEAD_BOUND for
dscores): the kernel computes in fp64 and rounds once, so it owes nothing more than the fp32 head in front of it."""
import ctypes as C

import numpy as np
import pytest
import torch

import distill_numpy as dn
from helpers import rel_err
from mvfnet_amd import synth
from test_head_optimizer_gpu import HEAD_BOUND, LOSS_BOUND, close

pytestmark = pytest.mark.gpu

P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)  # noqa: E731
F32, BF16 = torch.float32, torch.bfloat16
CLASSES = 400


def _lib():
    from mvfnet_amd import _lib as L
    return L.lib, L.check


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ------------------------------------------------------------------------------------------------ 1. the kernel against fp64
def _kernel(s, z, T, a, dsc, part, with_terms=True):
    """One mvf_distill_loss call on copies of the host arrays; loss / terms start as NaN.  -> rc, dict of host arrays."""
    lib, _ = _lib()
    dev = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()  # noqa: E731
    s_d, z_d, dsc_d, part_d = dev(s), dev(z), dev(dsc), dev(part)
    loss_d, terms_d = torch.full((1,), float("nan"), device="cuda"), torch.full((2,), float("nan"), device="cuda")
    rc = lib.mvf_distill_loss(P(s_d), P(z_d), s.shape[0], s.shape[1], C.c_float(T), C.c_float(a), P(dsc_d), P(part_d), P(loss_d), P(terms_d) if with_terms else None,
                              _stream())
    torch.cuda.synchronize()
    return rc, dict(dscores=dsc_d.cpu().numpy(), loss_part=part_d.cpu().numpy(), loss=loss_d.cpu().numpy(), terms=terms_d.cpu().numpy())


def _inputs(clips, classes, scale, seed=0):
    gen = np.random.default_rng((clips * 1009 + classes) * 31 + int(scale) + seed)
    s = (gen.standard_normal((clips, classes)) * scale).astype(np.float32)
    z = (gen.standard_normal((clips, classes)) * scale).astype(np.float32)          # drawn independently of the student's
    dsc = (gen.standard_normal((clips, classes)) / clips).astype(np.float32)        # arbitrary finite incoming values: the kernel is tested alone
    part = (gen.standard_normal(clips) * 3 + 5).astype(np.float32)
    return s, z, dsc, part


@pytest.mark.parametrize("classes", [1, 10, 257, 400, 1000])
def test_kernel_vs_fp64(classes):
    """257 / 400 / 1000 classes: one thread of the 256 takes a second element, some do, all take three or four; 7 clips: the means' lanes are not all used.
    Worst errors observed on an MI355X over the whole grid -- the fp32 rounding of the outputs, nothing else: loss_part 5.8e-8, loss 6.3e-8, terms 5.4e-8
    (bound 1e-5), dscores 5.9e-8 (bound 5e-5); each run prints its own."""
    worst = dict(loss_part=0.0, loss=0.0, terms=0.0, dscores=0.0)
    for clips in (1, 7):
        for scale in (1, 40, 200):
            s, z, dsc, part = _inputs(clips, classes, scale)
            for T in (1, 4, 20):
                for a in (0.5, 0.9, 1.0):
                    rc, got = _kernel(s, z, T, a, dsc, part)
                    assert rc == 0
                    ref = dn.distill_loss(s, z, T, a, dsc, part, raw=True)
                    what = "clips=%d classes=%d scale=%g T=%g a=%g " % (clips, classes, scale, T, a)
                    close(got["loss_part"], ref["loss_part"], LOSS_BOUND, what + "loss_part")
                    close(got["loss"], np.array([ref["loss"]]), LOSS_BOUND, what + "loss")
                    close(got["terms"], ref["terms"], LOSS_BOUND, what + "terms")
                    close(got["dscores"], ref["dscores"], HEAD_BOUND, what + "dscores")
                    for k in worst:
                        worst[k] = max(worst[k], rel_err(got[k], np.asarray(ref[k]).reshape(got[k].shape)))
    print("classes=%d worst rel_err: loss_part %.3g loss %.3g terms %.3g (bound %g), dscores %.3g (bound %g)" %
          (classes, worst["loss_part"], worst["loss"], worst["terms"], LOSS_BOUND, worst["dscores"], HEAD_BOUND))


def test_kernel_exact_cases():
    s, z, dsc, part = _inputs(7, 257, 40)
    z[1], z[4], z[6] = s[1], s[4], s[6]              # three rows of the teacher hold the student's bits
    T, a = 4.0, 0.9
    rc, got = _kernel(s, z, T, a, dsc, part)
    assert rc == 0
    keep = 1.0 - np.float64(np.float32(a))
    for i in (1, 4, 6):
        assert np.array_equal(got["loss_part"][i:i + 1], (keep * part[i:i + 1].astype(np.float64)).astype(np.float32))
        assert np.array_equal(got["dscores"][i], (keep * dsc[i].astype(np.float64)).astype(np.float32))
    assert not np.array_equal(got["dscores"][0], (keep * dsc[0].astype(np.float64)).astype(np.float32))
    # every row equal: the distillation term is exactly 0
    rc, same = _kernel(s, s.copy(), T, a, dsc, part)
    assert rc == 0 and same["terms"][1] == 0.0
    assert np.array_equal(same["loss_part"], (keep * part.astype(np.float64)).astype(np.float32))
    assert np.array_equal(same["dscores"], (keep * dsc.astype(np.float64)).astype(np.float32))
    # one class: exactly 0, whatever the two scores are
    rc, one = _kernel(s[:, :1], z[:, 1:2], T, a, dsc[:, :1], part)
    assert rc == 0 and one["terms"][1] == 0.0
    assert np.array_equal(one["loss_part"], (keep * part.astype(np.float64)).astype(np.float32))
    assert np.array_equal(one["dscores"], (keep * dsc[:, :1].astype(np.float64)).astype(np.float32))
    # two runs: identical bits; terms == NULL: the same other outputs, terms untouched
    rc, again = _kernel(s, z, T, a, dsc, part)
    assert rc == 0 and all(np.array_equal(got[k], again[k]) for k in got)
    rc, bare = _kernel(s, z, T, a, dsc, part, with_terms=False)
    assert rc == 0 and all(np.array_equal(got[k], bare[k]) for k in ("dscores", "loss_part", "loss")) and np.isnan(bare["terms"]).all()


def test_kernel_refusals_touch_nothing():
    lib, _ = _lib()
    nan, inf = float("nan"), float("inf")
    clips, classes = 3, 10
    t = {k: torch.full(shape, nan, device="cuda") for k, shape in (("s", (clips, classes)), ("z", (clips, classes)), ("dsc", (clips, classes)), ("part", (clips,)),
                                                                    ("loss", (1,)), ("terms", (2,)))}

    def call(s="s", z="z", n=clips, k=classes, T=4.0, a=0.5, dsc="dsc", part="part", loss="loss"):
        p = lambda name: P(t[name]) if name else None  # noqa: E731
        return lib.mvf_distill_loss(p(s), p(z), n, k, C.c_float(T), C.c_float(a), p(dsc), p(part), p(loss), P(t["terms"]), _stream())
    cases = [dict(s=None), dict(z=None), dict(dsc=None), dict(part=None), dict(loss=None), dict(n=0), dict(n=-2), dict(k=0), dict(k=-1)]
    cases += [dict(T=v) for v in (0.0, -2.0, nan, inf, -inf)] + [dict(a=v) for v in (0.0, -0.1, 1.5, nan, inf)]
    for kw in cases:
        assert call(**kw) == -1, (kw, lib.mvf_last_error())                  # MVF_EINVAL
        assert b"distill_loss" in lib.mvf_last_error()
    torch.cuda.synchronize()
    assert all(bool(torch.isnan(v).all()) for v in t.values())
    # a NaN or inf in a teacher row reaches that row's outputs and the loss, and no other row
    s, z, dsc, part = _inputs(3, 10, 1)
    for bad in (nan, inf, -inf):
        zz = z.copy()
        zz[1, 3] = bad
        rc, got = _kernel(s, zz, 4.0, 0.5, dsc, part)
        assert rc == 0 and np.isnan(got["loss_part"][1]) and np.isnan(got["dscores"][1]).all() and np.isnan(got["loss"][0]) and np.isnan(got["terms"][1])
        assert np.isfinite(got["loss_part"][[0, 2]]).all() and np.isfinite(got["dscores"][[0, 2]]).all() and np.isfinite(got["terms"][0])


# ------------------------------------------------------------------------------------------------ models
_VALS = {}


def _model(seed=0, dropout=0.5, train_cfg=None):
    import mvfnet_amd
    m = mvfnet_amd.build_recognizer(mvfnet_amd.mvfnet_config(50, 4, dropout_ratio=dropout), train_cfg, dict(average_clips=None))
    sd = m.state_dict()
    if seed not in _VALS:
        _VALS[seed] = synth.synth_state_dict({"r50/" + k: tuple(v.shape) for k, v in sd.items()}, seed=seed)
    m.load_state_dict({k: torch.from_numpy(_VALS[seed]["r50/" + k]) for k in sd})
    return m.cuda()


@pytest.fixture(scope="module")
def teacher():
    """One teacher for the module: nothing may change it (test_teacher_is_untouched checks exactly that)."""
    return _model(seed=1).eval()


def _engine(dtype, teacher=None, dropout=0.5, use_plan=False, T=4.0, alpha=0.5):
    from mvfnet_amd.distill import KnowledgeDistillation
    m = _model(0, dropout).train()
    eng = m.train_engine(dtype=dtype)
    eng.use_plan = use_plan
    if teacher is not None:
        eng.distill = KnowledgeDistillation(teacher, temperature=T, alpha=alpha)
    return m, eng


def _clips(b=2, seed=3):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(b, 4, 3, 64, 64, device="cuda", generator=gen), torch.randint(0, CLASSES, (b, 1), device="cuda", generator=gen)


def _own_scores(teacher, imgs, dtype):
    """The teacher's own forward_test path (average_clips=None) in `dtype`."""
    teacher.backbone.engine_dtype = dtype
    teacher.backbone.invalidate_engine()
    try:
        return teacher(imgs, return_loss=False, return_numpy=False).clone()
    finally:
        teacher.backbone.engine_dtype = F32
        teacher.backbone.invalidate_engine()


def _check_step(saved, loss, terms, part_ce, dsc_ce, T, alpha):
    """loss / dscores / terms of a distilled step against the restatement on (saved scores, teacher scores) and the fp64 cross-entropy part."""
    ref = dn.distill_loss(saved["scores"], saved["teacher_scores"], T, alpha, dsc_ce, part_ce, raw=True)
    close(np.array([loss]), np.array([ref["loss"]]), LOSS_BOUND, "loss")
    close(saved["dscores"], ref["dscores"], HEAD_BOUND, "dscores")
    close(np.array([terms["loss_ce"], terms["loss_kd"]]), ref["terms"], LOSS_BOUND, "terms")
    return ref


# ------------------------------------------------------------------------------------------------ 4. forward_stem
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_forward_stem_equals_forward(teacher, dtype):
    from mvfnet_amd.engine import BackboneEngine
    lib, check = _lib()
    be = BackboneEngine(teacher.backbone, dtype)
    x = _clips()[0].reshape(8, 3, 64, 64).contiguous()
    with torch.no_grad():
        want = be.forward(x)
        shape = be.stem_operand_shape(8, 64, 64)
        assert shape == (8, 70, 72, 4)
        xp = torch.full(shape, float("nan"), device="cuda").to(dtype)
        check(lib.mvf_stem_prep(P(x), 8, 3, 64, 64, 3, shape[2], P(xp), 0 if dtype == F32 else 1, _stream()), "stem_prep")
        got = be.forward_stem(xp, 8, 64, 64)
        out = torch.full_like(want, float("nan"))
        assert be.forward_stem(xp, 8, 64, 64, out=out) is out
        torch.cuda.synchronize()
        assert got.dtype == dtype and torch.isfinite(got.float()).all() and torch.equal(got, want) and torch.equal(out, want)
        with pytest.raises(TypeError, match="this engine was built for"):
            be.forward_stem(xp.to(BF16 if dtype == F32 else F32), 8, 64, 64)
        for bad in (xp[:, :-1], xp[:, :, :-2], xp[:4], xp[..., :3]):
            with pytest.raises(ValueError, match="stem operand"):
                be.forward_stem(bad.contiguous(), 8, 64, 64)
        with pytest.raises(ValueError, match="stem operand"):
            be.forward_stem(xp, 8, 64, 66)
        with pytest.raises(ValueError, match="stem operand"):
            be.forward_stem(xp.transpose(1, 2), 8, 64, 64)


# ------------------------------------------------------------------------------------------------ 5. one engine step
@pytest.mark.parametrize("dropout", [0.0, 0.5], ids=["p0", "p0.5"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
def test_engine_step(teacher, dtype, dropout):
    imgs, labels = _clips(3)
    T, alpha = 4.0, 0.5
    runs = {}
    for run in ("a", "b", "plain"):                  # an engine each: every forward starts from the same BatchNorm state
        torch.manual_seed(11)                        # the dropout mask
        m, eng = _engine(dtype, teacher if run != "plain" else None, dropout, T=T, alpha=alpha)
        loss = eng.forward(imgs, labels)
        saved = {k: eng.saved[k].cpu().numpy().copy() for k in ("scores", "dscores") + (("teacher_scores",) if run != "plain" else ())}
        eng.backward()
        torch.cuda.synchronize()
        runs[run] = (float(loss), saved, eng.flat_grads.clone(), eng.distill_terms() if run != "plain" else None)
        if run == "plain":
            assert "teacher_scores" not in saved and eng._distill_terms is None
            with pytest.raises(RuntimeError, match="no step has run"):
                eng.distill_terms()
    loss, saved, grads, terms = runs["a"]
    own = _own_scores(teacher, imgs, dtype)
    assert np.array_equal(saved["teacher_scores"], own.cpu().numpy()) and np.isfinite(saved["teacher_scores"]).all()
    part_ce, dsc_ce = dn.cross_entropy(saved["scores"], labels.reshape(-1).cpu().numpy())
    ref = _check_step(saved, loss, terms, part_ce, dsc_ce, T, alpha)
    assert ref["terms"][1] > 0.0 and abs((1 - alpha) * terms["loss_ce"] + alpha * terms["loss_kd"] - loss) <= LOSS_BOUND * abs(loss)
    assert torch.isfinite(grads).all() and torch.equal(grads, runs["b"][2]) and runs["b"][0] == loss
    assert np.array_equal(saved["scores"], runs["plain"][1]["scores"])              # the student's forward is what it was ...
    assert not torch.equal(grads, runs["plain"][2]) and loss != runs["plain"][0]     # ... its loss and gradient are not


@pytest.mark.parametrize("mode", ["soft_labels", "label_smoothing"])
def test_soft_targets_are_post_processed_alike(teacher, mode):
    """The kernel only post-processes what the head left: with the soft-target head in front of it the cross-entropy part is sum_k t_k (lse - s_k)."""
    imgs, labels = _clips(2)
    T, alpha = 2.0, 0.9
    m, eng = _engine(BF16, teacher, dropout=0.0, T=T, alpha=alpha)
    lab = labels.reshape(-1).cpu().numpy()
    if mode == "soft_labels":
        tg = np.random.default_rng(2).random((2, CLASSES)).astype(np.float32)
        tg /= tg.sum(1, keepdims=True)
        loss = eng.forward(imgs, torch.from_numpy(tg).cuda())
    else:
        eng.label_smooth_eps = 0.1
        tg = np.full((2, CLASSES), np.float32(0.1) / CLASSES, dtype=np.float64)
        tg[np.arange(2), lab] += 1.0 - np.float64(np.float32(0.1))
        loss = eng.forward(imgs, labels)
    saved = {k: eng.saved[k].cpu().numpy().copy() for k in ("scores", "dscores", "teacher_scores")}
    eng.backward()
    s = saved["scores"].astype(np.float64)
    lse = dn._lse(s)
    tg = tg.astype(np.float64)
    part_ce = (tg * (lse - s)).sum(1)
    dsc_ce = (np.exp(s - lse) * tg.sum(1, keepdims=True) - tg) / 2
    _check_step(saved, float(loss), eng.distill_terms(), part_ce, dsc_ce, T, alpha)


# ------------------------------------------------------------------------------------------------ 6. the teacher sees the erased, blended operand
@pytest.mark.parametrize("source", ["f32", "u8"])
def test_teacher_scores_the_erased_blended_operand(teacher, source):
    from mvfnet_amd.blending import MixupBlending
    from mvfnet_amd.erasing import RandomErasing
    from mvfnet_amd.preprocess import FramePipeline
    lib, check = _lib()
    dtype = BF16
    m, eng = _engine(dtype, teacher, dropout=0.0)
    eng.erasing, eng.blending = RandomErasing(probability=1.0, mode="pixel", seed=5), MixupBlending(alpha=0.8, seed=3)
    imgs, labels = _clips(3)
    if source == "u8":
        mean, std = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]
        fr = np.random.RandomState(2).randint(0, 256, (3, 4, 72, 80, 3)).astype(np.uint8)
        win = np.stack([np.full(12, 3), np.full(12, 7), np.repeat([0, 1, 0], 4)], 1).astype(np.int32)
        eng.input_pipeline, eng.input_window = FramePipeline(mean, std, to_rgb=True, crop_size=64), torch.from_numpy(win).cuda()
        imgs = torch.from_numpy(fr).cuda()
    loss = eng.forward(imgs, labels)
    xp, got = eng.saved["xp"].clone(), eng.saved["teacher_scores"].clone()
    eng.backward()
    assert tuple(xp.shape) == (12, 70, 72, 4) and xp.dtype == dtype and torch.isfinite(loss).all()
    with torch.no_grad():
        feat = eng.distill.backbone_engine(dtype).forward_stem(xp, 12, 64, 64)
        want = teacher.cls_head.engine().scores(feat, 4)
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    if source == "f32":                              # and that operand is not the plain one: erase and blend ran in front of the teacher
        plain = torch.empty_like(xp)
        check(lib.mvf_stem_prep(P(imgs.reshape(12, 3, 64, 64).contiguous()), 12, 3, 64, 64, 3, 72, P(plain), 1, _stream()), "stem_prep")
        assert not torch.equal(plain, xp) and not torch.equal(_own_scores(teacher, imgs, dtype), got)


# ------------------------------------------------------------------------------------------------ 7. the teacher is untouched, the student's stores are its own
def test_teacher_is_untouched_and_absent_from_the_students_stores(teacher, tmp_path):
    from mvfnet_amd.checkpoint import save_checkpoint
    before = {k: v.clone() for k, v in teacher.state_dict().items()}
    student = _model(0, 0.5, train_cfg=dict(distill=dict(type="KnowledgeDistillation", teacher=teacher, temperature=2.0, alpha=0.7))).train()
    plain_keys = sorted(_model(0, 0.5).state_dict())
    eng = student.train_engine(dtype=BF16, lr=0.01)
    assert eng.distill is student.distill and eng.distill.teacher is teacher
    imgs, labels = _clips(2)
    n_flat = eng.flat_params.numel()
    loss = student(imgs, labels)["loss_cls"]         # the model API: forward_train + autograd's backward
    loss.backward()
    eng.step()
    for _ in range(3):
        eng.train_step(imgs, labels)
    torch.cuda.synchronize()
    terms = eng.distill_terms()
    assert np.isfinite([terms["loss_ce"], terms["loss_kd"]]).all() and terms["loss_kd"] > 0.0 and torch.isfinite(eng.flat_params).all()
    after = teacher.state_dict()
    assert sorted(after) == sorted(before) and all(torch.equal(after[k], before[k]) for k in before)
    assert not teacher.training and not any(p.requires_grad for p in teacher.parameters()) and all(p.grad is None for p in teacher.parameters())
    path = str(tmp_path / "student.pth")
    save_checkpoint(student, path, optimizer=eng.optimizer_state_dict())
    ckpt = torch.load(path, map_location="cpu", weights_only=False)
    assert sorted(ckpt["state_dict"]) == plain_keys and not any("teacher" in k or "distill" in k for k in ckpt["state_dict"])
    n_params = len(list(student.parameters()))
    assert len(ckpt["optimizer"]["state"]) == n_params and len(ckpt["optimizer"]["param_groups"][0]["params"]) == n_params
    assert eng.flat_params.numel() == n_flat and sorted(student.state_dict()) == plain_keys
    student.eval()
    assert eng.distill is None
    student.train()
    assert eng.distill is student.distill


def test_step_refusals(teacher):
    import mvfnet_amd
    from mvfnet_amd.distill import KnowledgeDistillation
    imgs, labels = _clips(1)
    m, eng = _engine(BF16, None, dropout=0.0)
    cpu_teacher = mvfnet_amd.build_recognizer(mvfnet_amd.mvfnet_config(50, 4), None, None)
    for kd, text in ((KnowledgeDistillation(cpu_teacher), "the teacher is on cpu"), (KnowledgeDistillation(m), "the student itself"),
                     (KnowledgeDistillation(teacher, dtype=F32), "no conversion pass")):
        m.train().requires_grad_(True)               # (KnowledgeDistillation(m) froze the student and put it in eval mode: one reason it is refused)
        eng.distill = kd
        count = eng.forward_count
        with pytest.raises(ValueError, match=text):
            eng.train_step(imgs, labels)
        with pytest.raises(ValueError, match=text):
            eng.forward(imgs, labels)
        assert eng.forward_count == count and eng.saved is None          # refused before the step began
    eng.distill = None
    assert torch.isfinite(eng.train_step(imgs, labels)).all()


# ------------------------------------------------------------------------------------------------ 8. launch plans
def test_distilled_steps_run_eagerly_and_plans_survive_them(teacher):
    from mvfnet_amd.distill import KnowledgeDistillation
    gen = torch.Generator(device="cuda").manual_seed(3)
    batches = [(torch.randn(2, 4, 3, 64, 64, device="cuda", generator=gen), torch.randint(0, CLASSES, (2, 1), device="cuda", generator=gen)) for _ in range(3)]
    kinds = ["plain"] * 6 + ["distill"] * 3 + ["plain"] * 3
    out = {}
    for use_plan in (True, False):
        torch.manual_seed(7)
        m, eng = _engine(BF16, None, use_plan=use_plan)
        kd = KnowledgeDistillation(teacher, temperature=4.0, alpha=0.5)
        losses, seen = [], []
        for i, kind in enumerate(kinds):
            eng.distill = kd if kind == "distill" else None
            imgs, labels = batches[i % 3]
            losses.append(eng.train_step(imgs.clone(), labels.clone(), lr=0.01).clone())
            st = list(getattr(eng, "_plans", {}).values())
            seen.append((len(st), st[0]["plan"] if st else None, st[0]["eager"] if st else None, st[0]["tries"] if st else None))
        torch.cuda.synchronize()
        out[use_plan] = (torch.cat(losses), eng.flat_params.clone(), seen, eng)
    loss_p, par_p, seen, eng_p = out[True]
    assert not getattr(out[False][3], "_plans", None)
    plan = seen[5][1]
    assert plan is not None and seen[3][1] is plan                                   # accepted at the fourth plain step, replayed since
    assert all(s == seen[5] for s in seen[6:])                                       # distilled steps: no plan recorded, none touched, no eager / try counted
    assert eng_p._plan_key(*batches[0]) is not None and len(eng_p._plans) == 1
    eng_p.distill = kd
    assert eng_p._plan_key(*batches[0]) is None
    assert torch.equal(loss_p, out[False][0]), (loss_p, out[False][0])
    assert torch.equal(par_p, out[False][1])
    assert not torch.equal(loss_p[6:9], loss_p[:3])
    # an engine that never sets distill records the plan it always did: the same ops as the engine above recorded
    torch.manual_seed(7)
    m, fresh = _engine(BF16, None, use_plan=True)
    for i in range(6):
        fresh.train_step(batches[i % 3][0].clone(), batches[i % 3][1].clone(), lr=0.01)
    torch.cuda.synchronize()
    st = list(fresh._plans.values())
    assert len(st) == 1 and st[0]["plan"] is not None and list(fresh._plans) == list(eng_p._plans)
    assert st[0]["plan"].n_ops == plan.n_ops and list(st[0]["plan"].names) == list(plan.names) and "mvf_distill_loss" not in list(plan.names)
    assert not any(k[0] in ("teacher_scores", "distill_terms") for k in fresh._bufs)


# ------------------------------------------------------------------------------------------------ 9. the training signal
KD_STEPS, KD_LR = 12, 0.01


def test_distillation_term_falls_on_a_fixed_batch(teacher):
    """alpha = 1, T = 2, dropout 0, one fixed batch, fp32: the student is trained on the teacher's scores alone, so loss_kd must fall.  The run is
    bit-reproducible; KD_STEPS and KD_LR were picked once, from the trajectories at lr 0.002 / 0.01 / 0.05 (the first falls slowly, the last turns round after
    nine steps), for a fall to under half with room to spare.  Observed on an MI355X: loss_kd 0.764745 after the first step, 0.214347 after the twelfth."""
    imgs, labels = _clips(2)
    m, eng = _engine(F32, teacher, dropout=0.0, T=2.0, alpha=1.0)
    kd = []
    for _ in range(KD_STEPS):
        eng.train_step(imgs, labels, lr=KD_LR)
        kd.append(eng.distill_terms()["loss_kd"])
    print("loss_kd per step: %s" % " ".join("%.6g" % v for v in kd))
    assert np.isfinite(kd).all() and kd[-1] < 0.5 * kd[0], kd


# ------------------------------------------------------------------------------------------------ 10. accumulation, guard, precise BN, eval
class _Counting(object):
    def __init__(self, kd):
        self.kd, self.calls, self.temperature, self.alpha = kd, 0, kd.temperature, kd.alpha

    def teacher_scores(self, *a, **k):
        self.calls += 1
        return self.kd.teacher_scores(*a, **k)


def test_accumulation_and_precise_bn(teacher):
    imgs, labels = _clips(2)
    other = _clips(2, seed=9)
    m, eng = _engine(BF16, teacher, dropout=0.0, T=4.0, alpha=0.5)
    counter = eng.distill = _Counting(eng.distill)
    l1 = eng.accumulate_step(imgs, labels).clone()
    l2 = eng.accumulate_step(*other).clone()
    terms = eng.distill_terms()
    eng.apply_accumulated(lr=0.01)
    torch.cuda.synchronize()
    assert counter.calls == 2 and float(l1) != float(l2)
    assert torch.equal(eng.accumulated_loss, (l1 * 1.0 + l2) / 2.0)
    assert abs(0.5 * terms["loss_ce"] + 0.5 * terms["loss_kd"] - float(l2)) <= LOSS_BOUND * abs(float(l2))      # the micro-batch losses are the combined ones
    assert eng.precise_bn([(imgs, labels), other], num_iters=2) == 2
    assert counter.calls == 2 and eng.distill is counter and eng.saved is None
    eng.train_step(imgs, labels)
    assert counter.calls == 3


def test_guard_skips_a_step_whose_teacher_is_poisoned():
    """A teacher of its own: this test writes a NaN into it."""
    poisoned = _model(seed=1).eval()
    imgs, labels = _clips(2)
    m, eng = _engine(BF16, poisoned, dropout=0.0)
    eng.enable_step_guard()
    eng.train_step(imgs, labels, lr=0.01)
    assert eng.guard_state() == dict(skipped_last=False, skipped=0, consecutive=0, steps=1)
    par, bufs = eng.flat_params.clone(), [b.clone() for b in m.buffers()]
    with torch.no_grad():
        poisoned.cls_head.new_fc.bias[7] = float("nan")
    loss = eng.train_step(imgs, labels, lr=0.01)
    assert eng.guard_state() == dict(skipped_last=True, skipped=1, consecutive=1, steps=2) and bool(torch.isnan(loss).all())
    assert torch.equal(eng.flat_params, par) and all(torch.equal(a, b) for a, b in zip(m.buffers(), bufs))


def test_eval_mode_forward_is_what_it_was(teacher):
    imgs, _ = _clips(2)
    plain = _model(0).eval()
    with_kd = _model(0, train_cfg=dict(distill=dict(type="KnowledgeDistillation", teacher=teacher))).eval()
    a = plain(imgs, return_loss=False, return_numpy=False)
    b = with_kd(imgs, return_loss=False, return_numpy=False)
    with_kd.train().train_engine(dtype=F32)
    c = with_kd.eval()(imgs, return_loss=False, return_numpy=False)
    torch.cuda.synchronize()
    assert torch.isfinite(a).all() and torch.equal(a, b) and torch.equal(a, c)
