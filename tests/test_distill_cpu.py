"""CPU: knowledge distillation -- everything that needs no device: the fp64 restatement of mvf_distill_loss (distill_numpy.py) against torch's own
cross_entropy / kl_div in float64, values and autograd gradient; the configuration check and every refusal of distill.py; the student's parameters and
state_dict with and without a teacher; the header / ctypes declaration and the entry point's argument failures (from host addresses that are never read);
the runner's log line over a stub engine; a warning-free compile of csrc/distill.hip under the project's flags."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import distill_numpy as dn


# ------------------------------------------------------------------------------------------------ the restatement against torch, float64
@pytest.mark.parametrize("clips,classes,scale,T,alpha", [(1, 1, 1.0, 1.0, 0.5), (7, 10, 1.0, 4.0, 0.5), (3, 257, 40.0, 20.0, 0.9), (7, 400, 1.0, 20.0, 1.0),
                                                          (2, 1000, 200.0, 1.0, 0.5), (5, 400, 40.0, 4.0, 0.25)])
def test_restatement_equals_torch_in_float64(clips, classes, scale, T, alpha):
    """(1 - a) * F.cross_entropy + a * T * T * F.kl_div(log_softmax(s / T), softmax(z / T), 'batchmean') and its autograd gradient with respect to the
    scores, to 1e-12 relative.  T and alpha are fp32-representable here (the restatement rounds them to fp32, as the C ABI does)."""
    gen = torch.Generator().manual_seed(clips * 1009 + classes)
    s = (torch.randn(clips, classes, generator=gen) * scale).float()
    z = (torch.randn(clips, classes, generator=gen) * scale).float()
    lab = torch.randint(0, classes, (clips,), generator=gen)
    a = float(np.float32(alpha))
    sd = s.double().requires_grad_(True)
    ce = F.cross_entropy(sd, lab)
    kd = F.kl_div(F.log_softmax(sd / T, dim=1), F.softmax(z.double() / T, dim=1), reduction="batchmean")
    loss = (1.0 - a) * ce + a * T * T * kd
    loss.backward()
    part, dsc = dn.cross_entropy(s.numpy(), lab.numpy())
    out = dn.distill_loss(s.numpy(), z.numpy(), T, alpha, dsc, part, raw=True)
    rel = lambda got, ref: float(np.abs(got - ref).max()) / max(float(np.abs(ref).max()), 1e-300)  # noqa: E731
    e_loss, e_grad = rel(np.float64(out["loss"]), loss.item()), rel(out["dscores"], sd.grad.numpy())
    e_terms = max(rel(out["terms"][0], ce.item()), abs(out["terms"][1] - T * T * kd.item()) / max(abs(T * T * kd.item()), 1e-300) if classes > 1 else 0.0)
    print("loss %.3g grad %.3g terms %.3g" % (e_loss, e_grad, e_terms))
    assert e_loss < 1e-12 and e_grad < 1e-12 and e_terms < 1e-12
    if classes == 1:
        assert out["terms"][1] == 0.0


def test_restatement_exact_cases():
    gen = np.random.default_rng(3)
    s = (gen.standard_normal((4, 33)) * 7).astype(np.float32)
    part, dsc = gen.standard_normal(4).astype(np.float32), gen.standard_normal((4, 33)).astype(np.float32)
    out = dn.distill_loss(s, s.copy(), 3.0, 0.7, dsc, part)
    keep = 1.0 - np.float64(np.float32(0.7))
    assert out["terms"][1] == 0.0
    assert np.array_equal(out["loss_part"], (keep * part.astype(np.float64)).astype(np.float32))
    assert np.array_equal(out["dscores"], (keep * dsc.astype(np.float64)).astype(np.float32))
    one = dn.distill_loss(s[:, :1], s[:, 1:2], 3.0, 0.7, dsc[:, :1], part)
    assert one["terms"][1] == 0.0 and np.array_equal(one["dscores"], (keep * dsc[:, :1].astype(np.float64)).astype(np.float32))


# ------------------------------------------------------------------------------------------------ configuration and refusals
def _model(train_cfg=None, **kw):
    import mvfnet_amd
    kw.setdefault("n_segment", 4)
    return mvfnet_amd.build_recognizer(mvfnet_amd.mvfnet_config(50, **kw), train_cfg, dict(average_clips=None))


@pytest.fixture(scope="module")
def teacher():
    return _model(num_classes=10)


def test_config_parsing(teacher):
    from mvfnet_amd.distill import KnowledgeDistillation, build_distill
    assert build_distill(None) is None
    kd = build_distill(dict(type="KnowledgeDistillation", teacher=teacher))
    assert isinstance(kd, KnowledgeDistillation) and (kd.temperature, kd.alpha) == (4.0, 0.5) and kd.teacher is teacher
    assert build_distill(kd) is kd
    kd = build_distill(dict(type="KnowledgeDistillation", teacher=teacher, temperature=np.float32(2.0), alpha=1))
    assert (kd.temperature, kd.alpha) == (2.0, 1.0)
    with pytest.raises(ValueError, match="unknown key 'temp'"):
        build_distill(dict(type="KnowledgeDistillation", teacher=teacher, temp=2.0))
    with pytest.raises(ValueError, match="'type'"):
        build_distill(dict(teacher=teacher))
    with pytest.raises(ValueError, match="'KnowledgeDistillation' is built"):
        build_distill(dict(type="HintLoss", teacher=teacher))
    with pytest.raises(ValueError, match="'teacher' is needed"):
        build_distill(dict(type="KnowledgeDistillation", alpha=0.5))
    for bad in (0, 0.0, -0.1, 1.0001, 2, float("nan"), float("inf"), True, "0.5", None):
        with pytest.raises(ValueError, match="alpha"):
            KnowledgeDistillation(teacher, alpha=bad)
    with pytest.raises(ValueError, match="leave distill out"):
        KnowledgeDistillation(teacher, alpha=0)
    for bad in (0, 0.0, -4.0, float("nan"), float("inf"), -float("inf"), True, "4", None):
        with pytest.raises(ValueError, match="temperature"):
            KnowledgeDistillation(teacher, temperature=bad)
    with pytest.raises(ValueError, match="Recognizer2D"):
        KnowledgeDistillation(teacher.backbone)
    with pytest.raises(ValueError, match="unknown key 'weights'"):
        KnowledgeDistillation(dict(model={}, weights="x.pth"))
    with pytest.raises(ValueError, match="checkpoint"):
        KnowledgeDistillation(dict(model={}))


def test_teacher_refusals(teacher):
    import mvfnet_amd
    from mvfnet_amd.distill import KnowledgeDistillation
    cfg = lambda t, **kw: dict(distill=dict(type="KnowledgeDistillation", teacher=t, **kw))  # noqa: E731
    with pytest.raises(ValueError, match="num_classes=10, the student 400"):
        _model(cfg(teacher))
    with pytest.raises(ValueError, match="n_segment=4, the student 8"):
        _model(cfg(teacher), num_classes=10, n_segment=8)
    kd = KnowledgeDistillation(teacher)
    with pytest.raises(ValueError, match="the student itself"):
        kd.check_student(teacher, device=False)
    headless = mvfnet_amd.mvfnet_config(50, 4)
    headless["cls_head"] = None
    with pytest.raises(ValueError, match="no class head"):
        KnowledgeDistillation(mvfnet_amd.build_recognizer(headless, None, None))
    teacher.cls_head.extract_feat = True
    try:
        with pytest.raises(ValueError, match="extract_feat=True"):
            KnowledgeDistillation(teacher)
    finally:
        teacher.cls_head.extract_feat = False
    # a request for another teacher dtype: refused when the student's storage dtype is known, before anything is built
    kd = KnowledgeDistillation(teacher, dtype=torch.float32)
    with pytest.raises(ValueError, match="no conversion pass"):
        kd.backbone_engine(torch.bfloat16)
    # a teacher on another device (meta stands in for a second GPU)
    other = _model(num_classes=10)
    kd = KnowledgeDistillation(other)
    other.to("meta")
    with pytest.raises(ValueError, match="the teacher is on meta, the student on cpu"):
        kd.check_student(teacher)


def test_teacher_from_config_and_checkpoint(tmp_path, teacher):
    import mvfnet_amd
    from mvfnet_amd.checkpoint import save_checkpoint
    from mvfnet_amd.distill import KnowledgeDistillation
    path = str(tmp_path / "teacher.pth")
    save_checkpoint(teacher, path)
    kd = KnowledgeDistillation(dict(model=mvfnet_amd.mvfnet_config(50, 4, num_classes=10), checkpoint=path), temperature=2.0)
    got, want = kd.teacher.state_dict(), teacher.state_dict()
    assert sorted(got) == sorted(want) and all(torch.equal(got[k], want[k]) for k in want)
    assert not kd.teacher.training and not any(p.requires_grad for p in kd.teacher.parameters())


def test_student_is_what_it_was_and_teacher_is_frozen(teacher):
    teacher.train()
    teacher.requires_grad_(True)
    plain = _model(num_classes=10)
    student = _model(dict(distill=dict(type="KnowledgeDistillation", teacher=teacher, temperature=2.0, alpha=0.9)), num_classes=10)
    assert sorted(student.state_dict()) == sorted(plain.state_dict())
    assert sum(p.numel() for p in student.parameters()) == sum(p.numel() for p in plain.parameters())
    assert len(list(student.modules())) == len(list(plain.modules())) and all(m is not teacher for m in student.modules())
    assert student.distill.teacher is teacher and (student.distill.temperature, student.distill.alpha) == (2.0, 0.9)
    assert not teacher.training and not any(m.training for m in teacher.modules()) and not any(p.requires_grad for p in teacher.parameters())
    student.train()                                  # the student's mode does not reach the teacher
    assert student.training and not teacher.training
    assert plain.distill is None


# ------------------------------------------------------------------------------------------------ the C ABI
def test_header_declares_and_lib_binds_the_entry_point():
    from mvfnet_amd import _lib
    assert "mvf_distill_loss" in _lib.declared_symbols() and hasattr(_lib.lib, "mvf_distill_loss")
    args = _lib.lib.mvf_distill_loss.argtypes
    assert len(args) == 11 and [i for i, a in enumerate(args) if a is C.c_float] == [4, 5] and C.c_double not in args
    assert args[2] is C.c_int and args[3] is C.c_int and _lib.lib.mvf_distill_loss.restype is C.c_int
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(_lib.__file__)), "include", "mvfnet_hip.h")).read()
    assert "float temperature, float alpha," in hdr and "fp64" in hdr[hdr.index("Knowledge distillation"):hdr.index("int mvf_distill_loss")]


def test_argument_failures_return_before_any_launch():
    from mvfnet_amd import _lib
    lib = _lib.lib
    host = (C.c_float * 64)()
    a = C.cast(host, C.c_void_p)
    nan, inf = float("nan"), float("inf")
    cases = [((None, a, 2, 4, 4.0, 0.5, a, a, a, a), b"NULL scores"), ((a, None, 2, 4, 4.0, 0.5, a, a, a, a), b"NULL teacher_scores"),
             ((a, a, 2, 4, 4.0, 0.5, None, a, a, a), b"NULL dscores"), ((a, a, 2, 4, 4.0, 0.5, a, None, a, a), b"NULL loss_part"),
             ((a, a, 2, 4, 4.0, 0.5, a, a, None, a), b"NULL loss"), ((a, a, 0, 4, 4.0, 0.5, a, a, a, a), b"clips=0"), ((a, a, -1, 4, 4.0, 0.5, a, a, a, a), b"clips=-1"),
             ((a, a, 2, 0, 4.0, 0.5, a, a, a, a), b"classes=0")]
    cases += [((a, a, 2, 4, t, 0.5, a, a, a, a), b"temperature") for t in (0.0, -1.0, nan, inf, -inf)]
    cases += [((a, a, 2, 4, 4.0, al, a, a, a, None), b"alpha") for al in (0.0, -0.5, 1.0000001, 2.0, nan, inf)]
    for args, text in cases:
        assert lib.mvf_distill_loss(*(args + (None,))) == -1, (args, lib.mvf_last_error())
        assert b"distill_loss" in lib.mvf_last_error() and text in lib.mvf_last_error(), (args, lib.mvf_last_error())
    assert all(v == 0.0 for v in host)


# ------------------------------------------------------------------------------------------------ the runner over a stub engine
class _Engine(object):
    flat_ema, max_norm, initial_lr = None, None, None
    norm_out = [1.5]
    accumulated_loss = 0.75

    def __init__(self, distill=None):
        self.reads = 0
        if distill is not None:
            self.distill = distill

    def train_step(self, imgs, labels, lr=None):
        return 0.25

    def accumulate_step(self, imgs, labels):
        pass

    def apply_accumulated(self, lr=None):
        pass

    def enable_step_guard(self):
        pass

    def guard_state(self):
        return dict(skipped_last=False, skipped=3, consecutive=0, steps=0)

    def enable_train_accuracy(self, k=(1, 5)):
        pass

    def train_accuracy(self):
        return dict(count=4, top1=0.5, top5=0.75)

    def distill_terms(self):
        self.reads += 1
        return dict(loss_ce=1.25, loss_kd=0.0625)


class _Model(object):
    def __init__(self, eng):
        self.eng = eng

    def train_engine(self, **opt):
        return self.eng

    def train(self, mode=True):
        return self


BATCH = dict(img_group="x", label="y")
BASE = "Epoch [1] iter %d lr 0.01000 loss_cls 0.2500 grad_norm 1.500"
KD = " loss_ce 1.2500 loss_kd 0.0625"


def test_runner_log_line_with_and_without_distill():
    from mvfnet_amd.runner import Runner
    # without: character for character what it was -- an engine without the attribute, and one with distill = None
    for eng in (_Engine(), ):
        lines = []
        Runner(_Model(eng), logger=lines.append, log_interval=2, lr=0.01, warmup=None).train_epoch([BATCH] * 4)
        assert lines == [BASE % 2, BASE % 4] and eng.reads == 0
    eng, lines = _Engine(), []
    eng.distill = None
    Runner(_Model(eng), logger=lines.append, log_interval=1, lr=0.01, warmup=None, nonfinite_guard={}, train_accuracy={}).train_epoch([BATCH])
    assert lines == [(BASE % 1) + " top1 0.5000 top5 0.7500 skipped 3"] and eng.reads == 0
    # with: the two fields directly behind the accuracy fields, in front of ` skipped N`; read only at the log points
    eng, lines = _Engine(distill=object()), []
    Runner(_Model(eng), logger=lines.append, log_interval=2, lr=0.01, warmup=None, nonfinite_guard={}, train_accuracy={}).train_epoch([BATCH] * 4)
    assert lines == [(BASE % i) + " top1 0.5000 top5 0.7500" + KD + " skipped 3" for i in (2, 4)] and eng.reads == 2
    eng, lines = _Engine(distill=object()), []
    Runner(_Model(eng), logger=lines.append, log_interval=1, lr=0.01, warmup=None).train_epoch([BATCH])
    assert lines == [(BASE % 1) + KD]
    eng, lines = _Engine(distill=object()), []
    Runner(_Model(eng), logger=lines.append, log_interval=1, lr=0.01, warmup=None, accumulate=2, nonfinite_guard={}).train_epoch([BATCH] * 2)
    assert lines == ["Epoch [1] iter 1 lr 0.01000 loss_cls 0.7500 grad_norm 1.500" + KD + " skipped 3"]


# ------------------------------------------------------------------------------------------------ the build
def test_distill_kernels_compile_without_warnings(tmp_path):
    from mvfnet_amd import build
    if not os.path.exists(build.HIPCC):
        pytest.skip("no hipcc on this machine")
    src = os.path.join(build.HERE, "csrc", "distill.hip")
    cmd = [build.HIPCC] + [f for f in build.FLAGS if f != "-shared"] + ["-Werror", "-c", src, "-o", str(tmp_path / "distill.o")]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT)
    assert p.returncode == 0 and not p.stdout.strip(), p.stdout.decode()
