"""Knowledge distillation (Hinton et al. 2015) for fine-tuning: train_cfg=dict(distill=dict(type='KnowledgeDistillation', teacher=..., temperature=4.0, alpha=0.5)).

The train engine and the inference engine consume the same stem operand -- (frames, h + 6, wp, 4) in the storage dtype, what mvf_stem_prep or the uint8 /
YUV / addressed frame kernels produce and mvf_stem_erase / mvf_stem_blend modify --, so the teacher scores exactly the pixels the student sees: after
RandAugment, erasing and blending, behind every input path, with no second upload, crop or input pipeline.  Per step:

    teacher_scores = HeadEngine.scores(BackboneEngine.forward_stem(xp))        the teacher's eval-mode launch chain, on the train engine's launch stream
    mvf_head_train_fwd[_soft](...)                                               the student's head: scores, and the cross-entropy's dscores / loss_part / loss
    mvf_distill_loss(scores, teacher_scores, T, alpha, dscores, loss_part, loss) (1 - alpha) * CE + alpha * T^2 * KL(softmax(z / T) || softmax(s / T)), in place

The object below only holds the teacher and the two numbers; the arithmetic is csrc/distill.hip's (include/mvfnet_hip.h states it).  The teacher is a second
Recognizer2D in eval mode with no parameter requiring a gradient.  It is NOT a submodule of the student: it sits in a plain tuple, so the student's
parameters(), state_dict(), flat parameter store, optimizer segments, averaged weights and checkpoints are what they are without it.
"""
import numbers

import numpy as np

DISTILL_KEYS = ("teacher", "temperature", "alpha", "dtype")
TEACHER_KEYS = ("model", "checkpoint")


def _real(v, name):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, numbers.Real) or not np.isfinite(v):
        raise ValueError("KnowledgeDistillation: %s must be a finite number (got %r)" % (name, v))
    return float(v)


def _n_segment(model):
    cfg = getattr(model, "module_cfg", None)
    return cfg.get("n_segment") if cfg else None


def _build_teacher(cfg):
    """dict(model=<recognizer config>, checkpoint=<path>) -> a Recognizer2D with the checkpoint's weights."""
    unknown = sorted(k for k in cfg.keys() if k not in TEACHER_KEYS)
    if unknown:
        raise ValueError("distill teacher: unknown key %s (known: %s)" % (", ".join(map(repr, unknown)), ", ".join(TEACHER_KEYS)))
    if cfg.get("model") is None or cfg.get("checkpoint") is None:
        raise ValueError("distill teacher: dict(model=<recognizer config>, checkpoint=<path>) is expected, got keys %s" % sorted(cfg.keys()))
    from .builder import build_recognizer
    from .checkpoint import load_checkpoint
    model = build_recognizer(cfg["model"], None, dict(average_clips=None))
    load_checkpoint(model, cfg["checkpoint"], map_location="cpu", strict=True)
    return model


class KnowledgeDistillation(object):
    """teacher: a built Recognizer2D, or dict(model=<recognizer config>, checkpoint=<path>) (built here, loaded strictly, and moved to the student's device at
    its first step).  temperature: finite, > 0.  alpha in (0, 1]: the weight of the distillation term; alpha = 0 means "do not configure it".
    dtype: None -- the teacher's backbone engine is built in the student's storage dtype (a bf16 student gets a bf16 teacher) and rebuilt when that changes;
    any other request is refused at the first step: a conversion pass between two storage types is not built."""

    def __init__(self, teacher, temperature=4.0, alpha=0.5, dtype=None):
        self.temperature = _real(temperature, "temperature")
        if self.temperature <= 0.0:
            raise ValueError("KnowledgeDistillation: temperature=%r must be positive" % (temperature,))
        self.alpha = _real(alpha, "alpha")
        if not 0.0 < self.alpha <= 1.0:
            raise ValueError("KnowledgeDistillation: alpha=%r is outside (0, 1]%s" % (alpha, " (alpha = 0 is plain training: leave distill out)" if self.alpha == 0.0 else ""))
        self.dtype = dtype
        self._owned = hasattr(teacher, "keys")
        if self._owned:
            teacher = _build_teacher(teacher)
        from .recognizers.recognizer2d import Recognizer2D
        if not isinstance(teacher, Recognizer2D):
            raise ValueError("KnowledgeDistillation: teacher must be a built Recognizer2D or dict(model=..., checkpoint=...), got %s" % type(teacher).__name__)
        if not teacher.with_cls_head:
            raise ValueError("KnowledgeDistillation: the teacher has no class head: there are no scores to distil")
        if getattr(teacher.cls_head, "extract_feat", False):
            raise ValueError("KnowledgeDistillation: the teacher's head has extract_feat=True: it returns features, not scores")
        teacher.eval()
        teacher.requires_grad_(False)
        self._held = (teacher,)                  # a plain tuple, not a module attribute of anybody: never a submodule of the student
        self._engine = None                      # (BackboneEngine, its dtype)

    @property
    def teacher(self):
        return self._held[0]

    def __repr__(self):
        return "KnowledgeDistillation(teacher=%s, temperature=%g, alpha=%g)" % (type(self.teacher).__name__, self.temperature, self.alpha)

    def check_student(self, student, device=True):
        """ValueError unless this teacher can teach `student` (a Recognizer2D); called when the student is built and again before a step's first teacher
        launch.  device=False leaves the device out (a student that has just been built is still on the host)."""
        t = self.teacher
        if t is student:
            raise ValueError("KnowledgeDistillation: the teacher is the student itself (its scores would carry no signal, and eval() would stop its training)")
        nc_s, nc_t = getattr(student.cls_head, "num_classes", None), t.cls_head.num_classes
        if nc_s != nc_t:
            raise ValueError("KnowledgeDistillation: the teacher has num_classes=%r, the student %r" % (nc_t, nc_s))
        if _n_segment(t) != _n_segment(student):
            raise ValueError("KnowledgeDistillation: the teacher has n_segment=%r, the student %r: they could not read one stem operand" % (_n_segment(t), _n_segment(student)))
        if device:
            dev_s, dev_t = next(student.parameters()).device, next(t.parameters()).device
            if dev_s != dev_t:
                if not self._owned:
                    raise ValueError("KnowledgeDistillation: the teacher is on %s, the student on %s" % (dev_t, dev_s))
                t.to(dev_s)                      # a teacher built here from its config follows the student
                self._engine = None

    def check_step(self, student, dtype):
        """What TrainEngine asks before a step's first launch: check_student, and the teacher's storage dtype against the student's `dtype`."""
        self.check_student(student)
        self.check_dtype(dtype)

    def check_dtype(self, dtype):
        if self.dtype is not None and self.dtype != dtype:
            raise ValueError("KnowledgeDistillation: a %s teacher for a %s student is not built (no conversion pass between storage types); leave dtype out" %
                             (self.dtype, dtype))

    def invalidate_engine(self):
        """Drop the packed, BatchNorm-folded copy of the teacher's backbone (after loading other weights into the teacher)."""
        self._engine = None

    def backbone_engine(self, dtype):
        """The teacher's BackboneEngine in `dtype`, the student's storage dtype: built at the first step, rebuilt when the dtype changes."""
        self.check_dtype(dtype)
        if self._engine is None or self._engine[1] != dtype:
            from .engine import BackboneEngine
            self._engine = (BackboneEngine(self.teacher.backbone, dtype), dtype)
        return self._engine[0]

    def teacher_scores(self, xp, b, t, h, w, out=None, student=None):
        """The teacher's (b, classes) fp32 scores of the stem operand xp (b * t, h + 6, wp, 4), on the device.  Called by TrainEngine._forward inside its
        _on_stream context: every launch goes to the stream that is current there, the train engine's launch stream.  out: the buffer to write them into."""
        import torch
        if student is not None:
            self.check_student(student)
        teacher = self.teacher
        if teacher.training:
            teacher.eval()                       # it stays in eval mode whatever was called on it in between
        if next(teacher.parameters()).device != xp.device:
            raise ValueError("KnowledgeDistillation: the teacher is on %s, the stem operand on %s" % (next(teacher.parameters()).device, xp.device))
        n_seg = _n_segment(teacher)
        if n_seg is not None and n_seg != t:
            raise ValueError("KnowledgeDistillation: clips of %d frames for a teacher with n_segment=%d" % (t, n_seg))
        with torch.no_grad():
            feat = self.backbone_engine(xp.dtype).forward_stem(xp, b * t, h, w)
            return teacher.cls_head.engine().scores(feat, t, out=out)


def build_distill(cfg):
    """train_cfg['distill'] -> a KnowledgeDistillation: dict(type='KnowledgeDistillation', teacher=..., temperature=..., alpha=...), an object with
    teacher_scores(), or None."""
    if cfg is None or hasattr(cfg, "teacher_scores"):
        return cfg
    if not hasattr(cfg, "keys") or cfg.get("type") is None:
        raise ValueError("distill config: a dict with a 'type' is expected, got %r" % (cfg,))
    args = {k: cfg[k] for k in cfg.keys()}
    kind = args.pop("type")
    if kind != "KnowledgeDistillation":
        raise ValueError("distill type %r: 'KnowledgeDistillation' is built" % (kind,))
    unknown = sorted(k for k in args if k not in DISTILL_KEYS)
    if unknown:
        raise ValueError("distill config: unknown key %s (known: %s)" % (", ".join(map(repr, unknown)), ", ".join(DISTILL_KEYS)))
    if "teacher" not in args:
        raise ValueError("distill config: a 'teacher' is needed (a Recognizer2D or dict(model=..., checkpoint=...))")
    return KnowledgeDistillation(**args)
