"""TSN classification head for 2D backbones, MI355X-native.

Mirror of the reference's `codes/models/heads/tsn_clshead.py` (TSNClsHead :6-122) + `heads/base.py` (BaseHead
:8-45) for the avg-consensus configuration MVFNet uses: same constructor arguments, the FC is `new_fc`
(state_dict keys cls_head.new_fc.{weight,bias}), `fcn_testing` flag, `init_weights`, `loss`.

forward(x, num_seg): spatial average pool -> (dropout) -> new_fc -> reshape(-1, num_seg, classes) -> mean over
segments (tsn_clshead.py:71-98); with fcn_testing the 1x1x1 Conv3d + mean[T,H,W] branch (:99-117).  Both are
"mean over the clip's T*H*W positions, then FC" up to fp rounding (pooling, consensus and FC are linear;
SURVEY.md 2.2 measured 1e-5), which is how the HIP head kernel computes them in eval mode.

extract_feat=True (the reference's feature_extractor.py entry point; tsn_clshead.py:89-90, :110-112): eval-mode forward returns that mean
itself, (clips, in_channels) fp32, for both branches; in training mode it is refused.

consensus_cfg=dict(type='TRN' | 'TRNmultiscale', num_frames=T) (tsn_clshead.py:39-44, :63-67; heads/relation.py): the temporal-relation head.  new_fc is
Linear(in_channels, 256), `segmental_consensus` the reference's RelationModule / RelationModuleMultiScale tree (same state_dict keys), and forward is pool ->
(dropout) -> new_fc -> per relation relu(W1 relu(concat f) + b1) -> sum of (W2 h + b2) over the step's relations, in the HIP kernels of csrc/trn_head.hip.  The
relations of the scales below T are drawn per forward from numpy's global generator, in training AND in eval, as the reference does.
DIVERGENCE from the reference: its head passes in_channels as the relation module's img_feature_dim while new_fc emits 256 features per frame, so with
in_channels != 256 its RelationModule.forward raises ("shape '[4, 16384]' is invalid for input of size 8192"); it runs only at in_channels == 256.  This head
builds the relation module with img_feature_dim = 256 whatever in_channels is: at in_channels == 256 the module tree and the numbers are the reference
head's, otherwise those of the reference's RelationModule / RelationModuleMultiScale classes constructed with 256.  init_weights touches new_fc only, as the
reference does.  2 <= T <= 16.  fcn_testing / extract_feat and consensus_cfg keys other than type / num_frames are refused with ValueError.
"""
import numbers

import torch
import torch.nn as nn

from ..builder import HEADS
from .relation import IMG_FEATURE_DIM, RELATION_TYPES, check_num_frames, return_TRN


LOSS_TYPES = ("CrossEntropyLoss", "BCELossWithLogits", "SigmoidFocalLoss", "CBFocalLoss", "AsymmetricLossMultiLabel")
BCE_KEYS = ("type", "pos_weight", "target_threshold", "sum_classes")
# the focal family (csrc/focal.hip): one element function, three ways to name its settings
FOCAL_KEYS = {"SigmoidFocalLoss": ("type", "gamma", "alpha", "class_weight", "target_threshold", "sum_classes"),
              "AsymmetricLossMultiLabel": ("type", "gamma_neg", "gamma_pos", "clip", "class_weight", "target_threshold", "sum_classes"),
              "CBFocalLoss": ("type", "samples_per_cls", "beta", "gamma", "alpha", "sum_classes")}


def class_balanced_weights(samples_per_cls, beta=0.9999):
    """The class-balanced weights of Cui et al. ("Class-Balanced Loss Based on Effective Number of Samples"): w_k = (1 - beta) / (1 - beta ** n_k), formed in
    fp64 and normalised so that they sum to the number of classes; a float64 numpy array.  Every n_k an integer >= 1, 0 <= beta < 1 (beta = 0: all ones).
    In CBFocalLoss the weight multiplies COLUMN k of the loss matrix: the project's own definition -- Cui et al. weight a sample by the class of its single
    label, which is undefined with several labels per row."""
    import numpy as np
    if isinstance(beta, bool) or not isinstance(beta, numbers.Real) or not 0.0 <= beta < 1.0:
        raise ValueError("class_balanced_weights: beta must lie in [0, 1), got %r" % (beta,))
    try:
        raw = list(samples_per_cls)
    except TypeError:
        raise ValueError("class_balanced_weights: samples_per_cls must be a sequence of integers >= 1, got %r" % (samples_per_cls,))
    if not raw or any(isinstance(v, bool) or not isinstance(v, numbers.Integral) or v < 1 for v in raw):
        raise ValueError("class_balanced_weights: samples_per_cls must be a non-empty sequence of integers >= 1, got %r" % (samples_per_cls,))
    n = np.asarray([int(v) for v in raw], dtype=np.float64)
    w = (1.0 - float(beta)) / (1.0 - np.power(float(beta), n))
    return w * (len(raw) / w.sum())


def _gamma(name, v):
    if isinstance(v, bool) or not isinstance(v, numbers.Real) or not (v == 0 or 1.0 <= v <= 16.0):
        raise ValueError("TSNClsHead: loss_cls %s must be 0 or lie in [1, 16], got %r" % (name, v))
    return float(v)


def _check_focal(kind, cfg, num_classes):
    keys = FOCAL_KEYS[kind]
    unknown = sorted(k for k in cfg.keys() if k not in keys)
    if unknown:
        raise ValueError("TSNClsHead: loss_cls %s: unknown key %s (known: %s)" % (kind, ", ".join(map(repr, unknown)), ", ".join(keys)))
    alpha, margin, cw = None, 0.0, cfg.get("class_weight")
    if kind == "AsymmetricLossMultiLabel":
        gp, gn = _gamma("gamma_pos", cfg.get("gamma_pos", 1.0)), _gamma("gamma_neg", cfg.get("gamma_neg", 4.0))
        clip = cfg.get("clip", 0.05)
        if clip is not None:
            if isinstance(clip, bool) or not isinstance(clip, numbers.Real) or not 0.0 <= clip < 1.0:
                raise ValueError("TSNClsHead: loss_cls clip must be None or lie in [0, 1), got %r" % (clip,))
            margin = float(clip)
    else:
        gp = gn = _gamma("gamma", cfg.get("gamma", 2.0))
        alpha = cfg.get("alpha", 0.25 if kind == "SigmoidFocalLoss" else None)
        if alpha is not None:
            if isinstance(alpha, bool) or not isinstance(alpha, numbers.Real) or not 0.0 <= alpha <= 1.0:
                raise ValueError("TSNClsHead: loss_cls alpha must be None or lie in [0, 1], got %r" % (alpha,))
            alpha = float(alpha)
    if kind == "CBFocalLoss":
        if "samples_per_cls" not in cfg.keys():
            raise ValueError("TSNClsHead: loss_cls CBFocalLoss needs samples_per_cls, %d integers >= 1" % num_classes)
        try:
            w = class_balanced_weights(cfg["samples_per_cls"], cfg.get("beta", 0.9999))
        except ValueError as e:
            raise ValueError("TSNClsHead: loss_cls CBFocalLoss: %s" % e)
        if len(w) != num_classes:
            raise ValueError("TSNClsHead: loss_cls samples_per_cls holds %d entries for num_classes=%d" % (len(w), num_classes))
        cw = tuple(float(v) for v in w)
    elif cw is not None:
        try:
            cw = tuple(float(v) for v in cw)
        except (TypeError, ValueError):
            raise ValueError("TSNClsHead: loss_cls class_weight must be None or a sequence of %d numbers, got %r" % (num_classes, cfg.get("class_weight")))
        if len(cw) != num_classes:
            raise ValueError("TSNClsHead: loss_cls class_weight holds %d entries for num_classes=%d" % (len(cw), num_classes))
    thr, sc = cfg.get("target_threshold"), cfg.get("sum_classes", False)
    if thr is not None:
        if isinstance(thr, bool) or not isinstance(thr, numbers.Real) or thr != thr or thr in (float("inf"), float("-inf")):
            raise ValueError("TSNClsHead: loss_cls target_threshold must be None or a finite number, got %r" % (thr,))
        thr = float(thr)
    if not isinstance(sc, bool):
        raise ValueError("TSNClsHead: loss_cls sum_classes must be a bool, got %r" % (sc,))
    return dict(kind="focal", type=kind, gamma_pos=gp, gamma_neg=gn, margin=margin, alpha=alpha, class_weight=cw, target_threshold=thr, sum_classes=sc)


def check_loss_cls(cfg, num_classes):
    """loss_cls of the head: None / dict(type='CrossEntropyLoss') -> None (softmax cross-entropy, the default), or
    dict(type='BCELossWithLogits', pos_weight=None | sequence of num_classes numbers, target_threshold=None | finite float, sum_classes=False) -> a dict
    with the three settings (pos_weight a tuple of floats or None), or one of the focal family (csrc/focal.hip; the arithmetic is in include/mvfnet_hip.h):
      dict(type='SigmoidFocalLoss', gamma=2.0, alpha=0.25 | None, class_weight=None, target_threshold=None, sum_classes=False)
      dict(type='AsymmetricLossMultiLabel', gamma_neg=4.0, gamma_pos=1.0, clip=0.05, class_weight=None, target_threshold=None, sum_classes=False)
      dict(type='CBFocalLoss', samples_per_cls=[...], beta=0.9999, gamma=2.0, alpha=None, sum_classes=False)      -- class_weight = class_balanced_weights
    -> a dict with kind='focal' and gamma_pos, gamma_neg, margin, alpha, class_weight (a tuple or None), target_threshold, sum_classes.
    Any other type raises NotImplementedError; an unknown key or a bad value ValueError."""
    if cfg is None:
        return None
    if not hasattr(cfg, "keys") or "type" not in cfg.keys():
        raise ValueError("TSNClsHead: loss_cls must be None or a dict with a 'type', got %r" % (cfg,))
    kind = cfg["type"]
    if kind not in LOSS_TYPES:
        raise NotImplementedError("TSNClsHead: loss_cls type %r is not built (built: %s)" % (kind, ", ".join(LOSS_TYPES)))
    if kind == "CrossEntropyLoss":
        extra = sorted(k for k in cfg.keys() if k != "type")
        if extra:
            raise ValueError("TSNClsHead: loss_cls CrossEntropyLoss takes no options here, got %s" % ", ".join(map(repr, extra)))
        return None
    if kind in FOCAL_KEYS:
        return _check_focal(kind, cfg, num_classes)
    unknown = sorted(k for k in cfg.keys() if k not in BCE_KEYS)
    if unknown:
        raise ValueError("TSNClsHead: loss_cls BCELossWithLogits: unknown key %s (known: %s)" % (", ".join(map(repr, unknown)), ", ".join(BCE_KEYS)))
    pw, thr, sc = cfg.get("pos_weight"), cfg.get("target_threshold"), cfg.get("sum_classes", False)
    if pw is not None:
        try:
            pw = tuple(float(v) for v in pw)
        except (TypeError, ValueError):
            raise ValueError("TSNClsHead: loss_cls pos_weight must be None or a sequence of %d numbers, got %r" % (num_classes, cfg.get("pos_weight")))
        if len(pw) != num_classes:
            raise ValueError("TSNClsHead: loss_cls pos_weight holds %d entries for num_classes=%d" % (len(pw), num_classes))
    if thr is not None:
        if isinstance(thr, bool) or not isinstance(thr, numbers.Real) or thr != thr or thr in (float("inf"), float("-inf")):
            raise ValueError("TSNClsHead: loss_cls target_threshold must be None or a finite number, got %r" % (thr,))
        thr = float(thr)
    if not isinstance(sc, bool):
        raise ValueError("TSNClsHead: loss_cls sum_classes must be a bool, got %r" % (sc,))
    return dict(pos_weight=pw, target_threshold=thr, sum_classes=sc)


@HEADS.register_module
class TSNClsHead(nn.Module):
    def __init__(self, spatial_type="avg", spatial_size=7, consensus_cfg=dict(type="avg", dim=1), with_avg_pool=False,
                 temporal_feature_size=1, spatial_feature_size=1, dropout_ratio=0.8, in_channels=1024, num_classes=101,
                 init_std=0.001, fcn_testing=False, extract_feat=False, label_smooth_eps=0.0, loss_cls=None):
        super().__init__()
        self.loss_cls = check_loss_cls(loss_cls, num_classes)
        self._pos_weight_dev = None
        self._class_weight_dev = None
        self._focal_params = None
        if isinstance(label_smooth_eps, bool) or not isinstance(label_smooth_eps, numbers.Real) or not 0.0 <= label_smooth_eps < 1.0:
            raise ValueError("TSNClsHead: label_smooth_eps must lie in [0, 1) (got %r)" % (label_smooth_eps,))
        self.label_smooth_eps = float(label_smooth_eps)
        relation = consensus_cfg.get("type") in RELATION_TYPES
        if spatial_type != "avg" or not (relation or (consensus_cfg.get("type") == "avg" and consensus_cfg.get("dim", 1) == 1)):
            raise NotImplementedError("TSNClsHead: only spatial_type='avg' with the 'avg' consensus over dim 1 (the MVFNet configuration) or the "
                                      "'TRN' / 'TRNmultiscale' relation consensus is built")
        if with_avg_pool or temporal_feature_size != 1 or spatial_feature_size != 1:
            raise NotImplementedError("TSNClsHead: with_avg_pool / feature sizes != 1 are not built")
        self.spatial_type, self.spatial_size = spatial_type, spatial_size
        self.consensus_type = consensus_cfg["type"] if relation else "avg"
        self.dropout_ratio, self.in_channels, self.num_classes, self.init_std = dropout_ratio, in_channels, num_classes, init_std
        self.dropout = nn.Dropout(p=dropout_ratio) if dropout_ratio != 0 else None
        if relation:
            # Every refusal before a module is built, let alone a launch.  The reference's fcn_testing branch would load new_fc's 256 rows into a num_classes
            # Conv3d, and its extract_feat branch skips new_fc: neither is a configuration of the relation head.
            unknown = sorted(k for k in consensus_cfg.keys() if k not in ("type", "num_frames"))
            if unknown:
                raise ValueError("TSNClsHead: consensus_cfg %s: unknown key %s (known: 'type', 'num_frames')" % (self.consensus_type, ", ".join(map(repr, unknown))))
            if "num_frames" not in consensus_cfg.keys():
                raise ValueError("TSNClsHead: consensus_cfg %s needs num_frames (the recognizer's n_segment)" % self.consensus_type)
            self.num_frames = check_num_frames(self.consensus_type, consensus_cfg["num_frames"])
            if fcn_testing:
                raise ValueError("TSNClsHead: fcn_testing=True is not a configuration of the %s relation head" % self.consensus_type)
            if extract_feat:
                raise ValueError("TSNClsHead: extract_feat=True is not a configuration of the %s relation head" % self.consensus_type)
            # img_feature_dim = 256 = what new_fc emits, NOT in_channels as the reference passes (see the module docstring)
            self.segmental_consensus = return_TRN(self.consensus_type, IMG_FEATURE_DIM, self.num_frames, num_classes)
            self.new_fc = nn.Linear(in_channels, IMG_FEATURE_DIM)
        else:
            self.new_fc = nn.Linear(in_channels, num_classes)
        self.fcn_testing = fcn_testing
        self.extract_feat = extract_feat
        self._engine = None

    @property
    def is_relation_head(self):
        return self.consensus_type in RELATION_TYPES

    def init_weights(self):
        nn.init.normal_(self.new_fc.weight, 0, self.init_std)
        nn.init.constant_(self.new_fc.bias, 0)
        self._engine = None

    def _apply(self, fn, *a, **k):
        self._engine = None
        self._pos_weight_dev = None
        self._class_weight_dev = None
        return super()._apply(fn, *a, **k)

    def bce_settings(self, device):
        """None for the default loss; else (pos_weight, target_threshold, sum_classes) as mvf_bce_loss takes them: a persistent fp32 device tensor (uploaded
        once per device) or None, a float with NaN = off, 0 / 1."""
        if self.loss_cls is None or self.loss_cls.get("kind") == "focal":
            return None
        pw = None
        if self.loss_cls["pos_weight"] is not None:
            pw, dev = self._pos_weight_dev, torch.device(device)
            if pw is None or pw.device.type != dev.type or (dev.index is not None and pw.device.index != dev.index):
                pw = self._pos_weight_dev = torch.tensor(self.loss_cls["pos_weight"], dtype=torch.float32, device=device)
        thr = self.loss_cls["target_threshold"]
        return pw, float("nan") if thr is None else thr, int(self.loss_cls["sum_classes"])

    def focal_settings(self, device):
        """None unless loss_cls is one of the focal family; else (class_weight, params) as mvf_focal_loss takes them: a persistent fp32 device tensor
        (uploaded once per device) or None, and the _lib.FocalParams struct (host memory, built once: it is immutable for the head's life -- a launch
        plan records its address; other settings need another head)."""
        if self.loss_cls is None or self.loss_cls.get("kind") != "focal":
            return None
        cw = None
        if self.loss_cls["class_weight"] is not None:
            cw, dev = self._class_weight_dev, torch.device(device)
            if cw is None or cw.device.type != dev.type or (dev.index is not None and cw.device.index != dev.index):
                cw = self._class_weight_dev = torch.tensor(self.loss_cls["class_weight"], dtype=torch.float32, device=device)
        if self._focal_params is None:
            from .._lib import FocalParams
            lc = self.loss_cls
            self._focal_params = FocalParams(gamma_pos=lc["gamma_pos"], gamma_neg=lc["gamma_neg"], margin=lc["margin"],
                                             alpha=-1.0 if lc["alpha"] is None else lc["alpha"],
                                             target_threshold=float("nan") if lc["target_threshold"] is None else lc["target_threshold"],
                                             sum_classes=int(lc["sum_classes"]))
        return cw, self._focal_params

    def load_state_dict(self, *a, **k):
        self._engine = None
        return super().load_state_dict(*a, **k)

    def engine(self):
        if self._engine is None:
            from ..engine import HeadEngine
            if self.is_relation_head:
                self._engine = HeadEngine(self.new_fc, self.new_fc.weight.device, relation=self.segmental_consensus, relation_type=self.consensus_type)
            else:
                self._engine = HeadEngine(self.new_fc, self.new_fc.weight.device)
        return self._engine

    def invalidate_engine(self):
        self._engine = None

    def forward(self, x, num_seg, relations=None):
        """x: (N*T, C, h, w) features [or (clips, C, T, h, w) with fcn_testing] -> (clips, num_classes) scores, or with extract_feat the
        (clips, in_channels) consensus of the pooled features.  relations (relation heads only): the int32 (R, 1 + T) table to evaluate instead of
        this forward's draw (heads/relation.py)."""
        if self.is_relation_head:
            if num_seg != self.num_frames:
                raise ValueError("TSNClsHead: consensus_cfg num_frames=%d, but the features come in clips of %d frames" % (self.num_frames, num_seg))
            if x.dim() != 4:
                raise ValueError("TSNClsHead: the %s relation head takes (N*T, C, h, w) features, got %s" % (self.consensus_type, tuple(x.shape)))
        elif relations is not None:
            raise ValueError("TSNClsHead: relations= is an argument of the 'TRN' / 'TRNmultiscale' heads")
        if self.extract_feat and self.training:
            raise NotImplementedError("TSNClsHead: extract_feat=True is an eval-mode path (feature extraction); call .eval() first")
        if not x.is_cuda:
            raise RuntimeError("TSNClsHead: mvfnet_amd runs on MI355X tensors only; no CPU fallback (tests use oracle/)")
        if self.training and self.dropout is not None and torch.is_grad_enabled():
            raise RuntimeError("TSNClsHead: in training the head runs inside Recognizer2D.forward_train (HIP train engine)")
        if x.dim() == 5:                                    # fcn_testing view (clips, C, T, h, w) of the NHWC buffer
            clips, c, t, h, w = x.shape
            feat = x.permute(0, 2, 3, 4, 1).reshape(clips * t, h, w, c)
        else:
            feat = x.permute(0, 2, 3, 1)                     # logical NCHW -> physical NHWC (no copy if channels-last)
        if not feat.is_contiguous():
            feat = feat.contiguous()
        if self.extract_feat:
            return self.engine().features(feat, num_seg)
        if self.is_relation_head:
            return self.engine().scores(feat, num_seg, relations=relations)
        return self.engine().scores(feat, num_seg)

    def loss(self, cls_score, labels):
        """reference heads/base.py:40-45: {'loss_cls': F.cross_entropy(cls_score, labels)} (mean over the clips), computed by the
        HIP cross-entropy kernel of the train head (mvf_ce_loss, csrc/head.hip); no autograd through it -- Recognizer2D.forward_train is the
        path that trains (scores, loss and their gradients in one fused head).
        labels: integers (B,) / (B, 1), or a floating-point (B, num_classes) matrix of soft labels (mvf_ce_loss_soft).  In training mode integer labels are
        smoothed with label_smooth_eps (mvf_soft_targets) as mmaction's head does.
        With loss_cls = BCELossWithLogits the loss is mvf_bce_loss against a target matrix: a bool / uint8 / floating-point (B, num_classes) matrix as it
        is (multi-hot labels), integer labels through mvf_soft_targets.  With one of the focal family (SigmoidFocalLoss, CBFocalLoss,
        AsymmetricLossMultiLabel) the same, through mvf_focal_loss."""
        import ctypes as C
        from .._lib import lib
        from . import loss_calls
        if not cls_score.is_cuda:
            raise RuntimeError("TSNClsHead.loss: mvfnet_amd runs on MI355X tensors only; no CPU fallback (tests use oracle/)")
        s = cls_score.detach().to(torch.float32).contiguous()
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        bce, focal = self.bce_settings(s.device), self.focal_settings(s.device)
        if (bce is not None or focal is not None) and labels.dtype in (torch.bool, torch.uint8) and labels.dim() == 2 and tuple(labels.shape) == tuple(s.shape):
            labels = labels.to(torch.float32)                # multi-hot labels
        soft = labels.is_floating_point() and labels.dim() == 2 and tuple(labels.shape) == tuple(s.shape)
        eps = self.label_smooth_eps if self.training else 0.0
        if soft and eps > 0.0:
            raise ValueError("TSNClsHead.loss: soft (B, num_classes) labels are taken as they are; label_smooth_eps needs integer labels")
        if soft:
            tgt = labels.detach().to(device=s.device, dtype=torch.float32).contiguous()
        else:
            tgt = labels.reshape(-1).to(device=s.device, dtype=torch.int64).contiguous()
            if tgt.numel() != s.shape[0]:
                raise ValueError("TSNClsHead.loss: %d labels for %d score rows" % (tgt.numel(), s.shape[0]))
            # loss_cls = BCELossWithLogits or one of the focal family always runs against a target matrix: mvf_soft_targets' one-hot / smoothed one
            if bce is not None or focal is not None or eps > 0.0:
                tgt, soft = loss_calls.targets_for(lib, tgt, None, None, s.shape[0], s.shape[1], eps, torch.empty_like(s), stream), True
        part = torch.empty(s.shape[0], dtype=torch.float32, device=s.device)
        out = torch.empty(1, dtype=torch.float32, device=s.device)
        loss_calls.stand_alone_loss(lib, loss_calls.loss_kind(bce, focal, soft), s, tgt, s.shape[0], s.shape[1], None, part, out, stream)
        return dict(loss_cls=out.reshape(()))
