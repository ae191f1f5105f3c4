"""Recognizer2D -- the mmaction-style model API of the reference, MI355X-native.

Mirror of `codes/models/recognizers/base.py` (BaseRecognizer :11-82) and `recognizer2d.py` (Recognizer2D :8-179):
built by `build_recognizer(cfg.model, train_cfg, test_cfg)`, children `backbone` / `cls_head` (same state_dict
prefixes), MVF inserted from `module_cfg`, `forward(img_group, label, return_loss=True, return_numpy=True)`.
"""
import torch
import torch.nn as nn

from ..builder import RECOGNIZERS, build_backbone, build_head


class _TrainStepFn(torch.autograd.Function):
    """Whole-model autograd node: forward = HIP train forward + loss, backward = HIP backward chain."""

    @staticmethod
    def forward(ctx, eng, imgs, labels, *params):
        ctx.eng = eng
        ctx.n = len(params)
        loss = eng.forward(imgs, labels).reshape(())
        ctx.token = eng.forward_count          # the engine keeps ONE step's activations: backward must belong to the latest forward
        return loss

    @staticmethod
    def backward(ctx, gout):
        eng = ctx.eng
        if ctx.token != eng.forward_count or eng.saved is None:
            raise RuntimeError("Recognizer2D: backward() of a loss whose activations are gone -- the HIP train engine keeps one step "
                               "(call loss.backward() before the next forward_train, and only once)")
        eng.backward()
        eng.flat_grads.mul_(gout)
        grads = []
        for p in eng.model.parameters():
            v = eng.grad_of(p)
            # a parameter whose .grad IS the flat-buffer view (engine.attach_grads()) already holds its gradient: handing the same
            # memory to autograd's AccumulateGrad would add it to itself; everything else gets its own copy
            aliased = p.grad is not None and p.grad.data_ptr() == v.data_ptr()
            grads.append(None if aliased else v.clone())
        return (None, None, None) + tuple(grads)


@RECOGNIZERS.register_module
class Recognizer2D(nn.Module):
    def __init__(self, modality="RGB", backbone=None, cls_head=None, fcn_testing=False, module_cfg=None,
                 nonlocal_cfg=None, train_cfg=None, test_cfg=None):
        super().__init__()
        if modality != "RGB":
            raise NotImplementedError("only modality='RGB' is built (the MVFNet configs)")
        if nonlocal_cfg:
            raise NotImplementedError("non-local blocks are out of scope")
        if backbone is None or backbone.get("type") != "ResNet":
            raise NotImplementedError("Recognizer2D: backbone type 'ResNet' is the one built here")
        self.fp16_enabled = False
        self.backbone = build_backbone(backbone)
        self.cls_head = build_head(cls_head) if cls_head is not None else None
        if getattr(self.cls_head, "is_relation_head", False):
            # the 'TRN' / 'TRNmultiscale' head (heads/relation.py) concatenates the clip's frames in order: its num_frames is the recognizer's n_segment
            if fcn_testing:
                raise ValueError("Recognizer2D: fcn_testing=True is not a configuration of the %s relation head" % self.cls_head.consensus_type)
            n_seg = module_cfg.get("n_segment") if module_cfg else None
            if n_seg is not None and n_seg != self.cls_head.num_frames:
                raise ValueError("Recognizer2D: cls_head consensus_cfg num_frames=%d, module_cfg n_segment=%d: they must be equal" % (self.cls_head.num_frames, n_seg))
        self.init_weights()
        self.fcn_testing, self.modality = fcn_testing, modality
        self.train_cfg, self.test_cfg = train_cfg, test_cfg
        # train_cfg=dict(blending=dict(type='MixupBlending' | 'CutmixBlending', alpha=...)): batch blending on the device, in forward_train only
        from ..blending import build_blending
        blend_cfg = train_cfg.get("blending") if hasattr(train_cfg, "get") else getattr(train_cfg, "blending", None)
        self.blending = build_blending(blend_cfg)
        # train_cfg=dict(erasing=dict(type='RandomErasing', probability=..., mode='pixel' | 'rand' | 'const', ...)): RandomErasing on the device, likewise
        from ..erasing import build_erasing
        erase_cfg = train_cfg.get("erasing") if hasattr(train_cfg, "get") else getattr(train_cfg, "erasing", None)
        self.erasing = build_erasing(erase_cfg)
        # train_cfg=dict(randaug=dict(type='RandAugment', config='rand-m7-n4-mstd0.5-inc1')): RandAugment on the uploaded uint8 frames, likewise
        from ..randaug import build_randaug
        randaug_cfg = train_cfg.get("randaug") if hasattr(train_cfg, "get") else getattr(train_cfg, "randaug", None)
        self.randaug = build_randaug(randaug_cfg)
        self.module_cfg = dict(module_cfg) if module_cfg else module_cfg
        # train_cfg=dict(distill=dict(type='KnowledgeDistillation', teacher=..., temperature=4.0, alpha=0.5)): the teacher scores the step's stem operand and
        # the loss becomes (1 - alpha) * CE + alpha * T^2 * KL on the device, likewise.  A plain object, not a module: the teacher is no submodule of this model
        from ..distill import build_distill
        distill_cfg = train_cfg.get("distill") if hasattr(train_cfg, "get") else getattr(train_cfg, "distill", None)
        self.distill = build_distill(distill_cfg)
        if self.distill is not None and hasattr(self.distill, "check_student"):
            self.distill.check_student(self, device=False)
        # train_cfg=dict(drop_path=dict(type='DropPath', rate=0.05)): stochastic depth on the bottlenecks' residual branches, drawn per clip, likewise
        from ..droppath import build_drop_path
        drop_cfg = train_cfg.get("drop_path") if hasattr(train_cfg, "get") else getattr(train_cfg, "drop_path", None)
        self.drop_path = build_drop_path(drop_cfg)
        self.in_channels = 3
        if self.module_cfg:
            # reference recognizer2d.py:45-59: weights are initialised/loaded BEFORE the MVF wrappers exist
            self.module_name = self.module_cfg.pop("type")
            if self.module_name != "MVF":
                raise NotImplementedError("module_cfg type %r: only 'MVF' is built" % self.module_name)
            from ..modules.MVF import make_multi_view_fusion
            make_multi_view_fusion(self.backbone, **self.module_cfg)
            self.backbone.invalidate_engine()

    @property
    def with_cls_head(self):
        return self.cls_head is not None

    def init_weights(self):
        self.backbone.init_weights()
        if self.with_cls_head:
            self.cls_head.init_weights()

    def extract_feat(self, img_group):
        return self.backbone(img_group)

    def average_clip(self, cls_score):
        """reference base.py:43-74."""
        if self.test_cfg is None:
            self.test_cfg = dict(average_clips=None)
        if "average_clips" not in self.test_cfg:
            raise KeyError('"average_clips" must defined in test_cfg\'s keys')
        return self.cls_head.engine().average(cls_score, self.test_cfg["average_clips"])

    def set_input_pipeline(self, pipeline):
        """Feed the model DECODED uint8 frames -- `img_group` (B, frames, Hs, Ws, 3) uint8 plus an optional `window=` (frames, 3)
        int32 of per-frame (y0, x0, flip) -- instead of the normalised fp32 tensor: `pipeline` is a preprocess.FramePipeline
        (the config's img_norm_cfg + crop size); crop, flip, Normalize and FormatShape then run inside the stem's input kernel.
        With a preprocess.ResamplingFramePipeline, `window=` is the (frames, 11) int32 row table (train_rows / val_rows / test_rows,
        collate_frames) and Resize / RandomResizedCrop run in that kernel too: frames of any resolution, zero padded to one Hs x Ws.
        With a preprocess.JitterFramePipeline, `window=` is the (frames, 23) int32 table of jitter_rows (geometry + ColorJitter's map).
        With a preprocess.GatherFramePipeline (forward_test only), `img_group` holds a video's DISTINCT decoded frames and `window=` is the
        (images, 12) or (images, 24) int32 table of gather_rows / video_test_table: one row per output image, its trailing `src` column
        naming the frame the image is cut from, so clips and oversampling crops share one upload; 11 / 23 columns mean "no gather".
        With a preprocess.Yuv420FramePipeline, `img_group` is (B, frames, 3 * Hs / 2, pitch) uint8, decoder-native I420 or NV12 frames, with
        any of the tables above; the colour conversion runs in that kernel too.
        With a preprocess.AddressedFramePipeline, `img_group` is (B, frames, S) uint8 -- one slot of S bytes per frame, each frame at its own
        size and row pitch, packed or YUV 4:2:0 (collate_addressed_frames), or any contiguous uint8 tensor whose first two dimensions are
        B and the frame count -- and `window=` is the (images, 16) or (images, 28) int32 table of address_rows: one row per output image,
        its five trailing columns the byte offsets and pitches of the planes the image is cut from.  forward_test takes any row count
        (clips and crops share planes); forward_train takes exactly B * frames rows, so portrait and landscape clips train in one batch
        without padding to a common bounding box."""
        self.input_pipeline = pipeline
        self.backbone.input_pipeline = pipeline
        return self

    def forward(self, img_group, label=None, return_loss=True, return_numpy=True, **kwargs):
        if return_loss:
            return self.forward_train(img_group, label, **kwargs)
        return self.forward_test(img_group, return_numpy, **kwargs)

    # ---- training ---------------------------------------------------------------------------------------------
    def train_engine(self, **opt):
        """The HIP training engine bound to this model (created on first use; parameters become views of one flat
        buffer).  opt: lr, momentum, weight_decay, max_norm (defaults = the reference's optimizer config)."""
        if getattr(self, "_train_engine", None) is None:
            from ..train_engine import TrainEngine
            self._train_engine = TrainEngine(self, **opt)
            self._set_soft_options(self._train_engine, self.training)
        elif opt:                                  # an engine exists already: the options must not be dropped silently
            self._train_engine.set_options(**opt)
        return self._train_engine

    def train(self, mode=True):
        """The engine's blending / label smoothing follow the model's mode (engine.train_step users, e.g. the runner, never pass through forward_train)."""
        super().train(mode)
        if getattr(self, "_train_engine", None) is not None:
            self._set_soft_options(self._train_engine, mode)
        return self

    def _set_soft_options(self, eng, training):
        """The ONE place train_cfg['blending'], train_cfg['erasing'], train_cfg['randaug'], train_cfg['distill'], train_cfg['drop_path'] and the head's label_smooth_eps reach the engine: only while the model trains.  Called
        when the engine is created, whenever the mode changes (train() / eval()) and by forward_train.  engine.blending / engine.erasing / engine.randaug / engine.distill /
        engine.label_smooth_eps are plain attributes: whoever drives engine.train_step directly may also set them by hand, until the next of these calls."""
        eng.blending = self.blending if training else None
        eng.erasing = self.erasing if training else None
        eng.randaug = self.randaug if training else None
        eng.distill = self.distill if training else None       # train_cfg['distill'] (distill.py): the same rule
        eng.drop_path = self.drop_path if training else None   # train_cfg['drop_path'] (droppath.py): the same rule
        eng.label_smooth_eps = float(getattr(self.cls_head, "label_smooth_eps", 0.0)) if training else 0.0
        # the head's loss (loss_cls) is no augmentation: it holds in either mode.  None = softmax cross-entropy.
        if getattr(self.cls_head, "loss_cls", None) is not None:
            eng.bce = self.cls_head.bce_settings(eng.device)
        else:
            eng.bce = None
        # the focal family (SigmoidFocalLoss, CBFocalLoss, AsymmetricLossMultiLabel): bce_settings is None for it, and focal_settings for everything else
        focal = getattr(self.cls_head, "focal_settings", None)
        eng.focal = focal(eng.device) if focal is not None and getattr(self.cls_head, "loss_cls", None) is not None else None

    def forward_train(self, imgs, labels, **kwargs):
        """imgs [B, T, 3, H, W], labels [B, 1] -> {'loss_cls': scalar tensor} (reference recognizer2d.py:132-149).
        labels may also be a floating-point (B, num_classes) matrix of soft labels -- or, with the head's loss_cls = BCELossWithLogits or one of the focal family, a bool / uint8
        (B, num_classes) matrix of multi-hot labels.  While self.training, train_cfg['erasing'] (RandomErasing),
        train_cfg['blending'] (Mixup / CutMix) and the head's label_smooth_eps are applied on the device (mvfnet_amd/erasing.py, mvfnet_amd/blending.py).
        The returned loss supports .backward(): gradients land in the parameters' .grad (copies of the engine's flat gradient
        buffer; after engine.attach_grads() the .grad tensors ARE views of it), as the reference's DistOptimizerHook expects.
        A gather table (preprocess.gather_rows: a `src` column) is refused with a ValueError: training makes one image per frame.  An
        addressed table (preprocess.address_rows: 16 / 28 columns) names its source too, and is taken when it has exactly B * T rows."""
        if not imgs.is_cuda:
            raise RuntimeError("Recognizer2D: mvfnet_amd runs on MI355X tensors only; no CPU fallback (tests use oracle/)")
        pipe, window = getattr(self, "input_pipeline", None), kwargs.get("window")
        if window is not None and getattr(pipe, "gathers", lambda rows: False)(window):
            from ..preprocess import ADDR_COLS, JITTER_COLS, RESAMPLE_COLS
            if window.shape[-1] not in (RESAMPLE_COLS + ADDR_COLS, JITTER_COLS + ADDR_COLS):
                raise ValueError("Recognizer2D.forward_train: a gather table (src column, %d columns) is a test-time input -- training makes one "
                                 "image per frame; use the 11- / 23-column table" % window.shape[-1])
            n = int(window.reshape(-1, window.shape[-1]).shape[0])                # an addressed table names its planes: one row per frame
            if imgs.dim() < 2 or n != imgs.shape[0] * imgs.shape[1]:
                raise ValueError("Recognizer2D.forward_train: an addressed table of %d rows for frames %s -- training makes one image per "
                                 "frame, B * T rows" % (n, tuple(imgs.shape)))
        if self.with_cls_head and getattr(self.cls_head, "extract_feat", False):
            raise NotImplementedError("Recognizer2D.forward_train: cls_head.extract_feat=True is an eval-mode path (feature extraction)")
        # BatchNorms in eval mode (backbone norm_eval=True / frozen stages / partial_norm, reference resnet.py:496-527) normalise with
        # their running statistics and keep them; parameters excluded from training (frozen_stages: a prefix of model.parameters();
        # norm_frozen / partial_norm: BatchNorm weights / biases in scattered places) are skipped by the optimizer kernel
        eng = self.train_engine()
        eng.trainable_offset()
        eng.input_pipeline, eng.input_window = getattr(self, "input_pipeline", None), kwargs.get("window")
        self._set_soft_options(eng, self.training)
        if (eng.bce is not None or eng.focal is not None) and torch.is_tensor(labels) and labels.dtype in (torch.bool, torch.uint8) and labels.dim() == 2 \
                and tuple(labels.shape) == (imgs.shape[0], self.cls_head.num_classes):
            # multi-hot labels: the fp32 target matrix is made HERE, in front of the engine's recorded region (a torch op inside it is dropped on replay)
            labels = labels.to(device=imgs.device, dtype=torch.float32)
        eng.dropout = self.cls_head.dropout_ratio if (self.cls_head.dropout is not None and self.cls_head.training) else 0.0
        params = [p for p in self.parameters()]
        loss = _TrainStepFn.apply(eng, imgs, labels, *params)
        return dict(loss_cls=loss)

    def forward_test(self, imgs, return_numpy=True, **kwargs):
        """imgs [B, clips*crops*T, 3, H, W] -> (1 | clips, num_classes) (reference recognizer2d.py:151-179)."""
        if not imgs.is_cuda:
            raise RuntimeError("Recognizer2D: mvfnet_amd runs on MI355X tensors only; no CPU fallback (tests use oracle/)")
        with torch.no_grad():
            if imgs.dtype == torch.uint8:                                 # decoded frames (B, frames, Hs, Ws, 3), see set_input_pipeline
                k = getattr(getattr(self, "input_pipeline", None), "frame_dims", 3)      # YUV 4:2:0 frames are (3 * Hs / 2, pitch): 2
                x = imgs.reshape((-1,) + tuple(imgs.shape[-k:]))
                self.backbone.engine().input_window = kwargs.get("window")
            else:
                x = imgs.reshape((-1, self.in_channels) + tuple(imgs.shape[3:]))
            feat = self.extract_feat(x)                                   # (B*frames, 2048, h, w), channels-last
            if self.with_cls_head:
                num_seg = self.module_cfg["n_segment"] if self.module_cfg else self.backbone.engine().n_images(x, kwargs.get("window")) // imgs.shape[0]
                # with fcn_testing the reference reshapes to (clips, C, T, h, w) and runs a 1x1x1 conv + mean; the head
                # kernel computes the same mean-then-FC directly from the channels-last features
                cls_score = self.cls_head(feat, num_seg)
                cls_score = self.average_clip(cls_score)
            else:
                cls_score = feat
        return cls_score.cpu().numpy() if return_numpy else cls_score
