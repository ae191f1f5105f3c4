"""mmcv-free runner shell around the HIP engines: the host-side control flow of the reference's `codes/core/train.py`
(set_random_seed :23-29, parse_losses :32-49, batch_processor :52-60, train_network :63-76, build_optimizer :79-156,
_dist_train / _non_dist_train :159-252) and `codes/core/test.py` (single_gpu_test :12-39, multi_gpu_test :42-89,
collect_results_gpu :147-185), with the schedule the shipped config uses (lr_config: step [90,130] x0.1, linear warm-up 25070
iters from ratio 0.01; mmcv 0.4.3 semantics).  `train_recognizer.py` needs only its imports swapped:

    from mvfnet_amd.runner import init_dist, set_random_seed, train_network      # was: from codes.core import ...
    from mvfnet_amd import build_recognizer                                      # was: from codes.models import ...

What is different by design: the optimizer is not a torch.optim object stepping 161 tensors but a facade (`EngineSGD`) over the
train engine's fused clip + SGD kernel on ONE flat parameter buffer -- same hyper-parameters, same `state_dict()` wire format
(torch.optim.SGD's), same per-parameter `paramwise_options` -- and `EngineAdamW` over its fused Adam / AdamW step for
`optimizer = dict(type='AdamW' | 'Adam', ...)` and `EngineLamb` over its fused LAMB step for `optimizer = dict(type='Lamb', ...)`, with `lr_config` policies 'cosine' and 'poly' beside 'step'; `fp16 = dict(loss_scale=...)` in a config selects the engine's
bf16 storage mode (fp32 master weights / gradients / statistics as the reference's Fp16OptimizerHook keeps them,
codes/core/fp16/hooks.py:12-136; bf16's exponent range makes the loss scale a no-op, it is accepted and ignored).
Host batches are staged through pinned memory and uploaded on a copy stream one batch ahead (the reference's scatter
puts that copy on the critical path, parallel/_functions.py:21-26)."""
import os
import random
import re

import numpy as np
import torch
import torch.distributed as dist

from .checkpoint import load_checkpoint, save_checkpoint
from .dist import get_dist_info, init_dist  # noqa: F401  (re-exported: train_recognizer.py imports init_dist from the core package)
from .ema import check_ema, check_precise_bn
from .diagnostics import check_layer_stats, skip_note, summary as _layer_summary
from .guard import check_nonfinite_guard
from .metrics import check_train_accuracy


def set_random_seed(seed):
    """reference train.py:23-29."""
    random.seed(seed)
    np.random.seed(seed)
    torch.manual_seed(seed)
    if torch.cuda.is_available():
        torch.cuda.manual_seed_all(seed)
    os.environ["PYTHONHASHSEED"] = str(seed)


class Config(dict):
    """Attribute-style dict (what train_network reads from an mmcv Config: cfg.optimizer, cfg.get('fp16'), ...)."""

    def __getattr__(self, k):
        try:
            v = self[k]
        except KeyError:
            raise AttributeError(k)
        return Config(v) if isinstance(v, dict) and not isinstance(v, Config) else v

    def __setattr__(self, k, v):
        self[k] = v


def _cfg_get(cfg, key, default=None):
    if isinstance(cfg, dict):
        return cfg.get(key, default)
    return getattr(cfg, key, default) if not hasattr(cfg, "get") else cfg.get(key, default)


def step_lr(base_lr, epoch, it, steps=(90, 130), gamma=0.1, warmup="linear", warmup_iters=25070, warmup_ratio=0.01):
    """lr at (epoch, global iteration) -- mmcv LrUpdaterHook 'step' policy + linear warm-up."""
    lr = base_lr * (gamma ** sum(1 for s in steps if epoch >= s))
    if warmup is None or it >= warmup_iters:
        return lr
    if warmup == "linear":
        return lr * (1 - (1 - it / float(warmup_iters)) * (1 - warmup_ratio))
    if warmup == "constant":
        return lr * warmup_ratio
    if warmup == "exp":
        return lr * warmup_ratio ** (1 - it / float(warmup_iters))
    raise NotImplementedError("lr_config warmup %r (mmcv LrUpdaterHook knows None, 'constant', 'linear', 'exp')" % (warmup,))


def _progress(epoch, it, by_epoch, max_epochs, max_iters, who):
    progress, max_progress = (epoch, max_epochs) if by_epoch else (it, max_iters)
    if not max_progress or max_progress <= 0:
        raise ValueError("%s: %s is not known (Runner.run sets it; pass it when calling the function directly)" % (who, "max_epochs" if by_epoch else "max_iters"))
    return progress / float(max_progress)


def cosine_lr(base_lr, epoch, it, max_epochs=None, max_iters=None, min_lr=None, min_lr_ratio=None, by_epoch=True, warmup=None, warmup_iters=0,
              warmup_ratio=0.1):
    """lr at (epoch, global iteration) -- mmcv CosineAnnealingLrUpdaterHook:

        target + 0.5 * (base - target) * (1 + cos(pi * progress / max_progress)),      target = min_lr, or base * min_lr_ratio

    exactly one of min_lr / min_lr_ratio is given.  by_epoch (default): progress / max_progress = epoch / max_epochs -- the rate is constant within an epoch --
    else iter / max_iters.  The warm-up forms of step_lr are applied on top, as step_lr applies them (to the annealed rate, while iter < warmup_iters)."""
    if (min_lr is None) == (min_lr_ratio is None):
        raise ValueError("cosine lr policy: give exactly one of min_lr and min_lr_ratio")
    target = base_lr * min_lr_ratio if min_lr_ratio is not None else min_lr
    f = _progress(epoch, it, by_epoch, max_epochs, max_iters, "cosine lr policy")
    lr = target + 0.5 * (base_lr - target) * (1.0 + np.cos(np.pi * f))
    return step_lr(float(lr), 0, it, (), 1.0, warmup, warmup_iters, warmup_ratio)


def poly_lr(base_lr, epoch, it, max_epochs=None, max_iters=None, power=1.0, min_lr=0.0, by_epoch=True, warmup=None, warmup_iters=0, warmup_ratio=0.1):
    """lr at (epoch, global iteration) -- mmcv PolyLrUpdaterHook:

        (base - min_lr) * (1 - progress / max_progress) ** power + min_lr

    with progress / max_progress = epoch / max_epochs when by_epoch (default), else iter / max_iters; warm-up on top as in step_lr."""
    f = _progress(epoch, it, by_epoch, max_epochs, max_iters, "poly lr policy")
    lr = (base_lr - min_lr) * (1.0 - f) ** power + min_lr
    return step_lr(float(lr), 0, it, (), 1.0, warmup, warmup_iters, warmup_ratio)


def check_lr_policy(cfg):
    """lr_config / Runner(lr_policy=): None or dict(policy='step') -> None (the step schedule of lr_steps / lr_gamma); dict(policy='cosine', min_lr= |
    min_lr_ratio=, by_epoch=True) or dict(policy='poly', power=1.0, min_lr=0.0, by_epoch=True) -> a checked copy.  Keys that belong to the step policy or the
    warm-up (step, gamma, warmup, warmup_iters, warmup_ratio) are the runner's own arguments and are ignored here."""
    if cfg is None:
        return None
    cfg = dict(cfg)
    policy = cfg.get("policy", "step")
    if not isinstance(policy, str) or policy.lower() not in ("step", "cosine", "cosineannealing", "poly"):
        raise NotImplementedError("lr_config policy %r: 'step', 'cosine' and 'poly' are built" % (policy,))
    policy = {"cosineannealing": "cosine"}.get(policy.lower(), policy.lower())
    if policy == "step":
        return None
    out = dict(policy=policy, by_epoch=bool(cfg.get("by_epoch", True)))
    if policy == "cosine":
        out.update(min_lr=cfg.get("min_lr"), min_lr_ratio=cfg.get("min_lr_ratio"))
        if (out["min_lr"] is None) == (out["min_lr_ratio"] is None):
            raise ValueError("lr_config policy 'cosine': give exactly one of min_lr and min_lr_ratio")
    else:
        out.update(power=float(cfg.get("power", 1.0)), min_lr=float(cfg.get("min_lr", 0.0)))
    return out


def parse_losses(losses):
    """reference train.py:32-49: mean of every tensor, 'loss' = sum of the entries whose key contains 'loss'."""
    log_vars = {}
    for name, value in losses.items():
        if isinstance(value, torch.Tensor):
            log_vars[name] = value.mean()
        elif isinstance(value, (list, tuple)):
            log_vars[name] = sum(v.mean() for v in value)
        else:
            raise TypeError("%s is not a tensor or list of tensors" % name)
    loss = sum(v for k, v in log_vars.items() if "loss" in k)
    log_vars["loss"] = loss
    return loss, {k: float(v.detach()) for k, v in log_vars.items()}


def batch_processor(model, data, train_mode=True):
    losses = model(**data)
    loss, log_vars = parse_losses(losses)
    return dict(loss=loss, log_vars=log_vars, num_samples=len(data["img_group"]))


# ------------------------------------------------------------------------------------------------ optimizer
def paramwise_multipliers(model, paramwise_options):
    """{parameter: (lr_mult, decay_mult)} by the reference's rules (train.py:117-153): BatchNorm / GroupNorm weights and biases
    (names matching (bn|gn)(\\d+)?.(weight|bias)) get weight_decay * norm_decay_mult; every other `.bias` gets lr * bias_lr_mult
    and weight_decay * bias_decay_mult; parameters with requires_grad False keep the global setting."""
    bias_lr_mult = paramwise_options.get("bias_lr_mult", 1.0)
    bias_decay_mult = paramwise_options.get("bias_decay_mult", 1.0)
    norm_decay_mult = paramwise_options.get("norm_decay_mult", 1.0)
    out = {}
    for name, p in model.named_parameters():
        if not p.requires_grad:
            continue
        if re.search(r"(bn|gn)(\d+)?.(weight|bias)", name):
            out[p] = (1.0, norm_decay_mult)
        elif name.endswith(".bias"):
            out[p] = (bias_lr_mult, bias_decay_mult)
    return out


class EngineSGD(object):
    """The optimizer object `build_optimizer` returns: torch.optim.SGD's surface (param_groups, state_dict, load_state_dict,
    zero_grad, step) over the train engine's flat buffers.  `step()` = all-reduce / world (when a process group is up) + global
    L2 clip (if `grad_clip` was given) + the SGD update, one fused launch sequence."""

    def __init__(self, model, lr, momentum=0.0, dampening=0.0, weight_decay=0.0, nesterov=False, paramwise=None, dtype=None):
        if dampening:
            raise NotImplementedError("SGD dampening != 0 is not built")
        model = model.module if hasattr(model, "module") else model
        opt = dict(lr=lr, momentum=momentum, weight_decay=weight_decay, max_norm=None)
        if dtype is not None:
            opt["dtype"] = dtype
        self.model, self.engine = model, model.train_engine(**opt)
        self.grad_clip = None           # dict(max_norm=..., norm_type=2), set by train_network / the optimizer hooks (dist.py)
        self.engine.max_norm = None
        self.engine.nesterov = bool(nesterov)
        self.engine.set_param_options(paramwise)
        self.param_groups = [dict(lr=lr, initial_lr=lr, momentum=momentum, dampening=0.0, weight_decay=weight_decay, nesterov=bool(nesterov),
                                  params=list(model.parameters()))]

    def zero_grad(self):
        """The engine's backward overwrites the whole flat gradient every step, so nothing is zeroed there; the `.grad` copies that
        autograd hands to the parameters under the hook flow (dist._engine_backed_iter: loss.backward()) are dropped so that they do
        not pile up as an ever-growing sum (torch.optim's set_to_none behaviour)."""
        for p in self.model.parameters():
            p.grad = None

    def step(self, lr=None):
        g = self.param_groups[0]
        self.engine.momentum, self.engine.weight_decay = g["momentum"], g["weight_decay"]
        return self.engine.step(g["lr"] if lr is None else lr)

    def state_dict(self):
        self.engine.lr = self.param_groups[0]["lr"]
        self.engine.initial_lr = self.param_groups[0].get("initial_lr", self.engine.lr)
        return self.engine.optimizer_state_dict()

    def load_state_dict(self, sd):
        self.engine.load_optimizer_state_dict(sd)
        g = self.param_groups[0]
        g.update(lr=self.engine.lr, momentum=self.engine.momentum, weight_decay=self.engine.weight_decay, nesterov=self.engine.nesterov)


class EngineAdamW(object):
    """What `build_optimizer` returns for type='AdamW' | 'Adam': torch.optim.AdamW's surface (param_groups, state_dict, load_state_dict, zero_grad, step) over
    the train engine's fused Adam step (mvf_adamw_step on the flat buffers: exp_avg / exp_avg_sq laid out like the parameters, the step count on the device).
    `step()` = all-reduce / world (when a process group is up) + global L2 clip (if `grad_clip` was given) + the update, one fused launch sequence."""

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, amsgrad=False, maximize=False, decoupled=True, paramwise=None,
                 dtype=None, **unknown):
        if amsgrad:
            raise NotImplementedError("AdamW amsgrad=True is not built")
        if maximize:
            raise NotImplementedError("AdamW maximize=True is not built")
        unknown = {k: v for k, v in unknown.items() if k not in ("foreach", "capturable", "differentiable", "fused") or v}
        if unknown:
            raise TypeError("optimizer config: unexpected keys %s" % sorted(unknown))
        model = model.module if hasattr(model, "module") else model
        opt = dict(lr=lr, weight_decay=weight_decay, max_norm=None, optimizer="adamw" if decoupled else "adam", betas=betas, eps=eps)
        if dtype is not None:
            opt["dtype"] = dtype
        self.model, self.engine = model, model.train_engine(**opt)
        self.grad_clip = None
        self.engine.max_norm = None
        self.engine.set_param_options(paramwise)
        self.param_groups = [dict(lr=lr, initial_lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False,
                                  decoupled_weight_decay=bool(decoupled), params=list(model.parameters()))]

    zero_grad = EngineSGD.zero_grad

    def step(self, lr=None):
        g = self.param_groups[0]
        self.engine.weight_decay = g["weight_decay"]
        if tuple(g["betas"]) != self.engine.betas or g["eps"] != self.engine.eps:
            self.engine.set_optimizer(self.engine.optimizer, betas=g["betas"], eps=g["eps"])
        return self.engine.step(g["lr"] if lr is None else lr)

    def state_dict(self):
        self.engine.lr = self.param_groups[0]["lr"]
        self.engine.initial_lr = self.param_groups[0].get("initial_lr", self.engine.lr)
        return self.engine.optimizer_state_dict()

    def load_state_dict(self, sd):
        self.engine.load_optimizer_state_dict(sd)
        self.param_groups[0].update(lr=self.engine.lr, betas=self.engine.betas, eps=self.engine.eps, weight_decay=self.engine.weight_decay)


class EngineLamb(object):
    """What `build_optimizer` returns for type='Lamb' (timm's class name): EngineAdamW's surface (param_groups, state_dict, load_state_dict, zero_grad, step)
    over the train engine's fused LAMB step (mvf_lamb_step on the flat buffers: exp_avg / exp_avg_sq laid out like the parameters, the step count and one
    trust ratio per parameter tensor on the device; engine.trust_ratios() reads them).  The defaults are timm's (lr 1e-3, betas (0.9, 0.999), eps 1e-6,
    weight_decay 0.01, trust_clip and always_adapt off); bias correction and grad_averaging are always on, so bias_correction=False / grad_averaging=False are
    refused, and timm's max_grad_norm is the runner's grad_clip.  `step()` = all-reduce / world (when a process group is up) + global L2 clip (if `grad_clip`
    was given) + the update, one fused launch sequence."""

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.01, trust_clip=False, always_adapt=False, bias_correction=True,
                 grad_averaging=True, max_grad_norm=None, paramwise=None, dtype=None, **unknown):
        if not grad_averaging:
            raise NotImplementedError("Lamb grad_averaging=False is not built")
        if not bias_correction:
            raise NotImplementedError("Lamb bias_correction=False is not built")
        if max_grad_norm is not None:
            raise NotImplementedError("Lamb max_grad_norm: the clip is the runner's, optimizer_config = dict(grad_clip=dict(max_norm=...))")
        if unknown:
            raise TypeError("optimizer config: unexpected keys %s" % sorted(unknown))
        model = model.module if hasattr(model, "module") else model
        opt = dict(lr=lr, weight_decay=weight_decay, max_norm=None, optimizer="lamb", betas=betas, eps=eps, trust_clip=bool(trust_clip),
                   always_adapt=bool(always_adapt))
        if dtype is not None:
            opt["dtype"] = dtype
        self.model, self.engine = model, model.train_engine(**opt)
        self.grad_clip = None
        self.engine.max_norm = None
        self.engine.set_param_options(paramwise)
        self.param_groups = [dict(lr=lr, initial_lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, lamb=True, trust_clip=bool(trust_clip),
                                  always_adapt=bool(always_adapt), bias_correction=True, grad_averaging=True, params=list(model.parameters()))]

    zero_grad = EngineSGD.zero_grad

    def step(self, lr=None):
        g, eng = self.param_groups[0], self.engine
        eng.weight_decay = g["weight_decay"]
        if tuple(g["betas"]) != eng.betas or g["eps"] != eng.eps or bool(g["trust_clip"]) != eng.trust_clip or bool(g["always_adapt"]) != eng.always_adapt:
            eng.set_optimizer("lamb", betas=g["betas"], eps=g["eps"], trust_clip=g["trust_clip"], always_adapt=g["always_adapt"])
        return eng.step(g["lr"] if lr is None else lr)

    state_dict = EngineAdamW.state_dict

    def load_state_dict(self, sd):
        eng = self.engine
        eng.load_optimizer_state_dict(sd)
        self.param_groups[0].update(lr=eng.lr, betas=eng.betas, eps=eng.eps, weight_decay=eng.weight_decay, trust_clip=eng.trust_clip, always_adapt=eng.always_adapt)


def build_optimizer(model, optimizer_cfg, dtype=None):
    """reference train.py:79-156 for the optimizer the MVFNet configs use: dict(type='SGD', lr, momentum, weight_decay, nesterov
    [, paramwise_options=dict(bias_lr_mult, bias_decay_mult, norm_decay_mult)]) -> EngineSGD, and for fine-tuning configs
    dict(type='AdamW' | 'Adam', lr, betas, eps, weight_decay[, paramwise_options]) -> EngineAdamW (amsgrad / maximize are refused) or
    dict(type='Lamb', lr, betas, eps, weight_decay, trust_clip, always_adapt[, paramwise_options]) -> EngineLamb (grad_averaging=False and unknown keys are
    refused).  Type names are case-sensitive: 'Lamb' is timm's class name."""
    cfg = dict(optimizer_cfg)
    kind = cfg.pop("type", "SGD")
    if kind not in ("SGD", "AdamW", "Adam", "Lamb"):
        raise NotImplementedError("optimizer type %r: the fused HIP optimizers are SGD, AdamW, Adam and Lamb" % kind)
    paramwise = cfg.pop("paramwise_options", None)
    target = model.module if hasattr(model, "module") else model
    if kind != "SGD" and not hasattr(target, "train_engine"):
        raise NotImplementedError("optimizer type %r: the fused %s step lives in a recognizer's train engine; %s has none"
                                  % (kind, "LAMB" if kind == "Lamb" else "Adam", type(target).__name__))
    mult = None
    if paramwise is not None:
        if not isinstance(paramwise, dict):
            raise TypeError("paramwise_options must be a dict")
        if ("bias_decay_mult" in paramwise or "norm_decay_mult" in paramwise) and cfg.get("weight_decay") is None:
            raise ValueError("weight_decay must be given explicitly when a decay multiplier is")        # train.py:123-125
        mult = paramwise_multipliers(target, paramwise)
    if kind == "Lamb":
        return EngineLamb(target, paramwise=mult, dtype=dtype, **cfg)
    if kind != "SGD":
        if kind == "Adam":
            cfg.setdefault("weight_decay", 0.0)          # (torch.optim.Adam's default; AdamW's is 1e-2)
        return EngineAdamW(target, paramwise=mult, dtype=dtype, decoupled=(kind == "AdamW"), **cfg)
    return EngineSGD(target, paramwise=mult, dtype=dtype, **cfg)


# ------------------------------------------------------------------------------------------------ input upload
class DevicePrefetcher(object):
    """Wraps a loader of host batches (dicts of CPU tensors): each batch is copied into pinned staging memory and uploaded on a
    copy stream ONE BATCH AHEAD of the consumer, so the H2D copy (154 MB fp32 / 38.5 MB uint8 per 32-clip step) overlaps the
    previous step's kernels instead of sitting at the head of the step (reference: MMDistributedDataParallel.scatter on the
    compute stream's critical path, parallel/distributed.py:54-62).  Batches already on the device pass through.
    [r3] A batch that is already pinned (DataLoader(pin_memory=True)) is uploaded straight from where it lies -- the staging memcpy of
    154 MB costs the host ~12 ms per step, more than the upload itself -- and lands in one of two PERSISTENT device buffers per key
    (no allocator traffic); a slot is refilled only after the step that read it (an event on the consumer's stream, waited for by
    the copy stream, never by the host).  The yielded tensors are therefore valid until the batch after the next is requested."""

    def __init__(self, loader, device=None):
        self.loader, self.device = loader, torch.device(device or "cuda")
        self.sampler = getattr(loader, "sampler", None)
        self.dataset = getattr(loader, "dataset", None)
        self._copy = None
        self._pinned = [{}, {}]
        self._device = [{}, {}]
        self._consumed = [None, None]      # the consumer's last kernel that READ each device slot: the next upload into it waits for that
        self._slot_event = [None, None]      # the upload that last READ each staging slot: must be complete before the host refills it

    def __len__(self):
        return len(self.loader)

    def _upload(self, batch, slot):
        out, any_host = {}, False
        if self._slot_event[slot] is not None:
            self._slot_event[slot].synchronize()      # two batches old: normally long done, never skipped
        if self._consumed[slot] is not None:          # the device buffers of this slot were read by the step two batches ago:
            torch.cuda.current_stream().wait_event(self._consumed[slot])      # the copy stream waits for that step, the host does not
        for k, v in batch.items():
            if not isinstance(v, torch.Tensor) or v.is_cuda:
                out[k] = v
                continue
            any_host = True
            src = v
            if not v.is_pinned():                     # pageable memory: stage through this slot's pinned buffer (a loader with pin_memory=True skips this copy)
                pin = self._pinned[slot].get(k)
                if pin is None or pin.shape != v.shape or pin.dtype != v.dtype:
                    pin = torch.empty(v.shape, dtype=v.dtype, pin_memory=True)
                    self._pinned[slot][k] = pin
                pin.copy_(v)
                src = pin
            dev = self._device[slot].get(k)           # persistent device-side landing buffers, two slots: no allocator traffic per step
            if dev is None or dev.shape != v.shape or dev.dtype != v.dtype:
                dev = torch.empty(v.shape, dtype=v.dtype, device=self.device)
                self._device[slot][k] = dev
            dev.copy_(src, non_blocking=True)
            out[k] = dev
        ev = None
        if any_host:
            ev = torch.cuda.Event()
            ev.record()
        self._slot_event[slot] = ev
        return out, ev

    def __iter__(self):
        if self.device.type != "cuda":
            for b in self.loader:
                yield b
            return
        if self._copy is None:
            self._copy = torch.cuda.Stream(device=self.device)
        it = iter(self.loader)
        slot, nxt = 0, None

        def fetch():
            try:
                b = next(it)
            except StopIteration:
                return None
            with torch.cuda.stream(self._copy):
                return self._upload(b, slot)

        nxt = fetch()
        while nxt is not None:
            cur, ev = nxt
            cur_slot = slot
            slot ^= 1
            nxt = fetch()                                  # the next batch's copy is in flight while the consumer runs this one
            if ev is not None:
                torch.cuda.current_stream().wait_event(ev)
            yield cur
            if ev is not None:                             # the consumer has queued its work on this batch: mark the slot's last reader
                done = torch.cuda.Event()
                done.record(torch.cuda.current_stream())
                self._consumed[cur_slot] = done


def build_dataloader(dataset, videos_per_gpu, workers_per_gpu=0, dist_mode=False, shuffle=True, drop_last=False, pin_memory=None):
    """A torch DataLoader over `dataset` (items: dict(img_group=tensor, label=tensor)): DistributedSampler (rank::world, as the
    reference's sampler.py:62-78 deals videos) when distributed.  Like the reference's build_dataloader (datasets/builder.py) the
    last, partial batch of an epoch is kept (drop_last=False: the engine's buffers are keyed by shape) -- the iteration count that
    drives the warm-up is the reference's.  pin_memory defaults to the reference's True (datasets/loader/build_loader.py:22) whenever a GPU
    is present: DevicePrefetcher then uploads straight from the loader's pinned batch (no staging memcpy).  Datasets / decode pipelines
    themselves are out of scope."""
    if pin_memory is None:
        pin_memory = torch.cuda.is_available()
    if isinstance(dataset, (torch.utils.data.DataLoader, list, tuple)) or not hasattr(dataset, "__getitem__"):
        return dataset                                     # already a loader / a list or iterable of ready batches
    sampler = None
    if dist_mode:
        rank, world = get_dist_info()
        sampler = torch.utils.data.distributed.DistributedSampler(dataset, world, rank, shuffle=shuffle)
    return torch.utils.data.DataLoader(dataset, batch_size=videos_per_gpu, sampler=sampler, shuffle=(shuffle and sampler is None),
                                       num_workers=workers_per_gpu, pin_memory=pin_memory, drop_last=drop_last)


# ------------------------------------------------------------------------------------------------ runner
def check_accumulate(k):
    """optimizer_config.accumulate / Runner(accumulate=): micro-batches per optimizer step, an integer >= 1."""
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1:
        raise ValueError("accumulate must be an integer >= 1 (micro-batches per optimizer step), got %r" % (k,))
    return int(k)


class Runner(object):
    """Epoch/iteration loop with the reference's hook order: lr update -> forward -> backward -> all-reduce/world ->
    clip -> step -> checkpoint every `ckpt_interval` epochs.  Uses the fused HIP TrainEngine (one flat all-reduce +
    one optimizer kernel)."""

    def __init__(self, model, work_dir=None, lr=0.015, momentum=0.9, weight_decay=1e-4, max_norm=40.0, lr_steps=(90, 130),
                 warmup_iters=25070, warmup_ratio=0.01, ckpt_interval=10, log_interval=20, logger=print, optimizer=None, dtype=None,
                 warmup="linear", lr_gamma=0.1, accumulate=1, ema=None, precise_bn=None, nonfinite_guard=None, lr_policy=None, train_accuracy=None,
                 layer_stats=None):
        """layer_stats = dict(interval=None, on_skip=True, top=1) (an empty dict gives the defaults; diagnostics.check_layer_stats): per-parameter statistics taken on
        the device (TrainEngine.enable_layer_stats).  Every `interval` optimizer steps (None: the log interval) the step in front of the log point is measured;
        at the log point, where the loop synchronises anyway, the logging rank reads the table, appends dict(epoch, iter, step, grad_scale, params) to
        `layer_stats_history` and adds to the END of the log line the `top` smallest and largest update_ratio among trained parameters and the `top` largest
        grad_norm, each with its name.  on_skip=True (needs nonfinite_guard) records every skipped step on the device: ` skipped N` is followed by
        ` (last: iter I, <kind> at <where>)` and the FloatingPointError text ends with the same diagnosis (TrainEngine.last_skip).
        train_accuracy = dict(k=(1, 5)) (an empty dict gives the default): the engine counts the top-k hits of every step's score matrix on the device
        (TrainEngine.enable_train_accuracy: one small launch per forward, outside the launch plans) and the log line gains ` top1 %.4f top5 %.4f` -- the
        accuracy over the steps since the previous log line -- after grad_norm, read where the loop synchronises anyway.  Steps under blending or with soft
        labels are not counted; a window without counted rows logs nan.  Under a process group each rank counts its own share and rank 0 logs its own.
        A model built with train_cfg=dict(distill=...) (distill.py) needs no option here: while its engine has `distill` set, loss_cls is the combined loss and
        the log line gains ` loss_ce %.4f loss_kd %.4f` -- the last step's two terms (TrainEngine.distill_terms) -- behind the accuracy fields.
        lr_policy = None (the step schedule of lr_steps / lr_gamma), dict(policy='cosine', min_lr= | min_lr_ratio=, by_epoch=True) or dict(policy='poly',
        power=1.0, min_lr=0.0, by_epoch=True): mmcv's CosineAnnealing / Poly updater hooks (cosine_lr / poly_lr) with the same warm-up on top; max_epochs and
        max_iters (optimizer steps) are learned in run().
        nonfinite_guard = dict(max_consecutive=100) (an empty dict gives the default): an optimizer step whose clip norm is not finite -- a NaN / inf in a
        gradient, or a sum of squares beyond fp32 -- is skipped on the device and the BatchNorm statistics go back to before it (TrainEngine.enable_step_guard);
        the counters are read where the loop synchronises anyway (the log interval, and always at epoch end): the log line gains `skipped N`, and
        max_consecutive skipped steps in a row raise FloatingPointError -- nothing has been poisoned by then, the live state and the last checkpoint are both
        usable.  `iter`, the learning-rate schedule and the EMA warm-up count ATTEMPTED steps, as a scheduler does under torch's GradScaler.  Checkpoints carry
        the total as meta['skipped_steps'].
        ema = dict(momentum=2e-4, warmup_steps=0) (either key may be left out): the engine keeps an exponential moving average of the parameters, one update
        per optimizer step inside the fused optimizer kernel (TrainEngine.enable_ema); checkpoints carry it as 'ema', hooks can score it (weights='ema').
        precise_bn = dict(num_iters=200, interval=1, weights='live' | 'ema' | 'both') (any key may be left out): an evaluation.PreciseBNHook over the loader this
        runner trains from recomputes the BatchNorm running statistics at epoch end, before the evaluation hooks ('ema' / 'both' need `ema`).
        accumulate = k > 1: gradient accumulation -- k loader batches (micro-batches, each under its own BatchNorm statistics) per optimizer step, the
        reference's 8 x 12-clip recipe on one GPU with videos_per_gpu=12, accumulate=8.  `iter`, the warm-up and the log interval then count OPTIMIZER steps."""
        self.model, self.work_dir = model, work_dir
        self.accumulate = check_accumulate(accumulate)
        self.lr_policy = check_lr_policy(lr_policy)
        self.max_epochs = self.max_iters = None      # known once run() is called: the cosine / poly schedules need them
        self.ema = check_ema(ema)                    # (refused before anything is built)
        self.precise_bn = check_precise_bn(precise_bn)
        self.nonfinite_guard = check_nonfinite_guard(nonfinite_guard)
        self.train_accuracy = check_train_accuracy(train_accuracy)
        self.layer_stats = check_layer_stats(layer_stats, guard_on=self.nonfinite_guard is not None)
        self.layer_stats_history = []
        if self.precise_bn is not None and self.precise_bn["weights"] != "live" and self.ema is None:
            raise ValueError("precise_bn: weights=%r needs averaged weights; set ema (ema_config) as well" % self.precise_bn["weights"])
        self.train_loader = None
        if optimizer is not None:                    # build_optimizer's object: hyper-parameters and param-wise options live there
            self.engine = optimizer.engine
            g = optimizer.param_groups[0]
            lr = g["lr"]
        else:
            opt = dict(lr=lr, momentum=momentum, weight_decay=weight_decay, max_norm=max_norm)
            if dtype is not None:
                opt["dtype"] = dtype
            self.engine = model.train_engine(**opt)
        self.optimizer = optimizer
        self.engine.max_norm = max_norm
        self.engine.initial_lr = lr          # the schedule's base rate: checkpoints carry it beside the current one (mmcv's 'initial_lr')
        self.base_lr, self.lr_steps, self.lr_gamma = lr, tuple(lr_steps), lr_gamma
        self.warmup, self.warmup_iters, self.warmup_ratio = warmup, warmup_iters, warmup_ratio
        self.ckpt_interval, self.log_interval, self.log = ckpt_interval, log_interval, logger
        self.epoch, self.iter = 0, 0
        self.hooks = []               # objects with after_train_epoch(runner), e.g. evaluation.EvalTopKAccuracyHook
        if self.ema is not None:
            self.engine.enable_ema(**self.ema)
        if self.nonfinite_guard is not None:
            self.engine.enable_step_guard()
        if self.train_accuracy is not None:
            self.engine.enable_train_accuracy(**self.train_accuracy)
        if self.layer_stats is not None:
            self.engine.enable_layer_stats(on_skip=self.layer_stats["on_skip"])
        if self.precise_bn is not None:
            from .evaluation import PreciseBNHook
            self.register_hook(PreciseBNHook(None, **self.precise_bn))

    def register_hook(self, hook):
        """Hooks run in registration order, except that one with `before_evaluation` set (evaluation.PreciseBNHook) runs before every hook without it."""
        if getattr(hook, "before_evaluation", False):
            k = next((i for i, h in enumerate(self.hooks) if not getattr(h, "before_evaluation", False)), len(self.hooks))
            self.hooks.insert(k, hook)
        else:
            self.hooks.append(hook)
        return hook

    def current_lr(self):
        if self.lr_policy is not None:
            pol = {k: v for k, v in self.lr_policy.items() if k != "policy"}
            fn = cosine_lr if self.lr_policy["policy"] == "cosine" else poly_lr
            return fn(self.base_lr, self.epoch, self.iter, self.max_epochs, self.max_iters, warmup=self.warmup, warmup_iters=self.warmup_iters,
                      warmup_ratio=self.warmup_ratio, **pol)
        return step_lr(self.base_lr, self.epoch, self.iter, self.lr_steps, self.lr_gamma, self.warmup, self.warmup_iters, self.warmup_ratio)

    def _check_guard(self):
        """Read the step guard's counters (a synchronising 16-byte read: called only where the loop synchronises anyway).  Returns ' skipped N' for the log
        line; raises once max_consecutive optimizer steps in a row have been skipped."""
        if self.nonfinite_guard is None:
            return ""
        st = self.engine.guard_state()
        last = ""
        if self.layer_stats is not None and self.layer_stats["on_skip"]:
            rec = self.engine.last_skip()            # (the record's step is the guard's count; the runner's iter runs ahead of it by a constant)
            last = skip_note(rec, None if rec is None else self.iter - (st["steps"] - rec["step"]))
        if st["consecutive"] >= self.nonfinite_guard["max_consecutive"]:
            raise FloatingPointError(
                "non-finite gradient norm in %d consecutive optimizer steps (max_consecutive=%d), seen between iter %d and iter %d of epoch %d; every one was "
                "skipped on the device: parameters, optimizer state, averaged weights and BatchNorm statistics are those of the last good step%s"
                % (st["consecutive"], self.nonfinite_guard["max_consecutive"], self.iter - st["consecutive"] + 1, self.iter, self.epoch + 1, last))
        return " skipped %d%s" % (st["skipped"], last)

    def _layer_interval(self):
        if self.layer_stats is None:
            return 0
        return self.layer_stats["interval"] or self.log_interval or 0

    def _arm_layer_stats(self):
        """In front of an optimizer step: measure it when the step lands on a statistics point."""
        iv = self._layer_interval()
        if iv and (self.iter + 1) % iv == 0:
            self.engine.measure_layer_stats()

    def _layer_note(self, rank):
        """Behind an optimizer step (iter counted): at a statistics point the logging rank reads the measured step's table (a synchronising read), files the
        full rows in layer_stats_history and returns the log line's suffix; '' elsewhere and with the option off."""
        iv = self._layer_interval()
        if not iv or self.iter % iv != 0 or rank != 0:
            return ""
        fig = self.engine.layer_stats()
        if fig is None:
            return ""
        self.layer_stats_history.append(dict(epoch=self.epoch + 1, iter=self.iter, **fig))
        return _layer_summary(fig["params"], self.layer_stats["top"])

    def _accuracy_note(self):
        """' top1 %.4f top5 %.4f' for the log line: the engine's window since the previous line (a synchronising 128-byte read, made on the logging rank only,
        where the line's loss and norm are read anyway), or '' with the option off."""
        if self.train_accuracy is None:
            return ""
        fig = self.engine.train_accuracy()
        return "".join(" top%d %.4f" % (kk, fig["top%d" % kk]) for kk in self.train_accuracy["k"])

    def _distill_note(self):
        """' loss_ce %.4f loss_kd %.4f' for the log line while the engine distils (engine.distill set: train_cfg['distill']): the two terms loss_cls combines,
        of the last step (an 8-byte synchronising read, on the logging rank only, where the line's loss and norm are read anyway); '' otherwise."""
        if getattr(self.engine, "distill", None) is None:
            return ""
        fig = self.engine.distill_terms()
        return " loss_ce %.4f loss_kd %.4f" % (fig["loss_ce"], fig["loss_kd"])

    def _apply_accumulated(self, rank):
        lr = self.current_lr()
        self._arm_layer_stats()
        self.engine.apply_accumulated(lr=lr)
        self.iter += 1
        layers = self._layer_note(rank)
        if self.log_interval and self.iter % self.log_interval == 0:
            note = self._check_guard()               # on every rank: all of them take the same decisions, so all of them stop together
            if rank == 0:
                self.log("Epoch [%d] iter %d lr %.5f loss_cls %.4f grad_norm %.3f%s%s%s" % (
                    self.epoch + 1, self.iter, lr, float(self.engine.accumulated_loss), float(self.engine.norm_out[0]), self._accuracy_note() + self._distill_note(), note, layers))

    def _train_epoch_accumulated(self, loader, rank):
        """One micro-step per loader batch; the optimizer runs after every k-th batch and after the epoch's last one (a shorter trailing group is applied
        with its real count: nothing is dropped and nothing carries over the epoch boundary, so a checkpoint never sees a partial group)."""
        pending = 0
        for data in loader:
            self.engine.accumulate_step(data["img_group"], data["label"])
            pending += 1
            if pending == self.accumulate:
                self._apply_accumulated(rank)
                pending = 0
        if pending:
            self._apply_accumulated(rank)

    def train_epoch(self, loader):
        self.model.train()
        self.train_loader = loader                   # (what a PreciseBNHook without a loader of its own draws its batches from)
        rank, _ = get_dist_info()
        if self.accumulate > 1:
            self._train_epoch_accumulated(loader, rank)
            loader = ()
        for data in loader:
            lr = self.current_lr()
            self._arm_layer_stats()
            loss = self.engine.train_step(data["img_group"], data["label"], lr=lr)
            self.iter += 1
            layers = self._layer_note(rank)
            if self.log_interval and self.iter % self.log_interval == 0:
                note = self._check_guard()           # on every rank: all of them take the same decisions, so all of them stop together
                if rank == 0:
                    self.log("Epoch [%d] iter %d lr %.5f loss_cls %.4f grad_norm %.3f%s%s%s" % (
                        self.epoch + 1, self.iter, lr, float(loss), float(self.engine.norm_out[0]), self._accuracy_note() + self._distill_note(), note, layers))
        self._check_guard()                          # always at epoch end, before a checkpoint is written
        self.epoch += 1
        if rank == 0 and self.work_dir and self.ckpt_interval and self.epoch % self.ckpt_interval == 0:
            self.save_checkpoint()
        for h in self.hooks:
            out = h.after_train_epoch(self)
            if out and rank == 0 and self.log:
                self.log("Epoch(val) [%d] %s" % (self.epoch, "  ".join("%s: %.4f" % kv for kv in out.items() if kv[0] != "epoch")))

    def run(self, loader, max_epochs):
        if isinstance(loader, (list, tuple)) and loader and not isinstance(loader[0], dict):
            loader = loader[0]        # mmcv Runner.run(data_loaders, workflow, max_epochs): the train loader is first (a list of dicts is a loader of batches)
        self.max_epochs = max_epochs
        if hasattr(loader, "__len__"):               # mmcv: max_iters = max_epochs * len(loader); under accumulation an iter is an optimizer step
            self.max_iters = max_epochs * (-(-len(loader) // self.accumulate))
        while self.epoch < max_epochs:
            if hasattr(getattr(loader, "sampler", None), "set_epoch"):
                loader.sampler.set_epoch(self.epoch)            # DistSamplerSeedHook
            self.train_epoch(loader)

    def save_checkpoint(self):
        """epoch_{n}.pth + latest.pth symlink; {'meta', 'state_dict', 'optimizer'} with the optimizer entry in torch.optim.SGD's
        state_dict layout (reference checkpoint.py:235-265, mmcv CheckpointHook)."""
        path = os.path.join(self.work_dir, "epoch_%d.pth" % self.epoch)
        self.engine.lr = self.current_lr()
        meta = dict(epoch=self.epoch, iter=self.iter)
        if self.nonfinite_guard is not None:
            meta["skipped_steps"] = self.engine.guard_state()["skipped"]
        save_checkpoint(self.model, path, optimizer=self.engine.optimizer_state_dict(), meta=meta,
                        ema=self.engine.ema_state_dict() if self.engine.flat_ema is not None else None)
        latest = os.path.join(self.work_dir, "latest.pth")
        if os.path.lexists(latest):
            os.remove(latest)
        os.symlink(os.path.basename(path), latest)
        return path

    def resume(self, filename):
        """mmcv Runner.resume: weights, epoch / iter from meta, optimizer state (torch.optim.SGD's layout -- a checkpoint written
        by the reference resumes here and vice versa; round 1's own flat layout is still read -- or torch.optim.AdamW's under the
        fused Adam forms: both moments and the device step count, so the next step equals the uninterrupted run's bit for bit)."""
        ckpt = load_checkpoint(self.model, filename, strict=True)
        meta = ckpt.get("meta", {})
        self.epoch, self.iter = meta.get("epoch", 0), meta.get("iter", 0)
        if self.nonfinite_guard is not None and "skipped_steps" in meta:      # (checkpoints without it load as before)
            self.engine.set_skipped_steps(meta["skipped_steps"])
        opt = ckpt.get("optimizer")
        if opt:
            lr, mom, wd = self.engine.lr, self.engine.momentum, self.engine.weight_decay
            kind, betas, eps = self.engine.optimizer, self.engine.betas, self.engine.eps
            self.engine.load_optimizer_state_dict(opt)
            self.engine.lr, self.engine.momentum, self.engine.weight_decay = lr, mom, wd      # the config's values win (lr follows the schedule)
            if kind != "sgd":
                self.engine.set_optimizer(kind, betas=betas, eps=eps)                          # (likewise; the moments and the step count are the checkpoint's)
        if ckpt.get("ema"):
            self.engine.load_ema_state_dict(ckpt["ema"])
            if self.ema is not None:                 # the config's momentum / warm-up win; the averaged weights and the update count are the checkpoint's
                self.engine.ema_momentum, self.engine.ema_warmup_steps = self.ema["momentum"], self.ema["warmup_steps"]
        elif self.ema is not None:
            self.engine.reset_ema()
            if self.log:
                self.log("resume: %s carries no averaged weights ('ema'); the average starts from the loaded weights" % filename)
        return ckpt


def as_config(cfg):
    """A plain dict, this package's Config, an mmcv Config (what the reference's train_recognizer.py passes: the settings live in
    `_cfg_dict`, `vars()` of it shows only _cfg_dict / _filename / _text) or any attribute namespace -> Config."""
    if isinstance(cfg, Config):
        return cfg
    if isinstance(cfg, dict):
        return Config(cfg)
    if hasattr(cfg, "_cfg_dict"):
        d = cfg._cfg_dict
        return Config(d.to_dict() if hasattr(d, "to_dict") else dict(d))
    if hasattr(cfg, "to_dict"):
        return Config(cfg.to_dict())
    return Config({k: v for k, v in vars(cfg).items() if not k.startswith("_")})


def train_network(model, dataset, cfg, distributed=False, validate=False, logger=None):
    """reference train.py:63-76 + _dist_train / _non_dist_train :159-252: loaders, model on the GPU (parameters broadcast from
    rank 0 when distributed), optimizer from cfg.optimizer, grad clip from cfg.optimizer_config, lr schedule from cfg.lr_config,
    (policy 'step', or 'cosine' / 'poly' as mmcv's CosineAnnealing / Poly updater hooks: Runner(lr_policy=...)), checkpoints from cfg.checkpoint_config, logging interval from cfg.log_config, optional fp16 section, resume_from /
    load_from, then run cfg.total_epochs.  cfg.ema_config = dict(momentum=..., warmup_steps=...) keeps averaged weights (Runner(ema=...)).
    cfg.precise_bn = dict(num_iters=..., interval=..., weights=...) recomputes the BatchNorm running statistics at epoch end (Runner(precise_bn=...)).
    cfg.nonfinite_guard = dict(max_consecutive=100) skips optimizer steps with a non-finite gradient norm on the device (Runner(nonfinite_guard=...)).
    cfg.train_accuracy = dict(k=(1, 5)) adds the training top-k accuracy, counted on the device, to the log line (Runner(train_accuracy=...)).
    cfg.layer_stats = dict(interval=None, on_skip=True, top=1) adds per-parameter gradient / weight / update figures at the log points and the diagnosis of
    every skipped step (Runner(layer_stats=...)).
    cfg.evaluation = dict(on_device=True) makes the validation hook of `validate` count its hits on the device (runner.device_test) instead of gathering rows.
    cfg.optimizer_config.accumulate = k (an integer >= 1, default 1) makes one optimizer step of k loader batches
    (gradient accumulation, Runner(accumulate=k)).  `dataset`: a torch Dataset of dict(img_group, label) items, a ready loader, or an
    iterable of batches (or a list whose first entry is the training one).  `validate` registers the reference's
    DistEvalTopKAccuracyHook(cfg.data.val, interval=cfg.eval_interval, k=(1, 5)) for a Dataset OBJECT under cfg.data.val."""
    cfg = as_config(cfg)
    accumulate = check_accumulate(_cfg_get(cfg.get("optimizer_config") or {}, "accumulate", 1))      # (refused before anything is built)
    ema = check_ema(cfg.get("ema_config"))
    precise_bn = check_precise_bn(cfg.get("precise_bn"))
    nonfinite_guard = check_nonfinite_guard(cfg.get("nonfinite_guard"))
    train_accuracy = check_train_accuracy(cfg.get("train_accuracy"))
    layer_stats = check_layer_stats(cfg.get("layer_stats"), guard_on=nonfinite_guard is not None)
    if precise_bn is not None and precise_bn["weights"] != "live" and ema is None:
        raise ValueError("precise_bn: weights=%r needs averaged weights; set ema_config as well" % precise_bn["weights"])
    lrc = cfg.get("lr_config") or {}
    lr_policy = check_lr_policy({k: _cfg_get(lrc, k) for k in ("policy", "by_epoch", "min_lr", "min_lr_ratio", "power") if _cfg_get(lrc, k) is not None})
    log = (logger.info if logger is not None and hasattr(logger, "info") else (logger or print))
    is_list_of_sets = isinstance(dataset, (list, tuple)) and dataset and not isinstance(dataset[0], dict)     # (a list of dicts = ready batches)
    datasets = dataset if is_list_of_sets else [dataset]
    data = cfg.get("data") or {}
    loaders = [build_dataloader(ds, _cfg_get(data, "videos_per_gpu", 1), _cfg_get(data, "workers_per_gpu", 0), dist_mode=distributed)
               for ds in datasets]
    model = model.cuda()
    if distributed:
        from .dist import MMDistributedDataParallel
        MMDistributedDataParallel(model)                              # broadcast of parameters + buffers from rank 0
    fp16_cfg = cfg.get("fp16")
    dtype = torch.bfloat16 if fp16_cfg is not None else None         # fp16 section -> bf16 storage engine (loss_scale accepted, not needed)
    optimizer = build_optimizer(model, cfg.optimizer, dtype=dtype)
    ocfg = cfg.get("optimizer_config") or {}
    clip = _cfg_get(ocfg, "grad_clip")
    steps = _cfg_get(lrc, "step", ())
    ck = cfg.get("checkpoint_config") or {}
    lg = cfg.get("log_config") or {}
    runner = Runner(model, cfg.get("work_dir"), max_norm=(_cfg_get(clip, "max_norm") if clip else None),
                    lr_steps=[steps] if isinstance(steps, int) else tuple(steps), warmup=_cfg_get(lrc, "warmup"),
                    warmup_iters=_cfg_get(lrc, "warmup_iters", 0), warmup_ratio=_cfg_get(lrc, "warmup_ratio", 0.1),
                    lr_gamma=_cfg_get(lrc, "gamma", 0.1), ckpt_interval=_cfg_get(ck, "interval", 0) or 0,
                    log_interval=_cfg_get(lg, "interval", 0) or 0, logger=log, optimizer=optimizer, accumulate=accumulate, ema=ema, precise_bn=precise_bn,
                    nonfinite_guard=nonfinite_guard, lr_policy=lr_policy, train_accuracy=train_accuracy, layer_stats=layer_stats)
    if clip and _cfg_get(clip, "norm_type", 2) != 2:
        raise NotImplementedError("grad_clip norm_type %r: the fused clip is the L2 norm" % _cfg_get(clip, "norm_type"))
    if validate:
        # reference train.py:192-196: DistEvalTopKAccuracyHook(cfg.data.val, interval=cfg.eval_interval, k=(1, 5)).  Here cfg.data.val
        # must be the Dataset OBJECT (items dict(img_group=...), video_infos[i]['label']) -- the dataset classes a config dict would
        # name are out of scope; a ready hook under cfg.eval_hook is taken as is.
        if cfg.get("eval_hook") is not None:
            runner.register_hook(cfg.get("eval_hook"))
        else:
            val = _cfg_get(data, "val")
            if val is None or isinstance(val, dict):
                raise NotImplementedError("validate=True: put the validation Dataset object under cfg.data.val (or a hook under cfg.eval_hook); "
                                          "building datasets from a config dict is out of scope")
            from .evaluation import DistEvalTopKAccuracyHook
            ev = cfg.get("evaluation") or {}
            runner.register_hook(DistEvalTopKAccuracyHook(val, interval=cfg.get("eval_interval", 1), k=(1, 5), dist=distributed,
                                                          on_device=bool(_cfg_get(ev, "on_device", False))))
    if cfg.get("resume_from"):
        runner.resume(cfg.get("resume_from"))
    elif cfg.get("load_from"):
        load_checkpoint(model, cfg.get("load_from"), map_location="cpu")
    train = DevicePrefetcher(loaders[0])
    runner.run(train, cfg.get("total_epochs", 1))
    return runner


# ------------------------------------------------------------------------------------------------ testing
def single_gpu_test(model, loader):
    """reference test.py:12-39: eval mode, no grad, one result row per video."""
    model.eval()
    results = []
    with torch.no_grad():
        for data in loader:
            img = data["img_group"]
            if torch.is_tensor(img) and not img.is_cuda and torch.cuda.is_available():      # a DataLoader's host batch: the reference's MMDataParallel scatters it to the device (test.py:24-27)
                img = img.cuda(non_blocking=True)
            results.append(model(return_loss=False, img_group=img))
    return results


def device_test(model, loader, labels, metrics, rank=None, world=None):
    """single_gpu_test without the per-video readback: every item's score rows stay on the device (forward_test(return_numpy=False)) and are counted there,
    `metrics.update(score, labels[i : i + rows])` with i the item's index in the full label list -- `rank + n * world` for the n-th item of a rank that scores
    the `rank::world` share, the order collect_results assumes.  `labels` (one integer per video; a list, an array, or an int64 device tensor) are uploaded once.  Nothing inside the loop waits for the
    device; the caller ends the pass with metrics.all_reduce() / metrics.compute().  A failing launch raises from the forward as it always did.
    With a metrics.DeviceMultiLabelMetrics, `labels` is the (videos, classes) multi-hot matrix and the rows are recorded for its mean average precision
    (the caller ends the pass with metrics.all_gather() / metrics.compute()).
    rank / world default to the process group's.  Returns `metrics`."""
    if rank is None or world is None:
        rank, world = get_dist_info()
    from .metrics import DeviceMultiLabelMetrics
    if isinstance(metrics, DeviceMultiLabelMetrics):
        # multi-label videos: `labels` is the (videos, classes) multi-hot matrix (bool / uint8 / any numbers, non-zero = positive), uploaded once as uint8
        if torch.is_tensor(labels) and labels.is_cuda and labels.dtype in (torch.uint8, torch.bool):
            lab_dev = labels
        else:
            lab = np.asarray(labels.cpu() if torch.is_tensor(labels) else labels)
            lab_dev = torch.from_numpy(np.ascontiguousarray((lab != 0).astype(np.uint8))).to(metrics.state.device)
        if lab_dev.dim() != 2 or lab_dev.shape[1] != metrics.num_classes:
            raise ValueError("device_test: a DeviceMultiLabelMetrics takes a (videos, %d) label matrix, got %s" % (metrics.num_classes, tuple(lab_dev.shape)))
        lab_dev = lab_dev.contiguous()
    elif torch.is_tensor(labels) and labels.is_cuda:       # already uploaded (int64, one per video)
        lab_dev = labels.reshape(-1)
    else:
        try:
            lab = np.asarray(labels.cpu() if torch.is_tensor(labels) else labels, dtype=np.int64).reshape(-1)
        except (TypeError, ValueError):
            raise ValueError("device_test: one integer label per video is required (multi-label videos: the host path, single_gpu_test + top_k_accuracy)")
        lab_dev = torch.from_numpy(lab).to(metrics.state.device)
    total = lab_dev.shape[0]
    model.eval()
    n = 0
    with torch.no_grad():
        for data in loader:
            img = data["img_group"]
            if torch.is_tensor(img) and not img.is_cuda and torch.cuda.is_available():
                img = img.cuda(non_blocking=True)
            score = model(return_loss=False, return_numpy=False, img_group=img)
            score = score.reshape(-1, score.shape[-1])
            rows = score.shape[0]
            if world > 1 and rows != 1:
                raise ValueError("device_test: %d score rows from one item of a rank::world share; a distributed pass takes one video per item" % rows)
            i = rank + n * world
            if i + rows > total:
                raise ValueError("device_test: item %d brings rows [%d, %d) but there are %d labels" % (n, i, i + rows, total))
            if score.dtype != torch.float32 or not score.is_contiguous():
                score = score.float().contiguous()
            metrics.update(score, lab_dev[i:i + rows])
            n += rows
    return metrics


def collect_results(part, size=None):
    """reference collect_results_gpu (test.py:147-185) for per-video score rows: every rank contributes its `rank::world` share
    (DistributedSampler order); the rows travel as one padded float tensor (instead of pickled bytes) and are re-interleaved on
    rank 0; padding beyond `size` is dropped.  Ranks with an empty shard (fewer videos than ranks) take part with zero rows."""
    rank, world = get_dist_info()
    if world == 1:
        return part if size is None else part[:size]
    dev = torch.device("cuda") if torch.cuda.is_available() and dist.get_backend() == "nccl" else torch.device("cpu")
    rows = [np.asarray(p_, dtype=np.float32).reshape(-1, np.asarray(p_).shape[-1]) for p_ in part]
    mine = torch.from_numpy(np.concatenate(rows, 0)).to(dev) if rows else torch.zeros(0, 0, device=dev)
    # (rows, classes) of every rank first: a rank with an empty shard does not know the row width
    shape = torch.tensor([mine.shape[0], mine.shape[1]], dtype=torch.int64, device=dev)
    shapes = [torch.zeros_like(shape) for _ in range(world)]
    dist.all_gather(shapes, shape)
    counts = [int(s_[0]) for s_ in shapes]
    mx, classes = max(counts), max(int(s_[1]) for s_ in shapes)
    pad = torch.zeros(mx, classes, device=dev)
    if mine.shape[0]:
        pad[: mine.shape[0]] = mine
    parts = [torch.zeros_like(pad) for _ in range(world)]
    dist.all_gather(parts, pad)
    if rank != 0:
        return None
    ordered = []
    for i in range(mx):                      # DistributedSampler deals the videos rank::world: re-interleave
        for r in range(world):
            if i < counts[r]:
                ordered.append(parts[r][i:i + 1].cpu().numpy())
    return ordered if size is None else ordered[:size]


def multi_gpu_test(model, loader, size=None):
    """reference test.py:42-89: every rank scores its share of the videos, rank 0 gets the ordered list (None elsewhere)."""
    return collect_results(single_gpu_test(model, loader), size)
