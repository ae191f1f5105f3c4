"""Checkpoint wire format of the reference (codes/utils/checkpoint.py): `{'meta': ..., 'state_dict': ..., 'optimizer': ...}`
written with torch.save; loading accepts a bare state_dict or that dict, strips a leading `module.` (DataParallel /
DDP wrappers, :93-95), is non-strict by default and reports missing / unexpected / size-mismatched keys (:178-217;
`num_batches_tracked` is ignored as missing).  Own implementation; no mmcv, no URL / model-zoo schemes (no network)."""
import os
import time
from collections import OrderedDict

import torch


def _unwrap(module):
    return module.module if hasattr(module, "module") and isinstance(getattr(module, "module"), torch.nn.Module) else module


def load_state_dict(module, state_dict, strict=False, logger=None):
    module = _unwrap(module)
    own = module.state_dict()
    unexpected, mismatched, loaded = [], [], set()
    with torch.no_grad():
        for name, value in state_dict.items():
            if name not in own:
                unexpected.append(name)
                continue
            value = value.data if isinstance(value, torch.nn.Parameter) else value
            if tuple(value.shape) != tuple(own[name].shape):
                mismatched.append("%s: checkpoint %s vs model %s" % (name, tuple(value.shape), tuple(own[name].shape)))
                continue
            own[name].copy_(value)
            loaded.add(name)
    missing = [k for k in own if k not in loaded and not k.endswith("num_batches_tracked")]
    msgs = []
    if unexpected:
        msgs.append("unexpected key in source state_dict: %s" % ", ".join(unexpected))
    if missing:
        msgs.append("missing keys in source state_dict: %s" % ", ".join(missing))
    if mismatched:
        msgs.append("size mismatch: %s" % "; ".join(mismatched))
    if msgs:
        text = "The model and loaded state dict do not match exactly\n" + "\n".join(msgs)
        if strict:
            raise RuntimeError(text)
        from .dist import get_dist_info
        if get_dist_info()[0] == 0:                       # the reference reports on rank 0 only (checkpoint.py:60-68)
            (logger.warning if logger is not None else print)(text)
    if hasattr(module, "invalidate_engine"):
        module.invalidate_engine()
    for m in module.modules():
        if hasattr(m, "invalidate_engine"):
            m.invalidate_engine()
    return dict(missing=missing, unexpected=unexpected, mismatched=mismatched)


def load_checkpoint(model, filename, map_location="cpu", strict=False, logger=None):
    if not isinstance(filename, str) or filename.startswith(("http://", "https://", "modelzoo://", "torchvision://", "open-mmlab://")):
        raise IOError("%r: only local checkpoint files are supported (no network in this build)" % (filename,))
    if not os.path.isfile(filename):
        raise IOError("%s is not a checkpoint file" % filename)
    ckpt = torch.load(filename, map_location=map_location, weights_only=False)
    if isinstance(ckpt, OrderedDict) or (isinstance(ckpt, dict) and "state_dict" not in ckpt):
        sd = ckpt
    elif isinstance(ckpt, dict):
        sd = ckpt["state_dict"]
    else:
        raise RuntimeError("No state_dict found in checkpoint file %s" % filename)
    if sd and all(k.startswith("module.") for k in sd):
        sd = OrderedDict((k[7:], v) for k, v in sd.items())
    load_state_dict(model, sd, strict, logger)
    return ckpt


def weights_to_cpu(state_dict):
    return OrderedDict((k, v.detach().cpu().clone()) for k, v in state_dict.items())


def save_checkpoint(model, filename, optimizer=None, meta=None, ema=None):
    """`ema` (TrainEngine.ema_state_dict()) is written as a top-level 'ema' entry beside meta / state_dict / optimizer; state_dict stays the LIVE weights, so
    the reference's loader and resume, which read only the keys they know (codes/utils/checkpoint.py:178-217), are unaffected."""
    meta = dict(meta or {})
    meta.update(time=time.asctime(), framework="mvfnet_amd")
    os.makedirs(os.path.dirname(os.path.abspath(filename)), exist_ok=True)
    ckpt = dict(meta=meta, state_dict=weights_to_cpu(_unwrap(model).state_dict()))
    if optimizer is not None:
        ckpt["optimizer"] = optimizer.state_dict() if hasattr(optimizer, "state_dict") else optimizer
    if ema is not None:
        ckpt["ema"] = ema
    torch.save(ckpt, filename)
    return filename


def averaged_state_dict(ckpt):
    """The state dict a user hands to inference: the checkpoint's averaged PARAMETERS (its 'ema' entry) with the BatchNorm running statistics measured under
    them where the entry carries some ('bn_stats': TrainEngine.precise_bn(weights='ema')), else -- and for every other buffer -- with the checkpoint's live
    buffers (running statistics are not averaged).  `ckpt`: a loaded checkpoint dict.  Every key of the 'ema' entry must be a key of state_dict with the
    same shape."""
    if not isinstance(ckpt, dict) or "state_dict" not in ckpt:
        raise ValueError("averaged_state_dict: not a checkpoint dict (no 'state_dict')")
    ema = ckpt.get("ema")
    if not ema or "state_dict" not in ema:
        raise KeyError("averaged_state_dict: the checkpoint has no 'ema' entry (it was written without averaged weights: set ema_config / Runner(ema=...))")
    out = OrderedDict((k, v.detach().clone()) for k, v in ckpt["state_dict"].items())
    strip = bool(out) and all(k.startswith("module.") for k in out)
    for name, value in list(ema["state_dict"].items()) + list((ema.get("bn_stats") or {}).items()):
        key = "module." + name if strip else name
        if key not in out:
            raise KeyError("averaged_state_dict: averaged parameter %s is not in the checkpoint's state_dict" % name)
        if tuple(value.shape) != tuple(out[key].shape):
            raise ValueError("averaged_state_dict: %s is %s in the 'ema' entry and %s in state_dict" % (name, tuple(value.shape), tuple(out[key].shape)))
        out[key] = value.detach().clone().to(out[key].dtype)
    return out


# ---- optimizer state: torch.optim.SGD's state_dict layout (what the reference's checkpoints hold, checkpoint.py:262-263) ---------
def sgd_state_dict(momentum_bufs, lr, momentum, weight_decay, nesterov=True, dampening=0.0, multipliers=None, initial_lr=None):
    """{'state': {i: {'momentum_buffer': t}}, 'param_groups': [...]} over n parameters in model.parameters() order;
    momentum_bufs[i] is None for a parameter that has not been stepped (torch creates the buffer at the first step).  One param
    group -- or, with `multipliers` = [(lr_mult, decay_mult)] per parameter, ONE GROUP PER PARAMETER as the reference's paramwise
    build_optimizer makes them (codes/core/train.py:131-153), so torch's load_state_dict finds the group structure it expects.
    Keys of a group = torch.optim.SGD's (older torch ignores the newer ones on load).  `lr` is the CURRENT (scheduled) rate;
    `initial_lr` (the schedule's base rate, x lr_mult per group) is stored beside it as mmcv's LrUpdaterHook does
    (`group.setdefault('initial_lr', group['lr'])` at before_run): without it a checkpoint written after warm-up or an lr step
    would resume under the reference's runner with the decayed rate as its base."""
    n = len(momentum_bufs)
    state = {i: {"momentum_buffer": b} for i, b in enumerate(momentum_bufs) if b is not None}
    base = lr if initial_lr is None else initial_lr

    def group(ids, lr_, wd_, base_):
        return dict(lr=lr_, initial_lr=base_, momentum=momentum, dampening=dampening, weight_decay=wd_, nesterov=bool(nesterov), maximize=False,
                    foreach=None, differentiable=False, fused=None, params=ids)

    if multipliers is None:
        return {"state": state, "param_groups": [group(list(range(n)), lr, weight_decay, base)]}
    return {"state": state, "param_groups": [group([i], lr * a, weight_decay * b, base * a) for i, (a, b) in enumerate(multipliers)]}


def sgd_momentum_buffers(opt_state, n_params):
    """Inverse: per-parameter momentum buffers (None where absent) in parameter order + the (first) param group's hyper-parameters.
    Handles any number of param groups (the reference's paramwise build_optimizer makes one group PER parameter,
    codes/core/train.py:131-153): the packed state ids are the concatenation of the groups' `params` lists."""
    groups = opt_state.get("param_groups")
    if not isinstance(groups, (list, tuple)) or "state" not in opt_state:
        raise ValueError("not a torch optimizer state_dict (keys: %s)" % sorted(opt_state))
    ids = [i for g in groups for i in g["params"]]
    if len(ids) != n_params:
        raise ValueError("optimizer state covers %d parameters, the model has %d" % (len(ids), n_params))
    state = opt_state["state"]
    bufs = []
    for i in ids:
        st = state.get(i, state.get(str(i)))
        bufs.append(None if not st else st.get("momentum_buffer"))
    return bufs, dict(groups[0])


# ---- optimizer state: torch.optim.AdamW's / Adam's state_dict layout (the engine's fused Adam forms, train_engine._apply_adamw) ---------
def adamw_state_dict(step, exp_avgs, exp_avg_sqs, lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled=True, multipliers=None, initial_lr=None):
    """{'state': {i: {'step', 'exp_avg', 'exp_avg_sq'}}, 'param_groups': [...]} over n parameters in model.parameters() order; exp_avgs[i] is None for a
    parameter that has not been stepped (torch creates its state at the first step).  `step` is the number of APPLIED steps, stored per parameter as a
    float32 scalar tensor as torch stores it.  One param group -- or, with `multipliers` = [(lr_mult, decay_mult)] per parameter, one group per parameter, as
    sgd_state_dict makes them.  Keys of a group = torch.optim.AdamW's (decoupled_weight_decay tells Adam from AdamW; older torch ignores the newer keys on
    load).  `lr` is the current rate, `initial_lr` the schedule's base rate, stored as sgd_state_dict stores it."""
    n = len(exp_avgs)
    state = {i: {"step": torch.tensor(float(step), dtype=torch.float32), "exp_avg": m, "exp_avg_sq": v}
             for i, (m, v) in enumerate(zip(exp_avgs, exp_avg_sqs)) if m is not None}
    base = lr if initial_lr is None else initial_lr

    def group(ids, lr_, wd_, base_):
        return dict(lr=lr_, initial_lr=base_, betas=(float(betas[0]), float(betas[1])), eps=float(eps), weight_decay=wd_, amsgrad=False, maximize=False,
                    foreach=None, capturable=False, differentiable=False, fused=None, decoupled_weight_decay=bool(decoupled), params=ids)

    if multipliers is None:
        return {"state": state, "param_groups": [group(list(range(n)), lr, weight_decay, base)]}
    return {"state": state, "param_groups": [group([i], lr * a, weight_decay * b, base * a) for i, (a, b) in enumerate(multipliers)]}


def adamw_moments(opt_state, n_params):
    """Inverse: (step, exp_avgs, exp_avg_sqs, first group): the moments per parameter (None where absent) in parameter order and the ONE step count the
    stepped parameters share -- the engine keeps a single counter, so a state whose parameters disagree is refused.  amsgrad / maximize states are refused."""
    groups = opt_state.get("param_groups")
    if not isinstance(groups, (list, tuple)) or "state" not in opt_state:
        raise ValueError("not a torch optimizer state_dict (keys: %s)" % sorted(opt_state))
    for g in groups:
        for k in ("amsgrad", "maximize"):
            if g.get(k):
                raise NotImplementedError("optimizer state with %s=True: not built" % k)
    ids = [i for g in groups for i in g["params"]]
    if len(ids) != n_params:
        raise ValueError("optimizer state covers %d parameters, the model has %d" % (len(ids), n_params))
    state = opt_state["state"]
    ms, vs, steps = [], [], set()
    for i in ids:
        st = state.get(i, state.get(str(i)))
        if not st:
            ms.append(None)
            vs.append(None)
            continue
        if "exp_avg" not in st or "exp_avg_sq" not in st or "step" not in st:
            raise ValueError("optimizer state of parameter %s has no step / exp_avg / exp_avg_sq (keys: %s): not an Adam / AdamW state" % (i, sorted(st)))
        ms.append(st["exp_avg"])
        vs.append(st["exp_avg_sq"])
        steps.add(int(round(float(st["step"]))))
    if len(steps) > 1:
        raise ValueError("optimizer state: the parameters' step counts differ (%s); the fused optimizer keeps one" % sorted(steps))
    return (steps.pop() if steps else 0), ms, vs, dict(groups[0])


# ---- optimizer state: the fused LAMB step (train_engine._apply_lamb).  THE PROJECT'S OWN FORMAT: Adam's wire layout with the groups marked lamb=True ---------
def lamb_state_dict(step, exp_avgs, exp_avg_sqs, lr, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.0, trust_clip=False, always_adapt=False, multipliers=None,
                    initial_lr=None):
    """adamw_state_dict's layout -- {'state': {i: {'step', 'exp_avg', 'exp_avg_sq'}}, 'param_groups': [...]}, `step` the number of APPLIED steps as a float32
    scalar per stepped parameter, one group or one per parameter under `multipliers` -- with groups that carry lamb=True, trust_clip, always_adapt,
    bias_correction=True and grad_averaging=True (the two timm options the fused step fixes) in place of Adam's amsgrad / decoupled_weight_decay keys.  The state
    entries are the ones timm's Lamb keeps, but timm's own files were not available to compare with: this is the project's format, written and read here."""
    n = len(exp_avgs)
    state = {i: {"step": torch.tensor(float(step), dtype=torch.float32), "exp_avg": m, "exp_avg_sq": v}
             for i, (m, v) in enumerate(zip(exp_avgs, exp_avg_sqs)) if m is not None}
    base = lr if initial_lr is None else initial_lr

    def group(ids, lr_, wd_, base_):
        return dict(lr=lr_, initial_lr=base_, betas=(float(betas[0]), float(betas[1])), eps=float(eps), weight_decay=wd_, lamb=True, trust_clip=bool(trust_clip),
                    always_adapt=bool(always_adapt), bias_correction=True, grad_averaging=True, params=ids)

    if multipliers is None:
        return {"state": state, "param_groups": [group(list(range(n)), lr, weight_decay, base)]}
    return {"state": state, "param_groups": [group([i], lr * a, weight_decay * b, base * a) for i, (a, b) in enumerate(multipliers)]}


def lamb_moments(opt_state, n_params):
    """Inverse, as adamw_moments: (step, exp_avgs, exp_avg_sqs, first group).  A state another optimizer kind wrote -- SGD's (no moments), Adam's / AdamW's (groups
    without lamb=True) -- is a ValueError: its moments mean nothing to this update."""
    step, ms, vs, group = adamw_moments(opt_state, n_params)
    if not all(g.get("lamb") for g in opt_state["param_groups"]):
        raise ValueError("optimizer state: not written by the LAMB optimizer (a param group lacks lamb=True)")
    return step, ms, vs, group
