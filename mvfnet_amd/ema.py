"""Averaged weights (EMA) and precise BatchNorm: the host side that needs no device -- the configuration checks and the per-step momentum.

The average itself lives in the train engine (TrainEngine.enable_ema: a flat fp32 buffer beside flat_params, updated by the fused optimizer kernels,
csrc/optim.hip / csrc/ema.hip); checkpoints carry it as a top-level 'ema' entry (checkpoint.averaged_state_dict).  Precise BatchNorm (TrainEngine.precise_bn, evaluation.PreciseBNHook)
recomputes the running statistics before evaluation, also for the averaged weights."""
import numpy as np

EMA_KEYS = ("momentum", "warmup_steps")
EMA_DEFAULTS = dict(momentum=2e-4, warmup_steps=0)


def check_ema(cfg):
    """cfg.ema_config / Runner(ema=): None (off) or dict(momentum=..., warmup_steps=...).  Returns None or a dict with both keys; an unknown key, a momentum
    outside (0, 1) or a negative / non-integer warmup_steps is refused."""
    if cfg is None:
        return None
    if not hasattr(cfg, "keys"):
        raise ValueError("ema_config must be None or dict(momentum=..., warmup_steps=...), got %r" % (cfg,))
    unknown = sorted(k for k in cfg.keys() if k not in EMA_KEYS)
    if unknown:
        raise ValueError("ema_config: unknown key %s (known: %s)" % (", ".join(map(repr, unknown)), ", ".join(EMA_KEYS)))
    out = dict(EMA_DEFAULTS)
    out.update({k: cfg[k] for k in cfg.keys()})
    m, w = out["momentum"], out["warmup_steps"]
    if isinstance(m, bool) or not isinstance(m, (int, float, np.floating)) or not 0.0 < float(m) < 1.0:      # (NaN fails the comparison)
        raise ValueError("ema_config: momentum must lie in (0, 1) (the weight of the NEW parameters per optimizer step), got %r" % (m,))
    if isinstance(w, bool) or not isinstance(w, (int, np.integer)) or w < 0:
        raise ValueError("ema_config: warmup_steps must be an integer >= 0, got %r" % (w,))
    return dict(momentum=float(m), warmup_steps=int(w))


def momentum_at(momentum, warmup_steps, t):
    """The weight of the new parameters in update number t (t = updates already made): max(momentum, 1 / (t + 1)) while t < warmup_steps -- a plain running
    mean of the first iterates -- then `momentum`."""
    return max(float(momentum), 1.0 / (t + 1)) if t < warmup_steps else float(momentum)


PRECISE_BN_KEYS = ("num_iters", "interval", "weights")
PRECISE_BN_DEFAULTS = dict(num_iters=200, interval=1, weights="live")
PRECISE_BN_WEIGHTS = ("live", "ema", "both")


def check_precise_bn(cfg):
    """cfg.precise_bn / Runner(precise_bn=): None (off) or dict(num_iters=..., interval=..., weights='live' | 'ema' | 'both').  Returns None or a dict with the
    three keys; an unknown key, a num_iters / interval that is not an integer >= 1 or another `weights` is refused."""
    if cfg is None:
        return None
    if not hasattr(cfg, "keys"):
        raise ValueError("precise_bn must be None or dict(num_iters=..., interval=..., weights=...), got %r" % (cfg,))
    unknown = sorted(k for k in cfg.keys() if k not in PRECISE_BN_KEYS)
    if unknown:
        raise ValueError("precise_bn: unknown key %s (known: %s)" % (", ".join(map(repr, unknown)), ", ".join(PRECISE_BN_KEYS)))
    out = dict(PRECISE_BN_DEFAULTS)
    out.update({k: cfg[k] for k in cfg.keys()})
    for k in ("num_iters", "interval"):
        v = out[k]
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
            raise ValueError("precise_bn: %s must be an integer >= 1, got %r" % (k, v))
        out[k] = int(v)
    if not isinstance(out["weights"], str) or out["weights"] not in PRECISE_BN_WEIGHTS:
        raise ValueError("precise_bn: weights must be one of %s, got %r" % (", ".join(map(repr, PRECISE_BN_WEIGHTS)), out["weights"]))
    return out
