"""Non-finite step guard: the host side that needs no device -- the configuration check.

The guard itself lives in the train engine (TrainEngine.enable_step_guard): the fused optimizer decides on the device whether the step's clip norm is finite
(csrc/optim.hip, mvf_sgd_step_guarded), a skipped step leaves parameters, momentum and the averaged weights untouched, and the BatchNorm running statistics
the step's forward passes have already moved are put back (csrc/precise_bn.hip, mvf_bn_stats_snapshot / mvf_bn_stats_restore).  The Runner reads the
counters where it synchronises anyway and stops the run after `max_consecutive` skipped steps in a row."""
import numpy as np

GUARD_KEYS = ("max_consecutive",)
GUARD_DEFAULTS = dict(max_consecutive=100)


def check_nonfinite_guard(cfg):
    """cfg.nonfinite_guard / Runner(nonfinite_guard=): None (off) or dict(max_consecutive=k); an empty dict gives the default.  Returns None or a dict with the
    key; an unknown key or a max_consecutive that is not an integer >= 1 (a bool is not an integer here) is refused."""
    if cfg is None:
        return None
    if not hasattr(cfg, "keys"):
        raise ValueError("nonfinite_guard must be None or dict(max_consecutive=...), got %r" % (cfg,))
    unknown = sorted(k for k in cfg.keys() if k not in GUARD_KEYS)
    if unknown:
        raise ValueError("nonfinite_guard: unknown key %s (known: %s)" % (", ".join(map(repr, unknown)), ", ".join(GUARD_KEYS)))
    out = dict(GUARD_DEFAULTS)
    out.update({k: cfg[k] for k in cfg.keys()})
    k = out["max_consecutive"]
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1:
        raise ValueError("nonfinite_guard: max_consecutive must be an integer >= 1 (skipped steps in a row before the run stops), got %r" % (k,))
    return dict(max_consecutive=int(k))
