"""Per-parameter training statistics and the diagnosis of a skipped step: the host side that needs no device.

The figures are taken on the device (csrc/layer_stats.hip: mvf_flat_segment_stats over the flat gradient / parameter buffers, mvf_bn_stats_nonfinite over the
BatchNorm running statistics) and read where the loop synchronises anyway (TrainEngine.layer_stats, TrainEngine.last_skip).  Here: the record layout, the
rows made of the figures, `diagnose` -- what a skipped step's record says about where the first NaN / inf came from --, the log line's summary, and the
configuration check of the runner option, beside guard.check_nonfinite_guard."""
import numpy as np

FLAT_STATS_DTYPE = np.dtype([("sumsq", "<f8"), ("absmax", "<f8"), ("n_nan", "<i8"), ("n_inf", "<i8")])      # mvf_flat_stats_t
KINDS = ("forward", "backward", "loss", "norm_overflow")
LAYER_STATS_KEYS = ("interval", "on_skip", "top")
LAYER_STATS_DEFAULTS = dict(interval=None, on_skip=True, top=1)


def check_layer_stats(cfg, guard_on=None):
    """cfg.layer_stats / Runner(layer_stats=): None (off) or dict(interval=None, on_skip=True, top=1); an empty dict gives the defaults.  Returns None or a
    dict with the three keys.  interval: None (the log interval) or an integer >= 1, in optimizer steps; on_skip: a bool -- diagnose every step the
    non-finite guard skips; top: an integer >= 1, how many names each figure of the log line shows.  An unknown key or a value of another kind is refused (a
    bool is not an integer here).  guard_on: None (not checked), or whether nonfinite_guard is configured: on_skip=True without the guard is refused."""
    if cfg is None:
        return None
    if not hasattr(cfg, "keys"):
        raise ValueError("layer_stats must be None or dict(interval=None, on_skip=True, top=1), got %r" % (cfg,))
    unknown = sorted(k for k in cfg.keys() if k not in LAYER_STATS_KEYS)
    if unknown:
        raise ValueError("layer_stats: unknown key %s (known: %s)" % (", ".join(map(repr, unknown)), ", ".join(LAYER_STATS_KEYS)))
    out = dict(LAYER_STATS_DEFAULTS)
    out.update({k: cfg[k] for k in cfg.keys()})
    iv, top = out["interval"], out["top"]
    if iv is not None and (isinstance(iv, bool) or not isinstance(iv, (int, np.integer)) or iv < 1):
        raise ValueError("layer_stats: interval must be None (the log interval) or an integer >= 1 (optimizer steps), got %r" % (iv,))
    if not isinstance(out["on_skip"], (bool, np.bool_)):
        raise ValueError("layer_stats: on_skip must be True or False, got %r" % (out["on_skip"],))
    if isinstance(top, bool) or not isinstance(top, (int, np.integer)) or top < 1:
        raise ValueError("layer_stats: top must be an integer >= 1 (names shown per figure of the log line), got %r" % (top,))
    if out["on_skip"] and guard_on is not None and not guard_on:
        raise ValueError("layer_stats: on_skip=True diagnoses the steps the non-finite guard skips; set nonfinite_guard as well, or on_skip=False")
    return dict(interval=None if iv is None else int(iv), on_skip=bool(out["on_skip"]), top=int(top))


def as_stats(a):
    """A host array of mvf_flat_stats_t records as a numpy structured array (any array of 32-byte records, or of 4 x 8-byte words per record)."""
    a = np.ascontiguousarray(a)
    return a if a.dtype == FLAT_STATS_DTYPE else a.reshape(-1).view(FLAT_STATS_DTYPE)


def rows(names, trained, grad, weight, update, grad_scale):
    """The per-parameter rows of one measured step, in parameter order: {name: dict(grad_norm, grad_absmax, weight_norm, update_norm, update_ratio, grad_nan,
    grad_inf, weight_nonfinite, update_nonfinite, trained)} from the three records (gradient, parameters before the step, parameters after - before).
    grad_norm / grad_absmax are scaled by the step's grad_scale: what the clip sees.  update_ratio is nan for a parameter of norm 0."""
    grad, weight, update = as_stats(grad), as_stats(weight), as_stats(update)
    out = {}
    for k, name in enumerate(names):
        wn, un = float(np.sqrt(weight["sumsq"][k])), float(np.sqrt(update["sumsq"][k]))
        out[name] = dict(grad_norm=float(np.sqrt(grad["sumsq"][k])) * float(grad_scale), grad_absmax=float(grad["absmax"][k]) * float(grad_scale), weight_norm=wn,
                         update_norm=un, update_ratio=un / wn if wn > 0.0 else float("nan"), grad_nan=int(grad["n_nan"][k]), grad_inf=int(grad["n_inf"][k]),
                         weight_nonfinite=int(weight["n_nan"][k] + weight["n_inf"][k]), update_nonfinite=int(update["n_nan"][k] + update["n_inf"][k]),
                         trained=bool(trained[k]))
    return out


def diagnose(step, bn_names, bn_counts, param_names, trained, grad):
    """What the record of a skipped step says: dict(step, kind, where, detail).

    bn_names / bn_counts: one entry per segment of the running-statistics table (mvf_bn_stats_nonfinite), in the table's order -- the forward order of the
    BatchNorms in training mode, running_mean before running_var; a name is the statistic's state_dict key.  param_names / trained / grad: one entry per
    parameter in model.parameters() order (stem first, head last), grad the mvf_flat_stats_t records of the step's gradient.  Either table may be empty.

      'forward'        some BatchNorm statistic is non-finite: the forward pass itself produced the NaN / inf (an input pixel, an overflow in bf16 storage).
                       where = the FIRST such BatchNorm in the table's order: everything behind it is poisoned by it.  This rule comes first: a poisoned
                       forward poisons the loss and every gradient as well.
      'backward'       statistics finite, some but not all trained parameters hold a non-finite gradient.  where = the LAST such parameter in parameter
                       order: the backward runs from the head to the stem and poisons everything below the layer that went wrong.
      'loss'           statistics finite, EVERY trained parameter's gradient holds a non-finite value, the head's included: the loss was not finite.
                       where = the last trained parameter (the head's).
      'norm_overflow'  not one non-finite element anywhere: the sum of squares left fp32.  where = the trained parameter with the largest absmax (the first
                       of equals); None when no parameter is trained.

    Frozen and norm_eval BatchNorms update no statistic and are not in the table: with every BatchNorm frozen a poisoned forward is reported as 'loss', and
    with some frozen `where` names the first BatchNorm in training mode behind the culprit.  Parameters that are not trained never enter the decision."""
    bn_counts = np.asarray(bn_counts, dtype=np.int64).reshape(-1)
    grad = as_stats(grad) if len(param_names) else np.zeros(0, FLAT_STATS_DTYPE)
    trained = np.asarray(trained, dtype=bool).reshape(-1)
    if len(bn_names) != bn_counts.size or len(param_names) != grad.size or trained.size != grad.size:
        raise ValueError("diagnose: %d / %d BatchNorm entries, %d / %d / %d parameter entries" % (len(bn_names), bn_counts.size, len(param_names), trained.size, grad.size))
    out = dict(step=int(step))
    bad_bn = np.flatnonzero(bn_counts > 0)
    if bad_bn.size:
        key = bn_names[int(bad_bn[0])]
        mod = key.rsplit(".", 1)[0] if key.rsplit(".", 1)[-1] in ("running_mean", "running_var") else key
        of_mod = [int(k) for k in bad_bn if bn_names[int(k)].rsplit(".", 1)[0] == mod]
        out.update(kind="forward", where=mod, detail=dict(statistics={bn_names[k]: int(bn_counts[k]) for k in of_mod}, batchnorms_hit=len(
            {bn_names[int(k)].rsplit(".", 1)[0] for k in bad_bn})))
        return out
    bad = trained & ((grad["n_nan"] + grad["n_inf"]) > 0)
    which = np.flatnonzero(bad)
    if which.size:
        k = int(which[-1])
        kind = "loss" if which.size == int(trained.sum()) else "backward"
        out.update(kind=kind, where=param_names[k], detail=dict(n_nan=int(grad["n_nan"][k]), n_inf=int(grad["n_inf"][k]), parameters_hit=int(which.size),
                                                                 trained=int(trained.sum())))
        return out
    pool = np.flatnonzero(trained)
    if not pool.size:
        out.update(kind="norm_overflow", where=None, detail=dict(absmax=0.0, sumsq=0.0))
        return out
    k = int(pool[int(np.argmax(grad["absmax"][pool]))])          # (argmax: the first of equals)
    out.update(kind="norm_overflow", where=param_names[k], detail=dict(absmax=float(grad["absmax"][k]), sumsq=float(grad["sumsq"][k]),
                                                                       total_sumsq=float(grad["sumsq"][pool].sum())))
    return out


def skip_note(rec, iteration=None):
    """' (last: iter I, <kind> at <where>)' for the log line and the error text; '' without a record.  iteration: the runner's iter of the skipped step."""
    if rec is None:
        return ""
    return " (last: iter %d, %s at %s)" % (rec["step"] if iteration is None else iteration, rec["kind"], rec["where"])


def summary(table, top=1):
    """The log line's suffix from one measured step's rows: the `top` smallest and largest update_ratio among trained parameters and the `top` largest
    grad_norm, each with its name.  Ties go to parameter order; a nan ratio (a parameter of norm 0, a non-finite update) is left out.  '' without a trained row."""
    pick = [(n, r) for n, r in table.items() if r["trained"]]
    ratio = [(r["update_ratio"], i, n) for i, (n, r) in enumerate(pick) if np.isfinite(r["update_ratio"])]
    norm = [(r["grad_norm"], i, n) for i, (n, r) in enumerate(pick) if not np.isnan(r["grad_norm"])]
    fmt = lambda items: ", ".join("%.3g %s" % (v, n) for v, _, n in items)      # noqa: E731
    parts = []
    if ratio:
        lo = sorted(ratio, key=lambda t: (t[0], t[1]))[:top]
        hi = sorted(ratio, key=lambda t: (-t[0], t[1]))[:top]
        parts.append(" upd/w min %s max %s" % (fmt(lo), fmt(hi)))
    if norm:
        parts.append(" gnorm max %s" % fmt(sorted(norm, key=lambda t: (-t[0], t[1]))[:top]))
    return "".join(parts)
