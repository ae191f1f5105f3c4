"""Evaluation metrics and the epoch-end hooks of the runner shell: top-k evaluation and precise BatchNorm before it.

Mirrors the reference's `codes/core/evaluation/accuracy.py` (softmax :4-7, confusion_matrix :10-47, mean_class_accuracy :50-70,
top_k_accuracy :83-100, get_weighted_score :103-124) and `eval_hooks.py` (DistEvalTopKAccuracyHook :86-104) in names, argument
meaning and error behaviour; the arithmetic is vectorised numpy over the (videos x classes) score matrix instead of a Python
loop per video.  Ties follow the reference: its top-k is `np.argsort(score)[-k:]` with numpy's default (unstable) sort kind, so which of several
exactly equal scores makes the cut is numpy's choice; the vectorised form issues the same argsort over the rows of the matrix
(the golden case with quantised scores pins that both give the same answer here) rather than counting strictly greater scores."""
import numpy as np


def softmax(x, dim=1):
    x = np.asarray(x)
    e = np.exp(x - np.max(x, axis=dim, keepdims=True))
    return e / e.sum(axis=dim, keepdims=True)


def _labels_i64(y, name):
    if isinstance(y, list):
        y = np.array(y)
    if not isinstance(y, np.ndarray):
        raise TypeError("%s must be list or np.ndarray, but got %s" % (name, type(y)))
    if not y.dtype == np.int64:
        raise TypeError("%s dtype must be np.int64, but got %s" % (name, y.dtype))
    return y


def confusion_matrix(y_pred, y_real):
    """Rows = real label, columns = predicted label, over the sorted set of labels that occur (accuracy.py:10-47)."""
    y_pred = _labels_i64(y_pred, "y_pred")
    y_real = _labels_i64(y_real, "y_real")
    label_set, inv = np.unique(np.concatenate((y_pred, y_real)), return_inverse=True)
    n = len(label_set)
    ip, ir = inv[: len(y_pred)], inv[len(y_pred):]
    m = min(len(ip), len(ir))                       # the reference zips the two lists
    mat = np.zeros((n, n), dtype=np.int64)
    np.add.at(mat, (ir[:m], ip[:m]), 1)
    return mat


def mean_class_accuracy(scores, labels):
    pred = np.argmax(scores, axis=1)
    cf = confusion_matrix(pred, labels).astype(float)
    cnt, hit = cf.sum(axis=1), np.diag(cf)
    return np.mean(np.where(cnt > 0, hit / np.where(cnt > 0, cnt, 1.0), 0.0))


def top_k_accuracy(scores, labels, k=(1,)):
    """Fraction of videos whose label set meets the top-k classes, one value per k (accuracy.py:83-100).  `labels[i]` is an
    int or an iterable of ints (multi-label videos count as hit if ANY of their labels is in the top k)."""
    scores = [np.asarray(s) for s in scores]
    n = len(scores)
    res = []
    single = all(isinstance(y, (int, np.integer)) for y in labels) and n > 0 and all(s.ndim == 1 and s.shape == scores[0].shape for s in scores)
    if single and len(labels) >= n:
        sc = np.stack(scores)                                           # (n, classes)
        order = np.argsort(sc, axis=1)                                  # the reference's call per row, same (default) sort kind
        lab = np.asarray(labels[:n], dtype=np.int64)
        for kk in k:
            top = order[:, -kk:]
            res.append(np.mean((top == lab[:, None]).any(axis=1)))
        return res
    for kk in k:                                                        # ragged / multi-label input: per-video sets
        hits = []
        for x, y in zip(scores, labels):
            ys = {y} if isinstance(y, (int, np.integer)) else set(y)
            hits.append(len(ys.intersection(np.argsort(x)[-kk:])) > 0)
        res.append(np.mean(hits))
    return res


def get_weighted_score(score_list, coeff_list):
    assert len(score_list) == len(coeff_list)
    num = len(score_list[0])
    for s in score_list[1:]:
        assert len(s) == num
    scores = np.array(score_list)                   # (predictors, samples, classes)
    return list(np.tensordot(np.array(coeff_list), scores, axes=(0, 0)))


def average_precision(scores, labels):
    """Per-class step-wise average precision of a (videos, classes) score matrix against (videos, classes) multi-hot labels (non-zero = positive):
    AP_c = (1 / |P_c|) * sum_{i in P_c} TP_i / N_i with N_i = #{j : s_jc >= s_ic} and TP_i = #{j in P_c : s_jc >= s_ic} -- scikit-learn's
    average_precision_score, what mmaction2 reports; summed over a tie group the terms are dTP * TP / N at that threshold, so ties need no special case.
    Rows holding a NaN score are left out of every class.  Returns (ap float64 (classes,), NaN where a class has no positive; positives int64 (classes,)).
    The definition csrc/multilabel_metrics.hip computes on the device (metrics.DeviceMultiLabelMetrics); here one sort per class."""
    s = np.asarray(scores, dtype=np.float64)
    y = np.asarray(labels) != 0
    if s.ndim != 2 or y.shape != s.shape:
        raise ValueError("average_precision: scores %s and labels %s must be two (videos, classes) matrices" % (s.shape, y.shape))
    keep = ~np.isnan(s).any(axis=1)
    s, y = s[keep], y[keep]
    n, classes = s.shape
    ap, positives = np.full(classes, np.nan), y.sum(axis=0).astype(np.int64)
    for c in range(classes):
        if positives[c] == 0:
            continue
        order = np.argsort(s[:, c], kind="stable")
        sc, yc = s[order, c], y[order, c]
        first = np.searchsorted(sc, sc[yc], side="left")          # rows [first, n) score >= the positive's
        below = np.concatenate(([0], np.cumsum(yc)))               # positives among the first k sorted rows
        ap[c] = np.sum((positives[c] - below[first]) / (n - first)) / positives[c]
    return ap, positives


def mean_average_precision(scores, labels):
    """The mean of average_precision over the classes with at least one positive (mmaction2's mean_average_precision); nan when no class has one."""
    ap, positives = average_precision(scores, labels)
    return float(np.mean(ap[positives > 0])) if (positives > 0).any() else float("nan")


def _multilabel_inputs(who, scores, labels):
    s = np.asarray(scores, dtype=np.float64)
    y = np.asarray(labels) != 0
    if s.ndim != 2 or y.shape != s.shape:
        raise ValueError("%s: scores %s and labels %s must be two (videos, classes) matrices" % (who, s.shape, y.shape))
    return s, y, ~np.isnan(s).any(axis=1)


def sample_average_precision(scores, labels):
    """Per-VIDEO step-wise average precision: average_precision taken along a row, AP_i = (1 / |P_i|) * sum_{c in P_i} TP_ic / N_ic with
    N_ic = #{k : s_ik >= s_ic} and TP_ic = #{k in P_i : s_ik >= s_ic}.  Returns (ap float64 (videos,), NaN for a row without a positive and for a row
    holding a NaN score; positives int64 (videos,), 0 for such a row).  What csrc/multilabel_f1.hip computes on the device."""
    s, y, keep = _multilabel_inputs("sample_average_precision", scores, labels)
    ap, positives = np.full(s.shape[0], np.nan), np.zeros(s.shape[0], dtype=np.int64)
    if keep.any():
        ap[keep], positives[keep] = average_precision(s[keep].T, y[keep].T)
    return ap, positives


def mmit_mean_average_precision(scores, labels):
    """The sample-wise mAP Multi-Moments in Time reports (mmaction2's mmit_mean_average_precision): the mean of sample_average_precision over the videos
    with at least one positive; nan when no video has one."""
    ap, positives = sample_average_precision(scores, labels)
    return float(np.mean(ap[positives > 0])) if (positives > 0).any() else float("nan")


def prf_from_counts(counts):
    """Precision / recall / F1 from (classes, 4) integer counts TP, FP, FN, TN.  Conventions: a ratio whose denominator is 0 is 0 (precision of a class
    never predicted, recall of a class without a positive, F1 = 2TP / (2TP + FP + FN) of a class with neither); micro_* come from the counts summed over
    the classes; macro_f1 is the mean of the per-class F1 over the classes with at least one positive (TP + FN > 0), nan when there is none."""
    counts = np.asarray(counts, dtype=np.int64).reshape(-1, 4)
    tp, fp, fn = (counts[:, i].astype(np.float64) for i in range(3))

    def ratio(a, b):
        return np.divide(a, b, out=np.zeros_like(np.asarray(a, dtype=np.float64)), where=np.asarray(b) > 0)
    f1 = ratio(2.0 * tp, 2.0 * tp + fp + fn)
    have = (counts[:, 0] + counts[:, 2]) > 0
    stp, sfp, sfn = tp.sum(), fp.sum(), fn.sum()
    return dict(counts=counts, precision=ratio(tp, tp + fp), recall=ratio(tp, tp + fn), f1=f1,
                micro_precision=float(ratio(stp, stp + sfp)), micro_recall=float(ratio(stp, stp + sfn)), micro_f1=float(ratio(2.0 * stp, 2.0 * stp + sfp + sfn)),
                macro_f1=float(np.mean(f1[have])) if have.any() else float("nan"))


def precision_recall_f1(scores, labels, threshold=None, thresholds=None):
    """Counts and precision / recall / F1 of "video i is predicted for class c iff s_ic >= theta_c", theta_c = thresholds[c] when given (one per class),
    else `threshold`; the thresholds are rounded to fp32, as the device path takes them (metrics.DeviceMultiLabelMetrics.compute(threshold=...)).  Rows
    holding a NaN score are left out.  Returns the dict of prf_from_counts (its conventions hold)."""
    s, y, keep = _multilabel_inputs("precision_recall_f1", scores, labels)
    th = check_thresholds("precision_recall_f1", threshold, thresholds, s.shape[1]).astype(np.float64)
    s, y = s[keep], y[keep]
    pred = s >= th[None, :]
    counts = np.stack([(pred & y).sum(axis=0), (pred & ~y).sum(axis=0), (~pred & y).sum(axis=0), (~pred & ~y).sum(axis=0)], axis=1).astype(np.int64)
    return prf_from_counts(counts)


def check_thresholds(who, threshold, thresholds, classes):
    """Exactly one of threshold (a number) / thresholds (one number per class), none NaN -> a float32 (classes,) array."""
    if (threshold is None) == (thresholds is None):
        raise ValueError("%s: give either threshold or thresholds" % who)
    if thresholds is None:
        if isinstance(threshold, bool) or not isinstance(threshold, (int, float, np.integer, np.floating)) or threshold != threshold:
            raise ValueError("%s: threshold must be a number, not NaN, got %r" % (who, threshold))
        return np.full(classes, threshold, dtype=np.float32)
    th = np.asarray(thresholds, dtype=np.float32).reshape(-1)
    if th.shape[0] != classes or np.isnan(th).any():
        raise ValueError("%s: thresholds must hold %d numbers, none NaN, got %r" % (who, classes, thresholds))
    return th


def best_f1_from_counts(best_tp, best_n, positives):
    """dict(best_f1 (classes,) = 2 TP / (N + |P_c|), NaN for a class without a positive; macro_best_f1 = its mean over the classes with one)."""
    tp, n, p = (np.asarray(a, dtype=np.float64).reshape(-1) for a in (best_tp, best_n, positives))
    f = np.full(tp.shape[0], np.nan)
    have = p > 0
    f[have] = 2.0 * tp[have] / (n[have] + p[have])
    return dict(best_f1=f, macro_best_f1=float(np.mean(f[have])) if have.any() else float("nan"))


def best_f1_thresholds(scores, labels):
    """Per class, the threshold (>=) with the best achievable F1.  The maximum over all thresholds is attained at a positive's score (raising a threshold
    to the next predicted positive drops only false positives), so the candidates are the positives i of the class, with F_i = 2 TP_i / (N_i + |P_c|)
    from average_precision's counts; fractions are compared exactly and ties go to the larger score.  Rows holding a NaN score are left out.  Returns
    dict(best_f1, best_threshold (NaN for a class without a positive), best_tp, best_n, positives, macro_best_f1)."""
    from fractions import Fraction
    s, y, keep = _multilabel_inputs("best_f1_thresholds", scores, labels)
    s, y = s[keep], y[keep]
    n, classes = s.shape
    positives = y.sum(axis=0).astype(np.int64)
    best_tp, best_n, best_th = np.zeros(classes, dtype=np.int64), np.zeros(classes, dtype=np.int64), np.full(classes, np.nan)
    for c in range(classes):
        if positives[c] == 0:
            continue
        order = np.argsort(s[:, c], kind="stable")
        sc, yc = s[order, c], y[order, c]
        first = np.searchsorted(sc, sc[yc], side="left")
        below = np.concatenate(([0], np.cumsum(yc)))
        tp, nn, sp = positives[c] - below[first], n - first, sc[yc]
        f = 2.0 * tp / (nn + positives[c])
        cand = np.nonzero(f >= f.max() * (1.0 - 1e-12))[0]          # the float picks the few candidates, the exact comparison the winner
        k = max(cand, key=lambda i: (Fraction(int(tp[i]), int(nn[i] + positives[c])), sp[i]))
        best_tp[c], best_n[c], best_th[c] = tp[k], nn[k], sp[k]
    return dict(best_threshold=best_th, best_tp=best_tp, best_n=best_n, positives=positives, **best_f1_from_counts(best_tp, best_n, positives))


WEIGHTS = ("live", "ema", "both")


class EvalTopKAccuracyHook(object):
    """After every `interval`-th training epoch: score the validation set with the model in eval mode (every rank its
    `rank::world` share, rows gathered on rank 0 -- `runner.multi_gpu_test`) and log top-k accuracy
    (eval_hooks.py:17-104; the reference exchanges pickled temp files through `work_dir`, here the rows travel as one
    all_gather of float tensors)."""

    def __init__(self, loader, labels, interval=1, k=(1, 5), weights="live", on_device=False, mean_class=False):
        """weights = 'live' (the parameters being trained), 'ema' (the averaged parameters the engine keeps: Runner(ema=...) / cfg.ema_config; scored inside
        engine.averaged_weights(), figures labelled 'ema top1 acc', ...) or 'both' (two passes over the validation set, both sets of figures).
        on_device = True: the pass is runner.device_test -- no score row leaves the device, the hits are counted there (metrics.DeviceMetrics), one all-reduce
        of the counters merges the ranks and ONE read ends the pass.  It needs one score row per video (test_cfg.average_clips 'prob' or 'score') and one
        integer label per video; ties at the k-th place go to the lower class index, where the host path leaves them to numpy's argsort.
        mean_class = True adds 'mean_class acc' (evaluation.mean_class_accuracy) to the figures of either path."""
        if weights not in WEIGHTS:
            raise ValueError("weights must be one of %s, got %r" % (", ".join(map(repr, WEIGHTS)), weights))
        self.loader, self.labels, self.interval, self.k, self.weights = loader, list(labels), interval, tuple(k), weights
        self.on_device, self.mean_class = bool(on_device), bool(mean_class)
        self._metrics, self._share = None, None      # the device counters (built at the first pass); (rank, world) of the loader's share, None = the process group's
        self.history = []

    def _score(self, runner, prefix):
        if self.on_device:
            return self._score_on_device(runner, prefix)
        from .runner import multi_gpu_test
        was_training = runner.model.training
        results = multi_gpu_test(runner.model, self.loader, size=len(self.labels))
        runner.model.train(was_training)
        if results is None:                          # not rank 0
            return None
        rows = [np.asarray(r).squeeze() for r in results]
        acc = top_k_accuracy(rows, self.labels, k=self.k)
        out = {"%stop%d acc" % (prefix, kk): float(a) for kk, a in zip(self.k, acc)}
        if self.mean_class:
            out["%smean_class acc" % prefix] = float(mean_class_accuracy(np.stack(rows), np.asarray(self.labels[:len(rows)], dtype=np.int64)))
        return out

    def _score_on_device(self, runner, prefix):
        from .dist import get_dist_info
        from .metrics import DeviceMetrics
        from .runner import device_test
        model = runner.model.module if hasattr(runner.model, "module") else runner.model
        test_cfg = getattr(model, "test_cfg", None)
        if test_cfg is None or test_cfg.get("average_clips") is None:
            raise ValueError("evaluation hook with on_device=True: test_cfg.average_clips=None leaves several score rows per video; the device counters "
                             "take one row per video (average_clips='prob' or 'score'), or use the host path (on_device=False)")
        if self._metrics is None:
            self._metrics = DeviceMetrics(model.cls_head.num_classes, k=self.k, confusion=self.mean_class)
        self._metrics.reset()
        rank, world = self._share if self._share is not None else get_dist_info()
        was_training = runner.model.training
        device_test(runner.model, self.loader, self.labels, self._metrics, rank=rank, world=world)
        runner.model.train(was_training)
        if world > 1:
            self._metrics.all_reduce()
        fig = self._metrics.compute()                # every rank holds the figures; rank 0 reports them
        if get_dist_info()[0] != 0:
            return None
        out = {"%stop%d acc" % (prefix, kk): float(fig["top%d" % kk]) for kk in self.k}
        if self.mean_class:
            out["%smean_class acc" % prefix] = float(fig["mean_class_acc"])
        return out

    def after_train_epoch(self, runner):
        if (runner.epoch % self.interval) != 0:
            return None
        out = {}
        if self.weights != "live":
            eng = getattr(runner, "engine", None)
            if eng is None or getattr(eng, "flat_ema", None) is None:
                raise RuntimeError("evaluation hook with weights=%r: the runner keeps no averaged weights; set ema_config (Runner(ema=dict(momentum=...)))" % self.weights)
        if self.weights != "ema":
            out = self._score(runner, "")
        if self.weights != "live":
            with runner.engine.averaged_weights():
                ema = self._score(runner, "ema ")
            out = None if out is None or ema is None else dict(out, **ema)
        if out is None:
            return None
        out["epoch"] = runner.epoch
        self.history.append(out)
        return out


class EvalMeanAPHook(EvalTopKAccuracyHook):
    """EvalTopKAccuracyHook for multi-label data: after every `interval`-th training epoch, score the validation set and log 'mAP' (mean_average_precision;
    'ema mAP' for the averaged weights).  labels: the (videos, classes) multi-hot matrix.  on_device = True: the pass is runner.device_test into a
    metrics.DeviceMultiLabelMetrics -- no score row leaves the device, the ranks' records are merged by all_gather() and ONE read ends the pass; it needs one
    score row per video (test_cfg.average_clips 'sigmoid', 'prob' or 'score').
    sample_map = True adds 'sample mAP' (mmit_mean_average_precision: the sample-wise mAP of Multi-Moments in Time); f1_threshold = a number adds 'micro F1'
    and 'macro F1' of "predicted iff the score >= f1_threshold" (precision_recall_f1 and its conventions; the scores are compared as the model returns
    them, probabilities under average_clips='sigmoid').  Both on either path, with the 'ema ' prefix as 'mAP'; without them the result is what it was."""

    def __init__(self, loader, labels, interval=1, weights="live", on_device=False, sample_map=False, f1_threshold=None):
        if weights not in WEIGHTS:
            raise ValueError("weights must be one of %s, got %r" % (", ".join(map(repr, WEIGHTS)), weights))
        lab = np.asarray(labels)
        if lab.ndim != 2:
            raise ValueError("EvalMeanAPHook: labels must be a (videos, classes) multi-hot matrix, got shape %s" % (lab.shape,))
        self.loader, self.labels, self.interval, self.weights = loader, (lab != 0).astype(np.uint8), interval, weights
        self.on_device = bool(on_device)
        if f1_threshold is not None:
            check_thresholds("EvalMeanAPHook", f1_threshold, None, 1)
        self.sample_map, self.f1_threshold = bool(sample_map), f1_threshold
        self._metrics, self._share = None, None
        self.history = []

    def _score(self, runner, prefix):
        if self.on_device:
            return self._score_on_device(runner, prefix)
        from .runner import multi_gpu_test
        was_training = runner.model.training
        results = multi_gpu_test(runner.model, self.loader, size=len(self.labels))
        runner.model.train(was_training)
        if results is None:                          # not rank 0
            return None
        rows = np.stack([np.asarray(r).squeeze() for r in results])
        out = {"%smAP" % prefix: mean_average_precision(rows, self.labels[:len(rows)])}
        if self.sample_map:
            out["%ssample mAP" % prefix] = mmit_mean_average_precision(rows, self.labels[:len(rows)])
        if self.f1_threshold is not None:
            fig = precision_recall_f1(rows, self.labels[:len(rows)], threshold=self.f1_threshold)
            out["%smicro F1" % prefix], out["%smacro F1" % prefix] = fig["micro_f1"], fig["macro_f1"]
        return out

    def _score_on_device(self, runner, prefix):
        from .dist import get_dist_info
        from .metrics import DeviceMultiLabelMetrics
        from .runner import device_test
        model = runner.model.module if hasattr(runner.model, "module") else runner.model
        test_cfg = getattr(model, "test_cfg", None)
        if test_cfg is None or test_cfg.get("average_clips") is None:
            raise ValueError("evaluation hook with on_device=True: test_cfg.average_clips=None leaves several score rows per video; the device record "
                             "takes one row per video (average_clips='sigmoid', 'prob' or 'score'), or use the host path (on_device=False)")
        rank, world = self._share if self._share is not None else get_dist_info()
        if self._metrics is None:
            self._metrics = DeviceMultiLabelMetrics(self.labels.shape[1], capacity=max(1, (len(self.labels) + world - 1) // world))
        if self._metrics.capacity != max(1, (len(self.labels) + world - 1) // world):      # a merged record from the last pass: start from a rank's own size
            self._metrics = DeviceMultiLabelMetrics(self.labels.shape[1], capacity=max(1, (len(self.labels) + world - 1) // world))
        self._metrics.reset()
        was_training = runner.model.training
        device_test(runner.model, self.loader, self.labels, self._metrics, rank=rank, world=world)
        runner.model.train(was_training)
        if world > 1:
            self._metrics.all_gather()
        fig = self._metrics.compute(sample_ap=self.sample_map, threshold=self.f1_threshold)      # every rank holds the figures; rank 0 reports them
        if get_dist_info()[0] != 0:
            return None
        out = {"%smAP" % prefix: float(fig["mAP"])}
        if self.sample_map:
            out["%ssample mAP" % prefix] = float(fig["sample_mAP"])
        if self.f1_threshold is not None:
            out["%smicro F1" % prefix], out["%smacro F1" % prefix] = float(fig["micro_f1"]), float(fig["macro_f1"])
        return out


class PreciseBNHook(object):
    """After every `interval`-th training epoch, BEFORE the evaluation hooks of that epoch (Runner.register_hook keeps hooks with `before_evaluation` in front):
    recompute the BatchNorm running statistics as the plain average of per-batch statistics over at most `num_iters` batches of the TRAINING loader with the
    weights held fixed (TrainEngine.precise_bn; mmaction2's PreciseBNHook, fvcore's update_bn_stats).  weights = 'live' (the modules' running statistics are
    overwritten, training continues from them), 'ema' (the averaged model's own statistics, used inside engine.averaged_weights() and carried by checkpoints)
    or 'both' (two passes over the loader's first batches).  loader = None: the loader the runner is training from."""

    before_evaluation = True

    def __init__(self, loader=None, num_iters=200, interval=1, weights="live"):
        from .ema import check_precise_bn
        cfg = check_precise_bn(dict(num_iters=num_iters, interval=interval, weights=weights))
        self.loader, self.num_iters, self.interval, self.weights = loader, cfg["num_iters"], cfg["interval"], cfg["weights"]
        self.history = []

    @staticmethod
    def _batches(loader):
        for data in loader:
            yield (data["img_group"], data["label"]) if hasattr(data, "keys") else tuple(data)

    def after_train_epoch(self, runner):
        if (runner.epoch % self.interval) != 0:
            return None
        eng = getattr(runner, "engine", None)
        if self.weights != "live" and (eng is None or getattr(eng, "flat_ema", None) is None):
            raise RuntimeError("precise BatchNorm with weights=%r: the runner keeps no averaged weights; set ema_config (Runner(ema=dict(momentum=...)))" % self.weights)
        loader = self.loader if self.loader is not None else getattr(runner, "train_loader", None)
        if loader is None:
            raise RuntimeError("precise BatchNorm: no loader was given and the runner has not trained from one yet")
        model = getattr(runner, "model", None)
        was_training = model.training if model is not None else True
        if model is not None:
            model.train()                            # (the backbone's train() keeps norm_eval / frozen stages in eval mode: those are not calibrated)
        used = {}
        for w in ("live", "ema"):
            if self.weights in (w, "both"):
                used[w] = eng.precise_bn(self._batches(loader), num_iters=self.num_iters, weights=w)
        if model is not None:
            model.train(was_training)
        self.history.append(dict(epoch=runner.epoch, batches=used))
        return None                                  # nothing to log as a figure


class DistEvalTopKAccuracyHook(EvalTopKAccuracyHook):
    """The reference's hook signature (eval_hooks.py:17-104): `DistEvalTopKAccuracyHook(dataset, interval=1, k=(1,), dist=True)`.
    `dataset`: anything with `__len__`, `__getitem__(i) -> dict(img_group=tensor, ...)` and `video_infos[i]['label']` (the reference's
    RawFramesDataset / VideoDataset in test_mode; building one from a config dict needs the dataset classes, which are out of scope
    here -- pass the object).  Every rank scores items `rank::world` one by one, as DistEvalHook.after_train_epoch does
    (collate([data], samples_per_gpu=1) = a batch dimension of one), the rows are gathered on rank 0 and top-k accuracy is logged."""

    def __init__(self, dataset, interval=1, k=(1,), dist=True, weights="live", on_device=False, mean_class=False):
        if isinstance(dataset, dict):
            raise TypeError("DistEvalTopKAccuracyHook: a dataset CONFIG dict needs the reference's dataset classes (out of scope here); "
                            "pass the Dataset object")
        if not (hasattr(dataset, "__getitem__") and hasattr(dataset, "__len__")):
            raise TypeError("dataset must be a Dataset object or a dict, not {}".format(type(dataset)))      # the reference's message
        self.dataset, self.dist = dataset, dist
        labels = [dataset.video_infos[i]["label"] for i in range(len(dataset))]
        super().__init__(_RankShare(dataset, dist), labels, interval, k, weights, on_device=on_device, mean_class=mean_class)
        if not dist:
            self._share = (0, 1)                     # every process scores every video: nothing to merge


class _RankShare(object):
    """items rank::world of a dataset as batches of one (what the reference's hook feeds the model)."""

    def __init__(self, dataset, dist=True):
        self.dataset, self.dist = dataset, dist

    def __iter__(self):
        import torch
        from .dist import get_dist_info
        rank, world = get_dist_info() if self.dist else (0, 1)
        for idx in range(rank, len(self.dataset), world):
            data = self.dataset[idx]
            img = data["img_group"]
            img = img if isinstance(img, torch.Tensor) else torch.as_tensor(np.asarray(img))
            out = {k: v for k, v in data.items() if k not in ("img_group", "label")}
            out["img_group"] = img.unsqueeze(0).cuda(non_blocking=True)
            yield out
