"""Device-side accuracy: top-k hits and confusion counts that stay on the device (csrc/metrics.hip, mvf_metrics_update).

`DeviceMetrics` owns the int64 state array whose layout include/mvfnet_hip.h publishes.  `update()` is one asynchronous launch on the current stream,
`all_reduce()` one SUM collective of the array, and `compute()` the ONE call that waits for the device: evaluation reads a few words per pass
(runner.device_test, EvalTopKAccuracyHook(on_device=True)) instead of one score row per video, and the train engine counts every step's score matrix for the
log line (TrainEngine.enable_train_accuracy, Runner(train_accuracy=...)).  The rules -- ties to the lower class index, rows with a bad label or a NaN counted
apart -- are the header's; tests/metrics_numpy.py restates them in numpy.

`check_train_accuracy` is the configuration check of the runner option, beside guard.check_nonfinite_guard."""
import ctypes as C

import numpy as np
import torch

from . import _lib

HEADER_WORDS = _lib.METRICS_CONFUSION
MAX_K = _lib.METRICS_MAX_K
TRAIN_ACCURACY_KEYS = ("k",)
TRAIN_ACCURACY_DEFAULTS = dict(k=(1, 5))


def check_k(k, who="k"):
    """A tuple of 1..8 integers >= 1 (an int is taken as a 1-tuple; a bool is not an integer here)."""
    if isinstance(k, (int, np.integer)) and not isinstance(k, bool):
        k = (k,)
    if not isinstance(k, (tuple, list)) or not 1 <= len(k) <= MAX_K:
        raise ValueError("%s must be a tuple of 1 to %d integers >= 1, got %r" % (who, MAX_K, k))
    for v in k:
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
            raise ValueError("%s must be a tuple of 1 to %d integers >= 1, got %r" % (who, MAX_K, k))
    return tuple(int(v) for v in k)


def check_train_accuracy(cfg):
    """cfg.train_accuracy / Runner(train_accuracy=): None (off) or dict(k=(1, 5)); an empty dict gives the default.  Returns None or a dict with the key; an
    unknown key, or a k that is not 1 to 8 integers >= 1, is refused.  The log line shows one `top<k>` figure per entry of k."""
    if cfg is None:
        return None
    if not hasattr(cfg, "keys"):
        raise ValueError("train_accuracy must be None or dict(k=(1, 5)), got %r" % (cfg,))
    unknown = sorted(k for k in cfg.keys() if k not in TRAIN_ACCURACY_KEYS)
    if unknown:
        raise ValueError("train_accuracy: unknown key %s (known: %s)" % (", ".join(map(repr, unknown)), ", ".join(TRAIN_ACCURACY_KEYS)))
    out = dict(TRAIN_ACCURACY_DEFAULTS)
    out.update({k: cfg[k] for k in cfg.keys()})
    return dict(k=check_k(out["k"], "train_accuracy: k"))


def mean_class_from_confusion(cf):
    """evaluation.mean_class_accuracy from the full classes x classes matrix: the mean, over the classes that occur as a label or as a prediction, of
    hits / videos of the class; a class that is only predicted contributes 0.  nan when the matrix is empty."""
    cf = np.asarray(cf, dtype=np.float64)
    cnt, hit = cf.sum(axis=1), np.diag(cf)
    occurs = (cnt > 0) | (cf.sum(axis=0) > 0)
    if not occurs.any():
        return float("nan")
    return float(np.mean(np.where(cnt > 0, hit / np.where(cnt > 0, cnt, 1.0), 0.0)[occurs]))


def figures_from_state(state, num_classes, k, confusion, strict=True):
    """The dict compute() returns, from a host copy of the state array."""
    state = np.asarray(state, dtype=np.int64).reshape(-1)
    want = HEADER_WORDS + (num_classes * num_classes if confusion else 0)
    if state.size != want:
        raise ValueError("metrics state of %d words for %d classes (confusion=%s): expected %d" % (state.size, num_classes, bool(confusion), want))
    count, invalid, nan_rows = (int(state[i]) for i in (_lib.METRICS_ROWS, _lib.METRICS_BAD_LABEL, _lib.METRICS_NAN_ROWS))
    if strict and (invalid or nan_rows):
        raise ValueError("device metrics: %d of %d rows have a label outside [0, %d) and %d hold a NaN score; compute(strict=False) returns the figures "
                         "with those rows counted as misses" % (invalid, count, num_classes, nan_rows))
    out = dict(count=count)
    for i, kk in enumerate(k):
        out["top%d" % kk] = int(state[_lib.METRICS_HITS + i]) / count if count else float("nan")
    cf = state[HEADER_WORDS:].reshape(num_classes, num_classes).copy() if confusion else None
    out.update(mean_class_acc=mean_class_from_confusion(cf) if confusion else None, confusion=cf, invalid=invalid, nan_rows=nan_rows)
    return out


class DeviceMetrics(object):
    """Top-k accuracy, mean class accuracy and the confusion matrix of everything passed to update() since the last reset(), counted on the device.

        m = DeviceMetrics(400, k=(1, 5))
        for scores, labels in ...:          # (rows, 400) fp32 and (rows,) int64, both on the device
            m.update(scores, labels)        # one launch on the current stream, no readback
        m.all_reduce()                      # under a process group: every rank then holds the totals
        m.compute()                         # the one synchronising call: dict(count, top1, top5, mean_class_acc, confusion, invalid, nan_rows)

    confusion=False keeps the 16 header words only (mean_class_acc and confusion come back as None).  record=n keeps the per-row rank (how many classes beat
    the label; -1 for a bad row) and prediction of up to n rows in two int32 device arrays, filled at a running offset the host keeps: records()."""

    def __init__(self, num_classes, k=(1, 5), confusion=True, record=0, device=None):
        if isinstance(num_classes, bool) or not isinstance(num_classes, (int, np.integer)) or num_classes < 1:
            raise ValueError("num_classes must be an integer >= 1, got %r" % (num_classes,))
        if isinstance(record, bool) or not isinstance(record, (int, np.integer)) or record < 0:
            raise ValueError("record must be an integer >= 0 (rows to keep), got %r" % (record,))
        self.num_classes, self.k, self.confusion, self.record = int(num_classes), check_k(k), bool(confusion), int(record)
        words = _lib.lib.mvf_metrics_state_words(self.num_classes, int(self.confusion))
        if words == 0:
            raise ValueError("num_classes=%d: the confusion matrix has more than 2^31 - 1 cells; pass confusion=False" % self.num_classes)
        self.device = torch.device(device if device is not None else "cuda")
        self.state = torch.zeros(words, dtype=torch.int64, device=self.device)
        self._ks = (C.c_int * len(self.k))(*self.k)
        self._rank = self._pred = None
        if self.record:
            self._rank = torch.full((self.record,), -1, dtype=torch.int32, device=self.device)
            self._pred = torch.full((self.record,), -1, dtype=torch.int32, device=self.device)
        self.recorded = 0            # rows in the record arrays: the running offset, kept on the host

    def update(self, scores, labels):
        """scores (rows, num_classes) fp32 contiguous, labels (rows,) or (rows, 1) int64, both on this object's device.  Asynchronous on the current stream."""
        if not (torch.is_tensor(scores) and torch.is_tensor(labels) and scores.is_cuda and labels.is_cuda):
            raise RuntimeError("DeviceMetrics.update: device tensors required (the host path is evaluation.top_k_accuracy); no CPU fallback")
        if scores.device != self.state.device or labels.device != self.state.device:
            raise RuntimeError("DeviceMetrics.update: scores on %s, labels on %s, state on %s" % (scores.device, labels.device, self.state.device))
        if scores.dtype != torch.float32 or scores.dim() != 2 or scores.shape[1] != self.num_classes or not scores.is_contiguous():
            raise ValueError("DeviceMetrics.update: scores must be a contiguous float32 (rows, %d) tensor, got %s %s" % (self.num_classes, scores.dtype, tuple(scores.shape)))
        rows = scores.shape[0]
        if labels.dtype != torch.int64 or tuple(labels.shape) not in ((rows,), (rows, 1)) or not labels.is_contiguous():
            raise ValueError("DeviceMetrics.update: labels must be a contiguous int64 (%d,) or (%d, 1) tensor, got %s %s" % (rows, rows, labels.dtype, tuple(labels.shape)))
        rank = pred = None
        if self.record:
            if self.recorded + rows > self.record:
                raise RuntimeError("DeviceMetrics.update: %d rows after %d recorded ones do not fit record=%d" % (rows, self.recorded, self.record))
            rank, pred = self._rank.data_ptr() + 4 * self.recorded, self._pred.data_ptr() + 4 * self.recorded
        _lib.check(_lib.lib.mvf_metrics_update(scores.data_ptr(), rows, self.num_classes, labels.data_ptr(), self._ks, len(self.k), self.state.data_ptr(),
                                               int(self.confusion), rank, pred, torch.cuda.current_stream(self.state.device).cuda_stream), "metrics_update")
        if self.record:
            self.recorded += rows

    def reset(self):
        self.state.zero_()
        if self.record:
            self._rank.fill_(-1)
            self._pred.fill_(-1)
        self.recorded = 0

    def all_reduce(self):
        """Sum the state over the default process group (every rank then holds the totals); nothing without one.  The record arrays stay per rank."""
        import torch.distributed as dist
        if dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1:
            dist.all_reduce(self.state)

    def compute(self, strict=True):
        """The one synchronising call: dict(count, top{k}..., mean_class_acc, confusion, invalid, nan_rows).  Top-k = hits / rows seen (bad rows are misses);
        mean_class_acc by the formula of evaluation.mean_class_accuracy from the confusion matrix (an int64 (classes, classes) numpy array).  strict=True
        raises ValueError naming the counts when a row had a label outside [0, num_classes) or a NaN score."""
        return figures_from_state(self.state.cpu().numpy(), self.num_classes, self.k, self.confusion, strict)

    def records(self):
        """(rank, pred): the int32 device arrays of the rows recorded so far, in update order (views: one .cpu() each is the whole prediction dump)."""
        if not self.record:
            raise RuntimeError("DeviceMetrics.records: built with record=0")
        return self._rank[:self.recorded], self._pred[:self.recorded]


def figures_from_ap(ap, positives, state, strict=True):
    """The dict DeviceMultiLabelMetrics.compute() returns, from host copies of the kernel's outputs and the record's state words."""
    ap, positives = np.asarray(ap, dtype=np.float64).reshape(-1), np.asarray(positives, dtype=np.int64).reshape(-1)
    state = np.asarray(state, dtype=np.int64).reshape(-1)
    nan_rows, overflow, seen = (int(state[i]) for i in (_lib.MULTILABEL_NAN_ROWS, _lib.MULTILABEL_OVERFLOW, _lib.MULTILABEL_SEEN))
    if strict and overflow:
        raise RuntimeError("device multi-label metrics: %d of %d rows did not fit the record; build it with a larger capacity" % (overflow, seen))
    have = positives > 0
    return dict(mAP=float(np.mean(ap[have])) if have.any() else float("nan"), ap=ap, positives=positives, classes_with_positives=int(have.sum()),
                rows=seen - overflow - nan_rows, nan_rows=nan_rows, overflow=overflow)


class DeviceMultiLabelMetrics(object):
    """Mean average precision of everything passed to update() since the last reset(), for multi-label data (several actions per video: Charades,
    Multi-Moments in Time, HVU), recorded and computed on the device (csrc/multilabel_metrics.hip).

        m = DeviceMultiLabelMetrics(157, capacity=1863)
        for scores, labels in ...:          # (rows, 157) fp32 and (rows, 157) uint8 / bool multi-hot, both on the device
            m.update(scores, labels)        # two launches on the current stream, no readback: the write offset lives in device memory
        m.all_gather()                      # under a process group: every rank then holds every rank's rows
        m.compute()                         # the one synchronising call: dict(mAP, ap, positives, classes_with_positives, rows, nan_rows, overflow)

    AP is the step-wise average precision of scikit-learn's average_precision_score (evaluation.mean_average_precision is the same definition in numpy);
    mAP is its mean over the classes with at least one positive.  `capacity` = the rows the record can hold (per rank): rows beyond it are counted and
    compute() raises.  A row holding a NaN score is left out of every class and counted in nan_rows (it still takes a slot).  Unused slots hold NaN scores
    and no label, which a comparison never counts: that is what lets all_gather() merge the ranks' records by plain concatenation."""

    def __init__(self, num_classes, capacity, device=None):
        for name, v in (("num_classes", num_classes), ("capacity", capacity)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
                raise ValueError("%s must be an integer >= 1, got %r" % (name, v))
        if num_classes > 65535 or capacity > 2 ** 31 - 1:
            raise ValueError("num_classes=%d / capacity=%d: at most 65535 classes and 2^31 - 1 rows" % (num_classes, capacity))
        self.num_classes, self.capacity = int(num_classes), int(capacity)
        self.device = torch.device(device if device is not None else "cuda")
        self.rec_scores = torch.full((self.num_classes, self.capacity), float("nan"), dtype=torch.float32, device=self.device)
        self.rec_labels = torch.zeros((self.num_classes, self.capacity), dtype=torch.uint8, device=self.device)
        self.state = torch.zeros(_lib.MULTILABEL_STATE_WORDS, dtype=torch.int64, device=self.device)
        self._pairs = None                    # (tp, nn) of the last compute(): int32 (num_classes, capacity) device arrays

    def update(self, scores, labels):
        """scores (rows, num_classes) fp32 contiguous, labels (rows, num_classes) uint8 or bool (non-zero = positive) contiguous, both on this object's
        device.  Asynchronous on the current stream."""
        if not (torch.is_tensor(scores) and torch.is_tensor(labels) and scores.is_cuda and labels.is_cuda):
            raise RuntimeError("DeviceMultiLabelMetrics.update: device tensors required (the host path is evaluation.mean_average_precision); no CPU fallback")
        if scores.device != self.state.device or labels.device != self.state.device:
            raise RuntimeError("DeviceMultiLabelMetrics.update: scores on %s, labels on %s, record on %s" % (scores.device, labels.device, self.state.device))
        if scores.dtype != torch.float32 or scores.dim() != 2 or scores.shape[1] != self.num_classes or not scores.is_contiguous():
            raise ValueError("DeviceMultiLabelMetrics.update: scores must be a contiguous float32 (rows, %d) tensor, got %s %s"
                             % (self.num_classes, scores.dtype, tuple(scores.shape)))
        if labels.dtype not in (torch.uint8, torch.bool) or tuple(labels.shape) != tuple(scores.shape) or not labels.is_contiguous():
            raise ValueError("DeviceMultiLabelMetrics.update: labels must be a contiguous uint8 / bool %s tensor, got %s %s"
                             % (tuple(scores.shape), labels.dtype, tuple(labels.shape)))
        _lib.check(_lib.lib.mvf_multilabel_record(scores.data_ptr(), labels.data_ptr(), scores.shape[0], self.num_classes, self.rec_scores.data_ptr(),
                                                  self.rec_labels.data_ptr(), self.capacity, self.state.data_ptr(),
                                                  torch.cuda.current_stream(self.state.device).cuda_stream), "multilabel_record")

    def reset(self):
        self.rec_scores.fill_(float("nan"))
        self.rec_labels.zero_()
        self.state.zero_()
        self._pairs = None

    def merge(self, records):
        """Replace this object's record by the concatenation of `records`, a list of (rec_scores, rec_labels, state) triples of equal class count on this
        device (what all_gather() collects; unused slots must hold NaN scores and no label, as reset() leaves them).  AP does not depend on the order of
        the rows, so nothing is re-interleaved.  No readback."""
        self.rec_scores = torch.cat([r[0] for r in records], dim=1).contiguous()
        self.rec_labels = torch.cat([r[1] for r in records], dim=1).contiguous()
        self.capacity = int(self.rec_scores.shape[1])
        state = torch.stack([r[2] for r in records]).sum(dim=0)
        state[_lib.MULTILABEL_SLOTS] = self.capacity          # every slot may hold a row: the padding is NaN
        self.state = state
        self._pairs = None

    def all_gather(self):
        """Under the default process group every rank ends up with every rank's rows (records padded to the longest capacity); nothing without one."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized() and dist.get_world_size() > 1):
            return
        world = dist.get_world_size()
        cap = torch.tensor([self.capacity], dtype=torch.int64, device=self.device)
        caps = [torch.zeros_like(cap) for _ in range(world)]
        dist.all_gather(caps, cap)
        longest = int(torch.stack(caps).max())                 # (a host read of one word per rank: capacities are host figures, not the pass's results)
        sc, lb = self.rec_scores, self.rec_labels
        if longest > self.capacity:
            sc = torch.cat([sc, torch.full((self.num_classes, longest - self.capacity), float("nan"), dtype=torch.float32, device=self.device)], dim=1).contiguous()
            lb = torch.cat([lb, torch.zeros((self.num_classes, longest - self.capacity), dtype=torch.uint8, device=self.device)], dim=1).contiguous()
        scs, lbs, sts = ([torch.empty_like(t) for _ in range(world)] for t in (sc, lb, self.state))
        dist.all_gather(scs, sc)
        dist.all_gather(lbs, lb)
        dist.all_gather(sts, self.state)
        self.merge(list(zip(scs, lbs, sts)))

    def compute(self, strict=True, sample_ap=False, threshold=None, thresholds=None, best_f1=False):
        """The one synchronising call: dict(mAP, ap (num_classes,) float64 with NaN where a class has no positive, positives (num_classes,) int64,
        classes_with_positives, rows, nan_rows, overflow).  strict=True raises RuntimeError when rows did not fit the record.
        Each option adds keys (csrc/multilabel_f1.hip; evaluation.py holds the same definitions in numpy); the defaults return exactly the dict above.
          sample_ap=True            sample_mAP (the sample-wise mAP of Multi-Moments in Time: the mean of the per-row AP over the rows with at least one
                                    positive, nan if none), sample_ap (slots,) float64 with NaN for such a row, rows_with_positives
          threshold= / thresholds=  a number, or one per class (none NaN): "predicted iff the recorded value >= it" (the values are compared as recorded:
                                    probabilities under average_clips='sigmoid').  counts (num_classes, 4) int64 = TP, FP, FN, TN; per-class precision,
                                    recall, f1; micro_precision, micro_recall, micro_f1, macro_f1.  Conventions (evaluation.prf_from_counts): a ratio with a
                                    zero denominator is 0 -- f1 = 2TP / (2TP + FP + FN) --, macro_f1 is the mean over the classes with at least one positive
          best_f1=True              best_f1, best_threshold (num_classes,): the best achievable F1 of each class and the threshold (>=) that attains it, a
                                    positive's score, ties to the larger score, NaN for a class without a positive; macro_best_f1 over the classes with one"""
        from .evaluation import best_f1_from_counts, check_thresholds, prf_from_counts
        dev, i32 = self.device, torch.int32
        stream = torch.cuda.current_stream(self.state.device).cuda_stream
        th = None
        if threshold is not None or thresholds is not None:
            th = check_thresholds("DeviceMultiLabelMetrics.compute", threshold, thresholds, self.num_classes)
        tp = torch.empty((self.num_classes, self.capacity), dtype=i32, device=dev)
        nn = torch.empty((self.num_classes, self.capacity), dtype=i32, device=dev)
        ap = torch.empty(self.num_classes, dtype=torch.float64, device=dev)
        positives = torch.empty(self.num_classes, dtype=torch.int64, device=dev)
        _lib.check(_lib.lib.mvf_multilabel_ap(self.rec_scores.data_ptr(), self.rec_labels.data_ptr(), self.capacity, self.num_classes, self.state.data_ptr(),
                                              tp.data_ptr(), nn.data_ptr(), ap.data_ptr(), positives.data_ptr(), stream), "multilabel_ap")
        self._pairs = (tp, nn)
        if sample_ap:
            s_ap = torch.empty(self.capacity, dtype=torch.float64, device=dev)
            s_pos = torch.empty(self.capacity, dtype=i32, device=dev)
            _lib.check(_lib.lib.mvf_multilabel_sample_ap(self.rec_scores.data_ptr(), self.rec_labels.data_ptr(), self.capacity, self.num_classes,
                                                         self.state.data_ptr(), s_ap.data_ptr(), s_pos.data_ptr(), stream), "multilabel_sample_ap")
        if th is not None:
            counts = torch.empty((self.num_classes, 4), dtype=torch.int64, device=dev)
            th_d = None if thresholds is None else torch.from_numpy(th).to(dev)
            _lib.check(_lib.lib.mvf_multilabel_prf(self.rec_scores.data_ptr(), self.rec_labels.data_ptr(), self.capacity, self.num_classes, self.state.data_ptr(),
                                                   C.c_float(float(th[0])), None if th_d is None else th_d.data_ptr(), counts.data_ptr(), stream), "multilabel_prf")
        if best_f1:
            b_tp, b_n = torch.empty(self.num_classes, dtype=i32, device=dev), torch.empty(self.num_classes, dtype=i32, device=dev)
            b_th = torch.empty(self.num_classes, dtype=torch.float32, device=dev)
            _lib.check(_lib.lib.mvf_multilabel_best_f1(self.rec_scores.data_ptr(), tp.data_ptr(), nn.data_ptr(), positives.data_ptr(), self.capacity,
                                                       self.num_classes, self.state.data_ptr(), b_tp.data_ptr(), b_n.data_ptr(), b_th.data_ptr(), stream),
                       "multilabel_best_f1")
        state = self.state.cpu().numpy()
        positives_h = positives.cpu().numpy()
        out = figures_from_ap(ap.cpu().numpy(), positives_h, state, strict)
        if sample_ap:
            slots = int(min(max(state[_lib.MULTILABEL_SLOTS], 0), self.capacity))
            sa, sp = s_ap.cpu().numpy()[:slots], s_pos.cpu().numpy()[:slots]
            have = sp > 0
            out.update(sample_mAP=float(np.mean(sa[have])) if have.any() else float("nan"), sample_ap=sa, rows_with_positives=int(have.sum()))
        if th is not None:
            out.update(prf_from_counts(counts.cpu().numpy()))
        if best_f1:
            out.update(best_f1_from_counts(b_tp.cpu().numpy(), b_n.cpu().numpy(), positives_h), best_threshold=b_th.cpu().numpy())
        return out

    def pairs(self):
        """(tp, nn, slots): the int32 (num_classes, capacity) device arrays of TP_i and N_i the last compute() made (0 / 0 for a row that is no positive of
        the class) and the number of slots they cover."""
        if self._pairs is None:
            raise RuntimeError("DeviceMultiLabelMetrics.pairs: compute() has not run since the last update of the record")
        return self._pairs[0], self._pairs[1], int(self.state[_lib.MULTILABEL_SLOTS])
