"""Temporal-relation consensus of TSNClsHead ('TRN' / 'TRNmultiscale'): the module tree of the reference's
segmental_consensuses/relation_consensus.py (RelationModule :7-33, RelationModuleMultiScale :36-99) and the host side of the relation table the HIP head reads
(csrc/trn_head.hip; the arithmetic is in include/mvfnet_hip.h).

The table: int32 (R, 1 + T), one relation per row -- (scale_index, f_0 ... f_{s-1}, -1 padding), scale index i being the s = T - i frame relation.  'TRN' and
T = 2 have the one row (0, 0 ... T-1).  'TRNmultiscale' has R = 1 + 3 (T - 2) rows: the T-frame relation, then for every further scale
min(3, C(T, s)) relations drawn with np.random.choice(len, n, replace=False) on numpy's GLOBAL generator, in scale order -- the reference's draw
(relation_consensus.py:81-92), in training and in eval: after np.random.seed(k) the table names the relations the reference sums, in its `act_all +=` order.
"""
import itertools

import numpy as np
import torch.nn as nn

RELATION_TYPES = ("TRN", "TRNmultiscale")
IMG_FEATURE_DIM = 256          # what new_fc emits per frame (tsn_clshead.py:64), and the TRN paper's feature width
MAX_FRAMES = 16                # MVF_TRN_MAX_FRAMES: the per-scale operands travel in the kernel arguments (15 sets)
SUBSAMPLE = 3                  # relation_consensus.py:42


class RelationModule(nn.Module):
    """relation_consensus.py:7-33: state_dict keys classifier.{1,3}.{weight,bias}."""
    num_bottleneck = 512

    def __init__(self, img_feature_dim, num_frames, num_class):
        super().__init__()
        self.num_frames, self.num_class, self.img_feature_dim = num_frames, num_class, img_feature_dim
        self.scales = [num_frames]
        self.classifier = nn.Sequential(nn.ReLU(), nn.Linear(num_frames * img_feature_dim, self.num_bottleneck), nn.ReLU(),
                                        nn.Linear(self.num_bottleneck, num_class))

    def scale_layers(self):
        return [(self.classifier[1], self.classifier[3])]

    def forward(self, x):
        raise RuntimeError("RelationModule: the relation consensus runs inside the HIP head (TSNClsHead.forward / the train engine); no CPU fallback")


class RelationModuleMultiScale(nn.Module):
    """relation_consensus.py:36-99: state_dict keys fc_fusion_scales.{i}.{1,3}.{weight,bias}, scales T, T-1, ..., 2."""
    num_bottleneck = 256

    def __init__(self, img_feature_dim, num_frames, num_class):
        super().__init__()
        self.num_frames, self.num_class, self.img_feature_dim = num_frames, num_class, img_feature_dim
        self.subsample_num = SUBSAMPLE
        self.scales = list(range(num_frames, 1, -1))
        self.fc_fusion_scales = nn.ModuleList(
            nn.Sequential(nn.ReLU(), nn.Linear(s * img_feature_dim, self.num_bottleneck), nn.ReLU(), nn.Linear(self.num_bottleneck, num_class))
            for s in self.scales)

    def scale_layers(self):
        return [(m[1], m[3]) for m in self.fc_fusion_scales]

    def forward(self, x):
        raise RuntimeError("RelationModuleMultiScale: the relation consensus runs inside the HIP head (TSNClsHead.forward / the train engine); no CPU fallback")


def return_TRN(relation_type, img_feature_dim, num_frames, num_class):
    if relation_type == "TRN":
        return RelationModule(img_feature_dim, num_frames, num_class)
    if relation_type == "TRNmultiscale":
        return RelationModuleMultiScale(img_feature_dim, num_frames, num_class)
    raise ValueError("Unknown TRN" + str(relation_type))


def scale_operands(module, tensor_of, grad_of=None):
    """The _lib.TrnScale host array mvf_trn_head_fwd / mvf_trn_head_bwd read at the call, one entry per scale of `module`, and the tensors it points into (keep
    them alive until the launches are queued).  tensor_of: parameter -> the fp32 contiguous device tensor to read; grad_of: parameter -> its gradient
    destination (the backward), or None.  Built per call: a re-homed parameter store moves the addresses."""
    from .._lib import TrnScale
    layers = module.scale_layers()
    arr, keep = (TrnScale * len(layers))(), []
    for i, (l1, l2) in enumerate(layers):
        for name, p in (("w1", l1.weight), ("b1", l1.bias), ("w2", l2.weight), ("b2", l2.bias)):
            v = tensor_of(p)
            keep.append(v)
            setattr(arr[i], name, v.data_ptr())
            if grad_of is not None:
                g = grad_of(p)
                keep.append(g)
                setattr(arr[i], "d" + name, g.data_ptr())
    return arr, keep


def check_num_frames(kind, num_frames):
    if kind not in RELATION_TYPES:
        raise ValueError("relation consensus: type must be one of %s, got %r" % (RELATION_TYPES, kind))
    if isinstance(num_frames, bool) or not isinstance(num_frames, (int, np.integer)) or not 2 <= num_frames <= MAX_FRAMES:
        raise ValueError("relation consensus: num_frames must be an integer in [2, %d], got %r" % (MAX_FRAMES, num_frames))
    return int(num_frames)


def relation_rows(kind, num_frames):
    """R: 1 for 'TRN' and for T = 2, else 1 + 3 (T - 2): every scale below T has C(T, s) >= T >= 3 relations, of which the draw takes 3."""
    t = check_num_frames(kind, num_frames)
    if kind == "TRN":
        return 1
    return 1 + sum(min(SUBSAMPLE, _n_relations(t, s)) for s in range(t - 1, 1, -1))


def _n_relations(t, s):
    n = 1
    for i in range(s):
        n = n * (t - i) // (i + 1)
    return n


def relation_sets(num_frames):
    """relations_scales of the reference: for every scale T, T-1, ..., 2 the list of itertools.combinations(range(T), scale)."""
    return [list(itertools.combinations(range(num_frames), s)) for s in range(num_frames, 1, -1)]


def _row(t, scale_index, frames):
    return [scale_index] + [int(f) for f in frames] + [-1] * (t - len(frames))


def draw_relation_table(kind, num_frames, choices=None):
    """The step's table, int32 (R, 1 + T).  Draws from numpy's global generator exactly as RelationModuleMultiScale.forward does (one np.random.choice per
    scale index >= 1, in scale order; none for 'TRN').  choices: a list that receives each draw (the recorded np.random.choice results)."""
    t = check_num_frames(kind, num_frames)
    rows = [_row(t, 0, range(t))]
    if kind == "TRNmultiscale":
        sets = relation_sets(t)
        for i in range(1, len(sets)):
            idx = np.random.choice(len(sets[i]), min(SUBSAMPLE, len(sets[i])), replace=False)
            if choices is not None:
                choices.append(np.asarray(idx).copy())
            rows.extend(_row(t, i, sets[i][int(j)]) for j in idx)
    return np.asarray(rows, dtype=np.int32)


def check_relation_table(table, kind, num_frames):
    """Refuses, with ValueError, a table the head must not run: not int32 (R, 1 + T); a scale index outside the head's scales; a first row that is not the
    T-frame relation, or a second one of it; frame indices that are not strictly ascending in [0, T); padding other than -1; more rows of a scale than the
    reference would draw, or the same relation twice; for 'TRN' anything but its one row.  Rows of scales >= 1 may come in any order (the draw makes them
    in scale order; the scores are their sum in table order).
    (A scale WITHOUT a row is allowed: it adds nothing to the scores and gets zero gradients.)  Returns the table as a contiguous int32 array."""
    t = check_num_frames(kind, num_frames)
    a = np.asarray(table)
    if a.dtype != np.int32 or a.ndim != 2 or a.shape[1] != 1 + t or a.shape[0] < 1:
        raise ValueError("relation table: needs int32 (R >= 1, 1 + T = %d), got %s %s" % (1 + t, a.dtype, tuple(a.shape)))
    n_scales = 1 if kind == "TRN" else t - 1
    if a.shape[0] > 1 + SUBSAMPLE * (n_scales - 1):
        raise ValueError("relation table: %d rows, at most %d for %s with T = %d" % (a.shape[0], 1 + SUBSAMPLE * (n_scales - 1), kind, t))
    seen = set()
    for r, row in enumerate(a.tolist()):
        si = row[0]
        if not 0 <= si < n_scales:
            raise ValueError("relation table: row %d: scale index %d outside [0, %d)" % (r, si, n_scales))
        if (r == 0) != (si == 0):
            raise ValueError("relation table: row %d: the T-frame relation (scale index 0) is the first row and only that" % r)
        s = t - si
        frames, padding = row[1:1 + s], row[1 + s:]
        if any(not 0 <= f < t for f in frames) or any(b <= a_ for a_, b in zip(frames, frames[1:])):
            raise ValueError("relation table: row %d: frames %s are not strictly ascending in [0, %d)" % (r, frames, t))
        if any(p != -1 for p in padding):
            raise ValueError("relation table: row %d: padding %s must be -1" % (r, padding))
        key = (si, tuple(frames))
        if key in seen:
            raise ValueError("relation table: row %d repeats the relation %s of scale index %d" % (r, frames, si))
        seen.add(key)
    for si in range(1, n_scales):
        n = sum(1 for k in seen if k[0] == si)
        if n > min(SUBSAMPLE, _n_relations(t, t - si)):
            raise ValueError("relation table: %d rows of scale index %d, the draw makes at most %d" % (n, si, min(SUBSAMPLE, _n_relations(t, t - si))))
    return np.ascontiguousarray(a)
