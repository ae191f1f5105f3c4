"""The per-row rules of mvf_metrics_update (include/mvfnet_hip.h) restated in numpy, fp64 comparisons and int64 counters: what the kernel tests compare the
device state against, word for word.

    state[0] rows seen      state[1] rows with a label outside [0, classes)      state[2] rows holding a NaN      state[3..8) zero
    state[8 + i] hits for ks[i]      state[16 + y * classes + pred] (with_confusion) the confusion matrix, row = real label, column = prediction

A bad label wins over a NaN; either kind of row moves its counter and word 0 and nothing else, rank = pred = -1.  On a valid row
rank = #{j : s_j > s_y, or s_j == s_y and j < y} (ties to the lower class index, +-inf ordinary values), hit_k iff rank < k, pred = the lowest index of the
maximum.  fp32 scores are exact in fp64 and only compared, never added: there is no tolerance to state."""
import numpy as np

HEADER, HITS, MAX_K = 16, 8, 8


def state_words(classes, with_confusion):
    return HEADER + (classes * classes if with_confusion else 0)


def rows_ref(scores, labels):
    """(rank, pred, kind) per row; kind 0 = valid, 1 = bad label, 2 = NaN row."""
    s = np.asarray(scores, dtype=np.float64)
    s = s.reshape(-1, s.shape[-1])
    y = np.asarray(labels).astype(np.int64).reshape(-1)
    rows, classes = s.shape
    assert y.shape == (rows,)
    rank, pred, kind = np.full(rows, -1, np.int64), np.full(rows, -1, np.int64), np.zeros(rows, np.int64)
    idx = np.arange(classes)
    for r in range(rows):
        if y[r] < 0 or y[r] >= classes:
            kind[r] = 1
            continue
        if np.isnan(s[r]).any():
            kind[r] = 2
            continue
        sy = s[r, y[r]]
        rank[r] = int(np.count_nonzero((s[r] > sy) | ((s[r] == sy) & (idx < y[r]))))
        pred[r] = int(np.flatnonzero(s[r] == s[r].max())[0])
    return rank, pred, kind


def metrics_ref(scores, labels, ks, with_confusion, state=None, rows=None):
    """The state after one mvf_metrics_update on `state` (zeros when None); returns (state, rank, pred) with rank / pred as int32 (the record arrays).
    rows = rows_ref(scores, labels) computed earlier (the per-row part does not depend on ks / with_confusion)."""
    s = np.asarray(scores)
    classes = s.shape[-1]
    ks = tuple(int(k) for k in ks)
    assert 1 <= len(ks) <= MAX_K and all(k >= 1 for k in ks) and classes >= 1
    state = np.zeros(state_words(classes, with_confusion), np.int64) if state is None else np.array(state, dtype=np.int64)
    assert state.shape == (state_words(classes, with_confusion),)
    rank, pred, kind = rows_ref(s, labels) if rows is None else rows
    y = np.asarray(labels).astype(np.int64).reshape(-1)
    state[0] += rank.shape[0]
    state[1] += int(np.count_nonzero(kind == 1))
    state[2] += int(np.count_nonzero(kind == 2))
    ok = kind == 0
    for i, k in enumerate(ks):
        state[HITS + i] += int(np.count_nonzero(ok & (rank < k)))
    if with_confusion:
        np.add.at(state, HEADER + y[ok] * classes + pred[ok], 1)
    return state, rank.astype(np.int32), pred.astype(np.int32)


def permutation_rows(rows, classes, seed, max_rank=10):
    """Tie-free rows: each a permutation of arange(classes) / 64 (exact in fp32, distinct by construction), with labels chosen so that the label's rank is
    drawn from 0 .. min(max_rank, classes) - 1.  Returns (scores fp32 (rows, classes), labels int64 (rows,), ranks int64 (rows,))."""
    rng = np.random.RandomState(seed)
    scores = np.stack([rng.permutation(classes) for _ in range(rows)]).astype(np.float32) / np.float32(64.0)
    ranks = rng.randint(0, min(max_rank, classes), size=rows).astype(np.int64)
    order = np.argsort(-scores, axis=1, kind="stable")            # order[r, q] = the class with q classes above it
    labels = order[np.arange(rows), ranks].astype(np.int64)
    return scores, labels, ranks
