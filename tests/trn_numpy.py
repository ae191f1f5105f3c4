"""The temporal-relation head (mvf_trn_head_fwd / mvf_trn_head_bwd, csrc/trn_head.hip) restated in numpy float64 from the text of include/mvfnet_hip.h, taking
the relation table explicitly.  Every stage is a function of its own that returns (value, magnitude): magnitude is sum |a_i b_i| + |bias| per output element
(abs(A) @ abs(B)), the quantity the forward-error bound gamma_n * magnitude of an fp32 sum of n terms is stated in -- it holds for any summation order, with
or without FMA.  forward() / backward() chain the stages.

scales: a list of (w1, b1, w2, b2), scale index i being the s = T - i frame relation: w1 (hidden, s * fdim), w2 (classes, hidden).
table: int (R, 1 + T): scale_index, the s frame indices, -1 padding."""
import numpy as np

U = 2.0 ** -24


def gamma(n):
    return n * U / (1.0 - n * U)


def f64(a):
    return np.asarray(a, dtype=np.float64)


def row_of(table, r, T):
    si = int(table[r, 0])
    return si, [int(v) for v in table[r, 1:1 + T - si]]


def stage_pool(feat, mask=None):
    """feat (frames, hw, c) -> pooled (frames, c): the mean over hw, times the pre-scaled dropout mask.  n = hw + 1 roundings."""
    feat = f64(feat)
    m = 1.0 if mask is None else f64(mask)
    return feat.mean(axis=1) * m, np.abs(feat).mean(axis=1) * np.abs(m)


def stage_fc(pooled, fc_w, fc_b):
    pooled, fc_w, fc_b = f64(pooled), f64(fc_w), f64(fc_b)
    return pooled @ fc_w.T + fc_b, np.abs(pooled) @ np.abs(fc_w).T + np.abs(fc_b)


def concat(f, clips, T, frames):
    """relu(concat of the relation's frames): (clips, s * fdim)."""
    fr = f64(f).reshape(clips, T, -1)
    return np.maximum(fr[:, frames, :], 0.0).reshape(clips, -1)


def stage_hidden(f, scales, table, clips, T):
    """-> pre-activations (R, clips, hidden) and their magnitudes; h = relu(pre)."""
    pre, mag = [], []
    for r in range(table.shape[0]):
        si, frames = row_of(table, r, T)
        w1, b1 = f64(scales[si][0]), f64(scales[si][1])
        a = concat(f, clips, T, frames)
        pre.append(a @ w1.T + b1)
        mag.append(np.abs(a) @ np.abs(w1).T + np.abs(b1))
    return np.stack(pre), np.stack(mag)


def stage_scores(h, scales, table, T):
    h = f64(h)
    val = mag = 0.0
    for r in range(table.shape[0]):
        si, _ = row_of(table, r, T)
        w2, b2 = f64(scales[si][2]), f64(scales[si][3])
        val = val + (h[r] @ w2.T + b2)
        mag = mag + (np.abs(h[r]) @ np.abs(w2).T + np.abs(b2))
    return val, mag


def forward(feat, T, fc_w, fc_b, scales, table, mask=None):
    """feat (clips * T, hw, c) -> dict(pooled, f, h, scores), float64."""
    clips = feat.shape[0] // T
    pooled, _ = stage_pool(feat, mask)
    f, _ = stage_fc(pooled, fc_w, fc_b)
    pre, _ = stage_hidden(f, scales, table, clips, T)
    h = np.maximum(pre, 0.0)
    scores, _ = stage_scores(h, scales, table, T)
    return dict(pooled=pooled, f=f, h=h, scores=scores)


def stage_dw2(dscores, h, scales, table, T):
    """-> lists per scale of (dw2, |.|), (db2, |.|)."""
    ds, h = f64(dscores), f64(h)
    out = []
    for si in range(len(scales)):
        dw = np.zeros_like(f64(scales[si][2]))
        mw, db, mb = np.zeros_like(dw), np.zeros(dw.shape[0]), np.zeros(dw.shape[0])
        for r in range(table.shape[0]):
            if int(table[r, 0]) != si:
                continue
            dw += ds.T @ h[r]
            mw += np.abs(ds).T @ np.abs(h[r])
            db += ds.sum(axis=0)
            mb += np.abs(ds).sum(axis=0)
        out.append((dw, mw, db, mb))
    return out


def stage_dh(dscores, h, scales, table, T):
    ds, h = f64(dscores), f64(h)
    val, mag = np.zeros_like(h), np.zeros_like(h)
    for r in range(table.shape[0]):
        w2 = f64(scales[int(table[r, 0])][2])
        val[r] = (ds @ w2) * (h[r] > 0)
        mag[r] = (np.abs(ds) @ np.abs(w2)) * (h[r] > 0)
    return val, mag


def stage_dw1(dh, f, scales, table, clips, T):
    dh = f64(dh)
    out = []
    for si in range(len(scales)):
        dw = np.zeros_like(f64(scales[si][0]))
        mw, db, mb = np.zeros_like(dw), np.zeros(dw.shape[0]), np.zeros(dw.shape[0])
        for r in range(table.shape[0]):
            if int(table[r, 0]) != si:
                continue
            a = concat(f, clips, T, row_of(table, r, T)[1])
            dw += dh[r].T @ a
            mw += np.abs(dh[r]).T @ np.abs(a)
            db += dh[r].sum(axis=0)
            mb += np.abs(dh[r]).sum(axis=0)
        out.append((dw, mw, db, mb))
    return out


def stage_df(dh, f, scales, table, clips, T):
    """-> df (clips * T, fdim), its magnitude, and the number of (row, position) terms gathered into each frame (T,)."""
    dh, f = f64(dh), f64(f)
    fdim = f.shape[1]
    val, mag, cnt = np.zeros((clips, T, fdim)), np.zeros((clips, T, fdim)), np.zeros(T, dtype=np.int64)
    for r in range(table.shape[0]):
        si, frames = row_of(table, r, T)
        w1 = f64(scales[si][0])
        for p, t in enumerate(frames):
            blk = w1[:, p * fdim:(p + 1) * fdim]
            val[:, t] += dh[r] @ blk
            mag[:, t] += np.abs(dh[r]) @ np.abs(blk)
            cnt[t] += 1
    gate = (f > 0).reshape(clips, T, fdim)
    return (val * gate).reshape(clips * T, fdim), (mag * gate).reshape(clips * T, fdim), cnt


def stage_dfc(df, pooled):
    df, pooled = f64(df), f64(pooled)
    return df.T @ pooled, np.abs(df).T @ np.abs(pooled), df.sum(axis=0), np.abs(df).sum(axis=0)


def stage_dpool(df, fc_w, hw, mask=None):
    df, fc_w = f64(df), f64(fc_w)
    m = 1.0 if mask is None else f64(mask)
    return (df @ fc_w) / hw * m, (np.abs(df) @ np.abs(fc_w)) / hw * np.abs(m)


def backward(dscores, cache, T, fc_w, scales, table, hw, mask=None):
    """-> dict(dfc_w, dfc_b, dscales = [(dw1, db1, dw2, db2)], dh, df, dpool, dfeat (clips * T, hw, c)), float64."""
    clips = cache["pooled"].shape[0] // T
    w2s = stage_dw2(dscores, cache["h"], scales, table, T)
    dh, _ = stage_dh(dscores, cache["h"], scales, table, T)
    w1s = stage_dw1(dh, cache["f"], scales, table, clips, T)
    df, _, _ = stage_df(dh, cache["f"], scales, table, clips, T)
    dfc_w, _, dfc_b, _ = stage_dfc(df, cache["pooled"])
    dpool, _ = stage_dpool(df, fc_w, hw, mask)
    dfeat = np.repeat(dpool[:, None, :], hw, axis=1)
    return dict(dfc_w=dfc_w, dfc_b=dfc_b, dscales=[(a[0], a[2], b[0], b[2]) for a, b in zip(w1s, w2s)], dh=dh, df=df, dpool=dpool, dfeat=dfeat)


def fixture_weights(golden, name):
    """The parameters of a case of tests/golden/trn_cases.npz, regenerated by name (mvfnet_amd.synth; the fixture stores none): {key: fp64 array}, and the
    restatement's fc_w, fc_b, scales."""
    from mvfnet_amd import synth
    seed = int(golden[name + "/seed"])
    keys = golden[name + "/keys"].tolist()
    shapes = {name + "/" + k: tuple(int(v) for v in s.split(",")) for k, s in zip(keys, golden[name + "/shapes"].tolist())}
    vals = {k[len(name) + 1:]: v.astype(np.float64) for k, v in synth.synth_state_dict(shapes, seed=seed).items()}
    pre = "segmental_consensus."
    if pre + "classifier.1.weight" in vals:
        stems = [pre + "classifier."]
    else:
        stems = [pre + "fc_fusion_scales.%d." % i for i in range(sum(1 for k in keys if k.endswith(".1.weight")))]
    scales = [(vals[s + "1.weight"], vals[s + "1.bias"], vals[s + "3.weight"], vals[s + "3.bias"]) for s in stems]
    return vals, vals["new_fc.weight"], vals["new_fc.bias"], scales


def table_from_choices(kind, T, choices):
    """The table the reference's forward evaluates, from its recorded np.random.choice results (one per scale below T, in scale order)."""
    import itertools
    rows = [[0] + list(range(T))]
    if kind == "TRNmultiscale":
        for i, idx in enumerate(choices, start=1):
            sets = list(itertools.combinations(range(T), T - i))
            rows.extend([i] + list(sets[int(j)]) + [-1] * i for j in idx)
    return np.asarray(rows, dtype=np.int32)


def ce_loss(scores, labels):
    """Mean softmax cross-entropy and its gradient, float64."""
    s = f64(scores)
    z = s - s.max(axis=1, keepdims=True)
    lse = np.log(np.exp(z).sum(axis=1, keepdims=True))
    p = np.exp(z - lse)
    n = s.shape[0]
    lab = np.asarray(labels).reshape(-1)
    loss = float(-(z - lse)[np.arange(n), lab].mean())
    p[np.arange(n), lab] -= 1.0
    return loss, p / n
