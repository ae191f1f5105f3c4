"""clip_grad_norm_ + LAMB with the arithmetic of timm's Lamb (optim/lamb.py; bias correction and grad_averaging on) restated in numpy from the text of
include/mvfnet_hip.h (mvf_lamb_step), in the style of adamw_numpy.py.  One table segment is one trust-ratio unit: per-segment lr * lr_mult and
weight_decay * decay_mult, lr_mult < 0 = the segment is excluded (gradient outside the norm, parameter and both moments untouched, ratio 0).

    d  = g * grad_scale * coef
    m' = b1 * m + (1 - b1) * d                      v' = b2 * v + (1 - b2) * d^2
    u  = (m' / (1 - b1^t)) / (sqrt(v') / sqrt(1 - b2^t) + eps) + wd_i * p
    wn = sqrt(sum_k p^2)  (p before the update)     un = sqrt(sum_k u^2)                     (fp64 sums, each rounded once)
    r_k = adapts_k and wn > 0 and un > 0 ? wn / un : 1,  adapts_k = (wd_k != 0) or always_adapt;   trust_clip: r_k = min(r_k, 1)
    p' = p - (lr_k * r_k) * u

ft = np.float64 is the reference and keeps fp64 state.  ft = np.float32 is the same update as an fp32 implementation makes it: every scalar (1 - b1, 1 - b2,
1 / (1 - b1^t), sqrt(1 - b2^t), wd_i, lr_k * r_k) is formed in double and rounded to fp32 ONCE, the arrays are fp32 throughout, the two norms are fp64 sums of
the fp32 values and the ratio is rounded to fp32 once.  Its distance from the fp64 reference is what the kernel tests scale their bounds from (LAMB_FP32 in
test_lamb_gpu.py; `python tests/lamb_numpy.py` prints the table)."""
import numpy as np

LR, BETAS, EPS, WD, MAX_NORM = 5e-3, (0.9, 0.999), 1e-6, 0.02, 40.0

SEG_N = 262144 + 3
# first, lr_mult, decay_mult: boundaries at odd offsets (7, 257, 1001), a one-element segment (1000), two excluded segments (256, 1001), decay_mult = 0
# segments (7, 257, 262146: ratio exactly 1 without always_adapt), a segment over more than 16 chunks (70000 .. 262146), six segments inside chunk 0
SEGMENTS = ((0, 1.0, 1.0), (7, 2.0, 0.0), (256, -1.0, 0.0), (257, 1.0, 0.0), (1000, 0.5, 0.5), (1001, -1.0, 1.0), (3000, 1.0, 1.0), (70000, 1.0, 1.0),
            (262146, 2.0, 0.0))


def seg_lens(n, segs):
    return np.diff([s[0] for s in segs] + [n])


def lamb_ref(p, m, v, g, gs, max_norm, t, segs=((0, 1.0, 1.0),), ft=np.float64, lr=LR, betas=BETAS, eps=EPS, wd=WD, trust_clip=0, always_adapt=0):
    """One step; t = the applied-step count after it (1 for the first).  Returns (p, m, v, ratios, norm, coef)."""
    n = p.size
    lens = seg_lens(n, segs)
    firsts = [s[0] for s in segs] + [n]
    lrm = np.array([s[1] for s in segs], dtype=np.float64)
    dcm = np.array([s[2] for s in segs], dtype=np.float64)
    excl = np.repeat(lrm < 0, lens)
    b1, b2 = float(betas[0]), float(betas[1])
    inv_bc1 = ft(1.0 / (1.0 - b1 ** t))
    bc2 = ft(np.sqrt(1.0 - b2 ** t))
    wd_k = wd * dcm                                                    # doubles, per segment
    wd_i = np.repeat(wd_k.astype(ft), lens)
    with np.errstate(all="ignore"):
        gg = ft(gs) * g.astype(ft)
        norm = ft(np.sqrt((gg[~excl].astype(np.float64) ** 2).sum()))
        coef = min(ft(1.0), ft(max_norm) / (norm + ft(1e-6))) if max_norm > 0 else ft(1.0)
        d = gg * coef
        pv = p.astype(ft)
        mn = ft(b1) * m.astype(ft) + ft(1.0 - b1) * d
        vn = ft(b2) * v.astype(ft) + ft(1.0 - b2) * (d * d)
        u = (mn * inv_bc1) / (np.sqrt(vn) / bc2 + ft(eps)) + wd_i * pv
        ratios = np.zeros(len(segs), dtype=np.float64)
        step = np.zeros(n, dtype=ft)
        for k in range(len(segs)):
            a, b = firsts[k], firsts[k + 1]
            if lrm[k] < 0:
                continue
            wn = np.sqrt((pv[a:b].astype(np.float64) ** 2).sum())
            un = np.sqrt((u[a:b].astype(np.float64) ** 2).sum())
            r = 1.0
            if (wd_k[k] != 0 or always_adapt) and wn > 0 and un > 0:
                r = float(ft(wn / un))
            if trust_clip:
                r = min(r, 1.0)
            ratios[k] = r
            step[a:b] = ft(lr * lrm[k] * r)
        pn = pv - step * u
    return np.where(excl, p, pn), np.where(excl, m, mn), np.where(excl, v, vn), ratios, float(norm), float(coef)


def lamb_grads(n, gs, step, gen, keep=None):
    """test_head_optimizer_gpu.sgd_grads: the scaled norm (over `keep`, the trained elements) is 100 (steps 0 and 2) or 10 (step 1).  Every element is of the
    size of the rest (|g| >= 0.25 of a unit normal's scale), so no update is a quotient of two roundings and every segment's un is far from 0."""
    import torch
    g = torch.randn(n, generator=gen).numpy().astype(np.float64)
    g = np.sign(g + (g == 0)) * (0.25 + np.abs(g))
    k = g if keep is None else np.where(keep, g, 0.0)
    return (g * ((10.0 if step == 1 else 100.0) / (gs * np.sqrt((k ** 2).sum())))).astype(np.float32)


def rel(got, ref):
    """max abs error over max abs reference."""
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.abs(np.asarray(got, dtype=np.float64) - ref).max() / max(np.abs(ref).max(), 1e-300))


def case_inputs(n, gs, segs=None):
    """Start state and the three gradients of a kernel-level case: (p0, m0, v0, [g0, g1, g2]); the moments start at zero as timm's do."""
    import torch
    gen = torch.Generator().manual_seed(n * 13 + int(gs * 1000) + (7 if segs is not None else 0))
    p0 = torch.randn(n, generator=gen).numpy()
    keep = None
    if segs is not None:
        keep = np.repeat(np.array([s[1] >= 0 for s in segs]), seg_lens(n, segs))
    return p0, np.zeros(n, np.float32), np.zeros(n, np.float32), [lamb_grads(n, gs, s, gen, keep) for s in range(3)]


def fp32_figures(n, gs, segs=None, **kw):
    """Worst distance over the three steps of the fp32 restatement from the fp64 one, each keeping its own state: (params, exp_avg, exp_avg_sq, ratios)."""
    p0, m0, v0, grads = case_inputs(n, gs, segs)
    tab = segs if segs is not None else ((0, 1.0, 1.0),)
    t = np.repeat(np.array([s[1] >= 0 for s in tab]), seg_lens(n, tab))
    a = [p0.astype(np.float64), m0.astype(np.float64), v0.astype(np.float64)]
    b = [p0.astype(np.float32), m0.astype(np.float32), v0.astype(np.float32)]
    worst = [0.0, 0.0, 0.0, 0.0]
    for s, g in enumerate(grads):
        mx = 0.0 if s == 2 else MAX_NORM
        ra = lamb_ref(a[0], a[1], a[2], g, gs, mx, s + 1, tab, **kw)
        rb = lamb_ref(b[0], b[1], b[2], g, gs, mx, s + 1, tab, ft=np.float32, **kw)
        a, b = list(ra[:3]), list(rb[:3])
        worst = [max(w, rel(y, x)) for w, x, y in zip(worst, [x[t] for x in a] + [ra[3]], [y[t] for y in b] + [rb[3]])]
    return tuple(worst)


if __name__ == "__main__":
    for n in (1, 255, 257, 5000, 262147):
        for gs in (1.0, 0.125):
            print("(%d, %s): (%.3e, %.3e, %.3e, %.3e)," % ((n, gs) + fp32_figures(n, gs)))
    print("('table', 0.125): (%.3e, %.3e, %.3e, %.3e)," % fp32_figures(SEG_N, 0.125, SEGMENTS))
    print("('table_always_adapt', 0.125): (%.3e, %.3e, %.3e, %.3e)," % fp32_figures(SEG_N, 0.125, SEGMENTS, always_adapt=1))
