"""clip_grad_norm_ + torch.optim.AdamW / Adam (non-amsgrad, non-maximize) restated in numpy, in the style of test_head_optimizer_gpu.sgd_ref: per-segment
lr * lr_mult and weight_decay * decay_mult, lr_mult < 0 = the segment is excluded (gradient outside the norm, parameter and both moments untouched).

    d  = g * grad_scale * coef
    decoupled = 0:  d = d + wd_i * p            decoupled = 1:  p = p * (1 - lr_i * wd_i)
    m' = b1 * m + (1 - b1) * d
    v' = b2 * v + (1 - b2) * d^2
    p' = p - (lr_i / (1 - b1^t)) * m' / (sqrt(v') / sqrt(1 - b2^t) + eps)

ft = np.float64 is the reference.  ft = np.float32 is the same update as an fp32 implementation makes it: every scalar (1 - b1, 1 - b2, 1 - lr_i * wd_i,
lr_i / (1 - b1^t), sqrt(1 - b2^t)) is formed in double and rounded to fp32 ONCE, as torch does with its Python scalars; the arrays are fp32 throughout.  Its
distance from the fp64 reference is what the kernel tests scale their bounds from (ADAMW_FP32 in test_adamw_gpu.py; tools: `python tests/adamw_numpy.py`)."""
import numpy as np

LR, BETAS, EPS, WD, MAX_NORM = 1e-3, (0.9, 0.999), 1e-8, 0.05, 40.0


def adamw_ref(p, m, v, g, gs, max_norm, t, decoupled=1, segs=((0, 1.0, 1.0),), ft=np.float64, lr=LR, betas=BETAS, eps=EPS, wd=WD):
    """One step; t = the step count after it (1 for the first).  Returns (p, m, v, norm, coef)."""
    n = p.size
    firsts = [s[0] for s in segs] + [n]
    lens = np.diff(firsts)
    lrm = np.repeat(np.array([s[1] for s in segs], dtype=np.float64), lens)
    dcm = np.repeat(np.array([s[2] for s in segs], dtype=np.float64), lens)
    excl = lrm < 0
    b1, b2 = float(betas[0]), float(betas[1])
    lr_i, wd_i = lr * lrm, wd * dcm                                    # doubles, per element
    step = (lr_i / (1.0 - b1 ** t)).astype(ft)
    shrink = (1.0 - lr_i * wd_i).astype(ft)
    bc2 = ft(np.sqrt(1.0 - b2 ** t))
    with np.errstate(all="ignore"):
        gg = ft(gs) * g.astype(ft)
        norm = ft(np.sqrt((gg[~excl].astype(np.float64) ** 2).sum()))
        coef = min(ft(1.0), ft(max_norm) / (norm + ft(1e-6))) if max_norm > 0 else ft(1.0)
        d = gg * coef
        pv = p.astype(ft)
        if decoupled:
            pv = pv * shrink
        else:
            d = d + wd_i.astype(ft) * pv
        mn = ft(b1) * m.astype(ft) + ft(1.0 - b1) * d
        vn = ft(b2) * v.astype(ft) + ft(1.0 - b2) * (d * d)
        pn = pv - step * (mn / (np.sqrt(vn) / bc2 + ft(eps)))
    return np.where(excl, p, pn), np.where(excl, m, mn), np.where(excl, v, vn), float(norm), float(coef)


def adamw_grads(n, gs, step, gen):
    """test_head_optimizer_gpu.sgd_grads: the scaled norm is 100 (steps 0 and 2) or 10 (step 1)."""
    import torch
    g = torch.randn(n, generator=gen).numpy()
    if n == 1 and g[0] == 0:
        g[0] = 1.0
    return (g * ((10.0 if step == 1 else 100.0) / (gs * np.sqrt((g.astype(np.float64) ** 2).sum())))).astype(np.float32)


def rel(got, ref):
    """max abs error over max abs reference."""
    ref = np.asarray(ref, dtype=np.float64)
    return float(np.abs(np.asarray(got, dtype=np.float64) - ref).max() / max(np.abs(ref).max(), 1e-300))


def case_seed(n, gs, decoupled):
    return n * 13 + int(gs * 1000) + 7 * decoupled


def case_inputs(n, gs, decoupled):
    """Start state and the three gradients of a kernel-level case: (p0, m0, v0, [g0, g1, g2]); the moments start at zero as torch's do."""
    import torch
    gen = torch.Generator().manual_seed(case_seed(n, gs, decoupled))
    p0 = torch.randn(n, generator=gen).numpy()
    return p0, np.zeros(n, np.float32), np.zeros(n, np.float32), [adamw_grads(n, gs, s, gen) for s in range(3)]


def fp32_figures(n, gs, decoupled):
    """Worst distance over the three steps of the fp32 restatement from the fp64 one, each keeping its own state: (params, exp_avg, exp_avg_sq)."""
    p0, m0, v0, grads = case_inputs(n, gs, decoupled)
    a = [p0.astype(np.float64), m0.astype(np.float64), v0.astype(np.float64)]
    b = [p0.astype(np.float32), m0.astype(np.float32), v0.astype(np.float32)]
    worst = [0.0, 0.0, 0.0]
    for s, g in enumerate(grads):
        mx = 0.0 if s == 2 else MAX_NORM
        a = list(adamw_ref(a[0], a[1], a[2], g, gs, mx, s + 1, decoupled)[:3])
        b = list(adamw_ref(b[0], b[1], b[2], g, gs, mx, s + 1, decoupled, ft=np.float32)[:3])
        worst = [max(w, rel(y, x)) for w, x, y in zip(worst, a, b)]
    return tuple(worst)


if __name__ == "__main__":
    for n in (1, 255, 257, 5000, 262147, 1048581):
        for gs in (1.0, 0.125):
            for dec in ((1,) if n == 1048581 else (0, 1)):
                print("(%d, %s, %d): (%.3e, %.3e, %.3e)," % ((n, gs, dec) + fp32_figures(n, gs, dec)))
