"""The last two stages of a training step through the C ABI, each against an fp64 restatement written here: the TSN head (tsn_clshead.py: per-frame
average pool -> dropout -> fc -> consensus mean over the segments -> cross-entropy; csrc/head.hip frame_pool / head_fc_seg / ce_loss / head_fc_bwd_w /
head_dpool / head_dfeat and its inference kernels head_pool / head_fc / average_clip) and the fused clip_grad_norm_ + SGD step (dist_utils.py:61-67 +
torch.optim.SGD; csrc/optim.hip sqsum_* / norm_finalize / sgd_kernel).  The references take the same explicit dropout mask, labels and segment table as
the kernels; inputs come from seeded generators.

Bounds.  Every bound is one the suite already uses for these kernels (test_train_gpu.py test_stem_wgrad_maxpool_head_sgd_vs_oracle, test_conv_gpu.py):
loss 1e-5, head tensors 5e-5, inference head 1e-5, gradient norm 1e-5, parameters and momentum 1e-6, all relative to the tensor's largest magnitude.  The
same operations restated in fp32 on the CPU (torch for the head, numpy for the optimizer) against the fp64 references sit at least 10 x under each of them
at every case below, except the optimizer's parameters and momentum at seven cases (SGD_FP32: 1.0e-7 ... 1.4e-7 against 1e-6), whose bound is 10 x the fp32
figure measured for that case; the worst figures of that run are next to each bound."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import rel_err
from mvfnet_amd import synth

pytestmark = pytest.mark.gpu

P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)  # noqa: E731
F32, BF16 = torch.float32, torch.bfloat16


def _lib():
    from mvfnet_amd import _lib as L
    return L.lib, L.check


def close(got, ref, bound, what):
    """max-norm relative error under `bound`, and every element within rtol = bound, atol = bound * max|ref|."""
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    assert np.isfinite(got).all(), what
    e = rel_err(got, ref)
    print("%s: rel_err %.3g (bound %g)" % (what, e, bound))
    assert e < bound, (what, e)
    np.testing.assert_allclose(got, ref, rtol=bound, atol=bound * float(np.abs(ref).max()) if ref.size else 0.0, err_msg=what)


# ------------------------------------------------------------------------------------------------ 1. head, training
# (clips, T, hw, c, classes): the path each case exists for.  per = ceil(classes / 25) classes per workgroup of head_fc_seg_kernel.
HEAD_CASES = {
    "c36_k10_empty_class_ranges": (3, 4, 9, 36, 10),            # c below one wave, per = 1, 15 of the 25 class ranges empty
    "degenerate_1x1x1x4x1": (1, 1, 1, 4, 1),
    "k174_per7_c260": (5, 3, 12, 260, 174),                     # half-empty rounds with clamped weight rows; c no multiple of 64 or 256
    "k400_per16_clips17": (17, 2, 4, 64, 400),                  # per = 16 exactly; clips cross head_fc_bwd_w's 16-clip register chunk
    "k401_per17_second_round_clips33": (33, 1, 4, 64, 401),     # the smallest class count whose ranges take the second round; three clip chunks
    "k700_per28_hw49_c2048_dfeat_grid_stride": (2, 8, 49, 2048, 700),   # the real map: hw * c = 100352 > 65536, head_dfeat's loop iterates
}
HEAD_BOUND = 5e-5      # fp32 torch on the CPU vs fp64, worst over all cases: see test_head_train_vs_fp64's docstring
LOSS_BOUND = 1e-5


def head_inputs(case, dtype, p):
    clips, T, hw, c, classes = case
    gen = torch.Generator().manual_seed(((clips * 31 + T) * 131 + hw) * 8191 + c * 701 + classes + int(p * 10) * 1000003)
    feat = torch.randn(clips * T, hw, c, generator=gen) + 0.5
    if dtype == BF16:
        feat = feat.to(BF16).float()             # the reference takes the rounded input: input rounding is not part of the error
    w = torch.randn(classes, c, generator=gen) / float(np.sqrt(c))
    b = torch.randn(classes, generator=gen)
    labels = torch.randint(0, classes, (clips,), generator=gen)
    labels[0], labels[-1] = 0, classes - 1
    mask = None
    if p > 0:
        mask = (torch.rand(clips * T, c, generator=gen) >= p).float() * (1.0 / (1.0 - p))      # pre-scaled keep mask
        assert 0 < int((mask == 0).sum()) < mask.numel() or mask.numel() <= 4
    return dict(case=case, feat=feat, w=w, b=b, labels=labels, mask=mask)


def head_ref(inp, ft=torch.float64):
    """pooled = mean_hw(feat) * mask, scores = mean_T(pooled @ W^T + b), loss = cross_entropy(scores, labels); gradients by autograd."""
    clips, T, hw, c, classes = inp["case"]
    feat, w, b = (inp[k].to(ft).clone().requires_grad_(True) for k in ("feat", "w", "b"))
    pooled = feat.mean(1)
    if inp["mask"] is not None:
        pooled = pooled * inp["mask"].to(ft)
    scores = (pooled @ w.t() + b).reshape(clips, T, classes).mean(1)
    scores.retain_grad()
    loss_part = F.cross_entropy(scores, inp["labels"], reduction="none")
    loss = loss_part.mean()
    loss.backward()
    out = dict(pooled=pooled, scores=scores, loss_part=loss_part, loss=loss, dscores=scores.grad, dfc_w=w.grad, dfc_b=b.grad, dfeat=feat.grad)
    return {k: v.detach().double().numpy() for k, v in out.items()}


def head_run(inp, dtype, with_mask=True):
    lib, check = _lib()
    clips, T, hw, c, classes = inp["case"]
    dev, dt, nan = "cuda", 0 if dtype == F32 else 1, float("nan")
    fg, wg, bg, lab = inp["feat"].to(dev, dtype).contiguous(), inp["w"].to(dev), inp["b"].to(dev), inp["labels"].to(dev)
    mg = inp["mask"].to(dev) if (with_mask and inp["mask"] is not None) else None
    pooled, scores, dsc = (torch.full(s, nan, device=dev) for s in ((clips * T, c), (clips, classes), (clips, classes)))
    lp, lo = torch.full((clips,), nan, device=dev), torch.full((1,), nan, device=dev)
    check(lib.mvf_head_train_fwd(P(fg), clips, T, hw, c, P(wg), P(bg), classes, P(lab), P(mg), P(pooled), P(scores), P(dsc), P(lp), P(lo), dt, None), "head_train_fwd")
    dfw, dfb, dpool = torch.full((classes, c), nan, device=dev), torch.full((classes,), nan, device=dev), torch.empty(clips, c, device=dev)
    dfeat = torch.full((clips * T, hw, c), nan, device=dev).to(dtype)
    check(lib.mvf_head_train_bwd(P(dsc), P(pooled), P(wg), P(mg), clips, T, hw, c, classes, P(dfw), P(dfb), P(dpool), P(dfeat), dt, None), "head_train_bwd")
    torch.cuda.synchronize()
    out = dict(pooled=pooled, scores=scores, loss_part=lp, loss=lo, dscores=dsc, dfc_w=dfw, dfc_b=dfb, dfeat=dfeat)
    return {k: v.float().cpu().double().numpy() for k, v in out.items()}


@pytest.mark.parametrize("p", [0.0, 0.5, 0.8], ids=["nomask", "p0.5", "p0.8"])
@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", list(HEAD_CASES))
def test_head_train_vs_fp64(name, dtype, p):
    """mvf_head_train_fwd / mvf_head_train_bwd with an explicit dropout mask against the fp64 restatement, at the class counts (174, 400, 401, 700), clip
    counts (17, 33) and the feature map (49 x 2048) at which the kernels take their other paths (HEAD_CASES).
    The same head in fp32 torch on the CPU against the fp64 reference, worst over the 6 cases x 3 masks x 2 input roundings: loss 1.2e-7 (bound 1e-5), scores
    1.8e-7, pooled 1.8e-7, dscores 1.5e-7, dfc_w 3.0e-7, dfc_b 2.7e-7, dfeat 1.1e-6 (bound 5e-5; the 2048 x 700 case, bf16-rounded input, p = 0.5): all more
    than 10 x under, so every case keeps the suite's existing bounds."""
    inp = head_inputs(HEAD_CASES[name], dtype, p)
    ref, got = head_ref(inp), head_run(inp, dtype)
    assert np.isfinite(got["loss"]).all()
    print("loss: |got - ref| / |ref| = %.3g" % (abs(got["loss"][0] - ref["loss"]) / max(abs(ref["loss"]), 1e-30)))
    assert abs(got["loss"][0] - ref["loss"]) <= LOSS_BOUND * abs(ref["loss"])
    for k in ("scores", "pooled", "dscores", "dfc_w", "dfc_b"):
        close(got[k], ref[k], HEAD_BOUND, k)
    if dtype == F32:
        close(got["dfeat"], ref["dfeat"], HEAD_BOUND, "dfeat")
    else:       # one bf16 rounding on the store
        assert np.isfinite(got["dfeat"]).all()
        d, r = np.abs(got["dfeat"] - ref["dfeat"]), np.abs(ref["dfeat"])
        print("dfeat (bf16): worst excess over 2^-8 |ref|, relative to max|ref|: %.3g" % (float((d - 2.0 ** -8 * r).max()) / max(float(r.max()), 1e-30)))
        assert (d <= 2.0 ** -8 * r + HEAD_BOUND * float(r.max())).all()
    if inp["mask"] is not None:
        dropped = inp["mask"].numpy() == 0
        assert (got["pooled"][dropped] == 0.0).all()
        assert (got["dfeat"][np.broadcast_to(dropped[:, None, :], got["dfeat"].shape)] == 0.0).all()
        # the mask reached the kernels: the same call without it gives another step
        free = head_run(inp, dtype, with_mask=False)
        assert not np.array_equal(free["pooled"], got["pooled"]) and not np.array_equal(free["scores"], got["scores"])
        if HEAD_CASES[name][4] > 1:          # one class: dscores = 0 and every gradient with it, mask or not
            assert not np.array_equal(free["dfeat"], got["dfeat"]) and not np.array_equal(free["dfc_w"], got["dfc_w"])


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", ["c36_k10_empty_class_ranges", "k401_per17_second_round_clips33"])
def test_fused_forms_equal_the_stand_alone_losses_on_their_own_scores(name, dtype):
    """mvf_head_train_fwd against mvf_ce_loss and mvf_head_train_fwd_soft against mvf_ce_loss_soft, with the p = 0.5 mask: dscores, loss_part and loss of the
    fused form are, bit for bit, the stand-alone loss run on the fused form's own scores, and pooled and scores hold the same bits in the hard and the soft
    form (one pair of score launches, one loss launcher behind both; the BCE and focal forms have this test in test_bce_gpu.py / test_focal_gpu.py)."""
    lib, check = _lib()
    inp = head_inputs(HEAD_CASES[name], dtype, 0.5)
    clips, T, hw, c, classes = inp["case"]
    dev, dt, nan = "cuda", 0 if dtype == F32 else 1, float("nan")
    fg, wg, bg, lab, mg = inp["feat"].to(dev, dtype).contiguous(), inp["w"].to(dev), inp["b"].to(dev), inp["labels"].to(dev), inp["mask"].to(dev)
    gen = torch.Generator().manual_seed(clips * 7 + classes)
    targets = (torch.rand(clips, classes, generator=gen) ** 3).to(dev)
    full = lambda *s: torch.full(s, nan, device=dev)  # noqa: E731
    got = {}
    for form, fused, alone, tg in (("hard", lib.mvf_head_train_fwd, lib.mvf_ce_loss, lab), ("soft", lib.mvf_head_train_fwd_soft, lib.mvf_ce_loss_soft, targets)):
        pooled, scores, dsc, lp, lo = full(clips * T, c), full(clips, classes), full(clips, classes), full(clips), full(1)
        check(fused(P(fg), clips, T, hw, c, P(wg), P(bg), classes, P(tg), P(mg), P(pooled), P(scores), P(dsc), P(lp), P(lo), dt, None), form)
        dsc2, lp2, lo2 = full(clips, classes), full(clips), full(1)
        check(alone(P(scores), P(tg), clips, classes, P(dsc2), P(lp2), P(lo2), None), form)
        torch.cuda.synchronize()
        assert torch.isfinite(dsc).all() and torch.isfinite(lp).all() and torch.isfinite(lo).all() and torch.isfinite(scores).all()
        for a, b_, what in ((dsc, dsc2, "dscores"), (lp, lp2, "loss_part"), (lo, lo2, "loss")):
            assert torch.equal(a.view(torch.int32), b_.view(torch.int32)), (form, what)
        got[form] = (pooled, scores)
    for a, b_, what in zip(got["hard"], got["soft"], ("pooled", "scores")):
        assert torch.equal(a.view(torch.int32), b_.view(torch.int32)), what


# ------------------------------------------------------------------------------------------------ 2. cross-entropy
@pytest.mark.parametrize("scale", [1, 40, 200])
@pytest.mark.parametrize("classes", [1, 10, 257, 400, 1000])
@pytest.mark.parametrize("clips", [1, 7])
def test_ce_loss_vs_fp64_log_softmax(clips, classes, scale):
    """mvf_ce_loss at score scales where fp32 exp overflows without the max-subtraction (above 88), with one row labelled by its arg-min (the largest
    loss the row can have); classes above 256 run ce_loss_kernel's class-stride loops.  loss_part is compared relative to its largest element: a row
    labelled by its arg-max at scale 200 has a loss of 1e-40, which fp32 cannot hold next to the row maximum.
    fp32 torch on the CPU vs fp64, worst over the 30 cases: loss_part 6.2e-8, loss 1.0e-7 (bound 1e-5), dscores 1.4e-7 (bound 5e-5)."""
    lib, check = _lib()
    gen = torch.Generator().manual_seed(clips * 100003 + classes * 211 + scale)
    s = torch.randn(clips, classes, generator=gen) * scale
    labels = torch.randint(0, classes, (clips,), generator=gen)
    labels[0] = int(s[0].argmin())
    s64 = s.double().requires_grad_(True)
    lp_ref = -F.log_softmax(s64, 1)[torch.arange(clips), labels]
    lp_ref.mean().backward()
    lp_ref, loss_ref, dsc_ref = lp_ref.detach().numpy(), float(lp_ref.mean()), s64.grad.numpy()
    dev, nan = "cuda", float("nan")
    sg, lab = s.to(dev), labels.to(dev)
    dsc, lp, lo = torch.full((clips, classes), nan, device=dev), torch.full((clips,), nan, device=dev), torch.full((1,), nan, device=dev)
    check(lib.mvf_ce_loss(P(sg), P(lab), clips, classes, P(dsc), P(lp), P(lo), None), "ce_loss")
    lp2, lo2 = torch.full((clips,), nan, device=dev), torch.full((1,), nan, device=dev)
    check(lib.mvf_ce_loss(P(sg), P(lab), clips, classes, None, P(lp2), P(lo2), None), "ce_loss")
    torch.cuda.synchronize()
    assert torch.isfinite(lp).all() and torch.isfinite(lo).all() and torch.isfinite(dsc).all()
    close(lp.cpu().numpy(), lp_ref, LOSS_BOUND, "loss_part")
    assert abs(float(lo) - loss_ref) <= LOSS_BOUND * abs(loss_ref), (float(lo), loss_ref)
    close(dsc.cpu().numpy(), dsc_ref, HEAD_BOUND, "dscores")
    assert torch.equal(lp2, lp) and torch.equal(lo2, lo)


# ------------------------------------------------------------------------------------------------ 3. inference head
# rows per clip = T * hw: head_pool_kernel's 16 row lanes take four rows each (r + 48 < rows) in the main loop, the rest in the tail
POOL_ROWS = {1: (1, 1), 15: (3, 5), 17: (1, 17), 48: (4, 12), 49: (1, 49), 63: (7, 9), 64: (8, 8), 65: (5, 13), 113: (1, 113), 392: (8, 49)}
INFER_BOUND = 1e-5     # fp32 torch on the CPU vs fp64, worst over all cases: pooled 2.1e-7, scores 3.0e-7


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("rows", list(POOL_ROWS), ids=lambda r: "rows%d" % r)
def test_head_pool_fc_vs_fp64(rows, dtype):
    """mvf_head_pool_fc against mean-then-linear in fp64: row counts on both sides of the four-rows-in-flight main loop (no main loop below 49 rows, main
    loop without a tail at 64, main loop then tail at 49, 63, 65, 113, 392), c = 4 (one channel lane), 68 (a second, mostly empty workgroup), 2048."""
    lib, check = _lib()
    T, hw = POOL_ROWS[rows]
    assert T * hw == rows
    clips, dev, nan = 3, "cuda", float("nan")
    for c in (4, 68, 2048):
        for classes in (10, 400):
            gen = torch.Generator().manual_seed(rows * 4099 + c * 17 + classes)
            feat = torch.randn(clips * T, hw, c, generator=gen) + 0.5
            if dtype == BF16:
                feat = feat.to(BF16).float()
            w, b = torch.randn(classes, c, generator=gen) / float(np.sqrt(c)), torch.randn(classes, generator=gen)
            pooled_ref = feat.double().reshape(clips, rows, c).mean(1)
            ref = pooled_ref @ w.double().t() + b.double()
            fg, wg, bg = feat.to(dev, dtype).contiguous(), w.to(dev), b.to(dev)
            pooled, out = torch.full((clips, c), nan, device=dev), torch.full((clips, classes), nan, device=dev)
            check(lib.mvf_head_pool_fc(P(fg), clips, T, hw, c, P(wg), P(bg), classes, P(pooled), P(out), 0 if dtype == F32 else 1, None), "head_pool_fc")
            torch.cuda.synchronize()
            close(pooled.cpu().numpy(), pooled_ref.numpy(), INFER_BOUND, "pooled c=%d" % c)
            close(out.cpu().numpy(), ref.numpy(), INFER_BOUND, "scores c=%d classes=%d" % (c, classes))


@pytest.mark.parametrize("classes", [10, 257, 2048])
@pytest.mark.parametrize("clips", [1, 30])
@pytest.mark.parametrize("kind,scale", [(0, 1), (1, 1), (2, 1), (2, 100)], ids=["copy", "score", "prob", "prob_scale100"])
def test_average_clip_vs_fp64(kind, scale, clips, classes):
    """mvf_average_clip (base.py:43-74): None = the scores themselves, bit for bit; 'score' = mean over clips; 'prob' = mean of softmax, also at a score
    scale where exp overflows without the max-subtraction.  257 and 2048 classes run the kernel's class-stride loops (256 threads)."""
    lib, check = _lib()
    gen = torch.Generator().manual_seed(kind * 7 + scale + clips * 1009 + classes)
    s = torch.randn(clips, classes, generator=gen) * scale
    sg = s.cuda()
    out = torch.full((clips if kind == 0 else 1, classes), float("nan"), device="cuda")
    check(lib.mvf_average_clip(P(sg), clips, classes, kind, P(out), None), "average_clip")
    torch.cuda.synchronize()
    if kind == 0:
        assert torch.equal(out.cpu(), s)
        return
    ref = (F.softmax(s.double(), 1) if kind == 2 else s.double()).mean(0, keepdim=True)
    close(out.cpu().numpy(), ref.numpy(), INFER_BOUND, "average_clip")        # fp32 on the CPU vs fp64: 1.2e-7


# ------------------------------------------------------------------------------------------------ 4. optimizer
LR, MOM, WD, MAX_NORM = 0.015, 0.9, 1e-4, 40.0
NORM_BOUND = 1e-5      # fp32 numpy vs fp64, worst over all cases and steps: 1.5e-7 (n = 1048581)
PARAM_BOUND = 1e-6     # 6.5e-8 ... 9.8e-8 where SGD_FP32 does not list the case
MOM_BOUND = 1e-6       # 1.1e-8 ... 9.4e-8 likewise
# The cases at which the same update in fp32 numpy is NOT 10 x under the 1e-6 the suite uses at n = 5000: (n, grad_scale) -> worst fp32-vs-fp64 figure over the
# three steps, (parameters, momentum); None = under 1e-7.  A parameter near the largest one rounds by half an ulp of it, 3e-8 ... 6e-8 of the maximum, at each
# of three steps.  Those cases are held to 10 x their own figure.
SGD_FP32 = {(1, 1.0): (1.002e-7, None), (255, 1.0): (1.072e-7, None), (5000, 1.0): (None, 1.069e-7), (262147, 1.0): (1.089e-7, 1.113e-7),
            (262147, 0.125): (1.028e-7, 1.126e-7), (1048581, 1.0): (None, 1.292e-7), (1048581, 0.125): (1.264e-7, 1.378e-7)}
SEG_DTYPE = np.dtype([("first", "<i8"), ("lr_mult", "<f4"), ("decay_mult", "<f4")])      # mvf_sgd_segment_t


def sgd_ref(p, buf, g, gs, max_norm, first, nesterov=1, segs=((0, 1.0, 1.0),), ft=np.float64):
    """clip_grad_norm_(max_norm) over the trained elements of gs * g, then torch.optim.SGD with per-segment lr * lr_mult and wd * decay_mult;
    lr_mult < 0: the segment is excluded (gradient outside the norm, parameter and momentum untouched).  Returns (p, buf, norm, coef)."""
    n = p.size
    firsts = [s[0] for s in segs] + [n]
    lens = np.diff(firsts)
    lrm, dcm = np.repeat(np.array([s[1] for s in segs], dtype=ft), lens), np.repeat(np.array([s[2] for s in segs], dtype=ft), lens)
    excl = lrm < 0
    with np.errstate(all="ignore"):
        gg = ft(gs) * g.astype(ft)
        norm = ft(np.sqrt((gg[~excl].astype(np.float64) ** 2).sum()))
        coef = min(ft(1.0), ft(max_norm) / (norm + ft(1e-6))) if max_norm > 0 else ft(1.0)
        d = gg * coef + ft(WD) * dcm * p
        b = d if first else ft(MOM) * buf + d
        new_p = p - ft(LR) * lrm * (d + ft(MOM) * b if nesterov else b)
    return np.where(excl, p, new_p), np.where(excl, buf, b), float(norm), float(coef)


def sgd_grads(n, gs, step, gen):
    """Gradients whose scaled norm is 100 (steps 0 and 2) or 10 (step 1) against max_norm = 40: step 0 clips, step 1 does not, step 2 runs with
    max_norm = 0 and must not clip."""
    g = torch.randn(n, generator=gen).numpy()
    if n == 1 and g[0] == 0:
        g[0] = 1.0
    return (g * ((10.0 if step == 1 else 100.0) / (gs * np.sqrt((g.astype(np.float64) ** 2).sum())))).astype(np.float32)


def run_sgd_steps(n, gs, segs=None, nesterov=1, offset=0, excluded_fill=None, seed=0):
    """Three steps of the flat (segs None) or segment form on views at `offset` into buffers with `offset` guard elements on either side; after every
    step norm, parameters and momentum against the fp64 reference, which keeps its own fp64 state across the steps."""
    lib, check = _lib()
    dev = "cuda"
    gen = torch.Generator().manual_seed(n * 13 + int(gs * 1000) + nesterov + seed)
    tab = segs if segs is not None else ((0, 1.0, 1.0),)
    fig = SGD_FP32.get((n, gs), (None, None)) if len(tab) == 1 else (None, None)          # the one-segment table is the flat case
    param_bound, mom_bound = (max(b_, 10 * (f_ or 0.0)) for b_, f_ in zip((PARAM_BOUND, MOM_BOUND), fig))
    firsts = [s[0] for s in tab] + [n]
    excl = np.repeat(np.array([s[1] < 0 for s in tab]), np.diff(firsts))
    p_ref, b_ref = torch.randn(n, generator=gen).numpy().astype(np.float64), np.full(n, 7.0)
    guard = np.float32(-123.25)

    def dev_buf(v):
        full = torch.full((n + 2 * offset,), float(guard), device=dev)
        full[offset:offset + n] = torch.from_numpy(v.astype(np.float32)).to(dev)
        return full
    pf, bf = dev_buf(p_ref), dev_buf(b_ref)
    pg, bg = pf[offset:offset + n], bf[offset:offset + n]
    p0, b0 = pg.clone(), bg.clone()
    norm = torch.full((2,), float("nan"), device=dev)
    ws = torch.empty(lib.mvf_sgd_workspace_bytes(n), dtype=torch.uint8, device=dev)
    tabg = None
    if segs is not None:
        tabg = torch.from_numpy(np.array(list(segs), dtype=SEG_DTYPE).view(np.uint8)).to(dev)
    for step in range(3):
        g = sgd_grads(n, gs, step, gen)
        if excluded_fill is not None:           # excluded elements outside the norm: finite norm = 100 or 10 over the rest
            keep = np.where(excl, np.float32(0), g)
            g = (keep * ((10.0 if step == 1 else 100.0) / (gs * np.sqrt((keep.astype(np.float64) ** 2).sum())))).astype(np.float32)
            g[excl] = np.resize(np.array(excluded_fill, dtype=np.float32), int(excl.sum()))
        max_norm, first = (0.0 if step == 2 else MAX_NORM), int(step == 0)
        p_ref, b_ref, n_ref, c_ref = sgd_ref(p_ref, b_ref, g, gs, max_norm, first, nesterov, tab)
        assert (c_ref < 0.5) if step == 0 else (c_ref == 1.0), (step, c_ref)
        gf = dev_buf(g)
        gg = gf[offset:offset + n]
        if segs is None:
            check(lib.mvf_sgd_nesterov_step(P(pg), P(gg), P(bg), n, gs, max_norm, LR, MOM, WD, first, P(norm), P(ws), ws.numel(), None), "sgd_nesterov_step")
        else:
            check(lib.mvf_sgd_step_segments(P(pg), P(gg), P(bg), n, gs, max_norm, LR, MOM, WD, first, nesterov, P(tabg), len(segs), P(norm), P(ws),
                                            ws.numel(), None), "sgd_step_segments")
        torch.cuda.synchronize()
        nrm, coef = float(norm[0]), float(norm[1])
        pn, bn = pg.cpu().numpy(), bg.cpu().numpy()
        print("step %d: norm %.3g, params %.3g, momentum %.3g" % (step, abs(nrm - n_ref) / n_ref, rel_err(pn[~excl], p_ref[~excl]), rel_err(bn[~excl], b_ref[~excl])))
        assert np.isfinite(nrm) and abs(nrm - n_ref) < NORM_BOUND * n_ref, (step, nrm, n_ref)
        assert abs(coef - c_ref) <= 2e-5 * c_ref, (step, coef, c_ref)          # the norm's bound, and one rounding of the division
        assert np.isfinite(pn).all() and np.isfinite(bn).all()
        assert rel_err(pn, p_ref) < param_bound, step
        assert (np.abs(bn - b_ref) <= mom_bound * np.abs(b_ref).max()).all(), step
        if excl.any():                          # excluded segments: parameters and momentum bit-unchanged
            e = torch.from_numpy(excl).to(dev)
            assert torch.equal(pg[e], p0[e]) and torch.equal(bg[e], b0[e]), step
        if offset:                              # nothing outside the views was written
            for full in (pf, bf, gf):
                assert bool((full[:offset] == float(guard)).all()) and bool((full[offset + n:] == float(guard)).all()), step


@pytest.mark.parametrize("gs", [1.0, 0.125])
@pytest.mark.parametrize("n", [1, 255, 257, 5000, 262144 + 3, 1048576 + 5], ids=lambda n: "n%d" % n)
def test_sgd_nesterov_step_vs_fp64(n, gs):
    """mvf_sgd_nesterov_step, three steps (clipping / not clipping / max_norm = 0): n above 262144 iterates sqsum_partial_kernel's grid-stride loop
    (1024 workgroups x 256), n above 1048576 the update's (4096 x 256); 1, 255 and 257 are the one-workgroup edges."""
    run_sgd_steps(n, gs)


@pytest.mark.parametrize("n", [257, 5000])
def test_sgd_nesterov_step_on_offset_views_leaves_the_neighbours_alone(n):
    """The engine calls the step on views of its flat buffers (flat_params[off:]): 4-byte aligned only.  Same bounds; the elements before and after the
    three views keep their bits."""
    run_sgd_steps(n, 0.125, offset=1)


SEG_N = 262144 + 3
# segment starts inside and on the edges of a workgroup's 256-element run (7, 256, 257, 1000, 1001), deep in the buffer and on its last element;
# multipliers as build_optimizer's paramwise options give them (bias_lr_mult = 2 with bias_decay_mult = 0, norm_decay_mult = 0, ...); lr_mult < 0 = excluded
SEGMENTS = ((0, 1.0, 1.0), (7, 2.0, 0.0), (256, -1.0, 0.0), (257, 1.0, 0.0), (1000, 0.5, 0.5), (1001, -1.0, 1.0), (70000, 1.0, 1.0), (262146, 2.0, 0.0))


@pytest.mark.parametrize("fill", [(1e30,), (float("nan"), float("inf"), -float("inf"))], ids=["excluded_1e30", "excluded_nan_inf"])
@pytest.mark.parametrize("nesterov", [0, 1], ids=["plain_momentum", "nesterov"])
def test_sgd_step_segments_vs_fp64(nesterov, fill):
    """mvf_sgd_step_segments over eight segments whose starts are no multiples of 256, mixed lr / decay multipliers and two excluded segments (one
    element at 256, 68999 elements from 1001) whose gradients would make the norm infinite (1e30 squared in fp32) or NaN if they entered it."""
    run_sgd_steps(SEG_N, 0.125, segs=SEGMENTS, nesterov=nesterov, excluded_fill=fill)


def test_sgd_step_segments_single_segment_equals_the_flat_reference():
    """nseg = 1, {0, 1, 1}, nesterov = 1 is the flat form: against the flat form's fp64 reference, same bounds."""
    run_sgd_steps(SEG_N, 0.125, segs=((0, 1.0, 1.0),), nesterov=1)


@pytest.mark.parametrize("form", ["plain", "ema", "guarded"])
@pytest.mark.parametrize("n", [1, 257, 5000, 1048576 + 5], ids=lambda n: "n%d" % n)
def test_sgd_one_segment_table_equals_the_flat_form_bit_for_bit(n, form):
    """The flat entry point against the segment entry point with the table {0, 1, 1} and nesterov = 1, from the same start state, over a clipping step with
    first_step = 1, a non-clipping one and one with max_norm = 0: parameters, momentum and norm_out (ema: and the average; guarded: mvf_sgd_step_guarded with
    segments = NULL against the table, with the average and the counters) equal as int32 bit patterns after every step.  n = 1048581 takes the update
    grid (4096 x 256) into a second sweep."""
    lib, check = _lib()
    dev, gs, ema_m = "cuda", 0.125, 0.25
    gen = torch.Generator().manual_seed(n * 7 + 3)
    start = [torch.randn(n, generator=gen).to(dev) for _ in range(3)]                     # parameters, momentum, average
    tab = torch.from_numpy(np.array([(0, 1.0, 1.0)], dtype=SEG_DTYPE).view(np.uint8)).to(dev)

    def side():
        return dict(p=start[0].clone(), b=start[1].clone(), e=start[2].clone(), norm=torch.full((2,), float("nan"), device=dev),
                    guard=torch.zeros(4, dtype=torch.int32, device=dev), ws=torch.empty(lib.mvf_sgd_workspace_bytes(n), dtype=torch.uint8, device=dev))

    def step(s, g, max_norm, first, seg):
        head = (P(s["p"]), P(g), P(s["b"]), n, gs, max_norm, LR, MOM, WD, first)
        segs = (1, P(tab), 1) if seg else ()
        tail = (P(s["norm"]), P(s["ws"]), s["ws"].numel(), None)
        if form == "plain":
            fn, mid = (lib.mvf_sgd_step_segments if seg else lib.mvf_sgd_nesterov_step), ()
        elif form == "ema":
            fn, mid = (lib.mvf_sgd_step_segments_ema if seg else lib.mvf_sgd_nesterov_step_ema), (P(s["e"]), ema_m)
        else:
            fn, segs, mid = lib.mvf_sgd_step_guarded, segs or (1, None, 0), (P(s["e"]), ema_m, P(s["guard"]))
        check(fn(*(head + segs + mid + tail)), "sgd %s, %s" % (form, "table" if seg else "flat"))

    flat, seg = side(), side()
    for k in range(3):
        g = torch.from_numpy(sgd_grads(n, gs, k, gen)).to(dev)
        before = flat["p"].clone()
        for s, with_table in ((flat, False), (seg, True)):
            step(s, g, 0.0 if k == 2 else MAX_NORM, int(k == 0), with_table)
        torch.cuda.synchronize()
        for name in ("p", "b", "norm", "e", "guard"):
            assert torch.equal(flat[name].view(torch.int32), seg[name].view(torch.int32)), (k, name)
        coef = float(flat["norm"][1])
        assert (coef < 0.5) if k == 0 else (coef == 1.0), (k, coef)
        assert not torch.equal(flat["p"], before), k                                      # a step was applied
        assert torch.equal(flat["e"], start[2]) == (form == "plain"), k                   # the average moves in the forms that keep one
        assert flat["guard"].tolist() == ([0, 0, 0, k + 1] if form == "guarded" else [0, 0, 0, 0]), k


# ------------------------------------------------------------------------------------------------ 5. one engine step with the shipped dropout
def _model(depth, T, dropout):
    import mvfnet_amd
    m = mvfnet_amd.build_recognizer(mvfnet_amd.mvfnet_config(depth, T, dropout_ratio=dropout), None, dict(average_clips=None))
    sd = m.state_dict()
    vals = synth.synth_state_dict({"r%d/" % depth + k: tuple(v.shape) for k, v in sd.items()})
    m.load_state_dict({k: torch.from_numpy(vals["r%d/" % depth + k]) for k in sd}, strict=True)
    return m.cuda().train()


@pytest.mark.parametrize("plan", [False, True], ids=["eager", "plan_replay"])
def test_train_step_with_dropout_vs_oracle_given_the_engines_mask(plan):
    """The shipped recipe's dropout_ratio = 0.5 at test_train_step_ragged_shapes_vs_oracle's (3, 3, 80, 112) shape, fp32: the mask the engine drew
    (TrainEngine._step_tensors, captured on the instance) goes to the CPU oracle (net_torch.forward_train(drop_mask=...)); loss, stage outputs and every
    gradient norm at that test's bounds.  plan_replay: the same comparison on a step replayed from the engine's launch plan (two eager steps, two
    recordings, then the replay; no optimizer step in between, so the parameters are the initial ones) -- stage outputs are not exposed by a replay."""
    from oracle import net_torch
    b, t, h, w = 3, 3, 80, 112
    torch.manual_seed(1234)
    m = _model(50, t, 0.5)
    eng = m.train_engine(dtype=F32)
    assert eng.dropout == 0.5
    masks, draw = [], eng._step_tensors

    def capture(imgs, labels):
        out = draw(imgs, labels)
        masks.append(out[1])
        return out
    eng._step_tensors = capture
    imgs_np, labels_np = synth.synth_clip_batch(b, t, h, w), synth.synth_labels(b)
    sd = {k: v.detach().cpu().clone() for k, v in m.state_dict().items()}
    leaves = {k: v.requires_grad_(True) for k, v in sd.items() if v.dtype.is_floating_point and "running" not in k}
    stages = {}
    if plan:
        eng.use_plan = True
        for i in range(eng.plan_warmup + 3):
            st = list(getattr(eng, "_plans", {}).values())
            replay = bool(st) and st[0]["plan"] is not None
            assert replay == (i == eng.plan_warmup + 2), (i, [(s_["eager"], s_["tries"]) for s_ in st])
            loss = eng._forward_backward(torch.from_numpy(imgs_np).cuda(), torch.from_numpy(labels_np).cuda(), exchange=True)
        assert len(masks) == eng.plan_warmup + 3
    else:
        loss = eng.forward(torch.from_numpy(imgs_np).cuda(), torch.from_numpy(labels_np).cuda(), stages=stages)
        eng.backward()
        assert len(masks) == 1
    torch.cuda.synchronize()
    mask = masks[-1].cpu()
    # the mask itself: a scaled keep mask of nn.Dropout(0.5) over the pooled (frames, channels) features
    n_el = b * t * 2048
    assert tuple(mask.shape) == (b * t, 2048) and bool(((mask == 0) | (mask == 2)).all())
    keep = float((mask == 2).sum()) / n_el
    assert abs(keep - 0.5) < 6 * np.sqrt(0.25 / n_el), keep
    ref_stages = {}
    ref_loss = net_torch.forward_train(torch.from_numpy(imgs_np), torch.from_numpy(labels_np), sd, depth=50, T=t, new_buffers={}, stages=ref_stages, drop_mask=mask)
    ref_loss.backward()
    ref_loss = float(ref_loss.detach())
    print("loss %.3g" % (abs(float(loss) - ref_loss) / abs(ref_loss)))
    assert abs(float(loss) - ref_loss) < 5e-5 * abs(ref_loss)
    if not plan:
        got = {k: v.float().cpu().permute(0, 3, 1, 2).contiguous().numpy() for k, v in stages.items() if k in ref_stages}
        assert len(got) >= 5
        for k in got:
            assert rel_err(got[k], ref_stages[k].detach().numpy()) < 2e-4, k
    params, errs = dict(m.named_parameters()), {}
    for k, leaf in leaves.items():
        if k in params and leaf.grad is not None:
            r = float(leaf.grad.double().norm())
            errs[k] = abs(float(eng.grad_of(params[k]).double().norm()) - r) / max(r, 1e-6)
    assert len(errs) > 150
    head = [v for k, v in errs.items() if k.startswith("cls_head") or k.startswith("backbone.layer4.2")]
    med, worst = np.median(list(errs.values())), max(errs.values())
    print("gradient norms: head / layer4.2 %.3g, median %.3g, worst %.3g" % (max(head), med, worst))
    assert max(head) < 3e-3, max(head)
    assert med < 3e-3 and worst < 5e-2, (med, worst)
