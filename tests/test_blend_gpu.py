"""GPU: batch blending and soft labels -- mvf_stem_blend / mvf_soft_targets (csrc/blend.hip), mvf_ce_loss_soft / mvf_head_train_fwd_soft (csrc/head.hip)
against the fp64 restatement in blend_numpy.py, and the train engine with them: a device-blended step equals the host-blended step bit for bit, a replayed
launch plan equals the eager steps bit for bit while lambda changes from step to step, the uint8 input path is blended behind the frame kernel, and eval is
untouched.  The reference project has neither feature: the semantics are those of include/mvfnet_hip.h.

Bounds.  Copies are compared bit for bit.  A blended fp32 element carries three fp32 roundings (1 - lam, the two products folded with the sum):
|out - v| <= 2^-22 max(|a|, |b|); bf16 adds one rounding to nearest of the result: 2^-8 |v|.  Targets: 2^-22 absolute (entries are at most 1).  Loss and head
bounds are the suite's own for these kernels (test_head_optimizer_gpu.py: loss 1e-5, head tensors 5e-5, relative to the tensor's largest magnitude); the same
soft-target arithmetic in fp32 torch on the CPU against fp64 over the grid of test 3 is worst 1.9e-7 for the loss and 1.3e-6 for dscores."""
import ctypes as C

import numpy as np
import pytest
import torch

import blend_numpy as BN
from test_head_optimizer_gpu import HEAD_BOUND, HEAD_CASES, LOSS_BOUND, close, head_inputs
from test_launch_plan_gpu import _engine

pytestmark = pytest.mark.gpu

P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)  # noqa: E731
F32, BF16 = torch.float32, torch.bfloat16
PAD = 3


def _lib():
    from mvfnet_amd import _lib as L
    return L.lib, L.check


def _wp(w):
    return (w + 2 * PAD + 2 + 1) // 2 * 2


# ------------------------------------------------------------------------------------------------ 1. the blend kernel
def blend_tables(b, h, w):
    """Tables for a batch of 3 or 4 clips.  Between them (in ONE table at b = 4): an empty box, a full-image box, a box with odd x0 and odd x1, a box
    touching two borders, partner == i with lam_px = 0.3, lam_px = 1, lam_px = 0; the partner column holds a 3-cycle (not an involution).  A bf16 unit is a
    pair of pixels at an even padded column: with the pad of 3 the boxes whose x0 or x1 is EVEN split a pair (`corner`'s x1, the one-pixel boxes), the odd ones
    end on a pair boundary -- both kinds are here."""
    odd, corner, full, empty = (2, 3, h - 2, w - 1 - (w % 2)), (0, 0, h // 2, w // 2 + 1), (0, 0, h, w), (0, 0, 0, 0)
    assert odd[1] % 2 == 1 and odd[3] % 2 == 1
    if b == 4:
        tabs = [([(1,) + empty, (2,) + odd, (0,) + corner, (3,) + full], [0.6, 1.0, 0.0, 0.3]),
                ([(1,) + full, (2,) + corner, (0,) + odd, (3,) + empty], [0.25, 0.7, 0.45, 0.3])]
    else:
        tabs = [([(1,) + empty, (2,) + odd, (0,) + corner], [0.6, 1.0, 0.0]),
                ([(0,) + empty, (0,) + full, (1,) + odd], [0.3, 0.7, 0.45]),
                ([(1,) + (h - 3, w - 4, h, w), (2,) + (1, 1, 2, 2), (0,) + (0, 3, h, 4)], [1.0, 0.5, 1.0])]
    return [(np.array(r, dtype=np.int32), np.stack([np.array(l, dtype=np.float32), np.array(l, dtype=np.float32)], 1)) for r, l in tabs]


def stem_operand(b, t, h, w, dtype, seed):
    """A stem operand as mvf_stem_prep lays it out: zero border, zero fourth channel, values already in the storage type."""
    gen = torch.Generator().manual_seed(seed)
    hp, wp = h + 2 * PAD, _wp(w)
    xp = torch.zeros(b, t, hp, wp, 4)
    xp[:, :, PAD:PAD + h, PAD:PAD + w, :3] = torch.randn(b, t, h, w, 3, generator=gen) * 1.5
    return xp.to(dtype)


def _bits(x):
    return x.view(torch.int32 if x.dtype == F32 else torch.int16)


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", [(3, 2, 10, 10), (4, 1, 9, 11)], ids=["3x2x10x10", "4x1x9x11"])
def test_stem_blend_vs_fp64(shape, dtype):
    lib, check = _lib()
    b, t, h, w = shape
    hp, wp = h + 2 * PAD, _wp(w)
    assert (hp, wp) == {(10, 10): (16, 18), (9, 11): (15, 20)}[(h, w)]
    xp = stem_operand(b, t, h, w, dtype, 17 * h + w)
    xg = xp.cuda()
    seen = set()
    for rows, wts in blend_tables(b, h, w):
        out = torch.full(xp.shape, float("nan"), dtype=dtype, device="cuda")
        rg, wg = torch.from_numpy(rows).cuda(), torch.from_numpy(wts).cuda()
        check(lib.mvf_stem_blend(P(xg), b, t, hp, wp, PAD, P(rg), P(wg), P(out), 0 if dtype == F32 else 1, None), "stem_blend")
        torch.cuda.synchronize()
        got = out.cpu()
        v, kind = BN.blend_ref(xp.float().numpy(), rows, wts, PAD)
        assert torch.isfinite(got.float()).all()
        x64 = xp.double().numpy()
        g64 = got.double().numpy()
        for i in range(b):
            p = int(rows[i, 0])
            k = np.broadcast_to(kind[i][None, :, :, None], x64[i].shape)
            seen.update(np.unique(kind[i]).tolist())
            gi, ai, bi = _bits(got[i]).numpy(), _bits(xp[i]).numpy(), _bits(xp[p]).numpy()
            assert np.array_equal(gi[k == BN.COPY_A], ai[k == BN.COPY_A]), "clip %d: own elements are not copies" % i
            assert np.array_equal(gi[k == BN.COPY_B], bi[k == BN.COPY_B]), "clip %d: box elements are not copies of the partner" % i
            m = k == BN.BLEND
            if m.any():
                err, big = np.abs(g64[i] - v[i])[m], np.maximum(np.abs(x64[i]), np.abs(x64[p]))[m]
                bound = 2.0 ** -22 * big + (2.0 ** -8 * np.abs(v[i])[m] if dtype == BF16 else 0.0)
                print("clip %d: blended elements, worst error / bound %.3g" % (i, float((err / np.maximum(bound, 1e-300)).max())))
                assert (err <= bound).all()
        border = torch.ones(hp, wp, dtype=torch.bool)
        border[PAD:PAD + h, PAD:PAD + w] = False
        assert (_bits(got)[:, :, border] == 0).all() and (_bits(got)[..., 3] == 0).all()          # bit-zero, not -0
    assert seen == {BN.COPY_A, BN.COPY_B, BN.BLEND}


# ------------------------------------------------------------------------------------------------ 2. targets
@pytest.mark.parametrize("with_rows", [True, False], ids=["rows", "norows"])
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("classes", [1, 10, 400])
def test_soft_targets(classes, eps, with_rows):
    lib, check = _lib()
    clips = 6
    gen = np.random.RandomState(classes * 7 + int(eps * 10))
    labels = gen.randint(0, classes, clips).astype(np.int64)
    rows = np.zeros((clips, 5), dtype=np.int32)
    rows[:, 0] = [1, 2, 0, 3, 5, 4]                       # a 3-cycle, a self-partner, a swap
    labels[5] = labels[4]                                 # a clip whose partner carries the same label
    wts = np.stack([np.ones(clips, dtype=np.float32), np.array([1.0, 0.25, 0.6, 0.3, 0.7, 0.0], dtype=np.float32)], 1)
    lg = torch.from_numpy(labels).cuda()
    rg, wg = (torch.from_numpy(rows).cuda(), torch.from_numpy(wts).cuda()) if with_rows else (None, None)
    out = torch.full((clips, classes), float("nan"), device="cuda")
    check(lib.mvf_soft_targets(P(lg), P(rg) if with_rows else None, P(wg) if with_rows else None, clips, classes, C.c_float(eps), P(out), None), "soft_targets")
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    r, q = (rows, wts) if with_rows else (None, None)
    if eps == 0:
        assert np.array_equal(got, BN.soft_targets_ref(labels, r, q, classes, 0.0, np.float32))
    ref = BN.soft_targets_ref(labels, r, q, classes, eps)
    print("targets: worst |t - ref| = %.3g (bound %.3g)" % (float(np.abs(got - ref).max()), 2.0 ** -22))
    assert (np.abs(got - ref) <= 2.0 ** -22).all()
    if not with_rows and eps == 0:
        assert np.array_equal(got, np.eye(classes, dtype=np.float32)[labels])


# ------------------------------------------------------------------------------------------------ 3. soft-target cross-entropy
@pytest.mark.parametrize("eps", [0.0, 0.1])
@pytest.mark.parametrize("scale", [1, 40, 200])
@pytest.mark.parametrize("classes", [1, 10, 257, 400, 1000])
@pytest.mark.parametrize("clips", [1, 7])
def test_ce_loss_soft_vs_fp64(clips, classes, scale, eps):
    """The grid of test_ce_loss_vs_fp64_log_softmax, against Mixup targets; row 0 carries its arg-min label (the largest loss the row can have)."""
    lib, check = _lib()
    gen = torch.Generator().manual_seed(clips * 100003 + classes * 211 + scale)
    s = torch.randn(clips, classes, generator=gen) * scale
    labels = torch.randint(0, classes, (clips,), generator=gen)
    labels[0] = int(s[0].argmin())
    rows = np.zeros((clips, 5), dtype=np.int32)
    rows[:, 0] = np.roll(np.arange(clips), -1)
    lam = np.array([1.0, 0.25, 0.6, 0.9, 0.5, 0.05, 0.0], dtype=np.float32)[:clips]
    wts = np.stack([lam, lam], 1)
    tgt = BN.soft_targets_ref(labels.numpy(), rows, wts, classes, eps, np.float32)
    lp_ref, loss_ref, dsc_ref = BN.ce_soft_ref(s.numpy(), tgt)
    dev, nan = "cuda", float("nan")
    sg, tg = s.to(dev), torch.from_numpy(tgt).to(dev)
    dsc, lp, lo = torch.full((clips, classes), nan, device=dev), torch.full((clips,), nan, device=dev), torch.full((1,), nan, device=dev)
    check(lib.mvf_ce_loss_soft(P(sg), P(tg), clips, classes, P(dsc), P(lp), P(lo), None), "ce_loss_soft")
    lp2, lo2 = torch.full((clips,), nan, device=dev), torch.full((1,), nan, device=dev)
    check(lib.mvf_ce_loss_soft(P(sg), P(tg), clips, classes, None, P(lp2), P(lo2), None), "ce_loss_soft")
    torch.cuda.synchronize()
    assert torch.isfinite(lp).all() and torch.isfinite(lo).all() and torch.isfinite(dsc).all()
    close(lp.cpu().numpy(), lp_ref, LOSS_BOUND, "loss_part")
    print("loss: |got - ref| / |ref| = %.3g" % (abs(float(lo) - loss_ref) / max(abs(loss_ref), 1e-30)))
    assert abs(float(lo) - loss_ref) <= LOSS_BOUND * abs(loss_ref), (float(lo), loss_ref)
    close(dsc.cpu().numpy(), dsc_ref, HEAD_BOUND, "dscores")
    assert torch.equal(lp2, lp) and torch.equal(lo2, lo)                     # dscores == NULL: the same loss bits
    if classes == 1:
        assert float(lo) == 0.0 and (lp == 0).all()                         # sum_k t_k (lse - s_k) is exactly 0 for one class
    if eps == 0:
        # one-hot targets agree with the integer-label kernel within the same bounds
        lab = labels.to(dev)
        onehot = torch.zeros(clips, classes, device=dev)
        onehot[torch.arange(clips), lab] = 1.0
        d1, l1, o1 = torch.full((clips, classes), nan, device=dev), torch.full((clips,), nan, device=dev), torch.full((1,), nan, device=dev)
        d0, l0, o0 = torch.full((clips, classes), nan, device=dev), torch.full((clips,), nan, device=dev), torch.full((1,), nan, device=dev)
        check(lib.mvf_ce_loss_soft(P(sg), P(onehot), clips, classes, P(d1), P(l1), P(o1), None), "ce_loss_soft")
        check(lib.mvf_ce_loss(P(sg), P(lab), clips, classes, P(d0), P(l0), P(o0), None), "ce_loss")
        torch.cuda.synchronize()
        close(l1.cpu().numpy(), l0.cpu().double().numpy(), LOSS_BOUND, "loss_part, one-hot vs labels")
        assert abs(float(o1) - float(o0)) <= LOSS_BOUND * abs(float(o0))
        close(d1.cpu().numpy(), d0.cpu().double().numpy(), HEAD_BOUND, "dscores, one-hot vs labels")


# ------------------------------------------------------------------------------------------------ 4. the train head with soft targets
def head_ref_soft(inp, tgt, ft=torch.float64):
    clips, T, hw, c, classes = inp["case"]
    feat, w, b = (inp[k].to(ft).clone().requires_grad_(True) for k in ("feat", "w", "b"))
    pooled = feat.mean(1)
    if inp["mask"] is not None:
        pooled = pooled * inp["mask"].to(ft)
    scores = (pooled @ w.t() + b).reshape(clips, T, classes).mean(1)
    scores.retain_grad()
    t = torch.from_numpy(np.asarray(tgt, dtype=np.float64))
    loss_part = (t * (torch.logsumexp(scores, 1, keepdim=True) - scores)).sum(1)
    loss = loss_part.mean()
    loss.backward()
    out = dict(pooled=pooled, scores=scores, loss_part=loss_part, loss=loss, dscores=scores.grad, dfc_w=w.grad, dfc_b=b.grad, dfeat=feat.grad)
    return {k: v.detach().double().numpy() for k, v in out.items()}


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("name", ["k174_per7_c260", "k401_per17_second_round_clips33"])
def test_head_train_soft_vs_fp64(name, dtype):
    """mvf_head_train_fwd_soft + mvf_head_train_bwd with Mixup targets (built by mvf_soft_targets) and a p = 0.5 dropout mask; bounds and the bf16 dfeat rule
    of test_head_train_vs_fp64."""
    lib, check = _lib()
    inp = head_inputs(HEAD_CASES[name], dtype, 0.5)
    clips, T, hw, c, classes = inp["case"]
    rows = np.zeros((clips, 5), dtype=np.int32)
    rows[:, 0] = np.roll(np.arange(clips), 1)
    lam = np.float32(0.37)
    wts = np.full((clips, 2), lam, dtype=np.float32)
    tgt32 = BN.soft_targets_ref(inp["labels"].numpy(), rows, wts, classes, 0.0, np.float32)
    ref = head_ref_soft(inp, tgt32)
    dev, dt, nan = "cuda", 0 if dtype == F32 else 1, float("nan")
    fg, wg, bg, lab, mg = inp["feat"].to(dev, dtype).contiguous(), inp["w"].to(dev), inp["b"].to(dev), inp["labels"].to(dev), inp["mask"].to(dev)
    tg, rg, qg = torch.full((clips, classes), nan, device=dev), torch.from_numpy(rows).to(dev), torch.from_numpy(wts).to(dev)
    check(lib.mvf_soft_targets(P(lab), P(rg), P(qg), clips, classes, C.c_float(0.0), P(tg), None), "soft_targets")
    pooled, scores, dsc = (torch.full(s_, nan, device=dev) for s_ in ((clips * T, c), (clips, classes), (clips, classes)))
    lp, lo = torch.full((clips,), nan, device=dev), torch.full((1,), nan, device=dev)
    check(lib.mvf_head_train_fwd_soft(P(fg), clips, T, hw, c, P(wg), P(bg), classes, P(tg), P(mg), P(pooled), P(scores), P(dsc), P(lp), P(lo), dt, None), "head_train_fwd_soft")
    dfw, dfb, dpool = torch.full((classes, c), nan, device=dev), torch.full((classes,), nan, device=dev), torch.empty(clips, c, device=dev)
    dfeat = torch.full((clips * T, hw, c), nan, device=dev).to(dtype)
    check(lib.mvf_head_train_bwd(P(dsc), P(pooled), P(wg), P(mg), clips, T, hw, c, classes, P(dfw), P(dfb), P(dpool), P(dfeat), dt, None), "head_train_bwd")
    torch.cuda.synchronize()
    assert np.array_equal(tg.cpu().numpy(), tgt32)
    got = {k: v.float().cpu().double().numpy() for k, v in dict(pooled=pooled, scores=scores, loss_part=lp, loss=lo, dscores=dsc, dfc_w=dfw, dfc_b=dfb, dfeat=dfeat).items()}
    print("loss: |got - ref| / |ref| = %.3g" % (abs(got["loss"][0] - ref["loss"]) / max(abs(ref["loss"]), 1e-30)))
    assert abs(got["loss"][0] - ref["loss"]) <= LOSS_BOUND * abs(ref["loss"])
    for k in ("scores", "pooled", "loss_part", "dscores", "dfc_w", "dfc_b"):
        close(got[k], ref[k], HEAD_BOUND, k)
    if dtype == F32:
        close(got["dfeat"], ref["dfeat"], HEAD_BOUND, "dfeat")
    else:       # one bf16 rounding on the store
        assert np.isfinite(got["dfeat"]).all()
        d, r = np.abs(got["dfeat"] - ref["dfeat"]), np.abs(ref["dfeat"])
        assert (d <= 2.0 ** -8 * r + HEAD_BOUND * float(r.max())).all()


def test_head_loss_takes_soft_labels_and_smooths_integer_labels_in_training():
    """TSNClsHead.loss: float (B, K) labels through mvf_ce_loss_soft; integer labels smoothed with label_smooth_eps in training mode only (mvf_soft_targets
    with rows == NULL); both against the fp64 restatement at the suite's loss bound.  Soft labels with eps > 0 are refused, as in the engine."""
    from mvfnet_amd.heads.tsn_clshead import TSNClsHead
    clips, classes = 5, 37
    gen = torch.Generator().manual_seed(23)
    s = torch.randn(clips, classes, generator=gen) * 3
    labels = torch.randint(0, classes, (clips, 1), generator=gen)
    soft = torch.rand(clips, classes, generator=gen)
    soft = soft / soft.sum(1, keepdim=True)
    head = TSNClsHead(in_channels=8, num_classes=classes, label_smooth_eps=0.1).cuda()

    def loss(lab):
        return float(head.loss(s.cuda(), lab.cuda())["loss_cls"])

    ref_hard = BN.ce_soft_ref(s.numpy(), BN.soft_targets_ref(labels.numpy(), None, None, classes, 0.0))[1]
    ref_smooth = BN.ce_soft_ref(s.numpy(), BN.soft_targets_ref(labels.numpy(), None, None, classes, 0.1))[1]
    ref_soft = BN.ce_soft_ref(s.numpy(), soft.numpy())[1]
    assert abs(ref_smooth - ref_hard) > 1e-3 * abs(ref_hard)
    head.train()
    got = loss(labels)
    print("smoothed: |got - ref| / |ref| = %.3g" % (abs(got - ref_smooth) / abs(ref_smooth)))
    assert abs(got - ref_smooth) <= LOSS_BOUND * abs(ref_smooth)
    with pytest.raises(ValueError, match="soft"):
        loss(soft)
    head.eval()                                        # eval: no smoothing; soft labels as they are
    got = loss(labels)
    assert abs(got - ref_hard) <= LOSS_BOUND * abs(ref_hard)
    got = loss(soft)
    print("soft: |got - ref| / |ref| = %.3g" % (abs(got - ref_soft) / abs(ref_soft)))
    assert abs(got - ref_soft) <= LOSS_BOUND * abs(ref_soft)
    head.train()
    head.label_smooth_eps = 0.0
    assert abs(loss(soft) - ref_soft) <= LOSS_BOUND * abs(ref_soft)
    with pytest.raises(ValueError):
        loss(soft[:, :5])                              # float labels that are no (B, K) matrix are not truncated to integers


# ------------------------------------------------------------------------------------------------ 5. - 8. the engine
def cutmix_table(h, w):
    """Three clips, partners in a 3-cycle, boxes as in test 1 (empty; odd x0 and x1; touching two borders); lam_lab from the box area."""
    rows = np.array([(1, 0, 0, 0, 0), (2, 2, 3, h - 2, w - 1 - (w % 2)), (0, 0, 0, h // 2, w // 2 + 1)], dtype=np.int32)
    area = (rows[:, 3] - rows[:, 1]) * (rows[:, 4] - rows[:, 2])
    wts = np.stack([np.ones(3, dtype=np.float32), (1.0 - area / float(h * w)).astype(np.float32)], 1)
    return rows, wts


def _steps(eng, m, imgs, labels, n=2):
    losses = [eng.train_step(imgs.clone(), labels.clone(), lr=0.01).clone() for _ in range(n)]
    torch.cuda.synchronize()
    return torch.cat(losses), eng.flat_params.clone(), [b_.clone() for b_ in m.buffers()]


def test_engine_device_blend_equals_host_blend_bit_for_bit():
    """Run A: CutMix on the device (ExplicitBlending) with integer labels.  Run B: no blending, the same pastes made on the host (pure copies, exact) and
    the soft (B, K) labels of blend_numpy handed in.  Same kernels from the stem on: losses, parameters and buffers are equal bit for bit.  Run C, plain
    labels on the unblended clips, differs: the table reached the kernels."""
    from mvfnet_amd.blending import ExplicitBlending
    gen = torch.Generator(device="cuda").manual_seed(3)
    imgs = torch.randn(3, 4, 3, 64, 64, device="cuda", generator=gen)
    labels = torch.randint(0, 400, (3, 1), device="cuda", generator=gen)
    rows, wts = cutmix_table(64, 64)
    out = {}
    for run in "ABC":
        torch.manual_seed(7)
        m, eng = _engine(F32, True)
        if run == "A":
            eng.blending = ExplicitBlending(rows, wts)
            out[run] = _steps(eng, m, imgs, labels)
        elif run == "B":
            pasted = torch.from_numpy(BN.paste_nchw(imgs.cpu().numpy(), rows)).cuda()
            soft = torch.from_numpy(BN.soft_targets_ref(labels.cpu().numpy(), rows, wts, 400, 0.0, np.float32)).cuda()
            assert not torch.equal(pasted, imgs)
            out[run] = _steps(eng, m, pasted, soft)
        else:
            out[run] = _steps(eng, m, imgs, labels)
    (la, pa, ba), (lb, pb, bb), (lc, pc, _) = out["A"], out["B"], out["C"]
    assert torch.isfinite(la).all()
    assert torch.equal(la, lb), (la, lb)
    assert torch.equal(pa, pb)
    for x, y in zip(ba, bb):
        assert torch.equal(x, y)
    assert not torch.equal(la, lc) and not torch.equal(pa, pc)


class _FirstDrawForever(object):
    """What a replay that froze the table would compute: the first draw, every step."""

    def __init__(self, inner):
        self.inner, self.first = inner, None

    def draw(self, b, h, w):
        if self.first is None:
            self.first = self.inner.draw(b, h, w)
        return self.first


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_replayed_blended_steps_equal_eager_steps_bit_for_bit(dtype):
    from mvfnet_amd.blending import MixupBlending
    gen = torch.Generator(device="cuda").manual_seed(3)
    batches = [(torch.randn(2, 4, 3, 64, 64, device="cuda", generator=gen), torch.randint(0, 400, (2, 1), device="cuda", generator=gen)) for _ in range(3)]
    lrs = [0.015, 0.01, 0.02, 0.005]
    steps = 9

    def run(use_plan, blending):
        torch.manual_seed(7)
        m, eng = _engine(dtype, use_plan)
        eng.blending = blending
        losses = [eng.train_step(batches[i % 3][0].clone(), batches[i % 3][1].clone(), lr=lrs[i % 4]).clone() for i in range(steps)]
        torch.cuda.synchronize()
        return eng, torch.cat(losses), eng.flat_params.clone(), [b_.clone() for b_ in m.buffers()]

    eng_p, loss_p, par_p, buf_p = run(True, MixupBlending(alpha=0.8, seed=5))
    eng_e, loss_e, par_e, buf_e = run(False, MixupBlending(alpha=0.8, seed=5))
    st = list(eng_p._plans.values())
    assert len(st) == 1 and st[0]["plan"] is not None and st[0]["eager"] == eng_p.plan_warmup and st[0]["tries"] == 2, [(s_["eager"], s_["tries"]) for s_ in st]
    plan = st[0]["plan"]
    assert "mvf_stem_blend" in plan.names and "mvf_soft_targets" in plan.names and "mvf_head_train_fwd_soft" in plan.names and "mvf_head_train_fwd" not in plan.names
    assert all(len(v) >= 1 for v in plan.slots.values())
    assert not getattr(eng_e, "_plans", None)
    assert torch.isfinite(loss_p).all()
    assert torch.equal(loss_p, loss_e), (loss_p, loss_e)
    assert torch.equal(par_p, par_e)
    for a, b in zip(buf_p, buf_e):
        assert torch.equal(a, b)
    # lambda and the partners are read from the device table at every replay: a run on the first draw alone gives other losses
    _, loss_f, _, _ = run(False, _FirstDrawForever(MixupBlending(alpha=0.8, seed=5)))
    assert torch.equal(loss_f[:1], loss_p[:1]) and not torch.equal(loss_f, loss_p)
    assert not torch.equal(loss_f[eng_p.plan_warmup + 2:], loss_p[eng_p.plan_warmup + 2:])              # ... on the replayed steps themselves


def test_callers_soft_labels_are_a_patched_slot_of_the_plan():
    """Soft (B, K) labels handed in by the caller, a fresh tensor with other values every step: the replayed steps equal the eager ones bit for bit, so the
    tensor's address is patched per run (the plan's `labels` slot) and nothing of the first recording's labels is frozen."""
    gen = torch.Generator(device="cuda").manual_seed(13)
    imgs = [torch.randn(2, 4, 3, 64, 64, device="cuda", generator=gen) for _ in range(2)]
    softs = []
    for _ in range(3):
        t_ = torch.rand(2, 400, device="cuda", generator=gen) ** 8
        softs.append(t_ / t_.sum(1, keepdim=True))
    out = {}
    for use_plan in (True, False):
        torch.manual_seed(7)
        m, eng = _engine(BF16, use_plan)
        losses = [eng.train_step(imgs[i % 2].clone(), softs[i % 3].clone(), lr=0.01).clone() for i in range(7)]
        torch.cuda.synchronize()
        out[use_plan] = (eng, torch.cat(losses), eng.flat_params.clone())
    eng_p = out[True][0]
    st = list(eng_p._plans.values())
    assert len(st) == 1 and st[0]["plan"] is not None and st[0]["tries"] == 2, [(s_["eager"], s_["tries"]) for s_ in st]
    plan = st[0]["plan"]
    assert "mvf_head_train_fwd_soft" in plan.names and "mvf_soft_targets" not in plan.names and len(plan.slots["labels"]) == 1
    assert torch.isfinite(out[True][1]).all() and len(set(out[True][1].tolist())) > 3
    assert torch.equal(out[True][1], out[False][1]) and torch.equal(out[True][2], out[False][2])


def test_a_plan_without_blending_is_not_replayed_with_it():
    from mvfnet_amd.blending import MixupBlending
    gen = torch.Generator(device="cuda").manual_seed(5)
    m, eng = _engine(BF16, True, dropout=0.0)
    a = (torch.randn(2, 4, 3, 64, 64, device="cuda", generator=gen), torch.randint(0, 400, (2, 1), device="cuda", generator=gen))
    for _ in range(5):
        eng.train_step(*a)
    assert len(eng._plans) == 1 and all(s["plan"] is not None and "mvf_stem_blend" not in s["plan"].names for s in eng._plans.values())
    n_plain = next(iter(eng._plans.values()))["plan"].n_ops
    eng.blending = MixupBlending(alpha=0.8, seed=1)
    for _ in range(5):
        eng.train_step(*a)
    eng.blending, eng.label_smooth_eps = None, 0.1
    for _ in range(5):
        eng.train_step(*a)
    torch.cuda.synchronize()
    assert len(eng._plans) == 3 and all(s["plan"] is not None for s in eng._plans.values())
    n_ops = sorted(s["plan"].n_ops for s in eng._plans.values())
    assert n_ops == [n_plain, n_plain + 1, n_plain + 2], (n_plain, n_ops)      # + soft_targets; + soft_targets + stem_blend
    assert torch.isfinite(eng.flat_params).all()
    soft = torch.zeros(2, 400, device="cuda")
    soft[:, 3] = 1.0
    with pytest.raises(ValueError, match="soft"):
        eng.train_step(a[0], soft)                     # soft labels and smoothing: refused, not silently combined


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_uint8_frames_are_blended_behind_the_frame_kernel(dtype):
    from mvfnet_amd.blending import ExplicitBlending
    from mvfnet_amd.preprocess import FramePipeline
    B, T, hs, ws, c = 3, 4, 72, 80, 64
    fr = torch.from_numpy(np.random.RandomState(2).randint(0, 256, (B, T, hs, ws, 3)).astype(np.uint8)).cuda()
    win = torch.from_numpy(np.stack([np.full(B * T, 3), np.full(B * T, 7), np.repeat([0, 1, 0], T)], 1).astype(np.int32)).cuda()
    labels = torch.tensor([[3], [111], [7]], device="cuda")
    rows, wts = cutmix_table(c, c)
    m, eng = _engine(dtype, False, dropout=0.0)
    eng.input_pipeline, eng.input_window = FramePipeline([123.675, 116.28, 103.53], [58.395, 57.12, 57.375], to_rgb=True, crop_size=c), win
    l0 = eng.forward(fr, labels).clone()
    xp0 = eng.saved["xp"].clone()
    eng.blending = ExplicitBlending(rows, wts)
    l1 = eng.forward(fr, labels).clone()
    xp1 = eng.saved["xp"].clone()
    torch.cuda.synchronize()
    nt, hp, wp, _ = xp0.shape
    want = BN.paste(_bits(xp0).cpu().numpy().reshape(B, T, hp, wp, 4), rows, pad=PAD)
    assert np.array_equal(_bits(xp1).cpu().numpy().reshape(B, T, hp, wp, 4), want)
    assert not torch.equal(xp1, xp0) and torch.isfinite(l1).all() and float(l1) != float(l0)


def test_eval_is_untouched_by_a_configured_blending():
    import mvfnet_amd
    from mvfnet_amd import synth
    cfg = mvfnet_amd.mvfnet_config(50, 4, dropout_ratio=0.5)
    cfg["cls_head"]["label_smooth_eps"] = 0.1
    m = mvfnet_amd.build_recognizer(cfg, dict(blending=dict(type="MixupBlending", alpha=0.2, seed=1)), dict(average_clips=None))
    sd = m.state_dict()
    vals = synth.synth_state_dict({"r50/" + k: tuple(v.shape) for k, v in sd.items()})
    m.load_state_dict({k: torch.from_numpy(vals["r50/" + k]) for k in sd})
    m = m.cuda().eval()
    gen = torch.Generator(device="cuda").manual_seed(1)
    x = torch.randn(2, 4, 3, 64, 64, device="cuda", generator=gen)
    with_cfg = m(x, None, return_loss=False)
    m.blending, m.cls_head.label_smooth_eps = None, 0.0
    without = m(x, None, return_loss=False)
    assert np.isfinite(with_cfg).all() and np.array_equal(with_cfg, without)
