"""GPU: RandomErasing on the stem operand -- mvf_stem_erase (csrc/erase.hip) against the fp64 restatement in erase_numpy.py, and the train engine with it:
an erased step equals the step on host-erased clips bit for bit, a replayed launch plan equals the eager steps bit for bit while table and key change from
step to step, the uint8 input path is erased behind the frame kernel, erasing comes before the blend, and an engine without it does what it did.  The
reference project has no such feature: the semantics are those of include/mvfnet_hip.h.

Bounds.  Untouched elements, the zero border / padding columns / fourth channel and constant fills are compared bit for bit (a colour is rounded once to the
storage type).  Noise: |got - v| <= 2^-17 in fp32 against the fp64 restatement.  Derivation: the value is r * cos(t) with r = sqrt(-2 ln u1) <= 5.77 and
t = fl(2 pi u2) < 6.2832; the error is dominated by the rounding of t (half an ulp of a number below 8: 2^-22 = 2.4e-7) times r, i.e. about 1.4e-6, next to
half an ulp of the result (at most 2^-22) and of r.  The numpy fp32 restatement of the same formula against fp64 is worst at 1.8e-6 over 2 x 10^6 draws; test 1
recomputes and prints that figure for its own key and planes.  2^-17 = 7.6e-6 leaves a factor of four for the device's 1-2 ulp logf / sinf / cosf.  bf16 adds
one rounding to nearest of the result: 2^-8 |v|, the suite's bound for one rounding to bf16.  A wrong generator is off by order 1 and cannot hide there."""
import ctypes as C

import numpy as np
import pytest
import torch

import erase_numpy as EN
from test_blend_gpu import PAD, _bits, _wp, stem_operand
from test_launch_plan_gpu import _engine

pytestmark = pytest.mark.gpu

P = lambda t: C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)  # noqa: E731
F32, BF16 = torch.float32, torch.bfloat16
KEY = np.array([0xDEADBEEF, 0x01234567], dtype=np.uint32)
NOISE_BOUND = 2.0 ** -17


def _lib():
    from mvfnet_amd import _lib as L
    return L.lib, L.check


def _erase(xg, boxes, fill, key, hp, wp, dtype):
    """mvf_stem_erase in place on the device tensor xg (planes, hp, wp, 4)."""
    lib, check = _lib()
    bg, fg = torch.from_numpy(boxes).cuda(), torch.from_numpy(fill).cuda()
    kg = torch.from_numpy(key.view(np.int32)).cuda()
    check(lib.mvf_stem_erase(P(xg), xg.shape[0], hp, wp, PAD, P(bg), boxes.shape[1], P(fg), P(kg), 0 if dtype == F32 else 1, None), "stem_erase")
    torch.cuda.synchronize()
    return xg


# ------------------------------------------------------------------------------------------------ 1. the kernel
def erase_tables(planes, h, w):
    """Two tables for 4 or 6 planes, max_boxes 1 and 3.  Between them: a plane with no box, a full-image box, a box with odd x0 and odd x1 and one with even x0
    and even x1 (a bf16 unit is a pair of pixels at an even PADDED column: with the pad of 3 an even image edge splits a pair, an odd one ends on a pair
    boundary), one-pixel boxes, boxes touching two borders, overlapping boxes of mode 1 then 2 and of mode 2 then 1 (the later slot wins), and modes outside
    {0, 1, 2} -- with a full-image box behind them -- that are treated as unused.  Colours carry a non-zero fourth word, which is ignored."""
    rs = np.random.RandomState(planes * 100 + h)
    odd, even = (2, 3, h - 2, w - 1 - (w % 2)), (1, 2, h - 1, 6)
    assert odd[1] % 2 == 1 and odd[3] % 2 == 1 and even[1] % 2 == 0 and even[3] % 2 == 0
    full = (0, 0, h, w)
    one = [[(0, 0, 0, 0, 0)], [full + (2,)], [odd + (1,)], [even + (2,)], [(4, 4, 5, 5, 1)], [full + (7,)]][:planes]
    three = [[(0, 0, h // 2 + 1, w // 2 + 1, 1), (2, 2, h - 1, w - 2, 2), full + (9,)],                  # mode 1 then 2: the noise wins the overlap
             [(1, 1, h - 2, w - 1, 2), (3, 0, h, w // 2, 1), (0, 0, 0, 0, 0)],                           # mode 2 then 1: the colour wins; bottom-left borders
             [(4, 5, 5, 6, 2), (0, 0, 1, 1, 1), (h - 1, w - 1, h, w, 1)],                                 # one-pixel boxes, two of them in corners
             [full + (-1,), full + (0,), (2, 4, 6, 8, 1)],                                                # unused slots in front of an even-edged box
             [full + (1,), (0, 0, 0, 0, 0), (0, 0, 0, 0, 0)],
             [(0, 0, 0, 0, 0), (0, w - 3, h, w, 2), odd + (2,)]][:planes]                                 # top-right-bottom borders, then an overlap of two noises
    out = []
    for tab in (one, three):
        boxes = np.array(tab, dtype=np.int32)
        fill = (rs.randn(planes, boxes.shape[1], 4) * 1.3).astype(np.float32)
        assert (fill.view(np.int32) & 0xFFFF).all()                     # no colour is a bf16 number already: the rounding to the storage type is visible
        out.append((boxes, fill))
    return out


@pytest.mark.parametrize("dtype", [F32, BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("shape", [(3, 2, 10, 10), (4, 1, 9, 11)], ids=["3x2x10x10", "4x1x9x11"])
def test_stem_erase_vs_fp64(shape, dtype):
    """See the module docstring for the bounds.  The CPU figure of the derivation -- numpy's fp32 restatement against fp64 -- is recomputed here for this
    test's key over all pixels of its planes and printed beside the device's worst error."""
    b, t, h, w = shape
    planes, hp, wp = b * t, h + 2 * PAD, _wp(w)
    assert (hp, wp) == {(10, 10): (16, 18), (9, 11): (15, 20)}[(h, w)]
    xp = stem_operand(b, t, h, w, dtype, 17 * h + w).reshape(planes, hp, wp, 4)
    cpu32 = float(np.abs(EN.plane_noise(planes, h, w, KEY, np.float32).astype(np.float64) - EN.plane_noise(planes, h, w, KEY)).max())
    print("numpy fp32 restatement against fp64, key %s, %d x %d x %d pixels: worst %.3g (bound %.3g)" % (KEY.tolist(), planes, h, w, cpu32, NOISE_BOUND))
    assert cpu32 <= NOISE_BOUND
    border = torch.ones(hp, wp, dtype=torch.bool)
    border[PAD:PAD + h, PAD:PAD + w] = False
    seen, widths = set(), []
    for boxes, fill in erase_tables(planes, h, w):
        widths.append(boxes.shape[1])
        got = _erase(xp.cuda().clone(), boxes, fill, KEY, hp, wp, dtype).cpu()
        v, kind = EN.erase_ref(xp.float().numpy(), boxes, fill, KEY, PAD)
        seen.update(np.unique(kind).tolist())
        assert torch.isfinite(got.float()).all()
        gb, xb = _bits(got).numpy(), _bits(xp).numpy()
        m = kind == EN.UNTOUCHED
        assert np.array_equal(gb[m], xb[m]), "elements outside all boxes changed"
        assert (_bits(got)[:, border] == 0).all() and (_bits(got)[..., 3] == 0).all()                   # bit-zero, not -0
        m = kind == EN.CONST
        want = _bits(torch.from_numpy(v.astype(np.float32)).to(dtype)).numpy()
        assert m.any() and np.array_equal(gb[m], want[m]), "constant fills are not the colour rounded once to the storage type"
        m = kind == EN.NOISE
        g64 = got.double().numpy()
        err = np.abs(g64 - v)[m]
        bound = NOISE_BOUND + (2.0 ** -8 * np.abs(v)[m] if dtype == BF16 else 0.0)
        print("max_boxes %d: %d noise elements, worst error %.3g, worst error / bound %.3g; mean %.3f var %.3f" %
              (boxes.shape[1], int(m.sum()), float(err.max()), float((err / bound).max()), float(g64[m].mean()), float(g64[m].var())))
        assert m.any() and (err <= bound).all()
    assert seen == {EN.UNTOUCHED, EN.CONST, EN.NOISE} and widths == [1, 3]


def test_a_box_beyond_the_image_is_clamped_to_the_operand():
    """A table check_erase_table would refuse: the kernel clamps it instead of addressing outside the tensor.  Everything outside the operand's interior --
    rows and columns of the pad -- and the guard planes around the tensor keep their bits."""
    b, t, h, w = 1, 2, 9, 11
    hp, wp = h + 2 * PAD, _wp(w)
    xp = stem_operand(b, t, h, w, F32, 5).reshape(2, hp, wp, 4)
    guard = torch.full((4, hp, wp, 4), 3.0).cuda()
    guard[1:3] = xp.cuda()
    boxes = np.array([[(-5, -7, 1 << 30, 1 << 30, 1)], [(-(1 << 31), 2, 4, 1 << 20, 1)]], dtype=np.int32)
    fill = np.full((2, 1, 4), 2.5, dtype=np.float32)
    _erase(guard[1:3], boxes, fill, KEY, hp, wp, F32)
    got = guard.cpu()
    assert (got[0] == 3.0).all() and (got[3] == 3.0).all()
    inner = torch.zeros(hp, wp, dtype=torch.bool)
    inner[PAD:hp - PAD, PAD:wp - PAD] = True
    assert torch.equal(got[1:3][:, ~inner], xp[:, ~inner]) and (got[1][inner][:, :3] == 2.5).all() and (got[1:3][..., 3] == 0).all()
    assert (got[2, PAD:PAD + 4, PAD + 2:wp - PAD, :3] == 2.5).all() and torch.equal(got[2, PAD + 4:], xp[1, PAD + 4:])


# ------------------------------------------------------------------------------------------------ 2. determinism
def test_noise_is_deterministic_keyed_and_independent_of_the_storage_type():
    b, t, h, w = 3, 2, 10, 10
    planes, hp, wp = b * t, h + 2 * PAD, _wp(w)
    boxes, fill = erase_tables(planes, h, w)[1]
    other = np.array([KEY[0], KEY[1] ^ 1], dtype=np.uint32)
    _, kind = EN.erase_ref(np.zeros((planes, hp, wp, 4)), boxes, fill, KEY, PAD)
    noise = kind == EN.NOISE
    got = {}
    for dtype in (F32, BF16):
        xp = stem_operand(b, t, h, w, dtype, 3).reshape(planes, hp, wp, 4)
        a1 = _erase(xp.cuda().clone(), boxes, fill, KEY, hp, wp, dtype).cpu()
        a2 = _erase(xp.cuda().clone(), boxes, fill, KEY, hp, wp, dtype).cpu()
        o = _erase(xp.cuda().clone(), boxes, fill, other, hp, wp, dtype).cpu()
        assert np.array_equal(_bits(a1).numpy(), _bits(a2).numpy())                                    # the same table and key: the same bits
        ab, ob = _bits(a1).numpy(), _bits(o).numpy()
        assert np.array_equal(ab[~noise], ob[~noise])                                                  # another key changes the noise and nothing else
        changed = float((ab[noise] != ob[noise]).mean())
        print("%s: %.4f of the noise elements change with the key" % (dtype, changed))
        assert changed > (0.999 if dtype == F32 else 0.9)                                              # (two bf16 numbers coincide now and then)
        got[dtype] = a1
    g32, g16 = got[F32].double().numpy()[noise], got[BF16].double().numpy()[noise]
    print("fp32 against bf16 noise: worst |d| / |v| = %.3g; bf16 == fp32 rounded once: %s" % (float((np.abs(g32 - g16) / np.abs(g32)).max()),
                                                                                           torch.equal(got[F32].to(BF16)[torch.from_numpy(noise)], got[BF16][torch.from_numpy(noise)])))
    assert (np.abs(g32 - g16) <= 2.0 ** -8 * np.abs(g32)).all()


# ------------------------------------------------------------------------------------------------ 3. - 8. the engine
def engine_table(b, t, h, w, modes):
    """One table for b clips of t frames, max_boxes 2, `modes` cycling over the used slots: clip 0 has no box, the others an odd-edged and an overlapping
    even-edged box (per frame shifted by the frame index: the table is per plane, not per clip)."""
    boxes = np.zeros((b, t, 2, 5), dtype=np.int32)
    k = 0
    for i in range(1, b):
        for f in range(t):
            boxes[i, f, 0] = (2 + f, 3, h - 2, w - 1 - (w % 2), modes[k % len(modes)])
            boxes[i, f, 1] = (0, 2 * f, h // 2, w // 2 + 2, modes[(k + 1) % len(modes)])
            k += 1
    fill = (np.random.RandomState(b * 10 + t).randn(b * t, 2, 4) * 1.2).astype(np.float32)
    return boxes.reshape(b * t, 2, 5), fill


def _clips(seed=3, b=3):
    gen = torch.Generator(device="cuda").manual_seed(seed)
    return torch.randn(b, 4, 3, 64, 64, device="cuda", generator=gen), torch.randint(0, 400, (b, 1), device="cuda", generator=gen)


def _steps(eng, m, imgs, labels, n=2):
    losses, grads = [], []
    for _ in range(n):
        losses.append(eng.train_step(imgs.clone(), labels.clone(), lr=0.01).clone())
        grads.append(eng.flat_grads.clone())
    torch.cuda.synchronize()
    return torch.cat(losses), grads, eng.flat_params.clone(), [b_.clone() for b_ in m.buffers()]


def _assert_same_run(a, b):
    (la, ga, pa, ba), (lb, gb, pb, bb) = a, b
    assert torch.isfinite(la).all()
    assert torch.equal(la, lb), (la, lb)
    for x, y in zip(ga, gb):
        assert torch.equal(x, y)
    assert torch.equal(pa, pb)
    for x, y in zip(ba, bb):
        assert torch.equal(x, y)


def test_engine_constant_erase_equals_the_step_on_host_erased_clips_bit_for_bit():
    """Run A: mode-1 boxes erased on the device (ExplicitErasing).  Run B: no erasing, the same boxes overwritten on the host with the same fp32 colours.
    fp32 storage, so the stem sees the same bits: losses, the flat gradient buffer, parameters and buffers are equal bit for bit over two steps.  Run C, the
    untouched clips, differs: the table reached the kernel."""
    from mvfnet_amd.erasing import ExplicitErasing
    imgs, labels = _clips()
    boxes, fill = engine_table(3, 4, 64, 64, [1])
    out = {}
    for run in "ABC":
        torch.manual_seed(7)
        m, eng = _engine(F32, True)
        x = imgs
        if run == "A":
            eng.erasing = ExplicitErasing(boxes, fill, KEY)
        elif run == "B":
            x = torch.from_numpy(EN.erase_nchw(imgs.cpu().numpy(), boxes, fill, KEY)).cuda()
            assert not torch.equal(x, imgs)
        out[run] = _steps(eng, m, x, labels)
    _assert_same_run(out["A"], out["B"])
    assert not torch.equal(out["A"][0], out["C"][0]) and not torch.equal(out["A"][2], out["C"][2])


def test_engine_noise_erase_equals_the_step_on_the_erased_operand_bit_for_bit():
    """mvf_stem_erase run alone on the prepared fp32 operand, the pad stripped: a plain engine on those clips equals the erasing engine on the original
    clips bit for bit (the stem operand of both holds the same bits), with boxes of both modes."""
    from mvfnet_amd.erasing import ExplicitErasing
    lib, check = _lib()
    imgs, labels = _clips()
    b, t, _, h, w = imgs.shape
    boxes, fill = engine_table(b, t, h, w, [2, 1, 2])
    assert (boxes[..., 4] == 2).any() and (boxes[..., 4] == 1).any()
    hp, wp = h + 2 * PAD, _wp(w)
    xp = torch.full((b * t, hp, wp, 4), float("nan"), device="cuda")
    check(lib.mvf_stem_prep(P(imgs.reshape(b * t, 3, h, w).contiguous()), b * t, 3, h, w, PAD, wp, P(xp), 0, None), "stem_prep")
    _erase(xp, boxes, fill, KEY, hp, wp, F32)
    erased = xp[:, PAD:PAD + h, PAD:PAD + w, :3].permute(0, 3, 1, 2).reshape(b, t, 3, h, w).contiguous()
    assert not torch.equal(erased, imgs) and torch.equal(erased[0], imgs[0])                           # clip 0 has no box
    out = {}
    for run in "AB":
        torch.manual_seed(7)
        m, eng = _engine(F32, True)
        if run == "A":
            eng.erasing = ExplicitErasing(boxes, fill, KEY)
        out[run] = _steps(eng, m, imgs if run == "A" else erased, labels)
    _assert_same_run(out["A"], out["B"])


class _Cycle(object):
    """Hands out the tables of `inner`'s first n draws in turn (n = 1: what a replay that froze table and key would compute)."""

    def __init__(self, inner, n):
        self.inner, self.n, self.seen, self.calls, self.max_boxes = inner, n, [], 0, inner.max_boxes

    def draw(self, b, t, h, w):
        if len(self.seen) < self.n:
            self.seen.append(self.inner.draw(b, t, h, w))
        self.calls += 1
        return self.seen[(self.calls - 1) % self.n]


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_replayed_erased_steps_equal_eager_steps_bit_for_bit(dtype):
    from mvfnet_amd.erasing import RandomErasing
    gen = torch.Generator(device="cuda").manual_seed(3)
    batches = [(torch.randn(2, 4, 3, 64, 64, device="cuda", generator=gen), torch.randint(0, 400, (2, 1), device="cuda", generator=gen)) for _ in range(3)]
    lrs = [0.015, 0.01, 0.02, 0.005]
    steps = 8

    def erasing():
        return RandomErasing(probability=1.0, mode="pixel", max_count=2, cube=False, seed=5)

    def run(use_plan, er):
        torch.manual_seed(7)
        m, eng = _engine(dtype, use_plan)
        eng.erasing = er
        losses = [eng.train_step(batches[i % 3][0].clone(), batches[i % 3][1].clone(), lr=lrs[i % 4]).clone() for i in range(steps)]
        torch.cuda.synchronize()
        return eng, torch.cat(losses), eng.flat_params.clone(), [b_.clone() for b_ in m.buffers()]

    probe = erasing()
    tabs = [probe.draw(2, 4, 64, 64) for _ in range(steps)]
    assert len(set(tuple(k.tolist()) for _, _, k in tabs)) == steps and len(set(bx.tobytes() for bx, _, _ in tabs)) == steps      # tables and keys all differ
    eng_p, loss_p, par_p, buf_p = run(True, erasing())
    eng_e, loss_e, par_e, buf_e = run(False, erasing())
    st = list(eng_p._plans.values())
    assert len(st) == 1 and st[0]["plan"] is not None and st[0]["eager"] == eng_p.plan_warmup and st[0]["tries"] == 2, [(s_["eager"], s_["tries"]) for s_ in st]
    plan = st[0]["plan"]
    assert plan.names.count("mvf_stem_erase") == 1 and plan.names.index("mvf_stem_erase") == plan.names.index("mvf_stem_prep") + 1
    assert steps - eng_p.plan_warmup - 2 >= 3                                                           # at least three replayed steps
    assert not getattr(eng_e, "_plans", None)
    assert torch.isfinite(loss_p).all()
    assert torch.equal(loss_p, loss_e), (loss_p, loss_e)
    assert torch.equal(par_p, par_e)
    for a, b in zip(buf_p, buf_e):
        assert torch.equal(a, b)
    # boxes and key are read from the device table at every replay: a run on the first draw alone gives other losses on the replayed steps
    _, loss_f, _, _ = run(False, _Cycle(erasing(), 1))
    assert torch.equal(loss_f[:1], loss_p[:1]) and not torch.equal(loss_f[eng_p.plan_warmup + 2:], loss_p[eng_p.plan_warmup + 2:])


def test_off_means_off_and_a_plan_without_erasing_is_not_replayed_with_it():
    """An engine whose erasing is None records what an engine without the feature records: the accepted plan of the same step with erasing on holds the same
    calls plus ONE mvf_stem_erase right behind mvf_stem_prep, under a key of its own; with erasing off again the first plan is replayed."""
    from mvfnet_amd.erasing import RandomErasing
    imgs, labels = _clips(5, b=2)
    m, eng = _engine(BF16, True, dropout=0.0)
    assert eng.erasing is None
    for _ in range(5):
        eng.train_step(imgs, labels)
    assert len(eng._plans) == 1 and eng._erase_table is None
    (key_plain, st_plain), = eng._plans.items()
    names_plain = list(st_plain["plan"].names)
    assert st_plain["plan"] is not None and "mvf_stem_erase" not in names_plain
    assert not any(k[0] == "erase_table" for k in eng._bufs) and "_table_stages" not in eng.__dict__      # nothing allocated for the feature
    assert not any(isinstance(k, tuple) and k and k[0] == "erasing" for k in key_plain)                   # the key of an existing configuration is unchanged
    eng.erasing = RandomErasing(probability=1.0, seed=1)
    for _ in range(5):
        eng.train_step(imgs, labels)
    assert len(eng._plans) == 2 and all(s["plan"] is not None for s in eng._plans.values())
    names_on = [s["plan"].names for k, s in eng._plans.items() if k != key_plain][0]
    i = names_on.index("mvf_stem_erase")
    assert names_on[i - 1] == "mvf_stem_prep" and names_on[:i] + names_on[i + 1:] == names_plain
    eng.erasing = None
    plan_before = st_plain["plan"]
    eng.train_step(imgs, labels)
    torch.cuda.synchronize()
    assert len(eng._plans) == 2 and eng._plans[key_plain]["plan"] is plan_before and torch.isfinite(eng.flat_params).all()


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_uint8_frames_are_erased_behind_the_frame_kernel(dtype):
    """A FramePipeline step with erasing against the fp32-input step on the host-normalised frames (oracle/frames_numpy.py, bit-equal to the frame kernel)
    with the same table: the stem operands are equal bit for bit -- the bound of test_blend_gpu.py's uint8 case --, and so are the losses, each path
    on an engine of its own (a second forward on ONE engine starts from moved running means, the shift of the batch statistics' sums)."""
    from oracle import frames_numpy as F
    from mvfnet_amd.erasing import ExplicitErasing
    from mvfnet_amd.preprocess import FramePipeline
    B, T, hs, ws, c = 3, 4, 72, 80, 64
    mean, std = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]
    fr = np.random.RandomState(2).randint(0, 256, (B, T, hs, ws, 3)).astype(np.uint8)
    win = np.stack([np.full(B * T, 3), np.full(B * T, 7), np.repeat([0, 1, 0], T)], 1).astype(np.int32)
    x = torch.from_numpy(F.frames_to_nchw(fr.reshape(B * T, hs, ws, 3), win, c, c, mean, std, to_rgb=True)).cuda().view(B, T, 3, c, c)
    labels = torch.tensor([[3], [111], [7]], device="cuda")
    boxes, fill = engine_table(B, T, c, c, [2, 1])
    out = {}
    for run in ("f32", "u8", "plain"):                           # an engine each: all three forwards start from the same BatchNorm state
        m, eng = _engine(dtype, False, dropout=0.0)
        eng.erasing = ExplicitErasing(boxes, fill, KEY) if run != "plain" else None
        if run == "f32":
            loss = eng.forward(x, labels).clone()
        else:
            eng.input_pipeline, eng.input_window = FramePipeline(mean, std, to_rgb=True, crop_size=c), torch.from_numpy(win).cuda()
            loss = eng.forward(torch.from_numpy(fr).cuda(), labels).clone()
        out[run] = (loss, eng.saved["xp"].clone())
    torch.cuda.synchronize()
    (l_f32, xp_f32), (l_u8, xp_u8), (l_plain, xp_plain) = out["f32"], out["u8"], out["plain"]
    assert np.array_equal(_bits(xp_u8).cpu().numpy(), _bits(xp_f32).cpu().numpy())
    assert torch.isfinite(l_u8).all() and torch.equal(l_u8, l_f32), (l_u8, l_f32)
    assert not torch.equal(xp_u8, xp_plain) and float(l_u8) != float(l_plain)
    nt = B * T
    _, kind = EN.erase_ref(np.zeros((nt, c + 2 * PAD, _wp(c), 4)), boxes, fill, KEY, PAD)
    un = torch.from_numpy(kind == EN.UNTOUCHED)
    assert torch.equal(_bits(xp_u8).cpu()[un], _bits(xp_plain).cpu()[un])                              # outside the boxes: the frame kernel's own bits


@pytest.mark.parametrize("dtype", [BF16, F32], ids=["bf16", "f32"])
def test_erasing_comes_before_the_blend(dtype):
    """Both on: saved['xp'] -- what the stem reads and its weight gradient sees -- is mvf_stem_prep, then mvf_stem_erase, then mvf_stem_blend, bit for bit;
    the other order gives another operand (the boxes of a clip would be blended into its partner's pixels unerased)."""
    from mvfnet_amd.blending import ExplicitBlending
    from mvfnet_amd.erasing import ExplicitErasing
    lib, check = _lib()
    imgs, labels = _clips()
    b, t, _, h, w = imgs.shape
    boxes, fill = engine_table(b, t, h, w, [2, 1])
    rows = np.array([(1, 0, 0, 0, 0), (2, 5, 7, 40, 33), (0, 0, 0, h // 2, w // 2 + 1)], dtype=np.int32)
    wts = np.array([[0.3, 0.3], [1.0, 0.7], [0.6, 0.6]], dtype=np.float32)
    m, eng = _engine(dtype, False, dropout=0.0)
    eng.erasing, eng.blending = ExplicitErasing(boxes, fill, KEY), ExplicitBlending(rows, wts)
    loss = eng.forward(imgs, labels).clone()
    got = eng.saved["xp"].clone()
    hp, wp, dt = h + 2 * PAD, _wp(w), 0 if dtype == F32 else 1
    xp = torch.full((b * t, hp, wp, 4), float("nan"), device="cuda").to(dtype)
    check(lib.mvf_stem_prep(P(imgs.reshape(b * t, 3, h, w).contiguous()), b * t, 3, h, w, PAD, wp, P(xp), dt, None), "stem_prep")
    rg, wg = torch.from_numpy(rows).cuda(), torch.from_numpy(wts).cuda()
    wrong = torch.empty_like(xp)
    check(lib.mvf_stem_blend(P(xp), b, t, hp, wp, PAD, P(rg), P(wg), P(wrong), dt, None), "stem_blend")
    _erase(wrong, boxes, fill, KEY, hp, wp, dtype)
    _erase(xp, boxes, fill, KEY, hp, wp, dtype)
    want = torch.empty_like(xp)
    check(lib.mvf_stem_blend(P(xp), b, t, hp, wp, PAD, P(rg), P(wg), P(want), dt, None), "stem_blend")
    torch.cuda.synchronize()
    assert torch.isfinite(loss).all() and got.shape == want.shape
    assert torch.equal(_bits(got), _bits(want)) and not torch.equal(_bits(got), _bits(wrong))


def _model(train_cfg):
    import mvfnet_amd
    from mvfnet_amd import synth
    m = mvfnet_amd.build_recognizer(mvfnet_amd.mvfnet_config(50, 4, dropout_ratio=0.5), train_cfg, dict(average_clips=None))
    sd = m.state_dict()
    vals = synth.synth_state_dict({"r50/" + k: tuple(v.shape) for k, v in sd.items()})
    m.load_state_dict({k: torch.from_numpy(vals["r50/" + k]) for k in sd})
    return m.cuda()


def test_eval_is_untouched_by_a_configured_erasing():
    """forward_test and an eval-mode training forward are bit-identical with erasing configured or not; in training mode the same model erases."""
    cfg = dict(erasing=dict(type="RandomErasing", probability=1.0, mode="pixel", seed=1))
    x, labels = _clips(1, b=2)
    out = {}
    for name, train_cfg in (("with", cfg), ("without", None)):
        m = _model(train_cfg).eval()
        scores = m(x, None, return_loss=False)
        eng = m.train_engine(dtype=F32)                          # created in eval mode: erasing does not reach it
        assert eng.erasing is None
        torch.manual_seed(0)                                     # (the dropout mask)
        out[name] = (scores, float(m(x, labels)["loss_cls"].detach()), m, eng)
        assert eng.erasing is None and eng._erase_table is None
    assert np.isfinite(out["with"][0]).all() and np.array_equal(out["with"][0], out["without"][0])
    assert out["with"][1] == out["without"][1]
    m, eng = out["with"][2:]
    m.train()
    assert eng.erasing is m.erasing and m.erasing is not None
    torch.manual_seed(0)
    l_on = float(m(x, labels)["loss_cls"].detach())
    assert eng._erase_table is not None and np.isfinite(l_on)
    m.eval()
    assert eng.erasing is None


class _Counting(object):
    def __init__(self, inner):
        self.inner, self.calls, self.max_boxes = inner, 0, inner.max_boxes

    def draw(self, b, t, h, w):
        self.calls += 1
        return self.inner.draw(b, t, h, w)


def test_precise_bn_draws_nothing_and_accumulation_and_the_guard_draw_per_micro_step():
    from mvfnet_amd.erasing import ExplicitErasing
    imgs, labels = _clips(9, b=2)
    boxes, fill = engine_table(2, 4, 64, 64, [2])
    m, eng = _engine(BF16, True, dropout=0.0)
    er = _Counting(ExplicitErasing(boxes, fill, KEY))
    eng.erasing = er
    assert eng.precise_bn([(imgs, labels)] * 2, num_iters=2) == 2
    assert er.calls == 0 and eng.erasing is er                     # switched off for the calibration forwards, and put back
    for _ in range(3):
        eng.accumulate_step(imgs, labels)
    assert er.calls == 3                                           # one table per micro-step
    eng.apply_accumulated(lr=0.01)
    eng.enable_step_guard()
    bad = imgs.clone()
    bad[0, 0, 0, 0, 0] = float("nan")
    eng.train_step(bad, labels, lr=0.01)
    assert er.calls == 4 and eng.guard_state()["skipped_last"]     # a step the guard skips has drawn its table
    eng.train_step(imgs, labels, lr=0.01)
    st = eng.guard_state()
    assert er.calls == 5 and not st["skipped_last"] and st["skipped"] == 1
    # erased steps carry hard labels: the training accuracy counts them
    eng.enable_train_accuracy()
    eng.train_step(imgs, labels, lr=0.01)
    assert eng.train_accuracy()["count"] == 2
    torch.cuda.synchronize()
    assert torch.isfinite(eng.flat_params).all()
