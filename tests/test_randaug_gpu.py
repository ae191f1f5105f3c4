"""GPU: RandAugment on the uint8 frames -- mvf_frames_randaug_u8 (csrc/randaug.hip) against the numpy restatement in randaug_numpy.py, which equals Pillow
bit for bit (test_randaug_cpu.py), and the train engine with it.  Everything is integer output: the device bytes are EQUAL to the restatement's, no tolerance."""
import numpy as np
import pytest
import torch

import randaug_numpy as RN
from helpers import library_names
from test_launch_plan_gpu import _engine

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
FILL = (124, 116, 104)
MEAN, STD = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]


def _ra():
    from mvfnet_amd import randaug
    return randaug


def _frames(n, hs, ws, seed=0):
    """Textured frames: a ramp plus noise (a spread histogram, neighbours that differ), the third channel darker in the upper half."""
    rng = np.random.RandomState(seed + 1000 * hs + ws)
    y, x = np.mgrid[0:hs, 0:ws]
    base = np.stack([(x * 255) // max(ws - 1, 1), (y * 255) // max(hs - 1, 1), ((x + y) * 255) // max(hs + ws - 2, 1)], -1)
    fr = np.clip(base[None] + rng.randint(-60, 61, size=(n, hs, ws, 3)), 0, 255).astype(np.uint8)
    fr[:, : hs // 2, :, 2] //= 3
    return fr


def _run(fr, table, t, sizes=None, order=0):
    """The device result, with the checks every call shares: the input is not written, a second run gives the same bytes."""
    RA = _ra()
    dev = torch.from_numpy(np.ascontiguousarray(fr)).cuda()
    keep = dev.clone()
    out = RA.apply(dev, table, t, sizes=sizes, order=order)
    again = RA.apply(dev, table, t, sizes=sizes, order=order, out=torch.full_like(dev, 0x5A))
    torch.cuda.synchronize()
    assert out.shape == dev.shape and out.dtype == torch.uint8 and out.data_ptr() != dev.data_ptr()
    assert torch.equal(dev, keep), "frames_hwc was written"
    assert torch.equal(out, again), "two runs differ"
    return out.cpu().numpy()


def _mismatch(got, want, table, t):
    bad = np.nonzero((got != want).reshape(got.shape[0], -1).any(1))[0]
    return [(int(i), table[i // t, :, 0].tolist(), int((got[i] != want[i]).sum())) for i in bad[:8]]


def op_rows(h, w, order):
    """Every kind, with arguments on both sides of its branches; (h, w) is the frame's own size."""
    RA = _ra()
    ops = [("Identity", 0), ("Invert", 0), ("Posterize", 0), ("Posterize", 3), ("Posterize", 7), ("Solarize", 0), ("Solarize", 100), ("Solarize", 256),
           ("SolarizeAdd", 0), ("SolarizeAdd", 60), ("SolarizeAdd", 110), ("AutoContrast", 0), ("Equalize", 0)]
    ops += [(n, f) for n in ("Brightness", "Contrast", "Color", "Sharpness") for f in (0.1, 0.55, 1.0, 1.45, 1.9)]
    ops += [("Rotate", 21.0), ("Rotate", -30.0), ("Rotate", 7.5), ("Rotate", 0.0), ("ShearX", 0.21), ("ShearY", -0.3), ("TranslateXRel", 0.315),
            ("TranslateYRel", -0.45), ("TranslateX", 0.5), ("TranslateY", -0.25)]
    return np.stack([RA.op_row(n, a, h, w, FILL, order) for n, a in ops])


# ------------------------------------------------------------------------------------------------ 1. the kernel
@pytest.mark.parametrize("order", [0, 1], ids=["bgr", "rgb"])
@pytest.mark.parametrize("hw", [(1, 1), (1, 2), (2, 5), (3, 3), (7, 5), (37, 53)], ids=lambda s: "%dx%d" % s)
def test_each_kind_alone(hw, order):
    """One frame per op, one layer, one launch: 7 x 5 has rows of 15 bytes and frames on odd bases, 3 x 3 a single interior pixel, 37 x 53 needs
    equalize's 255 clamp."""
    h, w = hw
    rows = op_rows(h, w, order)
    n = rows.shape[0]
    assert set(rows[:, 0].tolist()) == set(range(12))
    fr = _frames(n, h, w)
    table = rows[:, None, :]
    got = _run(fr, table, 1, order=order)
    want = RN.apply_layers(fr, table, 1, order=order)
    assert np.array_equal(got, want), _mismatch(got, want, table, 1)
    if hw == (37, 53):
        changed = (got != fr).reshape(n, -1).any(1)
        # the ops do something (autocontrast is the identity on a frame that spans 0 .. 255 already: the layer tests below cover it)
        assert all(changed[rows[:, 0] == k].any() for k in range(1, 12) if k != 5)


def test_autocontrast_for_every_lo_hi_pair():
    """10880 frames of 1 x 2 pixels, one (lo, hi) pair with lo < hi per channel: all 32640 pairs in one launch -- every fp64 table the kernel can build."""
    RA = _ra()
    lo, hi = np.triu_indices(256, 1)
    assert lo.size == 32640
    fr = np.stack([lo, hi], 1).reshape(10880, 3, 2).transpose(0, 2, 1).reshape(10880, 1, 2, 3).astype(np.uint8)
    table = np.broadcast_to(RA.op_row("AutoContrast", 0, 1, 2), (10880, 1, 16)).copy()
    got = _run(fr, table, 1)
    want = np.stack([RN.autocontrast_lut(fr[i, 0, :, c])[fr[i, 0, :, c]] for i in range(10880) for c in range(3)]).reshape(10880, 3, 2).transpose(0, 2, 1)
    assert np.array_equal(got.reshape(10880, 2, 3), want)
    assert (got.reshape(10880, 2, 3)[:, 0] == 0).all()                # lo * scale + (-lo * scale) is exactly 0; hi's value is whatever fp64 truncates to


def _mixed_table(h, w, order=0):
    """Two clips, four layers: statistics, blend and affine ops, different per clip and layer."""
    RA = _ra()
    clip0 = [("Equalize", 0), ("ColorIncreasing", 1.6), ("Rotate", 17.0), ("Contrast", 0.4)]
    clip1 = [("Sharpness", 1.8), ("AutoContrast", 0), ("ShearX", -0.25), ("SolarizeAdd", 70)]
    return np.stack([np.stack([RA.op_row(n, a, h, w, FILL, order) for n, a in c]) for c in (clip0, clip1)])


@pytest.mark.parametrize("layers", [1, 2, 3, 4])
def test_two_clips_four_layers_and_the_ping_pong_parity(layers):
    RA = _ra()
    t, h, w = 3, 22, 27
    table = np.ascontiguousarray(_mixed_table(h, w)[:, :layers])
    assert RA.stats_mask(table) == [0b1, 0b11, 0b11, 0b1011][layers - 1]
    fr = _frames(2 * t, h, w, seed=3)
    got = _run(fr, table, t)
    want = RN.apply_layers(fr, table, t)
    assert np.array_equal(got, want), _mismatch(got, want, table, t)
    assert not np.array_equal(got[:t], fr[:t]) and not np.array_equal(got[t:], fr[t:])


def test_a_padded_batch_keeps_its_padding():
    """40 x 56 holding clips of 37 x 53 and of 24 x 56 frames: every op works on the frame's own image, the other bytes are copied."""
    t, hs, ws = 2, 40, 56
    sizes = np.array([[37, 53]] * t + [[24, 56]] * t, dtype=np.int32)
    RA = _ra()
    clip0 = [("Rotate", -23.0), ("Equalize", 0), ("SharpnessIncreasing", 1.7), ("TranslateXRel", 0.3)]
    clip1 = [("ContrastIncreasing", 1.5), ("TranslateYRel", -0.4), ("AutoContrast", 0), ("Color", 0.2)]
    table = np.stack([np.stack([RA.op_row(n, a, hw[0], hw[1], FILL) for n, a in c]) for c, hw in ((clip0, (37, 53)), (clip1, (24, 56)))])
    fr = _frames(2 * t, hs, ws, seed=5)
    got = _run(fr, table, t, sizes=sizes)
    want = RN.apply_layers(fr, table, t, sizes=sizes)
    assert np.array_equal(got, want), _mismatch(got, want, table, t)
    assert np.array_equal(got[:t, 37:], fr[:t, 37:]) and np.array_equal(got[:t, :, 53:], fr[:t, :, 53:]) and np.array_equal(got[t:, 24:], fr[t:, 24:])
    full = _run(fr, table, t)                                       # without sizes the same table works on the whole extent: other bytes
    assert not np.array_equal(full, got)


def test_an_identity_table_returns_the_input():
    fr = _frames(4, 9, 11, seed=7)
    got = _run(fr, np.zeros((2, 3, 16), dtype=np.int32), 2)
    assert np.array_equal(got, fr)


def test_a_frame_that_spans_several_workgroups():
    """70 x 131: 27510 bytes, seven workgroups of the apply pass and one statistics workgroup that loops; every kind."""
    h, w = 70, 131
    rows = op_rows(h, w, 0)
    n = rows.shape[0]
    fr = _frames(n, h, w, seed=9)
    table = rows[:, None, :]
    got = _run(fr, table, 1)
    want = RN.apply_layers(fr, table, 1)
    assert np.array_equal(got, want), _mismatch(got, want, table, 1)


def test_apply_refuses_what_the_kernel_does_not_take():
    RA = _ra()
    fr = torch.zeros(4, 6, 8, 3, dtype=torch.uint8, device="cuda")
    table = np.zeros((2, 1, 16), dtype=np.int32)
    for bad in (lambda: RA.apply(fr.float(), table, 2), lambda: RA.apply(fr, table, 3), lambda: RA.apply(fr, table[:1], 2),
                lambda: RA.apply(fr, table, 2, sizes=np.array([[7, 8]] * 4)), lambda: RA.apply(fr, table, 2, sizes=np.array([[6, 8]] * 3)),
                lambda: RA.apply(fr, table, 2, out=torch.zeros(5, dtype=torch.uint8, device="cuda")), lambda: RA.apply(fr[..., :2], table, 2)):
        with pytest.raises(ValueError):
            bad()


# ------------------------------------------------------------------------------------------------ 2. the engine
B, T, HS, WS, CROP = 2, 4, 72, 80, 64


class _Names(object):
    """Stands in for a library object (the engine's handle, a module's `lib`): every call is made and its name noted."""

    def __init__(self, real, names):
        self._real, self._names = real, names

    def __getattr__(self, name):
        fn = getattr(self._real, name)

        def w(*args):
            self._names.append(name)
            return fn(*args)
        return w


def _recorded(monkeypatch, eng, fn):
    from mvfnet_amd import preprocess
    names = []
    with monkeypatch.context() as mp, library_names(eng, lib=_Names(eng.lib, names)):
        mp.setattr(preprocess, "lib", _Names(preprocess.lib, names))
        fn()
    torch.cuda.synchronize()
    return names


def _pipeline(kind):
    """-> (pipeline, window table, per-frame sizes or None)."""
    from mvfnet_amd import preprocess as P
    n = B * T
    if kind == "frame":
        win = np.stack([np.full(n, 3), np.full(n, 7), np.tile([0, 1], n // 2)], 1).astype(np.int32)
        return P.FramePipeline(MEAN, STD, to_rgb=True, crop_size=CROP), torch.from_numpy(win).cuda(), None
    fh, fw = 66, 70                                                 # the frames' own size inside the 72 x 80 extent
    row = [fh, fw, 0, 0, fh, fw, fh, fw, (fh - CROP) // 2, (fw - CROP) // 2, 0]
    rows = np.array([row] * n, dtype=np.int32)
    rows[1::2, 10] = 1
    if kind == "jitter":
        eye = np.concatenate([np.eye(3, dtype=np.float32).reshape(-1), np.zeros(3, dtype=np.float32)]).view(np.int32)
        rows = np.concatenate([rows, np.broadcast_to(eye, (n, 12))], 1)
        return P.JitterFramePipeline(MEAN, STD, to_rgb=True, crop_size=CROP), torch.from_numpy(rows).cuda(), rows[:, :2].copy()
    return P.ResamplingFramePipeline(MEAN, STD, to_rgb=True, crop_size=CROP), torch.from_numpy(rows).cuda(), rows[:, :2].copy()


@pytest.mark.parametrize("kind", ["frame", "resampling", "jitter"])
def test_engine_step_equals_the_step_on_frames_augmented_beforehand(kind, monkeypatch):
    """Run A: a train step on uint8 frames with ExplicitAugment.  Run B: a plain engine on the frames randaug.apply made beforehand (BGR stored order: the
    pipeline's to_rgb).  Loss, gradients, parameters and buffers are equal bit for bit; run C, the untouched frames, differs.  The engine's launch is one
    mvf_frames_randaug_u8 in front of the frame kernel, and nothing else changes."""
    RA = _ra()
    fr = torch.from_numpy(_frames(B * T, HS, WS, seed=11).reshape(B, T, HS, WS, 3)).cuda()
    labels = torch.tensor([[3], [111]], device="cuda")
    out, names = {}, {}
    for run in "ABC":
        torch.manual_seed(7)
        m, eng = _engine(F32, False, dropout=0.0)
        pipe, window, sizes = _pipeline(kind)
        hw = (HS, WS) if sizes is None else tuple(int(v) for v in sizes[0])
        table = _mixed_table(hw[0], hw[1], order=0)
        eng.input_pipeline, eng.input_window = pipe, window
        x = fr
        if run == "A":
            eng.randaug = RA.ExplicitAugment(table)
        elif run == "B":
            x = RA.apply(fr, table, T, sizes=sizes, order=0)
            assert not torch.equal(x, fr)
        keep = x.clone()
        loss = eng.train_step(x, labels, lr=0.01).clone()
        out[run] = (loss, eng.flat_grads.clone(), eng.flat_params.clone(), [b_.clone() for b_ in m.buffers()])
        names[run] = _recorded(monkeypatch, eng, lambda: eng.train_step(x, labels, lr=0.01))      # a second step: the first one of a process sizes workspaces
        assert torch.equal(x, keep)
        has = any(k[0] in ("randaug_out", "randaug_tmp", "randaug_ws", "randaug_table") for k in eng._bufs)
        assert has == (run == "A")                                  # off: nothing is allocated for the feature
    (la, ga, pa, ba), (lb, gb, pb, bb), (lc, _, pc, _) = out["A"], out["B"], out["C"]
    assert torch.isfinite(la).all() and torch.equal(la, lb), (la, lb)
    assert torch.equal(ga, gb) and torch.equal(pa, pb) and all(torch.equal(x, y) for x, y in zip(ba, bb))
    assert not torch.equal(la, lc) and not torch.equal(pa, pc)
    # off means off: the plain engine's launches hold no trace of the feature, and "on" is the same list plus one call right in front of the frame kernel
    assert "mvf_frames_randaug_u8" not in names["C"] and names["B"] == names["C"]
    i = names["A"].index("mvf_frames_randaug_u8")
    assert names["A"][i + 1].startswith("mvf_frames_") and names["A"][:i] + names["A"][i + 1:] == names["C"]


def test_rgb_stored_frames_use_the_rgb_grey_weights():
    """to_rgb=False: the stored order is RGB, and the engine tells the kernel so (the colour op's grey depends on it)."""
    from mvfnet_amd import preprocess as P
    RA = _ra()
    fr = torch.from_numpy(_frames(B * T, HS, WS, seed=13).reshape(B, T, HS, WS, 3)).cuda()
    labels = torch.tensor([[3], [111]], device="cuda")
    table = np.stack([np.stack([RA.op_row("Color", 0.3, HS, WS, FILL, 1), RA.op_row("Rotate", 12.0, HS, WS, FILL, 1)])] * B)
    losses = {}
    for run in ("on", "rgb", "bgr"):
        m, eng = _engine(F32, False, dropout=0.0)
        eng.input_pipeline, eng.input_window = P.FramePipeline(MEAN, STD, to_rgb=False, crop_size=CROP), None
        x = fr
        if run == "on":
            eng.randaug = RA.ExplicitAugment(table)
        else:
            x = RA.apply(fr, table, T, order=1 if run == "rgb" else 0)
        losses[run] = eng.forward(x, labels).clone()
    assert torch.equal(losses["on"], losses["rgb"]) and not torch.equal(losses["on"], losses["bgr"])


def test_eval_does_not_augment_and_precise_bn_and_accumulation(monkeypatch):
    import mvfnet_amd
    from mvfnet_amd import preprocess as P
    RA = _ra()

    class Counting(RA.RandAugment):
        calls = 0

        def draw(self, *a, **k):
            Counting.calls += 1
            return super().draw(*a, **k)
    m = mvfnet_amd.build_recognizer(mvfnet_amd.mvfnet_config(50, T, dropout_ratio=0.0), dict(randaug=Counting("rand-m7-n2-mstd0.5-inc1", prob=1.0)),
                                    dict(average_clips=None))
    eng = m.cuda().train().train_engine()
    eng.use_plan = False
    assert eng.randaug is m.randaug and isinstance(eng.randaug, Counting)
    eng.input_pipeline, eng.input_window = P.FramePipeline(MEAN, STD, to_rgb=True, crop_size=CROP), None
    fr = torch.from_numpy(_frames(B * T, HS, WS, seed=17).reshape(B, T, HS, WS, 3)).cuda()
    labels = torch.tensor([[3], [111]], device="cuda")
    names = _recorded(monkeypatch, eng, lambda: eng.train_step(fr, labels, lr=0.01))
    assert names.count("mvf_frames_randaug_u8") == 1 and Counting.calls == 1
    # accumulation draws per micro-step
    eng.accumulate_step(fr, labels)
    eng.accumulate_step(fr, labels)
    eng.apply_accumulated(lr=0.01)
    assert Counting.calls == 3
    # precise_bn switches it off for its forwards and puts it back
    names = _recorded(monkeypatch, eng, lambda: eng.precise_bn([(fr, labels)] * 2, num_iters=2))
    assert "mvf_frames_randaug_u8" not in names and Counting.calls == 3 and eng.randaug is m.randaug
    # eval: the configured object does not reach the engine
    m.eval()
    assert eng.randaug is None
    names = _recorded(monkeypatch, eng, lambda: eng.forward(fr, labels))
    assert "mvf_frames_randaug_u8" not in names and Counting.calls == 3 and eng._randaug_table is None
    m.train()
    assert eng.randaug is m.randaug
    torch.cuda.synchronize()
    assert torch.isfinite(eng.flat_params).all()


def test_the_three_refusals(monkeypatch):
    """Float images, decoder-native YUV planes and addressed input are refused with a ValueError before any launch."""
    from mvfnet_amd import preprocess as P
    RA = _ra()
    m, eng = _engine(F32, False, dropout=0.0)
    eng.randaug = RA.RandAugment("rand-m7-n2-mstd0.5-inc1")
    labels = torch.tensor([[3], [111]], device="cuda")
    fr = torch.zeros(B, T, HS, WS, 3, dtype=torch.uint8, device="cuda")
    cases = [(None, torch.zeros(B, T, 3, CROP, CROP, device="cuda"), "float"),
             (P.Yuv420FramePipeline(MEAN, STD, to_rgb=True, crop_size=CROP), torch.zeros(B, T, HS * 3 // 2, WS, dtype=torch.uint8, device="cuda"), "Yuv420"),
             (P.AddressedFramePipeline(MEAN, STD, to_rgb=True, crop_size=CROP), torch.zeros(B, T, HS * WS * 3, dtype=torch.uint8, device="cuda"), "Addressed")]
    for pipe, x, what in cases:
        eng.input_pipeline = pipe
        for call in (lambda: eng.forward(x, labels), lambda: eng.train_step(x, labels), lambda: eng.accumulate_step(x, labels)):
            def refused():
                with pytest.raises(ValueError, match=what):
                    call()
            assert _recorded(monkeypatch, eng, refused) == [], what
    # a gather table names its sources: not one row per frame of the batch
    eng.input_pipeline = P.GatherFramePipeline(MEAN, STD, to_rgb=True, crop_size=CROP)
    rows = eng.input_pipeline.center_window(B * T, HS, WS)
    eng.input_window = torch.cat([rows, torch.zeros(B * T, 1, dtype=torch.int32, device="cuda")], 1)
    with pytest.raises(ValueError, match="11- / 23-column"):
        eng.forward(fr, labels)
    eng.randaug = None                                               # by hand, as for erasing: the same engine runs plain steps again
    eng.input_pipeline, eng.input_window = P.FramePipeline(MEAN, STD, to_rgb=True, crop_size=CROP), None
    assert torch.isfinite(eng.train_step(fr, labels, lr=0.01)).all()
