"""mvf_frames_resample_u8 (uint8 frames -> resize / RandomResizedCrop -> crop / flip / normalise / stem layout) bit for bit against the
numpy restatement (tests/resample_numpy.py), against mvf_frames_prep_u8 for identity rows, and the engines fed uint8 frames + row tables
of the three shipped recipes against the same engines fed the fp32 tensor to_nchw makes from the same rows."""
import random

import numpy as np
import pytest
import torch

import resample_numpy as R

pytestmark = pytest.mark.gpu

MEAN, STD = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]


def _frames(n, hs, ws, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(n, hs, ws, 3)).astype(np.uint8)


def _rows(rng, n, Hs, Ws, h, w, mode):
    """Random valid rows for a padded (n, Hs, Ws, 3) batch and an h x w crop."""
    out = []
    for i in range(n):
        fh, fw = rng.randint(1, Hs + 1), rng.randint(1, Ws + 1)
        if mode == "one_pixel":
            bh = bw = 1
        else:
            bh, bw = rng.randint(1, fh + 1), rng.randint(1, fw + 1)
        by, bx = rng.randint(0, fh - bh + 1), rng.randint(0, fw - bw + 1)
        if mode == "borders":                                  # patches touching the frame's borders, corners included
            by, bx = [(0, 0), (fh - bh, fw - bw), (0, fw - bw), (fh - bh, 0)][i % 4]
        if mode == "area2":
            rh, rw = rng.randint(h, max(fh // 2, h) + 1), rng.randint(w, max(fw // 2, w) + 1)
            bh, bw = 2 * rh, 2 * rw
            fh, fw = max(fh, bh), max(fw, bw)
            by, bx = rng.randint(0, fh - bh + 1), rng.randint(0, fw - bw + 1)
        else:
            rh, rw = rng.randint(h, 3 * max(bh, h) + 1), rng.randint(w, 3 * max(bw, w) + 1)
        out.append((fh, fw, by, bx, bh, bw, rh, rw, rng.randint(0, rh - h + 1), rng.randint(0, rw - w + 1), rng.randint(0, 2)))
    return np.array(out, dtype=np.int32)


CASES = {
    # n, Hs, Ws, h, w, mode, to_rgb, div_255
    "up_down_odd": (8, 41, 57, 19, 23, "any", True, False),
    "borders": (8, 30, 26, 11, 9, "borders", True, False),
    "one_pixel_patch": (6, 9, 7, 5, 4, "one_pixel", True, False),
    "one_pixel_crop": (6, 13, 17, 1, 1, "any", True, False),
    "area_2x": (6, 48, 52, 12, 14, "area2", True, False),
    "bgr_div255": (6, 33, 35, 16, 12, "any", False, True),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_resample_nchw_bit_exact_vs_numpy(case):
    from mvfnet_amd.preprocess import ResamplingFramePipeline
    n, Hs, Ws, h, w, mode, to_rgb, div = CASES[case]
    rng = np.random.RandomState(sorted(CASES).index(case) + 1)
    rows = _rows(rng, n, max(Hs, 2 * h), max(Ws, 2 * w), h, w, mode)
    Hs, Ws = int(rows[:, 0].max()), int(rows[:, 1].max())
    fr = _frames(n, Hs, Ws, 7)
    mean, std = (MEAN, STD) if not div else ([0.485, 0.456, 0.406], [0.229, 0.224, 0.225])
    pipe = ResamplingFramePipeline(mean, std, to_rgb=to_rgb, div_255=div, crop_size=(w, h))
    got = pipe.to_nchw(torch.from_numpy(fr).cuda(), torch.from_numpy(rows).cuda()).cpu().numpy()
    want = R.frames_to_nchw(fr, rows, h, w, mean, std, to_rgb=to_rgb, div_255=div)
    assert np.array_equal(got, want)
    if mode == "area2":
        assert all(r[4] == 2 * r[6] and r[5] == 2 * r[7] for r in rows)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_resample_stem_layout_equals_stem_prep_of_the_nchw_output(dtype):
    from mvfnet_amd._lib import check, lib
    from mvfnet_amd.preprocess import ResamplingFramePipeline
    n, Hs, Ws, h, w, pad = 5, 50, 61, 40, 44, 3
    rows = _rows(np.random.RandomState(3), n, Hs, Ws, h, w, "any")
    fr = _frames(n, Hs, Ws, 3)
    pipe = ResamplingFramePipeline(MEAN, STD, to_rgb=True, crop_size=(w, h))
    wp = (w + 2 * pad + 2 + 1) // 2 * 2
    fr_t, rows_t = torch.from_numpy(fr).cuda(), torch.from_numpy(rows).cuda()
    got = pipe.to_stem(fr_t, rows_t, pad, wp, dtype)
    x = pipe.to_nchw(fr_t, rows_t)
    assert np.array_equal(x.cpu().numpy(), R.frames_to_nchw(fr, rows, h, w, MEAN, STD))
    ref = torch.full((n, h + 2 * pad, wp, 4), 7.0, dtype=dtype, device="cuda")
    check(lib.mvf_stem_prep(x.data_ptr(), n, 3, h, w, pad, wp, ref.data_ptr(), 0 if dtype == torch.float32 else 1,
                            torch.cuda.current_stream().cuda_stream), "stem_prep")
    iv = torch.int16 if dtype == torch.bfloat16 else torch.int32
    assert torch.equal(got.view(iv), ref.view(iv))


def test_padded_batch_of_three_frame_sizes_is_correct_per_frame():
    from mvfnet_amd.preprocess import ResamplingFramePipeline, collate_frames, train_rows, val_rows
    T, c = 3, 24
    shapes = [(30, 40), (45, 26), (17, 19)]
    clips = [_frames(T, hh, ww, 10 + k) for k, (hh, ww) in enumerate(shapes)]
    random.seed(4)
    np.random.seed(4)
    tabs = [train_rows(30, 40, T, input_size=c), val_rows(45, 26, T, scale=(float("inf"), 28), crop_size=c),
            train_rows(17, 19, T, input_size=c, flip_ratio=1.0)]
    fr, rows = collate_frames(list(zip(clips, tabs)), pad_to=(48, 48))
    pipe = ResamplingFramePipeline(MEAN, STD, to_rgb=True, crop_size=c)
    got = pipe.to_nchw(fr.cuda(), rows.cuda()).cpu().numpy().reshape(3, T, 3, c, c)
    for k in range(3):                                           # the numpy restatement sees the UNPADDED frames
        assert np.array_equal(got[k], R.frames_to_nchw(clips[k], tabs[k], c, c, MEAN, STD)), shapes[k]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_identity_rows_equal_frames_prep_u8(dtype):
    from mvfnet_amd.preprocess import FramePipeline, ResamplingFramePipeline
    n, hs, ws, h, w, pad = 6, 37, 53, 21, 32, 3
    fr = torch.from_numpy(_frames(n, hs, ws, 11)).cuda()
    rng = np.random.RandomState(5)
    win = np.stack([rng.randint(0, hs - h + 1, n), rng.randint(0, ws - w + 1, n), rng.randint(0, 2, n)], 1).astype(np.int32)
    rows = []
    for i, (y0, x0, f) in enumerate(win):                        # split the window between the patch origin and the crop offset
        oy, ox = (0, 0) if i % 2 else (y0 // 2, x0 // 3)
        by, bx = y0 - oy, x0 - ox
        bh, bw = hs - by, ws - bx
        rows.append((hs, ws, by, bx, bh, bw, bh, bw, oy, ox, f))
    rows = torch.tensor(rows, dtype=torch.int32, device="cuda")
    win = torch.from_numpy(win).cuda()
    a, b = FramePipeline(MEAN, STD, crop_size=(w, h)), ResamplingFramePipeline(MEAN, STD, crop_size=(w, h))
    assert torch.equal(a.to_nchw(fr, win), b.to_nchw(fr, rows))
    wp = (w + 2 * pad + 2 + 1) // 2 * 2
    iv = torch.int16 if dtype == torch.bfloat16 else torch.int32
    assert torch.equal(a.to_stem(fr, win, pad, wp, dtype).view(iv), b.to_stem(fr, rows, pad, wp, dtype).view(iv))
    assert torch.equal(a.to_nchw(fr, a.center_window(n, hs, ws, flip=True)), b.to_nchw(fr, b.center_window(n, hs, ws, flip=True)))


def test_resample_rejects_bad_rows_and_bad_scalars():
    from mvfnet_amd._lib import lib
    from mvfnet_amd.preprocess import ResamplingFramePipeline
    pipe = ResamplingFramePipeline(MEAN, STD, crop_size=16)
    fr = torch.zeros(2, 20, 24, 3, dtype=torch.uint8, device="cuda")
    good = [20, 24, 0, 0, 20, 24, 32, 32, 0, 0, 0]
    assert pipe.to_nchw(fr, torch.tensor([good, good], dtype=torch.int32)).shape == (2, 3, 16, 16)       # frames smaller than the crop
    with pytest.raises(TypeError):
        pipe.to_nchw(fr.float(), torch.tensor([good, good], dtype=torch.int32))
    with pytest.raises(ValueError):
        pipe.to_nchw(fr, None)
    with pytest.raises(ValueError):
        pipe.to_nchw(fr, torch.tensor([good], dtype=torch.int32))                                     # one row for two frames
    for k, v in [(0, 21), (1, 0), (2, 1), (3, -1), (4, 0), (5, 25), (6, 15), (7, 8), (8, 17), (9, -2), (10, 2)]:
        bad = list(good)
        bad[k] = v
        with pytest.raises(ValueError):
            pipe.to_nchw(fr, torch.tensor([good, bad], dtype=torch.int32))
    with pytest.raises(RuntimeError):
        ResamplingFramePipeline(MEAN, [1.0, 0.0, 1.0], crop_size=16).to_nchw(fr, torch.tensor([good, good], dtype=torch.int32))
    rows = torch.tensor([good, good], dtype=torch.int32, device="cuda")
    out = torch.empty(2, 22, 24, 4, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    args = dict(mean=pipe.mean, std=pipe.std)
    call = lambda rp, h, w, pad, wp, dt: lib.mvf_frames_resample_u8(fr.data_ptr(), 2, 20, 24, rp, h, w, args["mean"], args["std"], 1, 0,
                                                                   pad, wp, out.data_ptr(), None, dt, st)
    assert call(None, 16, 16, 3, 24, 0) != 0                     # rows NULL
    assert call(rows.data_ptr(), 16, 16, 3, 21, 0) != 0          # wp < w + 2 pad
    assert call(rows.data_ptr(), 16, 16, 3, 24, 5) != 0          # dtype
    assert call(rows.data_ptr(), 0, 16, 3, 24, 0) != 0           # h = 0
    assert call(rows.data_ptr(), 16, 16, -1, 24, 0) != 0         # pad < 0
    assert call(rows.data_ptr(), 16, 16, 3, 24, 0) == 0
    torch.cuda.synchronize()


# ---- end to end: the three shipped recipes through the public API ----------------------------------------------------------------------
def _r50(T):
    import mvfnet_amd
    from mvfnet_amd import synth
    m = mvfnet_amd.build_recognizer(mvfnet_amd.mvfnet_config(50, T), None, dict(average_clips=None))
    sd = m.state_dict()
    vals = synth.synth_state_dict({"r50/" + k: tuple(v.shape) for k, v in sd.items()})
    m.load_state_dict({k: torch.from_numpy(vals["r50/" + k]) for k in sd}, strict=True)
    return m.cuda()


def _clips(B, T, shapes, seed):
    return [_frames(T, hh, ww, seed + k) for k, (hh, ww) in enumerate(shapes[:B])]


SHAPES = [(72, 96), (90, 70), (80, 80), (66, 101)]


@pytest.mark.parametrize("streams", [1, 2])
def test_forward_test_with_val_and_test_rows_equals_the_fp32_tensor_path(streams):
    from mvfnet_amd.preprocess import ResamplingFramePipeline, collate_frames, test_rows, val_rows
    T, c = 4, 64
    m = _r50(T)
    m.eval()
    m.backbone.engine().streams = streams
    for recipe, B in (("val", 4), ("test", 2)):
        clips = _clips(B, T, SHAPES, 30)
        if recipe == "val":
            groups = [(f, val_rows(f.shape[1], f.shape[2], T, scale=(float("inf"), 72), crop_size=c)) for f in clips]
        else:                                                   # ThreeCrop: the clip's frames repeated once per crop
            groups = [(np.concatenate([f] * 3), test_rows(f.shape[1], f.shape[2], T, scale=(float("inf"), 72), crop_size=c)) for f in clips]
        fr, rows = collate_frames(groups)
        fr, rows = fr.cuda(), rows.cuda()
        pipe = ResamplingFramePipeline(MEAN, STD, to_rgb=True, crop_size=c)
        x = pipe.to_nchw(fr, rows).view(B, fr.shape[1], 3, c, c)
        m.set_input_pipeline(None)
        want = m(x, None, return_loss=False)
        m.set_input_pipeline(pipe)
        got = m(fr, None, return_loss=False, window=rows)
        assert np.array_equal(got, want), recipe
    m.set_input_pipeline(None)


def test_forward_train_with_train_rows_is_bit_identical_to_the_fp32_tensor_path():
    """One training step from uint8 frames + train_rows == the same step from to_nchw's fp32 tensor on an identical model: loss,
    every gradient and the BatchNorm running statistics, bit for bit."""
    from mvfnet_amd.preprocess import ResamplingFramePipeline, collate_frames, train_rows
    T, B, c = 4, 2, 64
    clips = _clips(B, T, SHAPES, 50)
    random.seed(11)
    np.random.seed(11)
    fr, rows = collate_frames([(f, train_rows(f.shape[1], f.shape[2], T, input_size=c)) for f in clips])
    fr, rows = fr.cuda(), rows.cuda()
    pipe = ResamplingFramePipeline(MEAN, STD, to_rgb=True, crop_size=c)
    x = pipe.to_nchw(fr, rows).view(B, T, 3, c, c)
    lab = torch.tensor([[5], [77]], device="cuda")
    res = []
    for u8 in (False, True):
        m = _r50(T)
        m.train()
        m.cls_head.dropout = None
        if u8:
            m.set_input_pipeline(pipe)
            loss = m(fr, lab, window=rows)["loss_cls"]
        else:
            loss = m(x, lab)["loss_cls"]
        loss.backward()
        torch.cuda.synchronize()
        res.append((loss.detach().clone(), {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None},
                    {k: v.detach().clone() for k, v in m.state_dict().items()}))
        del m
    (l0, g0, s0), (l1, g1, s1) = res
    assert torch.equal(l0, l1)
    assert g0.keys() == g1.keys() and len(g0) > 0
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k
    assert any("running_mean" in k for k in s0)
    for k in s0:
        assert torch.equal(s0[k], s1[k]), k
