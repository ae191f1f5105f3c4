"""mvf_frames_resample_color_u8 (uint8 frames -> resize / crop / flip -> ColorJitter's affine colour map -> normalise / stem layout) bit for
bit against the numpy restatement (tests/jitter_numpy.py), against mvf_frames_resample_u8 where the map is absent or the identity, and the
engines fed uint8 frames + 23-column tables of the TSN recipes against the same engines fed the fp32 tensor to_nchw makes from them."""
import random

import numpy as np
import pytest
import torch

import jitter_numpy as J

pytestmark = pytest.mark.gpu

MEAN, STD = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]
UNIT = ([0.485, 0.456, 0.406], [0.229, 0.224, 0.225])


def _frames(n, hs, ws, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(n, hs, ws, 3)).astype(np.uint8)


def _geometry(mode, n, hs, ws, h, w):
    """(n, 11) rows on whole hs x ws frames, one resample mode per table, the crop offset and the flip varying per frame."""
    rows = []
    for i in range(n):
        if mode == "identity":
            by, bx, bh, bw = i, 2 * i, hs - i, ws - 2 * i
            rh, rw = bh, bw
        elif mode == "area2":
            by, bx, rh, rw = i, i, h + 2 + i, w + 3
            bh, bw = 2 * rh, 2 * rw
        elif mode == "up":
            by, bx, bh, bw = 1, i, h // 2 + i, w // 3 + 1
            rh, rw = h + 5, w + i
        else:                                                   # generic bilinear down, not 2x
            by, bx, bh, bw = 0, i, hs - i, ws - i
            rh, rw = h + 1 + i % 2, w + 2
        flip = 1 if mode == "flip" else i % 2
        rows.append((hs, ws, by, bx, bh, bw, rh, rw, (rh - h) // 2, rw - w, flip))
    return np.array(rows, dtype=np.int32)


def _color(kind, n, seed):
    from mvfnet_amd.preprocess import color_identity, color_jitter_table
    random.seed(seed)
    np.random.seed(seed)
    if kind == "identity":
        return color_identity(n)
    return np.concatenate([color_jitter_table(1, color_space_aug=(kind == "full")) for _ in range(n)])      # a different map per frame


MODES = ["identity", "area2", "up", "down", "flip"]
CASES = [(m, c, rgb, div) for m in MODES for c in ("identity", "default", "full") for (rgb, div) in ((True, False), (False, True))]
CASES += [("down", "full", True, True), ("up", "full", False, False)]


@pytest.mark.parametrize("mode,kind,to_rgb,div", CASES, ids=["%s-%s-%s%s" % (m, c, "rgb" if r else "bgr", "-div255" if d else "") for m, c, r, d in CASES])
def test_jitter_nchw_bit_exact_vs_numpy(mode, kind, to_rgb, div):
    from mvfnet_amd.preprocess import JitterFramePipeline, jitter_rows
    n, hs, ws, h, w = 6, 64, 76, 19, 23
    fr = _frames(n, hs, ws, 7)
    rows = _geometry(mode, n, hs, ws, h, w)
    color = _color(kind, n, 1 + MODES.index(mode))
    mean, std = UNIT if div else (MEAN, STD)
    pipe = JitterFramePipeline(mean, std, to_rgb=to_rgb, div_255=div, crop_size=(w, h))
    got = pipe.to_nchw(torch.from_numpy(fr).cuda(), torch.from_numpy(jitter_rows(rows, color)).cuda()).cpu().numpy()
    want = J.frames_to_nchw(fr, rows, color, h, w, mean, std, to_rgb=to_rgb, div_255=div)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    if kind == "full":
        assert not np.array_equal(color[:, :9], np.tile(np.eye(3, dtype=np.float32).reshape(-1), (n, 1)))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_jitter_stem_layout_equals_stem_prep_of_the_nchw_output(dtype):
    from mvfnet_amd._lib import check, lib
    from mvfnet_amd.preprocess import JitterFramePipeline, jitter_rows
    n, hs, ws, h, w, pad = 5, 50, 61, 40, 44, 3
    rows = _geometry("down", n, hs, ws, h, w)
    color = _color("full", n, 3)
    fr = _frames(n, hs, ws, 3)
    pipe = JitterFramePipeline(MEAN, STD, to_rgb=True, crop_size=(w, h))
    wp = (w + 2 * pad + 2 + 1) // 2 * 2
    fr_t, tab = torch.from_numpy(fr).cuda(), torch.from_numpy(jitter_rows(rows, color)).cuda()
    got = pipe.to_stem(fr_t, tab, pad, wp, dtype)
    x = pipe.to_nchw(fr_t, tab)
    assert np.array_equal(x.cpu().numpy(), J.frames_to_nchw(fr, rows, color, h, w, MEAN, STD))
    ref = torch.full((n, h + 2 * pad, wp, 4), 7.0, dtype=dtype, device="cuda")
    check(lib.mvf_stem_prep(x.data_ptr(), n, 3, h, w, pad, wp, ref.data_ptr(), 0 if dtype == torch.float32 else 1,
                            torch.cuda.current_stream().cuda_stream), "stem_prep")
    iv = torch.int16 if dtype == torch.bfloat16 else torch.int32
    assert torch.equal(got.view(iv), ref.view(iv))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_no_table_eleven_columns_and_identity_equal_frames_resample_u8(dtype):
    from mvfnet_amd._lib import check, lib
    from mvfnet_amd.preprocess import JitterFramePipeline, ResamplingFramePipeline, color_identity, jitter_rows
    n, hs, ws, h, w, pad = 6, 48, 56, 21, 32, 3
    fr = torch.from_numpy(_frames(n, hs, ws, 11)).cuda()
    rows = np.concatenate([_geometry(m, 2, hs, ws, h, w) for m in ("identity", "down", "up")])
    rows_t = torch.from_numpy(rows).cuda()
    a, b = ResamplingFramePipeline(MEAN, STD, crop_size=(w, h)), JitterFramePipeline(MEAN, STD, crop_size=(w, h))
    wp = (w + 2 * pad + 2 + 1) // 2 * 2
    iv = torch.int16 if dtype == torch.bfloat16 else torch.int32
    want_x, want_s = a.to_nchw(fr, rows_t), a.to_stem(fr, rows_t, pad, wp, dtype)
    ident = torch.from_numpy(jitter_rows(rows, color_identity(n))).cuda()
    for tab in (rows_t, ident):                                  # 11 columns = no jitter; the identity map
        assert torch.equal(b.to_nchw(fr, tab).view(torch.int32), want_x.view(torch.int32))
        assert torch.equal(b.to_stem(fr, tab, pad, wp, dtype).view(iv), want_s.view(iv))
    # color = NULL straight at the C ABI
    st = torch.cuda.current_stream().cuda_stream
    x = torch.empty_like(want_x)
    s = torch.full_like(want_s, 7.0)
    check(lib.mvf_frames_resample_color_u8(fr.data_ptr(), n, hs, ws, rows_t.data_ptr(), None, h, w, a.mean, a.std, 1, 0, 0, w, None, x.data_ptr(), 0, st), "nchw")
    check(lib.mvf_frames_resample_color_u8(fr.data_ptr(), n, hs, ws, rows_t.data_ptr(), None, h, w, a.mean, a.std, 1, 0, pad, wp, s.data_ptr(), None,
                                           0 if dtype == torch.float32 else 1, st), "stem")
    assert torch.equal(x.view(torch.int32), want_x.view(torch.int32)) and torch.equal(s.view(iv), want_s.view(iv))


def test_padded_batch_of_three_frame_sizes_with_a_table_per_frame_is_correct_per_frame():
    from mvfnet_amd.preprocess import (JitterFramePipeline, center_crop_rows, collate_jitter_frames, color_jitter_table, jitter_rows,
                                       multi_scale_crop_rows, random_rescaled_crop_rows)
    T, c = 3, 24
    shapes = [(30, 40), (45, 26), (27, 29)]
    clips = [_frames(T, hh, ww, 10 + k) for k, (hh, ww) in enumerate(shapes)]
    random.seed(4)
    np.random.seed(4)
    geo = [multi_scale_crop_rows(30, 40, T, input_size=c), random_rescaled_crop_rows(45, 26, T, c, scale=(26, 32)), center_crop_rows(27, 29, T, c)]
    col = [color_jitter_table(T, True), color_jitter_table(T, True), color_jitter_table(T, False)]
    assert not np.array_equal(col[0][0], col[0][1]) or not np.array_equal(col[1][0], col[1][1])      # the maps differ within a clip
    fr, tab = collate_jitter_frames([(f, jitter_rows(g, cc)) for f, g, cc in zip(clips, geo, col)], pad_to=(48, 48))
    pipe = JitterFramePipeline(MEAN, STD, to_rgb=True, crop_size=c)
    got = pipe.to_nchw(fr.cuda(), tab.cuda()).cpu().numpy().reshape(3, T, 3, c, c)
    for k in range(3):                                           # the numpy restatement sees the UNPADDED frames
        assert np.array_equal(got[k], J.frames_to_nchw(clips[k], geo[k], col[k], c, c, MEAN, STD)), shapes[k]


def test_jitter_rejects_bad_tables_and_bad_scalars():
    """Bad scalars only: no bad pointer and no out-of-range row ever reaches a launch."""
    from mvfnet_amd._lib import lib
    from mvfnet_amd.preprocess import JitterFramePipeline, color_identity, jitter_rows
    pipe = JitterFramePipeline(MEAN, STD, crop_size=16)
    fr = torch.zeros(2, 20, 24, 3, dtype=torch.uint8, device="cuda")
    good = np.array([[20, 24, 0, 0, 20, 24, 32, 32, 0, 0, 0]] * 2, dtype=np.int32)
    tab = jitter_rows(good, color_identity(2))
    assert pipe.to_nchw(fr, torch.from_numpy(tab)).shape == (2, 3, 16, 16)
    with pytest.raises(TypeError):
        pipe.to_nchw(fr.float(), torch.from_numpy(tab))
    with pytest.raises(ValueError):
        pipe.to_nchw(fr, None)
    with pytest.raises(ValueError):
        pipe.to_nchw(fr, torch.from_numpy(tab[:1]))                                                   # one row for two frames
    with pytest.raises(ValueError):
        pipe.to_nchw(fr, torch.from_numpy(tab[:, :12].copy()))                                        # neither 11 nor 23 columns
    for k, v in [(0, 21), (4, 0), (8, 17), (10, 2)]:                                                  # the geometry columns, as the parent
        bad = tab.copy()
        bad[1, k] = v
        with pytest.raises(ValueError):
            pipe.to_nchw(fr, torch.from_numpy(bad))
    for v in (np.nan, np.inf, -np.inf):                                                               # non-finite coefficients
        bad = tab.copy()
        bad[1, 11 + 5] = np.array([v], dtype=np.float32).view(np.int32)[0]
        with pytest.raises(ValueError, match="finite"):
            pipe.to_nchw(fr, torch.from_numpy(bad))
    with pytest.raises(RuntimeError, match="std"):
        JitterFramePipeline(MEAN, [1.0, 0.0, 1.0], crop_size=16).to_nchw(fr, torch.from_numpy(tab))
    rows = torch.from_numpy(good).cuda()
    color = torch.from_numpy(color_identity(2)).cuda()
    out = torch.empty(2, 22, 24, 4, device="cuda")
    st = torch.cuda.current_stream().cuda_stream
    call = lambda fp, h, w, pad, wp, dt: lib.mvf_frames_resample_color_u8(fp, 2, 20, 24, rows.data_ptr(), color.data_ptr(), h, w, pipe.mean, pipe.std,   # noqa: E731
                                                                         1, 0, pad, wp, out.data_ptr(), None, dt, st)
    for args, word in [((None, 16, 16, 3, 24, 0), b"bad argument"),                                   # frames NULL
                       ((fr.data_ptr(), 16, 16, 3, 21, 0), b"wp=21"),                                 # wp < w + 2 pad
                       ((fr.data_ptr(), 16, 16, 3, 24, 5), b"bad dtype"),
                       ((fr.data_ptr(), 0, 16, 3, 24, 0), b"bad argument"),                           # h = 0
                       ((fr.data_ptr(), 16, 16, -1, 24, 0), b"bad argument")]:                        # pad < 0
        assert call(*args) == -1                                                                      # MVF_EINVAL
        msg = lib.mvf_last_error()
        assert b"frames_resample_color_u8" in msg and word in msg, msg
    assert call(fr.data_ptr(), 16, 16, 3, 24, 0) == 0
    torch.cuda.synchronize()


# ---- end to end: the TSN recipes through the public API --------------------------------------------------------------------------------
def _r50(T):
    import mvfnet_amd
    from mvfnet_amd import synth
    m = mvfnet_amd.build_recognizer(mvfnet_amd.mvfnet_config(50, T), None, dict(average_clips=None))
    sd = m.state_dict()
    vals = synth.synth_state_dict({"r50/" + k: tuple(v.shape) for k, v in sd.items()})
    m.load_state_dict({k: torch.from_numpy(vals["r50/" + k]) for k in sd}, strict=True)
    return m.cuda()


SHAPES = [(72, 96), (90, 70), (80, 80), (66, 101)]


@pytest.mark.parametrize("streams", [1, 2])
def test_forward_test_with_ten_crop_rows_equals_the_fp32_tensor_path(streams):
    from mvfnet_amd.preprocess import JitterFramePipeline, collate_jitter_frames, ten_crop_rows
    T, c, B = 4, 64, 2
    m = _r50(T)
    m.eval()
    m.backbone.engine().streams = streams
    clips = [_frames(T, hh, ww, 30 + k) for k, (hh, ww) in enumerate(SHAPES[:B])]
    # TenCrop: the clip's frames repeated once per crop; 11-column tables (no jitter at test time) promoted by the collate
    groups = [(np.concatenate([f] * 10), ten_crop_rows(f.shape[1], f.shape[2], T, crop_size=c)) for f in clips]
    fr, tab = collate_jitter_frames(groups)
    fr, tab = fr.cuda(), tab.cuda()
    assert tuple(tab.shape) == (B * 10 * T, 23)
    pipe = JitterFramePipeline(MEAN, STD, to_rgb=True, crop_size=c)
    x = pipe.to_nchw(fr, tab).view(B, fr.shape[1], 3, c, c)
    m.set_input_pipeline(None)
    want = m(x, None, return_loss=False)
    m.set_input_pipeline(pipe)
    got = m(fr, None, return_loss=False, window=tab)
    m.set_input_pipeline(None)
    assert np.array_equal(got, want)


def test_forward_train_with_multi_scale_crop_and_full_jitter_is_bit_identical_to_the_fp32_tensor_path():
    """One training step from uint8 frames + the 23-column table (MultiScaleCrop -> Flip -> ColorJitter(color_space_aug=True)) == the same
    step from to_nchw's fp32 tensor on an identical model: loss, every gradient and the BatchNorm running statistics, bit for bit."""
    from mvfnet_amd.preprocess import JitterFramePipeline, collate_jitter_frames, color_jitter_table, jitter_rows, multi_scale_crop_rows
    T, B, c = 4, 2, 64
    clips = [_frames(T, hh, ww, 50 + k) for k, (hh, ww) in enumerate(SHAPES[:B])]
    random.seed(11)
    np.random.seed(11)
    groups = []
    for f in clips:
        geo = multi_scale_crop_rows(f.shape[1], f.shape[2], T, input_size=c)
        groups.append((f, jitter_rows(geo, color_jitter_table(T, color_space_aug=True))))
    fr, tab = collate_jitter_frames(groups)
    assert not np.array_equal(tab[:, 11:20].numpy(), np.tile(np.eye(3, dtype=np.float32).reshape(-1).view(np.int32), (B * T, 1)))
    fr, tab = fr.cuda(), tab.cuda()
    pipe = JitterFramePipeline(MEAN, STD, to_rgb=True, crop_size=c)
    x = pipe.to_nchw(fr, tab).view(B, T, 3, c, c)
    lab = torch.tensor([[5], [77]], device="cuda")
    res = []
    for u8 in (False, True):
        m = _r50(T)
        m.train()
        m.cls_head.dropout = None
        if u8:
            m.set_input_pipeline(pipe)
            loss = m(fr, lab, window=tab)["loss_cls"]
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
