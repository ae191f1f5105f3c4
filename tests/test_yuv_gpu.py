"""mvf_frames_yuv420_gather_resample_u8 (decoder-native I420 / NV12 frames in the uint8 input) bit for bit against the packed-frame path fed
the numpy-converted frames (tests/yuv_numpy.py): Yuv420FramePipeline(yuv, table) == GatherFramePipeline(to_packed(yuv), table) for every
layout x standard x stored order x output over the shipped recipes' tables, against oracle/frames_numpy.py on the converted frames, and end
to end through BackboneEngine, Recognizer2D.forward_test and one training step.  Every comparison is torch.equal / np.array_equal: the
conversion is integer arithmetic and everything after it is the packed path's.  Planes are uniform random bytes, so Y < 16, every
saturation and every chroma value occur."""
import functools
import random

import numpy as np
import pytest
import torch

import yuv_numpy as Y
from oracle import frames_numpy as F

pytestmark = pytest.mark.gpu

MEAN, STD = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]
HS, WS, N = 60, 76, 4
LAYOUTS = {"i420": Y.I420, "nv12": Y.NV12}


class _Source(object):
    """Frames as planes: .yuv(layout) = the (n, 3 * Hs / 2, pitch) buffers handed to the new pipeline, .packed(standard, order) = the numpy
    conversion handed to the packed path.  `clips` = [(Y, U, V)]: several = a mixed-resolution collate (one row table per clip)."""

    def __init__(self, clips, pitch=None):
        self.clips, self.pitch = clips, pitch
        self.width = clips[0][0].shape[2] if pitch is not None else None

    def yuv(self, layout, tables):
        from mvfnet_amd.preprocess import collate_yuv_frames
        if len(self.clips) == 1:
            return torch.from_numpy(Y.pack(*self.clips[0], LAYOUTS[layout], pitch=self.pitch, fill_seed=9))
        return collate_yuv_frames(list(zip(self.clips, tables)), layout)[0]

    def packed(self, standard, order, tables):
        from mvfnet_amd.preprocess import collate_frames
        conv = [Y.planes_to_packed(*c, standard, order) for c in self.clips]
        if len(conv) == 1:
            return torch.from_numpy(conv[0])
        return collate_frames(list(zip(conv, tables)))[0]


@functools.lru_cache(maxsize=None)
def _cases():
    """name -> (source, [one table per clip], crop (w, h)).  A table with a src column belongs to a single-clip source."""
    from mvfnet_amd import preprocess as P
    base = _Source([Y.random_planes(N, HS, WS, 1)])
    random.seed(3)
    np.random.seed(3)
    cases = {}
    cases["train_rows"] = (base, [P.train_rows(HS, WS, N, input_size=24)], 24)
    cases["val_rows"] = (base, [P.val_rows(HS, WS, N, scale=(float("inf"), 40), crop_size=32)], 32)
    area = P.val_rows(HS, WS, N, scale=(float("inf"), 30), crop_size=24)                     # 60 x 76 -> 30 x 38: the exact-2x area mean
    assert (area[:, 4] == 2 * area[:, 6]).all() and (area[:, 5] == 2 * area[:, 7]).all()
    cases["val_rows_area2x"] = (base, [area], 24)
    cases["test_rows"] = (base, [P.gather_rows(P.test_rows(HS, WS, N, scale=(float("inf"), 40), crop_size=40), np.tile(np.arange(N), 3))], 40)
    ten = P.ten_crop_rows(HS, WS, N, crop_size=(36, 32))
    assert ten[:, 10].sum() * 2 == len(ten)
    cases["ten_crop_rows"] = (base, [P.gather_rows(ten, np.tile(np.arange(N), 10))], (36, 32))
    color = P.color_jitter_table(N, color_space_aug=True)
    assert not np.array_equal(color, P.color_identity(N))
    cases["multi_scale_crop_jitter"] = (base, [P.jitter_rows(P.multi_scale_crop_rows(HS, WS, N, input_size=(28, 24)), color)], (28, 24))
    inds = P.sample_frame_inds(7, 4, 2, 3, test_mode=True)                                    # 12 sampled frames of a 7-frame video
    distinct, table = P.video_test_table(inds, HS, WS, P.test_rows, scale=(float("inf"), 40), crop_size=40)
    assert len(distinct) < len(inds) and table.shape == (36, 12)
    cases["video_test_table"] = (_Source([Y.random_planes(len(distinct), HS, WS, 2)]), [table], 40)
    # boxes with odd by / bx (chroma sample of an absolute coordinate), odd sizes, up, down and identity resamples, flips
    odd = np.array([(HS, WS, 3, 5, 31, 41, 26, 30, 1, 2, 1), (HS, WS, 1, 1, 21, 33, 40, 50, 7, 9, 0),
                    (HS, WS, 5, 3, 48, 60, 24, 30, 0, 2, 1), (HS, WS, 7, 9, 30, 40, 30, 40, 3, 5, 1)], dtype=np.int32)
    cases["odd_boxes_and_flips"] = (base, [odd], (28, 24))
    wide = _Source([Y.random_planes(N, HS, WS, 4)], pitch=96)                                 # pitch > Ws: a decoder's aligned rows
    cases["pitch_above_width"] = (wide, [np.concatenate([odd[:2], P.train_rows(HS, WS, 2, input_size=(28, 24))])], (28, 24))
    a, b = Y.random_planes(2, 59, 75, 5), Y.random_planes(2, 45, 52, 6)                       # odd-sized clips in one even padded batch
    mixed = [np.concatenate([P.val_rows(59, 75, 1, scale=(float("inf"), 40), crop_size=(28, 24)), [(59, 75, 1, 3, 58, 72, 29, 36, 2, 5, 1)]]),
             np.concatenate([P.val_rows(45, 52, 1, scale=(float("inf"), 30), crop_size=(28, 24)), [(45, 52, 0, 0, 45, 52, 45, 52, 21, 24, 1)]])]
    cases["mixed_resolution_collate"] = (_Source([a, b]), [np.asarray(m, dtype=np.int32) for m in mixed], (28, 24))
    return cases


def _table(tables):
    return torch.from_numpy(np.concatenate(tables)).cuda()


@functools.lru_cache(maxsize=None)
def _want(name, standard, order):
    """The comparator, once per (case, standard, order): the packed-frame path on the numpy-converted frames -> (nchw, fp32 stem, bf16 stem)."""
    from mvfnet_amd.preprocess import GatherFramePipeline
    src, tables, crop = _cases()[name]
    pipe = GatherFramePipeline(MEAN, STD, to_rgb=True, crop_size=crop)
    fr, tab = src.packed(standard, order, tables).cuda(), _table(tables)
    h, w = pipe.crop_hw
    wp = (w + 6 + 2 + 1) // 2 * 2
    return pipe.to_nchw(fr, tab), pipe.to_stem(fr, tab, 3, wp, torch.float32), pipe.to_stem(fr, tab, 3, wp, torch.bfloat16)


@pytest.mark.parametrize("order", ["bgr", "rgb"])
@pytest.mark.parametrize("standard", [0, 1, 2])
@pytest.mark.parametrize("layout", ["i420", "nv12"])
def test_yuv_pipeline_equals_the_packed_pipeline_on_the_numpy_converted_frames(layout, standard, order):
    from mvfnet_amd.preprocess import Yuv420FramePipeline
    for name, (src, tables, crop) in _cases().items():
        pipe = Yuv420FramePipeline(MEAN, STD, to_rgb=True, crop_size=crop, layout=layout, standard=standard, order=order, pitch=src.pitch,
                                   width=src.width)
        fr, tab = src.yuv(layout, tables).cuda(), _table(tables)
        assert fr.dim() >= 3 and fr.shape[-2] % 3 == 0
        want = _want(name, standard, Y.BGR if order == "bgr" else Y.RGB)
        h, w = pipe.crop_hw
        wp = (w + 6 + 2 + 1) // 2 * 2
        assert pipe.n_out(fr, tab) == want[0].shape[0]
        got = (pipe.to_nchw(fr, tab), pipe.to_stem(fr, tab, 3, wp, torch.float32), pipe.to_stem(fr, tab, 3, wp, torch.bfloat16))
        for g, w_, iv in zip(got, want, (torch.int32, torch.int32, torch.int16)):
            assert g.shape == w_.shape and g.dtype == w_.dtype, name
            assert torch.equal(g.view(iv), w_.view(iv)), (name, g.dtype, tuple(g.shape))
        out = torch.full_like(want[2], 7.0)                                                  # a caller's buffer, as TrainEngine hands one
        assert pipe.to_stem(fr, tab, 3, wp, torch.bfloat16, out=out) is out and torch.equal(out.view(torch.int16), want[2].view(torch.int16))


def test_the_conversion_matters_to_the_comparison():
    """The sweep above would not notice a kernel that ignored `standard` or `order` if the converted frames did not differ: they do."""
    y, u, v = Y.random_planes(1, 8, 8, 1)
    seen = {(s, o): Y.planes_to_packed(y, u, v, s, o).tobytes() for s in (0, 1, 2) for o in (Y.BGR, Y.RGB)}
    assert len(set(seen.values())) == 6
    assert not torch.equal(_want("train_rows", 0, Y.BGR)[0], _want("train_rows", 2, Y.BGR)[0])
    assert not torch.equal(_want("train_rows", 0, Y.BGR)[0], _want("train_rows", 0, Y.RGB)[0])


@pytest.mark.parametrize("layout", ["i420", "nv12"])
def test_identity_rows_equal_the_oracle_on_the_numpy_converted_frames(layout):
    """Not only against the sibling kernel: a row without a resample is a (y0, x0, flip) window, which oracle/frames_numpy.py states."""
    from mvfnet_amd.preprocess import Yuv420FramePipeline
    planes = Y.random_planes(N, HS, WS, 8)
    h, w = 33, 41
    win = np.array([(0, 0, 0), (27, 35, 1), (13, 7, 0), (5, 20, 1)], dtype=np.int32)           # odd and even offsets, the frame's corners
    rows = np.array([(HS, WS, 0, 0, HS, WS, HS, WS, y0, x0, f) for (y0, x0, f) in win], dtype=np.int32)
    for standard, to_rgb, div in ((0, True, False), (1, False, True), (2, True, False)):
        pipe = Yuv420FramePipeline(MEAN, STD, to_rgb=to_rgb, div_255=div, crop_size=(w, h), layout=layout, standard=standard)
        got = pipe.to_nchw(torch.from_numpy(Y.pack(*planes, LAYOUTS[layout])).cuda(), torch.from_numpy(rows).cuda()).cpu().numpy()
        want = F.frames_to_nchw(Y.planes_to_packed(*planes, standard, Y.BGR), win, h, w, MEAN, STD, to_rgb, div)
        assert np.array_equal(got.view(np.int32), want.view(np.int32)), (standard, to_rgb, div)
    cw = pipe.center_window(N, HS, WS, flip=True)
    assert cw.tolist() == [[HS, WS, 0, 0, HS, WS, HS, WS, (HS - h) // 2, (WS - w) // 2, 1]] * N


def test_export_refuses_bad_geometry_and_enums():
    """Odd hs, pitch < ws, an odd pitch and unknown enums return MVF_EINVAL and set mvf_last_error; nothing is launched."""
    from mvfnet_amd._lib import lib
    from mvfnet_amd.preprocess import Yuv420FramePipeline
    pipe = Yuv420FramePipeline(MEAN, STD, crop_size=16)
    fr = torch.zeros(2, 30, 24, dtype=torch.uint8, device="cuda")
    rows = torch.tensor([[20, 24, 0, 0, 20, 24, 20, 24, 0, 0, 0]] * 2, dtype=torch.int32, device="cuda")
    out = torch.zeros(2, 3, 16, 16, device="cuda")

    def call(hs=20, ws=24, pitch=24, layout=0, standard=0, order=0):
        return lib.mvf_frames_yuv420_gather_resample_u8(fr.data_ptr(), 2, hs, ws, pitch, layout, standard, order, None, 2, rows.data_ptr(), None, 16, 16,
                                                        pipe.mean, pipe.std, 1, 0, 0, 16, None, out.data_ptr(), 0, None)
    assert call() == 0
    for kw, word in [(dict(hs=19), b"hs=19"), (dict(pitch=22), b"pitch=22"), (dict(pitch=25, ws=23), b"pitch=25"), (dict(layout=2), b"layout 2"),
                     (dict(standard=3), b"standard 3"), (dict(order=2), b"order 2")]:
        assert call(**kw) == -1, kw
        assert word in lib.mvf_last_error(), (kw, lib.mvf_last_error())
    torch.cuda.synchronize()
    # the pipeline: frame tensors that are no (3 * Hs / 2, even pitch) image, a pitch that is not the tensor's, rows outside the TRUE width
    with pytest.raises(ValueError, match="3 \\* Hs / 2"):
        pipe.to_nchw(torch.zeros(2, 31, 24, dtype=torch.uint8, device="cuda"), rows)
    with pytest.raises(ValueError, match="3 \\* Hs / 2"):
        pipe.to_nchw(torch.zeros(2, 30, 25, dtype=torch.uint8, device="cuda"), rows)
    with pytest.raises(ValueError, match="not pitch=32"):
        Yuv420FramePipeline(MEAN, STD, crop_size=16, pitch=32, width=24).to_nchw(fr, rows)
    with pytest.raises(ValueError, match="patch must lie"):
        Yuv420FramePipeline(MEAN, STD, crop_size=16, pitch=24, width=22).to_nchw(fr, rows)
    with pytest.raises(ValueError, match="patch must lie"):
        pipe.to_nchw(fr, torch.tensor([[21, 24, 0, 0, 21, 24, 21, 24, 0, 0, 0]] * 2, dtype=torch.int32))      # hs_i above Hs = 20
    with pytest.raises(ValueError, match="rows for"):
        pipe.to_nchw(fr, rows[:1])
    with pytest.raises(ValueError):
        pipe.to_nchw(fr, None)


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
def _r50(T, dtype=torch.float32):
    import mvfnet_amd
    from mvfnet_amd import synth
    m = mvfnet_amd.build_recognizer(mvfnet_amd.mvfnet_config(50, T), None, dict(average_clips=None))
    sd = m.state_dict()
    vals = synth.synth_state_dict({"r50/" + k: tuple(v.shape) for k, v in sd.items()})
    m.load_state_dict({k: torch.from_numpy(vals["r50/" + k]) for k in sd}, strict=True)
    m.backbone.engine_dtype = dtype
    return m.cuda()


def test_backbone_features_and_forward_test_on_a_small_video_are_bit_equal_to_the_packed_input():
    """A 24-frame 72 x 96 NV12 video, 4 overlapping clips of T = 4, Resize + ThreeCrop(64): BackboneEngine's features and forward_test's
    scores from the YUV frames == from the numpy-converted packed frames, on one stream and on two (the engine slices the table, not the
    frames)."""
    from mvfnet_amd.preprocess import GatherFramePipeline, Yuv420FramePipeline, sample_frame_inds, test_rows, video_test_table
    T, total, hs, ws, c = 4, 24, 72, 96, 64
    inds = sample_frame_inds(total, T, 4, 4, test_mode=True)
    distinct, table = video_test_table(inds, hs, ws, test_rows, scale=(float("inf"), 80), crop_size=c)
    assert len(distinct) < len(inds) and table.shape == (48, 12)
    planes = Y.random_planes(len(distinct), hs, ws, 77)
    yuv = torch.from_numpy(Y.pack(*planes, Y.NV12)).cuda()[None]                            # (1, frames, 108, 96)
    packed = torch.from_numpy(Y.planes_to_packed(*planes, 0, Y.BGR)).cuda()[None]          # (1, frames, 72, 96, 3)
    tab = torch.from_numpy(table).cuda()
    new, old = Yuv420FramePipeline(MEAN, STD, to_rgb=True, crop_size=c, layout="nv12"), GatherFramePipeline(MEAN, STD, to_rgb=True, crop_size=c)
    m = _r50(T, torch.bfloat16)
    m.eval()
    eng = m.backbone.engine()
    for streams in (1, 2):
        eng.streams = streams
        res = []
        for pipe, fr in ((old, packed), (new, yuv)):
            m.set_input_pipeline(pipe)
            eng = m.backbone.engine()
            eng.input_window = tab
            feat = eng.forward(fr[0]).clone()                                                # BackboneEngine on (frames, ...) + the table
            res.append((feat, m(fr, None, return_loss=False, window=tab)))
        m.set_input_pipeline(None)
        (f0, s0), (f1, s1) = res
        assert f0.shape[0] == 48 and torch.equal(f0.view(torch.int16), f1.view(torch.int16)), streams
        assert s0.shape == (12, 400) and np.isfinite(s0).all() and np.array_equal(s0, s1), streams


def test_one_training_step_is_bit_equal_to_the_packed_input():
    """One step from a mixed-resolution I420 collate (an odd-sized clip) + the 23-column table (MultiScaleCrop -> Flip -> ColorJitter) == the
    same step from the numpy-converted packed frames on an identical model: the loss and every gradient."""
    from mvfnet_amd import preprocess as P
    T, c = 4, 64
    shapes = [(72, 96), (89, 71)]
    clips = [Y.random_planes(T, hh, ww, 50 + k) for k, (hh, ww) in enumerate(shapes)]
    random.seed(11)
    np.random.seed(11)
    tables = [P.jitter_rows(P.multi_scale_crop_rows(hh, ww, T, input_size=c), P.color_jitter_table(T, color_space_aug=True)) for hh, ww in shapes]
    yuv, tab = P.collate_yuv_frames(list(zip(clips, tables)), "i420", cols=23)
    packed, tab2 = P.collate_jitter_frames([(Y.planes_to_packed(*cl, 0, Y.BGR), t) for cl, t in zip(clips, tables)])
    assert torch.equal(tab, tab2) and tuple(yuv.shape) == (2, T, 135, 96) and tuple(packed.shape) == (2, T, 89, 96, 3)
    lab = torch.tensor([[5], [77]], device="cuda")
    res = []
    for pipe, fr in ((P.JitterFramePipeline(MEAN, STD, to_rgb=True, crop_size=c), packed), (P.Yuv420FramePipeline(MEAN, STD, to_rgb=True, crop_size=c), yuv)):
        m = _r50(T)
        m.train()
        m.cls_head.dropout = None
        m.set_input_pipeline(pipe)
        loss = m(fr.cuda(), lab, window=tab.cuda())["loss_cls"]
        loss.backward()
        torch.cuda.synchronize()
        res.append((loss.detach().clone(), {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}))
        del m
    (l0, g0), (l1, g1) = res
    assert torch.isfinite(l0).all() and torch.equal(l0, l1)
    assert g0.keys() == g1.keys() and len(g0) > 0
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k
