"""mvf_frames_addressed_resample_u8 (frames where and how the decoder left them: per-image plane offsets and pitches) bit for bit against
the existing DENSE path on the same frames: AddressedFramePipeline == GatherFramePipeline (packed) / Yuv420FramePipeline (I420, NV12) on the
dense batch, over test_yuv_gpu.py's table set; one batch of four frame sizes with odd pitches and gaps between planes against the dense
collates; a different fill of the bytes no plane owns; two videos of different size in one launch; and end to end through BackboneEngine,
Recognizer2D.forward_test and one training step.  Every comparison is torch.equal / np.array_equal."""
import functools
import random

import numpy as np
import pytest
import torch

import addressed_numpy as A
import yuv_numpy as Y
from test_yuv_gpu import MEAN, STD, _cases, _r50, _table

pytestmark = pytest.mark.gpu

FORMATS = {"packed": A.PACKED, "i420": A.I420, "nv12": A.NV12}
IV = (torch.int32, torch.int32, torch.int16)


def _three(pipe, fr, tab):
    """(nchw, fp32 stem, bf16 stem) of one pipeline: the stem operands with their zero padding."""
    h, w = pipe.crop_hw
    wp = (w + 6 + 2 + 1) // 2 * 2
    return pipe.to_nchw(fr, tab), pipe.to_stem(fr, tab, 3, wp, torch.float32), pipe.to_stem(fr, tab, 3, wp, torch.bfloat16)


def _equal(got, want, what):
    for g, w_, iv in zip(got, want, IV):
        assert g.shape == w_.shape and g.dtype == w_.dtype, what
        assert torch.equal(g.view(iv), w_.view(iv)), (what, g.dtype, tuple(g.shape))


def _dense(fmt, standard, order, crop, pitch=None, width=None):
    from mvfnet_amd.preprocess import GatherFramePipeline, Yuv420FramePipeline
    if fmt == "packed":
        return GatherFramePipeline(MEAN, STD, to_rgb=True, crop_size=crop)
    return Yuv420FramePipeline(MEAN, STD, to_rgb=True, crop_size=crop, layout=fmt, standard=standard, order=order, pitch=pitch, width=width)


def _addressed(fmt, standard, order, crop):
    from mvfnet_amd.preprocess import AddressedFramePipeline
    return AddressedFramePipeline(MEAN, STD, to_rgb=True, crop_size=crop, format=fmt, standard=standard, order=order)


def _frames_of(fmt, clip, standard=0, order=Y.BGR):
    """One clip's (Y, U, V) planes -> its frames one by one in addressed_numpy's form; packed = the numpy conversion, as the dense packed path is fed."""
    if fmt == "packed":
        conv = Y.planes_to_packed(*clip, standard, order)
        return [conv[t] for t in range(conv.shape[0])]
    return [tuple(p[t] for p in clip) for t in range(clip[0].shape[0])]


def _odd(v):
    return v + 5 if v % 2 == 0 else v + 4


def _pitches(fmt, frames, tight):
    """Per frame (p0, p1): the row bytes, or -- not tight -- row bytes + 5 for packed, odd luma and chroma pitches above the row for YUV."""
    out = []
    for f in frames:
        w = f.shape[1] if fmt == "packed" else f[0].shape[1]
        rb0, rb1 = {"packed": (3 * w, 0), "i420": (w, (w + 1) // 2), "nv12": (w, 2 * ((w + 1) // 2))}[fmt]
        out.append((rb0, rb1) if tight else ((rb0 + 5, 0) if fmt == "packed" else (_odd(rb0), _odd(rb1))))
    return out


@functools.lru_cache(maxsize=None)
def _dense_want(name, fmt, standard, order):
    """The comparator, once per (case, format, standard, order): the dense pipeline on the dense batch."""
    src, tables, crop = _cases()[name]
    o = Y.BGR if order == "bgr" else Y.RGB
    fr = src.packed(standard, o, tables) if fmt == "packed" else src.yuv(fmt, tables)
    return _three(_dense(fmt, standard, order, crop, src.pitch, src.width), fr.cuda(), _table(tables))


def _case_addressed(name, fmt, standard, order):
    """The case's frames laid out tight, one after the other, and its table with the address columns in place of the src column (or
    appended: one image per frame)."""
    from mvfnet_amd.preprocess import address_rows
    src, tables, crop = _cases()[name]
    o = Y.BGR if order == "bgr" else Y.RGB
    frames = [f for c in src.clips for f in _frames_of(fmt, c, standard, o)]
    buf, addr = A.pack(frames, FORMATS[fmt], pitches=_pitches(fmt, frames, True), gaps=0, fill_seed=4)
    return torch.from_numpy(buf).cuda(), torch.from_numpy(address_rows(np.concatenate(tables), addr)).cuda(), crop


def _check_case(name, fmt, standard, order):
    fr, tab, crop = _case_addressed(name, fmt, standard, order)
    pipe = _addressed(fmt, standard, order, crop)
    want = _dense_want(name, fmt, standard, order)
    assert pipe.gathers(tab) and pipe.n_out(fr, tab) == want[0].shape[0]
    _equal(_three(pipe, fr, tab), want, (name, fmt, standard, order))
    out = torch.full_like(want[2], 7.0)                                                  # a caller's buffer, as TrainEngine hands one
    h, w = pipe.crop_hw
    assert pipe.to_stem(fr, tab, 3, (w + 6 + 2 + 1) // 2 * 2, torch.bfloat16, out=out) is out and torch.equal(out.view(torch.int16), want[2].view(torch.int16))


@pytest.mark.parametrize("fmt", ["packed", "i420", "nv12"])
def test_same_size_frames_at_tight_pitch_equal_the_dense_pipeline_over_the_table_set(fmt):
    names = list(_cases())
    assert {"train_rows", "val_rows", "val_rows_area2x", "test_rows", "ten_crop_rows", "multi_scale_crop_jitter", "video_test_table",
            "odd_boxes_and_flips"} <= set(names)
    for name in names:
        _check_case(name, fmt, 0, "bgr")


@pytest.mark.parametrize("order", ["bgr", "rgb"])
@pytest.mark.parametrize("standard", [0, 1, 2])
@pytest.mark.parametrize("fmt", ["packed", "i420", "nv12"])
def test_every_format_standard_and_order_on_one_case(fmt, standard, order):
    _check_case("odd_boxes_and_flips", fmt, standard, order)


def test_the_stem_operand_is_zero_padded():
    """The comparison above would not notice padding that both paths got wrong alike: the border of the stem operand is zero, and so is
    its fourth channel."""
    fr, tab, crop = _case_addressed("val_rows", "nv12", 0, "bgr")
    pipe = _addressed("nv12", 0, "bgr", crop)
    h, w = pipe.crop_hw
    wp = (w + 6 + 2 + 1) // 2 * 2
    for dt in (torch.float32, torch.bfloat16):
        out = torch.full((tab.shape[0], h + 6, wp, 4), 7.0, dtype=dt, device="cuda")
        pipe.to_stem(fr, tab, 3, wp, dt, out=out)
        inner = torch.zeros(h + 6, wp, dtype=torch.bool, device="cuda")
        inner[3:3 + h, 3:3 + w] = True
        assert bool((out[:, ~inner] == 0).all()) and bool((out[..., 3] == 0).all()) and bool((out[:, inner][..., :3] != 0).any())


# ---- one batch of four frame sizes, every frame at its own pitch, gaps between the planes ------------------------------------------------
SIZES = [(60, 76), (76, 60), (59, 75), (45, 52)]
TM = 2                                                                                  # frames per clip


@functools.lru_cache(maxsize=None)
def _mixed():
    """-> (clips as (Y, U, V) planes, one (TM, 11) table per clip, crop): per clip a Resize + CenterCrop row and an odd box, one flipped."""
    from mvfnet_amd import preprocess as P
    clips = [Y.random_planes(TM, h, w, 60 + k) for k, (h, w) in enumerate(SIZES)]
    boxes = [(60, 76, 3, 5, 31, 41, 26, 30, 1, 2, 1), (76, 60, 1, 1, 33, 21, 50, 40, 9, 7, 0), (59, 75, 1, 3, 58, 72, 29, 36, 2, 5, 1),
             (45, 52, 0, 0, 45, 52, 45, 52, 21, 24, 1)]
    tables = [np.concatenate([P.val_rows(h, w, 1, scale=(float("inf"), 30), crop_size=(28, 24)), [box]]).astype(np.int32)
              for (h, w), box in zip(SIZES, boxes)]
    return clips, tables, (28, 24)


@functools.lru_cache(maxsize=None)
def _mixed_want(fmt):
    """The dense path on collate_frames / collate_yuv_frames of the same clips."""
    from mvfnet_amd import preprocess as P
    clips, tables, crop = _mixed()
    if fmt == "packed":
        fr, tab = P.collate_frames([(Y.planes_to_packed(*c, 0, Y.BGR), t) for c, t in zip(clips, tables)])
    else:
        fr, tab = P.collate_yuv_frames(list(zip(clips, tables)), fmt)
    return _three(_dense(fmt, 0, "bgr", crop), fr.cuda(), tab.cuda())


def _mixed_addressed(fmt, fill_seed):
    from mvfnet_amd.preprocess import address_rows
    clips, tables, crop = _mixed()
    frames = [f for c in clips for f in _frames_of(fmt, c)]
    pitches = _pitches(fmt, frames, False)
    assert all(p0 % 2 == 1 and p1 % 2 == 1 for p0, p1 in pitches) or fmt == "packed"
    buf, addr = A.pack(frames, FORMATS[fmt], pitches=pitches, gaps=13, fill_seed=fill_seed)
    return buf, torch.from_numpy(address_rows(np.concatenate(tables), addr)).cuda(), crop


@pytest.mark.parametrize("fmt", ["packed", "i420", "nv12"])
def test_four_frame_sizes_with_own_pitches_and_gaps_equal_the_dense_collate(fmt):
    buf, tab, crop = _mixed_addressed(fmt, 1)
    pipe = _addressed(fmt, 0, "bgr", crop)
    got = _three(pipe, torch.from_numpy(buf).cuda(), tab)
    _equal(got, _mixed_want(fmt), fmt)
    # the same inputs with another fill of the bytes no plane owns: nothing of them reaches a result
    buf2, tab2, _ = _mixed_addressed(fmt, 2)
    assert torch.equal(tab, tab2) and not np.array_equal(buf, buf2)
    _equal(_three(pipe, torch.from_numpy(buf2).cuda(), tab2), got, (fmt, "fill"))
    # collate_addressed_frames' own layout of the same clips (aligned pitches, planes on 64-byte boundaries, a (B, T, S) tensor)
    from mvfnet_amd.preprocess import collate_addressed_frames
    clips, tables, _ = _mixed()
    groups = [(Y.planes_to_packed(*c, 0, Y.BGR), t) for c, t in zip(clips, tables)] if fmt == "packed" else list(zip(clips, tables))
    fr, t16 = collate_addressed_frames(groups, fmt, pitch_align=32, fill=255)
    assert tuple(fr.shape[:2]) == (len(SIZES), TM)
    _equal(_three(pipe, fr.cuda(), t16.cuda()), got, (fmt, "collate"))


def test_a_table_the_host_check_refuses_is_never_launched():
    buf, tab, crop = _mixed_addressed("i420", 1)
    pipe, fr = _addressed("i420", 0, "bgr", crop), torch.from_numpy(buf).cuda()
    for col, value, word in ((11, -1, "negative offset"), (12, 40, "pitch below"), (14, buf.size, "ends past"), (15, 3, "pitch below")):
        bad = tab.clone()
        bad[5, col] = value
        with pytest.raises(ValueError, match="row 5.*" + word):
            pipe.to_nchw(fr, bad)
    with pytest.raises(ValueError, match="does not use"):
        _addressed("packed", 0, "bgr", crop).to_nchw(fr, tab)                             # an I420 table handed to the packed format
    with pytest.raises(ValueError, match="ends past"):
        pipe.to_nchw(fr[:-1], tab)                                                       # the buffer one byte short of the last plane
    bad = tab.clone()
    bad[0, 4] += 1                                                                       # the geometry is checked against the row's own hs_i x ws_i
    with pytest.raises(ValueError, match="row 0.*its own hs_i x ws_i frame"):
        pipe.to_nchw(fr, bad)
    with pytest.raises(ValueError, match="16 / 28 columns"):
        pipe.to_nchw(fr, tab[:, :11])
    torch.cuda.synchronize()


@pytest.mark.parametrize("fmt", ["packed", "nv12"])
def test_two_videos_of_different_size_and_frame_count_in_one_launch(fmt):
    """Video 1: 7 frames of 60 x 76, 3 clips of 4; video 2: 5 frames of 45 x 52, 2 clips of 4.  Each video's rows share its planes through
    address_rows(video_test_table(...), addr); one launch == the concatenation of the two dense launches."""
    from mvfnet_amd import preprocess as P
    crop, recipe = 24, dict(scale=(float("inf"), 32), crop_size=24)
    videos = []
    for k, (hs, ws, total, clips) in enumerate([(60, 76, 7, 3), (45, 52, 5, 2)]):
        inds = P.sample_frame_inds(total, 4, 2, clips, test_mode=True)
        distinct, table = P.video_test_table(inds, hs, ws, P.test_rows, **recipe)
        videos.append((Y.random_planes(len(distinct), hs, ws, 80 + k), table))
    assert videos[0][1].shape[0] != videos[1][1].shape[0] and videos[0][0][0].shape[0] != videos[1][0][0].shape[0]
    want = []
    for planes, table in videos:
        fr = torch.from_numpy(Y.planes_to_packed(*planes, 0, Y.BGR) if fmt == "packed" else Y.pack(*planes, Y.NV12)).cuda()
        want.append(_three(_dense(fmt, 0, "bgr", crop), fr, torch.from_numpy(table).cuda()))
    want = [torch.cat(w_) for w_ in zip(*want)]
    frames = [f for planes, _ in videos for f in _frames_of(fmt, planes)]
    buf, addr = A.pack(frames, FORMATS[fmt], pitches=_pitches(fmt, frames, False), gaps=7, fill_seed=3)
    n0 = videos[0][0][0].shape[0]
    table = np.concatenate([P.address_rows(videos[0][1], addr[:n0]), P.address_rows(videos[1][1], addr[n0:])])
    assert table.shape == (want[0].shape[0], 16)
    _equal(_three(_addressed(fmt, 0, "bgr", crop), torch.from_numpy(buf).cuda(), torch.from_numpy(table).cuda()), want, fmt)


# ---- end to end ---------------------------------------------------------------------------------------------------------------------------
def test_backbone_features_and_forward_test_from_addressed_frames_are_bit_equal_to_the_dense_gather_input():
    """test_yuv_gpu.py's small video (24 frames of 72 x 96, 4 overlapping clips of T = 4, Resize + ThreeCrop(64)) as (1, n_src, S) addressed
    frames: BackboneEngine's features and forward_test's scores == from the dense gather input, on one stream and on two (every chain gets
    the whole byte tensor and its slice of the table)."""
    from mvfnet_amd import preprocess as P
    T, total, hs, ws, c = 4, 24, 72, 96, 64
    inds = P.sample_frame_inds(total, T, 4, 4, test_mode=True)
    distinct, table = P.video_test_table(inds, hs, ws, P.test_rows, scale=(float("inf"), 80), crop_size=c)
    assert len(distinct) < len(inds) and table.shape == (48, 12)
    packed = np.random.RandomState(77).randint(0, 256, size=(len(distinct), hs, ws, 3)).astype(np.uint8)
    slots, per_src = P.collate_addressed_frames([(packed, P.resize_rows(hs, ws, len(distinct), (8, 8), keep_ratio=False))], "packed", pitch_align=64)
    assert tuple(slots.shape[:2]) == (1, len(distinct))
    atab = torch.from_numpy(P.address_rows(table, P.split_address_rows(per_src.numpy())[1])).cuda()
    assert tuple(atab.shape) == (48, 16)
    inputs = ((P.GatherFramePipeline(MEAN, STD, to_rgb=True, crop_size=c), torch.from_numpy(packed).cuda()[None], torch.from_numpy(table).cuda()),
              (P.AddressedFramePipeline(MEAN, STD, to_rgb=True, crop_size=c), slots.cuda(), atab))
    m = _r50(T, torch.bfloat16)
    m.eval()
    eng = m.backbone.engine()
    for streams in (1, 2):
        eng.streams = streams
        res = []
        for pipe, fr, tab in inputs:
            m.set_input_pipeline(pipe)
            eng = m.backbone.engine()
            eng.input_window = tab
            feat = eng.forward(fr[0]).clone()                                            # BackboneEngine on (frames, ...) + the table
            res.append((feat, m(fr, None, return_loss=False, window=tab)))
        m.set_input_pipeline(None)
        (f0, s0), (f1, s1) = res
        assert f0.shape[0] == 48 and torch.equal(f0.view(torch.int16), f1.view(torch.int16)), streams
        assert s0.shape == (12, 400) and np.isfinite(s0).all() and np.array_equal(s0, s1), streams


def test_one_training_step_on_a_portrait_and_landscape_batch_is_bit_equal_to_the_dense_padded_batch():
    """A (B, T, S) batch of a 72 x 96 and a 96 x 72 clip + the 28-column table (MultiScaleCrop -> Flip -> ColorJitter, address) == the same
    step on collate_jitter_frames' 96 x 96 padded batch, on an identical model: the loss, every gradient and every updated parameter.
    forward_train refuses an addressed table of B * T + 1 rows, and a 12-column gather table as before."""
    from mvfnet_amd import preprocess as P
    T, c = 4, 64
    shapes = [(72, 96), (96, 72)]
    clips = [np.random.RandomState(50 + k).randint(0, 256, size=(T, hh, ww, 3)).astype(np.uint8) for k, (hh, ww) in enumerate(shapes)]
    random.seed(11)
    np.random.seed(11)
    tables = [P.jitter_rows(P.multi_scale_crop_rows(hh, ww, T, input_size=c), P.color_jitter_table(T, color_space_aug=True)) for hh, ww in shapes]
    dense, tab = P.collate_jitter_frames(list(zip(clips, tables)))
    slots, atab = P.collate_addressed_frames(list(zip(clips, tables)), "packed", cols=23)
    assert tuple(dense.shape) == (2, T, 96, 96, 3) and tuple(slots.shape) == (2, T, 72 * 96 * 3) and tuple(atab.shape) == (2 * T, 28)
    assert torch.equal(atab[:, :23], tab)
    lab = torch.tensor([[5], [77]], device="cuda")
    res = []
    for pipe, fr, tb in ((P.JitterFramePipeline(MEAN, STD, to_rgb=True, crop_size=c), dense, tab),
                         (P.AddressedFramePipeline(MEAN, STD, to_rgb=True, crop_size=c), slots, atab)):
        m = _r50(T)
        m.train()
        m.cls_head.dropout = None
        m.set_input_pipeline(pipe)
        if tb is atab:
            with pytest.raises(ValueError, match="addressed table of %d rows" % (2 * T + 1)):
                m(fr.cuda(), lab, window=torch.cat([tb, tb[:1]]).cuda())
            m.set_input_pipeline(P.GatherFramePipeline(MEAN, STD, to_rgb=True, crop_size=c))
            with pytest.raises(ValueError, match="gather table"):
                m(dense.cuda(), lab, window=torch.from_numpy(P.gather_rows(tab[:, :11].numpy(), np.arange(2 * T))).cuda())
            m.set_input_pipeline(pipe)
        loss = m(fr.cuda(), lab, window=tb.cuda())["loss_cls"]
        loss.backward()
        grads = {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}
        m.train_engine().step()
        torch.cuda.synchronize()
        res.append((loss.detach().clone(), grads, {k: p.detach().clone() for k, p in m.named_parameters()}))
        del m
    (l0, g0, p0), (l1, g1, p1) = res
    assert torch.isfinite(l0).all() and torch.equal(l0, l1)
    assert g0.keys() == g1.keys() and len(g0) > 0 and p0.keys() == p1.keys()
    for k in g0:
        assert torch.equal(g0[k], g1[k]), k
    for k in p0:
        assert torch.equal(p0[k], p1[k]), k
