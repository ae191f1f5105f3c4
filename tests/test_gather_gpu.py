"""mvf_frames_gather_resample_u8 (several output images per decoded frame) bit for bit against the existing exports run on the gathered
batch frames[src], against the numpy restatement (tests/gather_numpy.py) on the reference's own test recipes
(tests/golden/gather_cases.npz), whole-video forward_test from a video's distinct frames against the replicated-frames path and the fp32
tensor path, and TSNClsHead(extract_feat=True) against the head kernel's pooled buffer.  Every comparison of the input path is
torch.equal / np.array_equal: the index adds no arithmetic."""
import ctypes as C
import os
import random

import numpy as np
import pytest
import torch

import gather_numpy as G
from helpers import rel_err

pytestmark = pytest.mark.gpu

MEAN, STD = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]
GOLD = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gather_cases.npz"))


def _frames(n, hs, ws, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(n, hs, ws, 3)).astype(np.uint8)


def _mixed_batch():
    """Five source frames of three real sizes in one 60 x 76 padded batch, 14 output images: a row per image describing ITS source
    frame (identity, 2x area, up, down resamples; flips; several images per frame, one frame unused, out of order)."""
    hs, ws, h, w = 60, 76, 20, 24
    sizes = [(60, 76), (48, 64), (60, 50), (44, 76), (60, 76)]
    fr = np.zeros((5, hs, ws, 3), dtype=np.uint8)
    for k, (a, b) in enumerate(sizes):
        fr[k, :a, :b] = _frames(1, a, b, 20 + k)[0]
    src = np.array([4, 0, 0, 1, 2, 2, 2, 4, 0, 1, 4, 2, 0, 1], dtype=np.int32)          # frame 3 is never read
    rows = []
    for i, s in enumerate(src):
        fh, fw = sizes[s]
        kind = i % 4
        if kind == 0:                                          # no resample: a window
            by, bx, bh, bw = i % 3, i % 5, fh - 4, fw - 6
            rh, rw = bh, bw
        elif kind == 1:                                        # exactly 2x down
            rh, rw = h + 1, w + 1
            by, bx, bh, bw = 1, 0, 2 * rh, 2 * rw
        elif kind == 2:                                        # up
            by, bx, bh, bw = 3, 1, 12, 15
            rh, rw = h + 7, w + 3
        else:                                                  # generic down of the whole frame
            by, bx, bh, bw = 0, 0, fh, fw
            rh, rw = h + 5, w + 9
        rows.append((fh, fw, by, bx, bh, bw, rh, rw, (rh - h) // 2, rw - w, i % 2))
    return fr, src, np.array(rows, dtype=np.int32), h, w


def _color(n, seed):
    from mvfnet_amd.preprocess import color_jitter_table
    random.seed(seed)
    np.random.seed(seed)
    return np.concatenate([color_jitter_table(1, color_space_aug=True) for _ in range(n)])


@pytest.mark.parametrize("with_color", [False, True], ids=["plain", "color"])
def test_gather_export_equals_the_existing_exports_on_the_gathered_frames(with_color):
    """fp32 NCHW, fp32 and bf16 stem operands: (a) src_index = NULL == mvf_frames_resample_color_u8; (b) a table == the existing export run
    on frames[src]; (c) the pipeline classes agree with the raw exports."""
    from mvfnet_amd._lib import check, lib
    from mvfnet_amd.preprocess import GatherFramePipeline, JitterFramePipeline, gather_rows, jitter_rows
    fr, src, rows, h, w = _mixed_batch()
    n_src, hs, ws = fr.shape[:3]
    n = len(src)
    color = _color(n, 5) if with_color else None
    fr_t, src_t, rows_t = torch.from_numpy(fr).cuda(), torch.from_numpy(src).cuda(), torch.from_numpy(rows).cuda()
    col_t = torch.from_numpy(color).cuda() if with_color else None
    gathered = fr_t[src_t.long()].contiguous()                                            # what the host would have had to build and ship
    assert gathered.shape[0] == n > n_src
    pipe = GatherFramePipeline(MEAN, STD, to_rgb=True, crop_size=(w, h))
    parent = JitterFramePipeline(MEAN, STD, to_rgb=True, crop_size=(w, h))
    st = torch.cuda.current_stream().cuda_stream
    cp = col_t.data_ptr() if with_color else None
    pad = 3
    wp = (w + 2 * pad + 2 + 1) // 2 * 2
    table = gather_rows(jitter_rows(rows, color) if with_color else rows, src)
    assert table.shape == (n, 24 if with_color else 12)
    table_t = torch.from_numpy(table).cuda()
    plain_t = torch.from_numpy(jitter_rows(rows, color)).cuda() if with_color else rows_t

    def outputs(dtype):
        return (torch.full((n, 3, h, w), 7.0, device="cuda") if dtype is None
                else torch.full((n, h + 2 * pad, wp, 4), 7.0, dtype=dtype, device="cuda"))

    for dtype in (None, torch.float32, torch.bfloat16):                                   # None: the fp32 NCHW output
        iv = torch.int32 if dtype in (None, torch.float32) else torch.int16
        dt = 1 if dtype == torch.bfloat16 else 0
        p_, wp_ = (0, w) if dtype is None else (pad, wp)

        def ptrs(o):
            return (None, o.data_ptr()) if dtype is None else (o.data_ptr(), None)
        want, got_null, got_idx = outputs(dtype), outputs(dtype), outputs(dtype)
        check(lib.mvf_frames_resample_color_u8(gathered.data_ptr(), n, hs, ws, rows_t.data_ptr(), cp, h, w, pipe.mean, pipe.std, 1, 0, p_, wp_,
                                               *ptrs(want), dt, st), "existing export")
        check(lib.mvf_frames_gather_resample_u8(gathered.data_ptr(), n, hs, ws, None, n, rows_t.data_ptr(), cp, h, w, pipe.mean, pipe.std, 1, 0,
                                                p_, wp_, *ptrs(got_null), dt, st), "gather, NULL index")
        check(lib.mvf_frames_gather_resample_u8(fr_t.data_ptr(), n_src, hs, ws, src_t.data_ptr(), n, rows_t.data_ptr(), cp, h, w, pipe.mean,
                                                pipe.std, 1, 0, p_, wp_, *ptrs(got_idx), dt, st), "gather")
        assert torch.equal(got_null.view(iv), want.view(iv)), dtype
        assert torch.equal(got_idx.view(iv), want.view(iv)), dtype
        if not with_color:                                                                # and the colourless export
            base = outputs(dtype)
            check(lib.mvf_frames_resample_u8(gathered.data_ptr(), n, hs, ws, rows_t.data_ptr(), h, w, pipe.mean, pipe.std, 1, 0, p_, wp_, *ptrs(base),
                                             dt, st), "resample_u8")
            assert torch.equal(got_idx.view(iv), base.view(iv)), dtype
        # the classes: gather table on the distinct frames == the parent class on the gathered frames == pass-through of the plain table
        if dtype is None:
            a, b, c_ = pipe.to_nchw(fr_t, table_t), parent.to_nchw(gathered, plain_t), pipe.to_nchw(gathered, plain_t)
        else:
            a, b, c_ = (pipe.to_stem(fr_t, table_t, pad, wp, dtype), parent.to_stem(gathered, plain_t, pad, wp, dtype),
                        pipe.to_stem(gathered, plain_t, pad, wp, dtype))
        assert tuple(a.shape) == tuple(want.shape)
        for t in (a, b, c_):
            assert torch.equal(t.view(iv), want.view(iv)), dtype


def test_mixed_batch_equals_the_numpy_restatement():
    from mvfnet_amd.preprocess import GatherFramePipeline, gather_rows, jitter_rows
    fr, src, rows, h, w = _mixed_batch()
    color = _color(len(src), 9)
    pipe = GatherFramePipeline(MEAN, STD, to_rgb=True, crop_size=(w, h))
    got = pipe.to_nchw(torch.from_numpy(fr).cuda(), torch.from_numpy(gather_rows(jitter_rows(rows, color), src)).cuda()).cpu().numpy()
    want = G.frames_to_nchw(fr, src, rows, color, h, w, MEAN, STD)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    got = pipe.to_nchw(torch.from_numpy(fr).cuda(), torch.from_numpy(gather_rows(rows, src)).cuda()).cpu().numpy()
    assert np.array_equal(got.view(np.int32), G.frames_to_nchw(fr, src, rows, None, h, w, MEAN, STD).view(np.int32))


@pytest.mark.parametrize("k", range(GOLD["gc_args"].shape[0]))
def test_golden_recipes_from_distinct_frames_equal_the_numpy_restatement(k):
    """The reference's test recipes (SampleFrames + Resize + ThreeCrop / TenCrop / CenterCrop, tests/golden/make_gather_golden.py): the
    kernel fed the video's DISTINCT frames + video_test_table == the numpy restatement fed one frame per sampled index, repeats included."""
    from mvfnet_amd import preprocess as P
    total, clip_len, interval, num_clips, sth, H, W, recipe, short, cw, ch = (int(v) for v in GOLD["gc_args"][k])
    inds = GOLD["gc_inds"][GOLD["gc_inds_off"][k]:GOLD["gc_inds_off"][k + 1]]
    scale = (float("inf"), short)
    fn, kw = {0: (P.test_rows, dict(scale=scale, crop_size=(cw, ch))), 1: (P.val_rows, dict(scale=scale, crop_size=(cw, ch))),
              2: (P.ten_crop_rows, dict(crop_size=(cw, ch))), 3: (P.ten_crop_rows, dict(crop_size=(cw, ch), scale=scale)),
              4: (P.center_crop_rows, dict(crop_size=(cw, ch)))}[recipe]
    distinct, table = P.video_test_table(inds, H, W, fn, **kw)
    decoded = _frames(len(distinct), H, W, 100 + k)            # the video's distinct frames, as decoded
    pipe = P.GatherFramePipeline(MEAN, STD, to_rgb=True, crop_size=(cw, ch))
    got = pipe.to_nchw(torch.from_numpy(decoded).cuda(), torch.from_numpy(table).cuda()).cpu().numpy()
    rows, src = P.split_gather_rows(table)
    crops = len(rows) // len(inds)
    assert got.shape == (crops * len(inds), 3, ch, cw)
    # the restatement never sees the index: it gets the reference's img_group, one decoded frame per sampled index, once per crop
    position = {int(f): i for i, f in enumerate(distinct)}
    per_index = np.stack([decoded[position[int(f)]] for f in inds])
    want = G.frames_to_nchw(np.concatenate([per_index] * crops), None, rows, None, ch, cw, MEAN, STD)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))


def test_gather_pipeline_rejects_bad_tables():
    """No bad index and no out-of-range row ever reaches a launch."""
    from mvfnet_amd.preprocess import GatherFramePipeline, gather_rows
    pipe = GatherFramePipeline(MEAN, STD, crop_size=16)
    fr = torch.zeros(2, 20, 24, 3, dtype=torch.uint8, device="cuda")
    good = np.array([[20, 24, 0, 0, 20, 24, 32, 32, 0, 0, 0]] * 5, dtype=np.int32)
    tab = gather_rows(good, [0, 1, 1, 0, 1])
    assert pipe.to_nchw(fr, torch.from_numpy(tab)).shape == (5, 3, 16, 16)
    assert pipe.n_out(fr, torch.from_numpy(tab)) == 5
    for v in (-1, 2, 7):                                                                          # src outside [0, n_src)
        bad = tab.copy()
        bad[3, -1] = v
        with pytest.raises(ValueError, match="source frame"):
            pipe.to_nchw(fr, torch.from_numpy(bad))
    with pytest.raises(ValueError, match="columns"):
        pipe.to_nchw(fr, torch.from_numpy(tab[:, :10].copy()))                                    # 10 columns
    with pytest.raises(ValueError, match="columns"):
        pipe.to_nchw(fr, torch.from_numpy(np.concatenate([tab, tab[:, :1]], axis=1)))             # 13 columns
    with pytest.raises(ValueError):
        pipe.to_nchw(fr, None)
    for col, v in [(0, 21), (1, 25), (2, 1), (4, 0), (8, 17), (10, 2)]:                           # the patch leaves frame src's padded extent, ...
        bad = tab.copy()
        bad[2, col] = v
        with pytest.raises(ValueError, match="patch must lie"):
            pipe.to_nchw(fr, torch.from_numpy(bad))
    with pytest.raises(ValueError, match="output buffer"):
        pipe.to_stem(fr, torch.from_numpy(tab), 3, 24, torch.float32, out=torch.empty(2, 22, 24, 4, device="cuda"))
    with pytest.raises(ValueError, match="rows for"):                                # 11 columns = no gather: one row per frame
        pipe.to_nchw(fr, torch.from_numpy(good))
    torch.cuda.synchronize()


# ---- end to end -------------------------------------------------------------------------------------------------------------------------
def _r50(T, dtype=torch.float32, fcn=False, extract_feat=False, test_cfg=None):
    import mvfnet_amd
    from mvfnet_amd import synth
    cfg = mvfnet_amd.mvfnet_config(50, T, fcn_testing=fcn)
    if extract_feat:
        cfg["cls_head"]["extract_feat"] = True
    m = mvfnet_amd.build_recognizer(cfg, None, test_cfg or dict(average_clips=None))
    sd = m.state_dict()
    vals = synth.synth_state_dict({"r50/" + k: tuple(v.shape) for k, v in sd.items()})
    m.load_state_dict({k: torch.from_numpy(vals["r50/" + k]) for k in sd}, strict=True)
    m.backbone.engine_dtype = dtype
    return m.cuda()


def _video_case(T):
    """A 24-frame 72 x 96 video, 4 clips of T=4 frames every 4th frame: the clips overlap (10 distinct frames of 16 sampled), the shipped
    test recipe scaled down (Resize((inf, 72)) = identity size here would hide the resample: 80), ThreeCrop(64) -> 48 images = 12 clips."""
    from mvfnet_amd.preprocess import sample_frame_inds, test_rows, video_test_table
    total, hs, ws, c = 24, 72, 96, 64
    video = _frames(total, hs, ws, 77)
    inds = sample_frame_inds(total, T, 4, 4, test_mode=True)
    recipe = dict(scale=(float("inf"), 80), crop_size=c)
    distinct, table = video_test_table(inds, hs, ws, test_rows, **recipe)
    assert len(inds) == 16 and len(distinct) < len(inds) and table.shape == (48, 12)
    replicated = np.concatenate([video[inds]] * 3)                                         # today: the host builds 48 frames out of 10
    return video[distinct], table, replicated, test_rows(hs, ws, len(inds), **recipe), c


@pytest.mark.parametrize("fcn", [False, True], ids=["fc", "fcn_testing"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_forward_test_from_distinct_frames_equals_replicated_frames_and_the_fp32_tensor_path(dtype, fcn):
    from mvfnet_amd.preprocess import GatherFramePipeline, ResamplingFramePipeline
    T = 4
    decoded, table, replicated, rows, c = _video_case(T)
    m = _r50(T, dtype, fcn)
    m.eval()
    dec_t, tab_t = torch.from_numpy(decoded).cuda()[None], torch.from_numpy(table).cuda()
    rep_t, rows_t = torch.from_numpy(replicated).cuda()[None], torch.from_numpy(rows).cuda()
    gather, today = GatherFramePipeline(MEAN, STD, to_rgb=True, crop_size=c), ResamplingFramePipeline(MEAN, STD, to_rgb=True, crop_size=c)
    x = today.to_nchw(rep_t, rows_t).view(1, 48, 3, c, c)
    assert torch.equal(gather.to_nchw(dec_t, tab_t).view(1, 48, 3, c, c), x)
    for streams in (1, 2):
        assert m.backbone.engine().dtype == dtype
        m.backbone.engine().streams = streams
        m.set_input_pipeline(None)
        want = m(x, None, return_loss=False)                                               # the fp32 tensor path
        m.set_input_pipeline(today)
        mid = m(rep_t, None, return_loss=False, window=rows_t)                             # replicated frames + today's test_rows
        m.set_input_pipeline(gather)
        got = m(dec_t, None, return_loss=False, window=tab_t)                              # distinct frames + the gather table
        same = m(rep_t, None, return_loss=False, window=rows_t)                            # 11 columns through the new class: no gather
        m.set_input_pipeline(None)
        assert want.shape == (12, 400) and np.isfinite(want).all()
        assert np.array_equal(mid, want), streams
        assert np.array_equal(got, want), streams
        assert np.array_equal(same, want), streams


def test_forward_train_refuses_a_gather_table():
    from mvfnet_amd.preprocess import GatherFramePipeline
    T = 4
    decoded, table, _, _, c = _video_case(T)
    m = _r50(T)
    m.train()
    m.set_input_pipeline(GatherFramePipeline(MEAN, STD, to_rgb=True, crop_size=c))
    with pytest.raises(ValueError, match="gather table"):
        m(torch.from_numpy(decoded).cuda()[None], torch.tensor([[3]], device="cuda"), window=torch.from_numpy(table).cuda())


@pytest.mark.parametrize("fcn", [False, True], ids=["fc", "fcn_testing"])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
def test_extract_feat_returns_the_head_kernels_pooled_buffer(dtype, fcn):
    """TSNClsHead(extract_feat=True) in eval mode: bit-equal to the `pooled` buffer mvf_head_pool_fc writes for the same backbone features,
    and within 1e-5 (helpers.rel_err: max |a - ref| / max |ref|) of the fp64 mean over (num_seg, h, w) of the stored features -- the bound
    tests/test_conv_gpu.py puts on the same kernel's mean (there followed by the FC) against torch's.  average_clips='score' on the
    features goes through mvf_average_clip with classes = in_channels, same bound."""
    from mvfnet_amd._lib import check, lib
    T, B, c = 4, 3, 64
    m = _r50(T, dtype, fcn, extract_feat=True)
    m.eval()
    x = torch.randn(B, T, 3, c, c, generator=torch.Generator().manual_seed(3)).cuda()
    got = m(x, None, return_loss=False, return_numpy=False)
    assert got.dtype == torch.float32 and tuple(got.shape) == (B, 2048)
    with torch.no_grad():
        feat = m.extract_feat(x.view(B * T, 3, c, c)).permute(0, 2, 3, 1).contiguous()    # (B*T, h, w, 2048) as stored
    assert feat.dtype == dtype
    nt, h, w, ch = feat.shape
    head = m.cls_head
    pooled, scores = torch.empty(B, ch, device="cuda"), torch.empty(B, head.num_classes, device="cuda")
    P = lambda t: C.c_void_p(t.data_ptr())      # noqa: E731
    check(lib.mvf_head_pool_fc(P(feat), B, T, h * w, ch, P(head.new_fc.weight.detach().contiguous()), P(head.new_fc.bias.detach().contiguous()),
                               head.num_classes, P(pooled), P(scores), 0 if dtype == torch.float32 else 1, None), "mvf_head_pool_fc")
    torch.cuda.synchronize()
    assert torch.equal(got, pooled)
    want = feat.double().view(B, T * h * w, ch).mean(1).cpu().numpy()
    e = rel_err(got.cpu().numpy(), want)
    print("extract_feat %s fcn=%s: rel_err to the fp64 mean %.3g" % (dtype, fcn, e))
    assert e < 1e-5
    m.test_cfg = dict(average_clips="score")
    avg = m(x, None, return_loss=False)
    assert avg.shape == (1, 2048)
    e = rel_err(avg, want.mean(0, keepdims=True))
    print("extract_feat %s fcn=%s: average_clips='score' rel_err %.3g" % (dtype, fcn, e))
    assert e < 1e-5
    m.train()
    with pytest.raises(NotImplementedError, match="eval-mode"):
        m(x, torch.zeros(B, 1, dtype=torch.long, device="cuda"))
