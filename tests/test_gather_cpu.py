"""CPU: whole-video testing from a video's distinct frames -- video_test_table against what the reference's SampleFrames + Resize +
ThreeCrop / TenCrop / CenterCrop returned on index-coded images (tests/golden/make_gather_golden.py), the gather_rows / split_gather_rows
pair, and the C ABI of mvf_frames_gather_resample_u8 (header declaration, ctypes argtypes, host-side argument validation)."""
import ctypes
import os
import re

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLD = np.load(os.path.join(HERE, "golden", "gather_cases.npz"))
N_CASES = GOLD["gc_args"].shape[0]


def _recipe(P, recipe, short, crop):
    scale = (float("inf"), int(short))
    crop = (int(crop[0]), int(crop[1]))
    return {0: (P.test_rows, dict(scale=scale, crop_size=crop)), 1: (P.val_rows, dict(scale=scale, crop_size=crop)),
            2: (P.ten_crop_rows, dict(crop_size=crop)), 3: (P.ten_crop_rows, dict(crop_size=crop, scale=scale)),
            4: (P.center_crop_rows, dict(crop_size=crop))}[int(recipe)]


@pytest.mark.parametrize("k", range(N_CASES))
def test_video_test_table_reproduces_the_reference_source_frame_box_and_order(k):
    from mvfnet_amd import preprocess as P
    total, clip_len, interval, num_clips, sth, H, W, recipe, short, cw, ch = (int(v) for v in GOLD["gc_args"][k])
    want_inds = GOLD["gc_inds"][GOLD["gc_inds_off"][k]:GOLD["gc_inds_off"][k + 1]]
    want = GOLD["gc_out"][GOLD["gc_out_off"][k]:GOLD["gc_out_off"][k + 1]]
    inds = P.sample_frame_inds(total, clip_len, interval, num_clips, test_mode=True, sth_samples=sth)
    assert np.array_equal(inds, want_inds)
    fn, kw = _recipe(P, recipe, short, (cw, ch))
    distinct, table = P.video_test_table(inds, H, W, fn, **kw)
    assert np.array_equal(distinct, np.unique(want_inds)) and distinct.dtype == want_inds.dtype
    assert table.dtype == np.int32 and table.shape == (want.shape[0], 12)
    rows, src = P.split_gather_rows(table)
    assert np.array_equal(distinct[src], want[:, 0])                                             # the source frame, in the reference's order
    assert np.array_equal(rows[:, :6], np.tile([H, W, 0, 0, H, W], (len(rows), 1)))              # the whole frame is resized
    assert np.array_equal(rows[:, 6:8], want[:, 7:9])                                            # (rh, rw)
    mirrored = (want[:, 3] < want[:, 2]).astype(np.int64)
    assert np.array_equal(rows[:, 10], mirrored)
    left = np.where(mirrored == 1, want[:, 3], want[:, 2])                                       # a mirrored crop's box starts at its right pixel
    assert np.array_equal(rows[:, 8], want[:, 1]) and np.array_equal(rows[:, 9], left)           # (oy, ox)
    assert np.array_equal(want[:, 4] - want[:, 1] + 1, np.full(len(rows), ch)) and np.array_equal(want[:, 5:7], np.tile([ch, cw], (len(rows), 1)))
    # reshaping to (-1, clip_len) yields clips of ONE crop over consecutive sampled frames
    per = want_inds.size
    assert np.array_equal(distinct[src].reshape(-1, per), np.tile(want_inds, (len(rows) // per, 1)))
    if recipe in (2, 3):
        assert mirrored.sum() * 2 == len(rows)


def test_the_golden_cases_cover_shared_and_clamped_frames_and_the_shipped_recipe():
    a = GOLD["gc_args"]
    assert any(tuple(r[:8]) == (300, 8, 8, 10, 1, 256, 340, 0) for r in a.tolist())              # configs/MVFNet/K400 test recipe: 80 -> 240
    k = [tuple(r[:8]) for r in a.tolist()].index((300, 8, 8, 10, 1, 256, 340, 0))
    assert GOLD["gc_out_off"][k + 1] - GOLD["gc_out_off"][k] == 240
    shared = clamped = 0
    for k in range(N_CASES):
        inds = GOLD["gc_inds"][GOLD["gc_inds_off"][k]:GOLD["gc_inds_off"][k + 1]]
        shared += int(np.unique(inds).size < inds.size)
        clamped += int((inds == a[k, 0] - 1).sum() > 1)
    assert shared >= 3 and clamped >= 2
    assert {1, 2} <= set(a[:, 4].tolist()) and {0, 1, 2, 3, 4} <= set(a[:, 7].tolist())


def test_gather_rows_round_trip_and_errors():
    from mvfnet_amd import preprocess as P
    rows = P.test_rows(48, 64, 4, scale=(float("inf"), 32), crop_size=32)
    src = np.array([0, 1, 1, 2] * 3)
    t = P.gather_rows(rows, src)
    assert t.shape == (12, 12) and t.dtype == np.int32
    r, s = P.split_gather_rows(t)
    assert np.array_equal(r, rows) and np.array_equal(s, src) and s.dtype == np.int32
    j = P.jitter_rows(rows, P.color_jitter_table(12))
    t24 = P.gather_rows(j, src)
    assert t24.shape == (12, 24)
    r, s = P.split_gather_rows(t24)
    assert np.array_equal(r, j) and np.array_equal(s, src)
    with pytest.raises(ValueError, match="columns"):
        P.gather_rows(rows[:, :10], src)
    with pytest.raises(ValueError, match="source indices for"):
        P.gather_rows(rows, src[:5])
    with pytest.raises(ValueError, match="non-negative"):
        P.gather_rows(rows, -src)
    with pytest.raises(ValueError, match="columns"):
        P.split_gather_rows(rows)
    with pytest.raises(ValueError, match="no frame indices"):
        P.video_test_table([], 48, 64)


def test_pipeline_n_out_and_gathers_need_no_gpu():
    from mvfnet_amd import preprocess as P
    pipe = P.GatherFramePipeline(crop_size=32)
    assert isinstance(pipe, P.JitterFramePipeline) and pipe.crop_hw == (32, 32)
    inds = P.sample_frame_inds(40, 8, 2, 4, test_mode=True)
    distinct, table = P.video_test_table(inds, 48, 64, P.test_rows, scale=(float("inf"), 32), crop_size=32)
    frames = np.zeros((len(distinct), 48, 64, 3), dtype=np.uint8)
    assert len(distinct) < inds.size
    assert pipe.gathers(table) and pipe.n_out(frames, table) == 3 * inds.size
    rows, _ = P.split_gather_rows(table)
    assert not pipe.gathers(rows) and pipe.n_out(frames, rows) == len(distinct)
    assert not pipe.gathers(P.jitter_rows(rows)) and not pipe.gathers(None) and pipe.n_out(frames, None) == len(distinct)


def _prototype(name):
    src = open(os.path.join(os.path.dirname(HERE), "include", "mvfnet_hip.h")).read()
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, src)
    assert m, "%s is not declared in include/mvfnet_hip.h" % name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_declares_the_gather_export_with_matching_argtypes():
    from mvfnet_amd import _lib
    assert "mvf_frames_gather_resample_u8" in _lib.declared_symbols()
    params = _prototype("mvf_frames_gather_resample_u8")
    fn = _lib.lib.mvf_frames_gather_resample_u8
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == len(params) == 20
    fptr = ctypes.POINTER(ctypes.c_float)
    for p, t in zip(params, fn.argtypes):
        if p in ("const float* mean3", "const float* std3"):
            assert t is fptr, p
        elif "*" in p:
            assert t is ctypes.c_void_p, p
        else:
            assert p.startswith("int ") and t is ctypes.c_int, p
    # the gather export = the colour export + (src_index, n_out), everything else in the same order
    color = [p for p in _prototype("mvf_frames_resample_color_u8")]
    assert [p for p in params if p not in ("const int* src_index", "int n_out")] == [("int n_src" if p == "int n" else p) for p in color]


def test_gather_export_validates_scalars_without_a_gpu():
    """Every refusal below happens on the host side of the export, before any HIP call (the pointers are never dereferenced)."""
    from mvfnet_amd import _lib
    lib = _lib.lib
    mean, std = (ctypes.c_float * 3)(1, 2, 3), (ctypes.c_float * 3)(1, 1, 1)
    buf = ctypes.create_string_buffer(64)
    ptr = ctypes.addressof(buf)

    def call(frames=ptr, n_src=2, src=ptr, n_out=6, rows=ptr, h=16, w=16, std3=std, pad=3, wp=24, dt=0):
        return lib.mvf_frames_gather_resample_u8(frames, n_src, 20, 24, src, n_out, rows, None, h, w, mean, std3, 1, 0, pad, wp, ptr, None, dt, None)
    for kw, word in [(dict(frames=None), b"bad argument"), (dict(rows=None), b"bad argument"), (dict(n_src=0), b"bad argument"),
                     (dict(n_out=0), b"bad argument"), (dict(h=0), b"bad argument"), (dict(pad=-1), b"bad argument"),
                     (dict(src=None), b"n_src=2 != n_out=6"), (dict(wp=21), b"wp=21"), (dict(dt=5), b"bad dtype"),
                     (dict(std3=(ctypes.c_float * 3)(1, 0, 1)), b"std[1] is zero")]:
        assert call(**kw) == -1, kw                                                               # MVF_EINVAL
        msg = lib.mvf_last_error()
        assert b"frames_gather_resample_u8" in msg and word in msg, (kw, msg)


def test_extract_feat_head_is_built_and_refuses_what_is_not():
    import torch
    from mvfnet_amd.heads import TSNClsHead
    h = TSNClsHead(in_channels=64, num_classes=5, extract_feat=True)
    assert h.extract_feat
    with pytest.raises(NotImplementedError, match="eval-mode"):                                   # a fresh module is in training mode
        h(torch.zeros(4, 64, 2, 2), 4)
    h.eval()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        h(torch.zeros(4, 64, 2, 2), 4)
    for kw in (dict(with_avg_pool=True), dict(temporal_feature_size=2), dict(spatial_feature_size=7)):
        with pytest.raises(NotImplementedError):
            TSNClsHead(in_channels=64, num_classes=5, extract_feat=True, **kw)
