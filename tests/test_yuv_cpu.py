"""CPU: the YUV 4:2:0 frame input -- the integer conversion of include/mvfnet_hip.h against the rounded float definition over all 2^24
(Y, U, V) triples, collate_yuv_frames (layouts, odd sizes, pad_to), Yuv420FramePipeline's argument validation, and the C ABI of
mvf_frames_yuv420_gather_resample_u8 (header declaration, ctypes argtypes, host-side validation)."""
import ctypes
import os
import re

import numpy as np
import pytest

import yuv_numpy as Y

HERE = os.path.dirname(os.path.abspath(__file__))


def test_bt601_limited_constants_are_the_common_20_bit_ones():
    assert Y.constants(0) == (16, 1220542, 1673527, 852492, 409993, 2116026)


@pytest.mark.parametrize("standard", [0, 1, 2])
def test_integer_conversion_is_within_one_of_the_rounded_float_definition_for_every_triple(standard):
    """A condition, not a measurement: |integer - float| <= 1 for each of R, G, B over all 2^24 triples, and the int32 intermediates do
    not overflow (the largest magnitude, computed in int64, stays below 2^31)."""
    y_off, cy, cvr, cvg, cug, cub = Y.constants(standard)
    big = 255 * cy + (1 << 19) + 128 * max(cvr, cub, cvg + cug)
    assert big < (1 << 31), big
    u, v = np.meshgrid(np.arange(256), np.arange(256), indexing="ij")
    worst = 0
    for y in range(256):
        got = Y.convert(np.full_like(u, y), u, v, standard)
        want = Y.convert_float(np.full_like(u, y), u, v, standard)
        for a, b in zip(got, want):
            worst = max(worst, int(np.abs(a.astype(np.int32) - b.astype(np.int32)).max()))
    print("standard %d: largest |integer - float| = %d" % (standard, worst))
    assert worst <= 1


def test_to_packed_replicates_chroma_and_reads_both_layouts_alike():
    y, u, v = Y.random_planes(2, 6, 10, 3)
    for standard in (0, 1, 2):
        bgr = Y.planes_to_packed(y, u, v, standard, Y.BGR)
        assert bgr.shape == (2, 6, 10, 3) and bgr.dtype == np.uint8
        r, g, b = Y.convert(y[1, 3, 7], u[1, 1, 3], v[1, 1, 3], standard)
        assert tuple(bgr[1, 3, 7]) == (b, g, r)
        assert np.array_equal(Y.planes_to_packed(y, u, v, standard, Y.RGB), bgr[..., ::-1])
        for layout in (Y.I420, Y.NV12):
            for pitch in (10, 16):
                buf = Y.pack(y, u, v, layout, pitch=pitch, fill_seed=5)
                assert buf.shape == (2, 9, pitch)
                assert np.array_equal(Y.to_packed(buf, layout, standard, Y.BGR, width=10), bgr)
    # the layouts themselves: I420 = Y rows, the U plane, the V plane in rows of pitch / 2; NV12 = Y rows, interleaved U, V rows
    i420, nv12 = Y.pack(y, u, v, Y.I420), Y.pack(y, u, v, Y.NV12)
    assert np.array_equal(i420[:, :6], y) and np.array_equal(nv12[:, :6], y)
    assert np.array_equal(i420[0].reshape(-1)[60:75], u[0].reshape(-1)) and np.array_equal(i420[0].reshape(-1)[75:], v[0].reshape(-1))
    assert np.array_equal(nv12[0, 6:, 0::2], u[0]) and np.array_equal(nv12[0, 6:, 1::2], v[0])


def test_collate_yuv_frames_layouts_odd_sizes_and_pad_to():
    from mvfnet_amd import preprocess as P
    T = 2
    a, b = Y.random_planes(T, 12, 20, 1), Y.random_planes(T, 9, 13, 2)                 # an even clip and an odd-sized one (chroma 5 x 7)
    ra, rb = P.resize_rows(12, 20, T, (8, 8), keep_ratio=False), P.resize_rows(9, 13, T, (8, 8), keep_ratio=False)
    for name, layout in (("i420", Y.I420), ("nv12", Y.NV12)):
        fr, rows = P.collate_yuv_frames([(a, ra), (b, rb)], name)
        assert tuple(fr.shape) == (2, T, 18, 20) and str(fr.dtype) == "torch.uint8" and tuple(rows.shape) == (2 * T, 11)
        assert np.array_equal(rows.numpy(), np.concatenate([ra, rb]))
        assert np.array_equal(fr[0].numpy(), Y.pack(*a, layout))
        assert np.array_equal(fr[1].numpy(), Y.pack(*b, layout, pitch=20, hs=12))
        # the frames the buffers stand for: each clip's own, inside its (hs_i, ws_i)
        assert np.array_equal(Y.to_packed(fr[1].numpy(), layout, width=20)[:, :9, :13], Y.planes_to_packed(*b))
        # pad_to: rounded up to even; an I420 array (T, 3 h / 2, w) is taken as a clip
        fr2, _ = P.collate_yuv_frames([(Y.pack(*a, Y.I420), ra), (b, rb)], name, pad_to=(13, 21))
        assert tuple(fr2.shape) == (2, T, 21, 22)
        assert np.array_equal(fr2[0].numpy(), Y.pack(*a, layout, pitch=22, hs=14))
        assert np.array_equal(fr2[1].numpy(), Y.pack(*b, layout, pitch=22, hs=14))
        with pytest.raises(ValueError, match="larger than pad_to"):
            P.collate_yuv_frames([(a, ra), (b, rb)], name, pad_to=(12, 18))
    fr, rows = P.collate_yuv_frames([(b, rb)], "nv12")                                  # an odd clip alone: 10 x 14 planes
    assert tuple(fr.shape) == (1, T, 15, 14)
    jr = P.jitter_rows(rb)
    assert tuple(P.collate_yuv_frames([(b, jr)], 0, cols=23)[1].shape) == (T, 23)
    with pytest.raises(ValueError, match="no clips"):
        P.collate_yuv_frames([], "i420")
    with pytest.raises(ValueError, match="layout"):
        P.collate_yuv_frames([(a, ra)], "yv12")
    with pytest.raises(ValueError, match="rows do not describe"):
        P.collate_yuv_frames([(a, rb)], "i420")
    with pytest.raises(ValueError, match="T=2 frames"):
        P.collate_yuv_frames([(a, ra), (Y.random_planes(3, 12, 20, 1), np.concatenate([ra, ra[:1]]))], "i420")
    with pytest.raises(ValueError, match="chroma planes"):
        P.collate_yuv_frames([((b[0], b[1][:, :4], b[2]), rb)], "i420")
    with pytest.raises(ValueError, match="I420 clip"):
        P.collate_yuv_frames([(np.zeros((T, 10, 20), dtype=np.uint8), ra)], "i420")


def test_pipeline_argument_validation_needs_no_gpu():
    import torch
    from mvfnet_amd import preprocess as P
    pipe = P.Yuv420FramePipeline(crop_size=32)
    assert isinstance(pipe, P.GatherFramePipeline) and pipe.crop_hw == (32, 32)
    assert (pipe.layout, pipe.standard, pipe.order, pipe.pitch, pipe.frame_dims) == (0, 0, 0, None, 2)
    pipe = P.Yuv420FramePipeline([0, 0, 0], [1, 1, 1], to_rgb=False, crop_size=(24, 20), layout="nv12", standard="bt709", order="rgb", pitch=96, width=76)
    assert (pipe.layout, pipe.standard, pipe.order, pipe.pitch, pipe.width, pipe.crop_hw) == (1, 2, 1, 96, 76, (20, 24))
    assert P.Yuv420FramePipeline(standard="bt601-full").standard == 1 and P.Yuv420FramePipeline(layout=1, order=1).layout == 1
    for kw in (dict(layout="yv12"), dict(layout=2), dict(standard=3), dict(standard="bt2020"), dict(order="gbr"), dict(order=-1), dict(order=True),
               dict(pitch=75), dict(pitch=64, width=66), dict(width=0)):
        with pytest.raises(ValueError):
            P.Yuv420FramePipeline(**kw)
    # n_out / gathers: frames are (..., 3 * Hs / 2, pitch), so the frame count is the product of all but the last TWO dimensions
    pipe = P.Yuv420FramePipeline(crop_size=32)
    inds = P.sample_frame_inds(40, 8, 2, 4, test_mode=True)
    distinct, table = P.video_test_table(inds, 48, 64, P.test_rows, scale=(float("inf"), 32), crop_size=32)
    frames = np.zeros((1, len(distinct), 72, 64), dtype=np.uint8)
    assert pipe.gathers(table) and pipe.n_out(frames, table) == 3 * inds.size
    rows, _ = P.split_gather_rows(table)
    assert not pipe.gathers(rows) and pipe.n_out(frames, rows) == len(distinct) and pipe.n_out(frames, None) == len(distinct)
    # the frame tensor is checked before anything touches the device
    with pytest.raises(TypeError, match="CUDA uint8"):
        pipe.to_nchw(torch.zeros(2, 72, 64, dtype=torch.uint8), rows)
    with pytest.raises(TypeError, match="CUDA uint8"):
        pipe.to_nchw(torch.zeros(2, 72, 64), rows)


def test_every_pipeline_class_shares_one_to_nchw_and_one_to_stem():
    """One run path per ladder: no subclass redefines the pair, so a new layer cannot quietly fork them again."""
    from mvfnet_amd import preprocess as P
    for cls in (P.ResamplingFramePipeline, P.JitterFramePipeline, P.GatherFramePipeline, P.Yuv420FramePipeline):
        assert cls.to_nchw is P.FramePipeline.to_nchw and cls.to_stem is P.FramePipeline.to_stem and cls._run is P.FramePipeline._run
    assert (P.FramePipeline.frame_dims, P.GatherFramePipeline.frame_dims, P.Yuv420FramePipeline.frame_dims) == (3, 3, 2)


def _prototype(name):
    src = open(os.path.join(os.path.dirname(HERE), "include", "mvfnet_hip.h")).read()
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, src)
    assert m, "%s is not declared in include/mvfnet_hip.h" % name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_declares_the_yuv_export_with_matching_argtypes():
    from mvfnet_amd import _lib
    assert "mvf_frames_yuv420_gather_resample_u8" in _lib.declared_symbols()
    params = _prototype("mvf_frames_yuv420_gather_resample_u8")
    fn = _lib.lib.mvf_frames_yuv420_gather_resample_u8
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == len(params) == 24
    fptr = ctypes.POINTER(ctypes.c_float)
    for p, t in zip(params, fn.argtypes):
        if p in ("const float* mean3", "const float* std3"):
            assert t is fptr, p
        elif "*" in p:
            assert t is ctypes.c_void_p, p
        else:
            assert p.startswith("int ") and t is ctypes.c_int, p
    # the YUV export = the gather export + (pitch, layout, standard, order), everything else in the same order
    gather = [("const unsigned char* frames" if p == "const unsigned char* frames_hwc" else p) for p in _prototype("mvf_frames_gather_resample_u8")]
    assert [p for p in params if p not in ("int pitch", "int layout", "int standard", "int order")] == gather


def test_yuv_export_validates_scalars_without_a_gpu():
    """Every refusal below happens on the host side of the export, before any HIP call (the pointers are never dereferenced)."""
    from mvfnet_amd import _lib
    lib = _lib.lib
    mean, std = (ctypes.c_float * 3)(1, 2, 3), (ctypes.c_float * 3)(1, 1, 1)
    buf = ctypes.create_string_buffer(64)
    ptr = ctypes.addressof(buf)

    def call(frames=ptr, n_src=2, hs=20, ws=24, pitch=24, layout=0, standard=0, order=0, src=ptr, n_out=6, rows=ptr, h=16, w=16, std3=std, pad=3,
             wp=24, dt=0):
        return lib.mvf_frames_yuv420_gather_resample_u8(frames, n_src, hs, ws, pitch, layout, standard, order, src, n_out, rows, None, h, w, mean,
                                                        std3, 1, 0, pad, wp, ptr, None, dt, None)
    for kw, word in [(dict(hs=21), b"hs=21"), (dict(hs=0), b"hs=0"), (dict(ws=0), b"hs=20"), (dict(pitch=25, ws=23), b"pitch=25"),
                     (dict(pitch=22), b"pitch=22"), (dict(layout=2), b"layout 2"), (dict(layout=-1), b"layout -1"),
                     (dict(standard=3), b"standard 3"), (dict(standard=-1), b"standard -1"), (dict(order=2), b"order 2"),
                     (dict(frames=None), b"bad argument"), (dict(rows=None), b"bad argument"), (dict(n_src=0), b"bad argument"),
                     (dict(n_out=0), b"bad argument"), (dict(h=0), b"bad argument"), (dict(pad=-1), b"bad argument"),
                     (dict(src=None), b"n_src=2 != n_out=6"), (dict(wp=21), b"wp=21"), (dict(dt=5), b"bad dtype"),
                     (dict(std3=(ctypes.c_float * 3)(1, 0, 1)), b"std[1] is zero")]:
        assert call(**kw) == -1, kw                                                               # MVF_EINVAL
        msg = lib.mvf_last_error()
        assert b"frames_yuv420_gather_resample_u8" in msg and word in msg, (kw, msg)
