"""CPU: the addressed frame input -- collate_addressed_frames against tests/addressed_numpy.py's byte-by-byte reading (formats, odd sizes,
both orientations, alignments, slot_bytes), address_rows / split_address_rows, check_addresses' refusals, AddressedFramePipeline's
argument validation, and the C ABI of mvf_frames_addressed_resample_u8 (header declaration, ctypes argtypes, host-side validation)."""
import ctypes
import os
import re

import numpy as np
import pytest

import addressed_numpy as A
import yuv_numpy as Y

HERE = os.path.dirname(os.path.abspath(__file__))
FORMATS = {"packed": A.PACKED, "i420": A.I420, "nv12": A.NV12}
T = 2
SIZES = [(60, 76), (76, 60), (59, 75), (45, 52)]              # landscape, portrait, two odd sizes


def _clip(fmt, h, w, seed):
    """One clip of T frames in the form collate_addressed_frames takes: (T, h, w, 3) packed, or (Y, U, V) planes."""
    if fmt == "packed":
        return np.random.RandomState(seed).randint(0, 256, size=(T, h, w, 3)).astype(np.uint8)
    return Y.random_planes(T, h, w, seed)


def _frames_of(fmt, clip):
    """The clip's frames one by one, in addressed_numpy's form."""
    if fmt == "packed":
        return [clip[t] for t in range(T)]
    return [tuple(p[t] for p in clip) for t in range(T)]


def _same(fmt, got, want):
    if fmt == "packed":
        return np.array_equal(got, want)
    return all(np.array_equal(g, w) for g, w in zip(got, want))


def _row_bytes(fmt, w):
    """(luma / packed row bytes, chroma row bytes)."""
    cw = (w + 1) // 2
    return {"packed": (3 * w, 0), "i420": (w, cw), "nv12": (w, 2 * cw)}[fmt]


@pytest.mark.parametrize("pitch_align", [1, 32])
@pytest.mark.parametrize("fmt", ["packed", "i420", "nv12"])
def test_collate_addressed_frames_round_trips_through_unpack(fmt, pitch_align):
    from mvfnet_amd import preprocess as P
    clips = [_clip(fmt, h, w, 10 + k) for k, (h, w) in enumerate(SIZES)]
    rows = [P.resize_rows(h, w, T, (8, 8), keep_ratio=False) for h, w in SIZES]
    fr, table = P.collate_addressed_frames(list(zip(clips, rows)), fmt, pitch_align=pitch_align, fill=7)
    B = len(SIZES)
    assert fr.dim() == 3 and tuple(fr.shape[:2]) == (B, T) and str(fr.dtype) == "torch.uint8"
    assert tuple(table.shape) == (B * T, 11 + P.ADDR_COLS) and str(table.dtype) == "torch.int32"
    geo, addr = P.split_address_rows(table.numpy())
    assert np.array_equal(geo, np.concatenate(rows))
    sizes = [hw for hw in SIZES for _ in range(T)]
    got = A.unpack(fr.numpy(), addr, sizes, FORMATS[fmt])
    want = [f for c in clips for f in _frames_of(fmt, c)]
    assert len(got) == len(want) == B * T
    for k, (g, w_) in enumerate(zip(got, want)):
        assert _same(fmt, g, w_), k
    # every frame in its own slot, at its own pitch: the row bytes rounded up to pitch_align; planes on 64-byte boundaries
    S = fr.shape[2]
    for k, ((h, w), a) in enumerate(zip(sizes, addr)):
        rb0, rb1 = _row_bytes(fmt, w)
        assert a[1] == -(-rb0 // pitch_align) * pitch_align and a[4] == -(-rb1 // pitch_align) * pitch_align, (k, a)
        assert k * S <= a[0] < (k + 1) * S and a[0] % 64 == 0 and a[2] % 64 == 0 and a[3] % 64 == 0, (k, a)
    assert S % 64 == 0
    P.check_addresses(geo, addr, fmt, fr.numel())                                      # the collate's own output passes
    P.check_addresses(table[:, :11], table[:, 11:], FORMATS[fmt], fr.numel())          # CPU tensors and the format's number too
    # bytes no plane owns hold `fill`: zeroing every plane through the addresses leaves nothing else
    owned = np.zeros(fr.numel(), dtype=bool)
    for (h, w), (o0, p0, o1, o2, p1) in zip(sizes, addr.astype(np.int64)):
        rb0, rb1 = _row_bytes(fmt, w)
        for o, p, n, rb in [(o0, p0, h, rb0)] + ([(o1, p1, (h + 1) // 2, rb1)] if fmt != "packed" else []) + ([(o2, p1, (h + 1) // 2, rb1)] if fmt == "i420" else []):
            for y in range(n):
                assert not owned[o + y * p:o + y * p + rb].any()                        # planes do not overlap
                owned[o + y * p:o + y * p + rb] = True
    assert (fr.numpy().reshape(-1)[~owned] == 7).all()


@pytest.mark.parametrize("fmt", ["packed", "i420", "nv12"])
def test_slot_bytes_is_kept_and_a_larger_clip_is_refused(fmt):
    from mvfnet_amd import preprocess as P
    clips = [_clip(fmt, h, w, 20 + k) for k, (h, w) in enumerate(SIZES[2:])]
    rows = [P.resize_rows(h, w, T, (8, 8), keep_ratio=False) for h, w in SIZES[2:]]
    free, _ = P.collate_addressed_frames(list(zip(clips, rows)), fmt)
    slot = free.shape[2] + 1000
    fr, table = P.collate_addressed_frames(list(zip(clips, rows)), fmt, slot_bytes=slot)
    assert tuple(fr.shape) == (2, T, slot)
    geo, addr = P.split_address_rows(table.numpy())
    got = A.unpack(fr.numpy(), addr, [hw for hw in SIZES[2:] for _ in range(T)], FORMATS[fmt])
    for g, w_ in zip(got, [f for c in clips for f in _frames_of(fmt, c)]):
        assert _same(fmt, g, w_)
    assert (addr[:, 0] // slot == np.arange(2 * T)).all()
    P.collate_addressed_frames(list(zip(clips, rows)), fmt, slot_bytes=free.shape[2])  # exactly the largest frame's aligned bytes: fits
    with pytest.raises(ValueError, match="does not fit slot_bytes"):
        P.collate_addressed_frames(list(zip(clips, rows)), fmt, slot_bytes=free.shape[2] - 64)
    # a jitter table travels with its 23 columns; an I420 array is taken as a clip
    fr23, t23 = P.collate_addressed_frames([(clips[0], P.jitter_rows(rows[0]))], fmt, cols=23)
    assert tuple(t23.shape) == (T, 28)
    with pytest.raises(ValueError, match="no clips"):
        P.collate_addressed_frames([], fmt)
    with pytest.raises(ValueError, match="rows do not describe"):
        P.collate_addressed_frames([(clips[0], rows[1])], fmt)
    with pytest.raises(ValueError, match="format"):
        P.collate_addressed_frames(list(zip(clips, rows)), "yv12")


@pytest.mark.parametrize("fmt", ["packed", "i420", "nv12"])
def test_portrait_beside_landscape_costs_no_padding(fmt):
    """The issue's case at full size: a 256x454 clip beside a 454x256 one.  S is ONE frame's aligned byte count, below the dense
    collate's bounding-box frame."""
    from mvfnet_amd import preprocess as P
    shapes = [(256, 454), (454, 256)]
    clips = [_clip(fmt, h, w, 30 + k) for k, (h, w) in enumerate(shapes)]
    rows = [P.resize_rows(h, w, T, (8, 8), keep_ratio=False) for h, w in shapes]
    fr, _ = P.collate_addressed_frames(list(zip(clips, rows)), fmt)
    if fmt == "packed":
        one = 256 * 454 * 3
        dense, _ = P.collate_frames(list(zip(clips, rows)))
    else:
        one = 256 * 454                                                                # luma, then each chroma plane on a 64-byte boundary
        for _ in range(2 if fmt == "i420" else 1):
            one = -(-one // 64) * 64 + (128 * 227 if fmt == "i420" else 128 * 454)
        dense, _ = P.collate_yuv_frames(list(zip(clips, rows)), fmt)
    aligned = -(-one // 64) * 64
    dense_bytes = dense[0, 0].numel()
    print("%s: addressed slot %d bytes, one frame %d, dense per-frame %d (%.2fx)" % (fmt, fr.shape[2], one, dense_bytes, dense_bytes / fr.shape[2]))
    assert fr.shape[2] == aligned
    assert fr.shape[2] < dense_bytes
    assert dense_bytes == 454 * 454 * (3 if fmt == "packed" else 1.5)


def test_address_rows_round_trip_and_the_video_table():
    from mvfnet_amd import preprocess as P
    rng = np.random.RandomState(0)
    rows = P.val_rows(60, 76, 4, scale=(float("inf"), 40), crop_size=32)
    addr = rng.randint(0, 1 << 30, size=(4, 5)).astype(np.int32)
    for r in (rows, P.jitter_rows(rows, P.color_jitter_table(4, color_space_aug=True))):
        table = P.address_rows(r, addr)
        assert table.dtype == np.int32 and table.shape == (4, r.shape[1] + 5)
        back, a = P.split_address_rows(table)
        assert np.array_equal(back, r) and np.array_equal(a, addr)
    assert (P.ADDR_COLS, P.RESAMPLE_COLS + P.ADDR_COLS, P.JITTER_COLS + P.ADDR_COLS) == (5, 16, 28)
    # a gather table + one address row per SOURCE frame: src is replaced by addr[src]
    inds = P.sample_frame_inds(7, 4, 2, 3, test_mode=True)
    distinct, gtable = P.video_test_table(inds, 60, 76, P.test_rows, scale=(float("inf"), 40), crop_size=40)
    geo, src = P.split_gather_rows(gtable)
    per_src = rng.randint(0, 1 << 30, size=(len(distinct), 5)).astype(np.int32)
    table = P.address_rows(gtable, per_src)
    assert table.shape == (gtable.shape[0], 16) and len(distinct) < len(inds)
    g2, a2 = P.split_address_rows(table)
    assert np.array_equal(g2, geo) and np.array_equal(a2, per_src[src])
    t24 = P.gather_rows(P.jitter_rows(geo), src)
    assert np.array_equal(P.split_address_rows(P.address_rows(t24, per_src))[1], per_src[src])
    with pytest.raises(ValueError, match="address rows for"):
        P.address_rows(rows, addr[:3])
    with pytest.raises(ValueError, match="addressed frames"):
        P.address_rows(gtable, per_src[:-1])
    with pytest.raises(ValueError, match="columns"):
        P.address_rows(table, addr)
    with pytest.raises(ValueError, match="addr must be"):
        P.address_rows(rows, addr[:, :4])
    with pytest.raises(ValueError, match="fit int32"):
        P.address_rows(rows, addr.astype(np.int64) + (1 << 31))
    with pytest.raises(ValueError, match="16 or 28"):
        P.split_address_rows(gtable)


@pytest.mark.parametrize("fmt", ["packed", "i420", "nv12"])
def test_check_addresses_refuses_each_kind_of_bad_row(fmt):
    from mvfnet_amd import preprocess as P
    frames = [f for k, (h, w) in enumerate(SIZES) for f in _frames_of(fmt, _clip(fmt, h, w, 40 + k))[:1]]
    pitches = [(_row_bytes(fmt, w)[0] + 5, _row_bytes(fmt, w)[1] + 3) for _, w in SIZES]
    buf, addr = A.pack(frames, FORMATS[fmt], pitches=pitches, gaps=11, fill_seed=1)
    geo = np.array([(h, w, 0, 0, h, w, h, w, 0, 0, 0) for h, w in SIZES], dtype=np.int32)
    n = buf.size
    P.check_addresses(geo, addr, fmt, n)                          # the buffer ends with the last plane's last byte: tight
    used = {"packed": (0,), "i420": (0, 2, 3), "nv12": (0, 2)}[fmt]
    unused = [c for c in (2, 3, 4) if c not in used and not (c == 4 and fmt != "packed")]

    def bad(row, col, value, word, frames_bytes=n):
        a = addr.copy()
        a[row, col] = value
        with pytest.raises(ValueError, match=word) as e:
            P.check_addresses(geo, a, fmt, frames_bytes)
        assert "row %d" % row in str(e.value), str(e.value)
    for col in used:
        bad(2, col, -1, "negative offset")
    tight = buf.size
    rb0, rb1 = _row_bytes(fmt, SIZES[1][1])
    bad(1, 1, rb0 - 1, "pitch below")                               # one byte short
    P.check_addresses(geo[1:2], np.array([[0, rb0, 0, 0, 0]] if fmt == "packed" else [[0, rb0, 0, 0, rb1]], dtype=np.int32), fmt, 1 << 20)   # exactly the row bytes
    if fmt != "packed":
        bad(3, 4, _row_bytes(fmt, SIZES[3][1])[1] - 1, "pitch below")
    # the last plane of the last frame ends with the buffer: one byte less and its last byte == frames_bytes
    with pytest.raises(ValueError, match="ends past frames_bytes") as e:
        P.check_addresses(geo, addr, fmt, tight - 1)
    assert "row 3" in str(e.value)
    a = addr.copy()
    a[0, 0] += 1 << 20                                              # a luma plane pushed past the end
    with pytest.raises(ValueError, match="row 0.*ends past"):
        P.check_addresses(geo, a, fmt, n)
    for col in unused:
        bad(1, col, 1, "does not use")
    for fb in (1 << 31, 0, -5):
        with pytest.raises(ValueError, match="frames_bytes"):
            P.check_addresses(geo, addr, fmt, fb)
    with pytest.raises(ValueError, match="geometry rows"):
        P.check_addresses(geo[:3], addr, fmt, n)
    with pytest.raises(ValueError, match="format"):
        P.check_addresses(geo, addr, "yv12", n)
    # unpack reads the pack back, whatever the fill
    for g, w_ in zip(A.unpack(buf, addr, SIZES, FORMATS[fmt]), frames):
        assert _same(fmt, g, w_)
    buf2, addr2 = A.pack(frames, FORMATS[fmt], pitches=pitches, gaps=11, fill_seed=2)
    assert np.array_equal(addr, addr2) and not np.array_equal(buf, buf2)


def test_pipeline_argument_validation_needs_no_gpu():
    import torch
    from mvfnet_amd import preprocess as P
    pipe = P.AddressedFramePipeline(crop_size=32)
    assert isinstance(pipe, P.GatherFramePipeline) and pipe.crop_hw == (32, 32)
    assert (pipe.format, pipe.standard, pipe.order, pipe.frame_dims, pipe._COLS) == (0, 0, 0, 1, (16, 28))
    pipe = P.AddressedFramePipeline([0, 0, 0], [1, 1, 1], to_rgb=False, crop_size=(24, 20), format="nv12", standard="bt709", order="rgb")
    assert (pipe.format, pipe.standard, pipe.order, pipe.crop_hw) == (2, 2, 1, (20, 24))
    assert P.AddressedFramePipeline(format=1).format == 1 and P.AddressedFramePipeline(format="I420").format == 1
    for kw in (dict(format="yv12"), dict(format=3), dict(format=True), dict(standard=3), dict(order="gbr")):
        with pytest.raises(ValueError):
            P.AddressedFramePipeline(**kw)
    # one run path: the class redefines neither to_nchw / to_stem nor _run
    assert P.AddressedFramePipeline.to_nchw is P.FramePipeline.to_nchw and P.AddressedFramePipeline.to_stem is P.FramePipeline.to_stem
    assert P.AddressedFramePipeline._run is P.FramePipeline._run
    # gathers / n_out: the table names its source, so the row count is the image count whatever the frames' shape
    pipe = P.AddressedFramePipeline(crop_size=32)
    t16, t28 = np.zeros((6, 16), dtype=np.int32), np.zeros((5, 28), dtype=np.int32)
    frames = np.zeros((1, 3, 4096), dtype=np.uint8)
    assert pipe.gathers(t16) and pipe.gathers(t28) and pipe.n_out(frames, t16) == 6 and pipe.n_out(frames, t28) == 5
    for cols in (11, 12, 23, 24):
        assert not pipe.gathers(np.zeros((4, cols), dtype=np.int32))
    assert not P.GatherFramePipeline(crop_size=32).gathers(t16) and not P.Yuv420FramePipeline(crop_size=32).gathers(t28)
    with pytest.raises(TypeError, match="CUDA uint8"):
        pipe.to_nchw(torch.zeros(2, 4096, dtype=torch.uint8), t16)
    with pytest.raises(TypeError, match="CUDA uint8"):
        pipe.to_nchw(torch.zeros(2, 4096), t16)


def _prototype(name):
    src = open(os.path.join(os.path.dirname(HERE), "include", "mvfnet_hip.h")).read()
    m = re.search(r"\bint\s+%s\s*\(([^)]*)\)\s*;" % name, src)
    assert m, "%s is not declared in include/mvfnet_hip.h" % name
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_declares_the_addressed_export_with_matching_argtypes():
    from mvfnet_amd import _lib
    assert "mvf_frames_addressed_resample_u8" in _lib.declared_symbols()
    params = _prototype("mvf_frames_addressed_resample_u8")
    fn = _lib.lib.mvf_frames_addressed_resample_u8
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == len(params) == 21
    assert params == ["const unsigned char* frames", "long long frames_bytes", "int format", "int standard", "int order", "int n_out", "const int* rows",
                      "const int* addr", "const float* color", "int h", "int w", "const float* mean3", "const float* std3", "int to_rgb", "int div_255",
                      "int pad", "int wp", "void* out_stem", "float* out_nchw", "int dtype", "void* stream"]
    fptr = ctypes.POINTER(ctypes.c_float)
    for p, t in zip(params, fn.argtypes):
        if p in ("const float* mean3", "const float* std3"):
            assert t is fptr, p
        elif "*" in p:
            assert t is ctypes.c_void_p, p
        elif p.startswith("long long "):
            assert t is ctypes.c_longlong, p
        else:
            assert p.startswith("int ") and t is ctypes.c_int, p
    # from `n_out` on, the gather export's parameters with `addr` after `rows`
    gather = _prototype("mvf_frames_gather_resample_u8")
    assert [p for p in params[5:] if p != "const int* addr"] == gather[gather.index("int n_out"):]


def test_addressed_export_validates_scalars_without_a_gpu():
    """Every refusal below happens on the host side of the export, before any HIP call (the pointers are never dereferenced)."""
    from mvfnet_amd import _lib
    lib = _lib.lib
    mean, std = (ctypes.c_float * 3)(1, 2, 3), (ctypes.c_float * 3)(1, 1, 1)
    buf = ctypes.create_string_buffer(64)
    ptr = ctypes.addressof(buf)

    def call(frames=ptr, frames_bytes=1 << 20, format=0, standard=0, order=0, n_out=6, rows=ptr, addr=ptr, h=16, w=16, std3=std, pad=3, wp=24, dt=0):
        return lib.mvf_frames_addressed_resample_u8(frames, frames_bytes, format, standard, order, n_out, rows, addr, None, h, w, mean, std3, 1, 0, pad, wp,
                                                    ptr, None, dt, None)
    for kw, word in [(dict(format=3), b"format 3"), (dict(format=-1), b"format -1"), (dict(format=1, standard=3), b"standard 3"),
                     (dict(format=2, standard=-1), b"standard -1"), (dict(format=1, order=2), b"order 2"), (dict(format=2, order=-1), b"order -1"),
                     (dict(dt=5), b"bad dtype"), (dict(format=2, dt=2), b"bad dtype"), (dict(rows=None), b"bad argument"), (dict(addr=None), b"addr is NULL"),
                     (dict(frames=None), b"bad argument"), (dict(frames_bytes=0), b"frames_bytes=0"), (dict(frames_bytes=1 << 31), b"frames_bytes=2147483648"),
                     (dict(frames_bytes=-1), b"frames_bytes=-1"), (dict(wp=21), b"wp=21"), (dict(format=1, wp=21), b"wp=21"), (dict(n_out=0), b"bad argument"),
                     (dict(h=0), b"bad argument"), (dict(pad=-1), b"bad argument"), (dict(std3=(ctypes.c_float * 3)(1, 0, 1)), b"std[1] is zero")]:
        assert call(**kw) == -1, kw                                                               # MVF_EINVAL
        msg = lib.mvf_last_error()
        assert b"frames_addressed_resample_u8" in msg and word in msg, (kw, msg)
