"""Device side of the input pipeline: the host ships DECODED uint8 frames (a quarter of the bytes of the
normalised fp32 tensor the reference's DataLoader + scatter move, codes/core/parallel/distributed.py:40-62) and one HIP kernel
(csrc/frames_input.hip, include/mvfnet_hip.h) does resize -> crop -> flip -> ColorJitter -> Normalize -> FormatShape -> stem layout;
decoding is the only step left on the host.  Names and argument meaning mirror the reference's pipeline steps (augmentations.py):
`img_norm_cfg = dict(mean, std, to_rgb)`, `Flip(flip_ratio)`'s boolean, the crops' offsets.

Every pipeline class is `to_nchw(frames, table)` (the reference's fp32 tensor) and `to_stem(frames, table, pad, wp, dtype, out=None)`
(the stem conv's operand) over one int32 table with one row per image, which the engines carry through `window=`:
  FramePipeline             (y0, x0, flip) crop windows, or None: the frames are already at their final resolution;
  ResamplingFramePipeline   11 geometry columns (hs_i, ws_i, by, bx, bh, bw, rh, rw, oy, ox, flip): patch -> cv2 INTER_LINEAR resize -> crop,
                            `Resize` / `RandomResizedCrop` / the crops as `train_rows` / `val_rows` / `test_rows` / ... (`collate_frames`);
  JitterFramePipeline       11, or 11 + 12 colour columns: ColorJitter's affine map per frame as fp32 bit patterns (`color_jitter_table`,
                            `jitter_rows`, `collate_jitter_frames`);
  GatherFramePipeline       11 or 23, or either + 1 `src` column: the image is cut from frames[src], so a video's clips and crops share one
                            upload of its distinct frames (`gather_rows`, `video_test_table`);
  Yuv420FramePipeline       the same four tables over decoder-native planar YUV 4:2:0 frames, I420 or NV12, half the bytes of the packed
                            frames; the colour conversion runs in the kernel (`collate_yuv_frames`);
  AddressedFramePipeline    11 or 23 + 5 address columns (o0, p0, o1, o2, p1): the image is cut from planes at byte offsets of one flat
                            buffer, each frame at its own size and row pitch, packed or YUV 4:2:0 -- a decoder's surfaces as they lie,
                            both orientations in one batch without padding, videos of different sizes in one launch (`address_rows`,
                            `check_addresses`, `collate_addressed_frames`).
A table without the colour or src columns gives the narrower class's output bit for bit."""
import ctypes
import math
import random

import torch

from ._lib import check, lib

_DT = {torch.float32: 0, torch.bfloat16: 1}


def _ptr(t):
    return None if t is None else t.data_ptr()


def _ncols(table):
    """The column count of a 2-D (or deeper) table; 0 for None, a flat one or anything without a shape."""
    return int(table.shape[-1]) if table is not None and hasattr(table, "shape") and len(table.shape) > 1 else 0


def three_crop_offsets(img_h, img_w, crop_h, crop_w):
    """(x0, y0) of ThreeCrop's crops in the reference's order: left/top, right/bottom, middle (augmentations.py:487-510)."""
    if crop_h == img_h:
        s = (img_w - crop_w) // 2
        return [(0, 0), (2 * s, 0), (s, 0)]
    if crop_w == img_w:
        s = (img_h - crop_h) // 2
        return [(0, 0), (0, 2 * s), (0, s)]
    ws, hs = (img_w - crop_w) // 4, (img_h - crop_h) // 4
    return [(0, 2 * hs), (4 * ws, 2 * hs), (2 * ws, 2 * hs)]


def three_crop_windows(n_frames, img_h, img_w, crop_h, crop_w):
    """Window rows (y0, x0, flip) for ThreeCrop's oversampled group: crop-major, frame-minor, never mirrored (augmentations.py:512-530)."""
    return [(y0, x0, 0) for (x0, y0) in three_crop_offsets(img_h, img_w, crop_h, crop_w) for _ in range(n_frames)]


def flip_flag(flip_ratio, rng=None):
    """Flip's per-sample decision (augmentations.py:217): ONE `rand()` draw, mirrored when it is below flip_ratio."""
    import numpy as np
    return bool((rng if rng is not None else np.random).rand() < flip_ratio)


class FramePipeline(object):
    """Normalize(mean, std, to_rgb, div_255) + a crop size; per-frame windows (y0, x0, flip) select crop position and mirroring
    (mvf_frames_prep_u8).  The subclasses change what a table row is (_parse), what a frame is (_source) and the export (_launch)."""

    frame_dims = 3              # trailing dimensions of one frame, for the engines' flattening

    def __init__(self, mean=(123.675, 116.28, 103.53), std=(58.395, 57.12, 57.375), to_rgb=True, div_255=False, crop_size=224):
        self.mean = (ctypes.c_float * 3)(*[float(v) for v in mean])
        self.std = (ctypes.c_float * 3)(*[float(v) for v in std])
        self.to_rgb, self.div_255 = bool(to_rgb), bool(div_255)
        self.crop_hw = (crop_size, crop_size) if isinstance(crop_size, int) else (int(crop_size[1]), int(crop_size[0]))   # cfg is (w, h)

    def center_window(self, n, hs, ws, flip=False, device="cuda"):
        """CenterCrop's window for every frame (augmentations.py:342-396: x0 = (W - w) // 2, y0 = (H - h) // 2)."""
        h, w = self.crop_hw
        row = [(hs - h) // 2, (ws - w) // 2, int(bool(flip))]
        return torch.tensor([row] * n, dtype=torch.int32, device=device)

    def _source(self, frames):
        """-> (the frames flattened to (n_src, hs, ws, 3) contiguous, n_src, hs, ws)."""
        if frames.dtype != torch.uint8 or frames.shape[-1] != 3 or not frames.is_cuda:
            raise TypeError("%s expects a CUDA uint8 tensor (..., H, W, 3) of decoded frames, got %s %s" % (type(self).__name__, frames.dtype, tuple(frames.shape)))
        f = frames.reshape((-1,) + tuple(frames.shape[-3:])).contiguous()
        return (f,) + tuple(f.shape[:3])

    def _parse(self, window, n_src, hs, ws):
        """-> (geo, color, src) device tensors for _launch, None where the table has no such part."""
        h, w = self.crop_hw
        if h > hs or w > ws:
            raise ValueError("crop %dx%d larger than the frames %dx%d" % (h, w, hs, ws))
        if window is None:
            return None, None, None
        window = window.to(device="cuda", dtype=torch.int32).reshape(-1, 3).contiguous()
        if window.shape[0] != n_src:
            raise ValueError("window needs one (y0, x0, flip) row per frame: %d rows for %d frames" % (window.shape[0], n_src))
        lo, hi = window.min(0).values.tolist(), window.max(0).values.tolist()
        if lo[0] < 0 or lo[1] < 0 or hi[0] + h > hs or hi[1] + w > ws:
            raise ValueError("crop window leaves the %dx%d frame" % (hs, ws))
        return window, None, None

    def _launch(self, f, n_src, hs, ws, geo, color, src, n, pad, wp, out_stem, out_nchw, dt):
        h, w = self.crop_hw
        check(lib.mvf_frames_prep_u8(f.data_ptr(), n, hs, ws, _ptr(geo), h, w, self.mean, self.std, int(self.to_rgb), int(self.div_255), pad, wp,
                                     out_stem, out_nchw, dt, torch.cuda.current_stream().cuda_stream), "mvf_frames_prep_u8")

    def _run(self, frames, table, pad, wp, dtype, out, nchw):
        f, n_src, hs, ws = self._source(frames)
        geo, color, src = self._parse(table, n_src, hs, ws)
        n, (h, w) = n_src if geo is None else geo.shape[0], self.crop_hw
        shape = (n, 3, h, w) if nchw else (n, h + 2 * pad, wp, 4)
        if out is None:
            out = torch.empty(shape, dtype=dtype, device=f.device)
        elif tuple(out.shape) != shape or out.dtype != dtype or not out.is_contiguous():
            raise ValueError("%s: the output buffer %s %s does not hold the table's %d images %s %s"
                             % (type(self).__name__, out.dtype, tuple(out.shape), n, dtype, shape))
        self._launch(f, n_src, hs, ws, geo, color, src, n, pad, wp, None if nchw else out.data_ptr(), out.data_ptr() if nchw else None, _DT[dtype])
        return out

    def to_nchw(self, frames, rows=None):
        """-> (n, 3, h, w) fp32, what the reference's resize / crop + Flip [+ ColorJitter] + Normalize + FormatShape + ToTensor produce."""
        return self._run(frames, rows, 0, self.crop_hw[1], torch.float32, None, True)

    def to_stem(self, frames, rows, pad, wp, dtype, out=None):
        """-> (n, h + 2 pad, wp, 4) `dtype`: the zero-padded channels-last operand of the 7x7 stem conv (what mvf_stem_prep makes
        from the fp32 NCHW tensor), straight from the uint8 frames; into `out` when given."""
        return self._run(frames, rows, pad, wp, dtype, out, False)


# ---- resize geometry (host side; reference augmentations.py:13-68 Resize, :600-661 RandomResizedCrop, mmcv 0.4.3 imrescale / imcrop) --
RESAMPLE_COLS = 11          # (hs_i, ws_i, by, bx, bh, bw, rh, rw, oy, ox, flip): see include/mvfnet_hip.h mvf_frames_resample_u8


def rescale_size(h, w, scale):
    """The output size of mmcv 0.4.3 `imrescale(img, scale)` for an h x w image, in mmcv's (new_w, new_h) order: a number is the
    factor itself; a tuple gives f = min(max(scale) / max(h, w), min(scale) / min(h, w)); then (int(w * f + 0.5), int(h * f + 0.5)).
    Third-party code restated (mmcv is not in the build container): parity unpinned; the scale the reference hands it is pinned by
    tests/golden/make_resize_golden.py."""
    if isinstance(scale, (int, float)):
        if scale <= 0:
            raise ValueError("Invalid scale %s, must be positive." % (scale,))
        f = float(scale)
    else:
        f = min(max(scale) / max(h, w), min(scale) / min(h, w))
    return int(w * float(f) + 0.5), int(h * float(f) + 0.5)


def resized_hw(hs, ws, scale, keep_ratio=True):
    """(rh, rw) of `Resize(scale, keep_ratio)` (augmentations.py:37-61): imrescale's size, or the exact (w, h) `scale` handed to imresize."""
    if keep_ratio:
        rw, rh = rescale_size(hs, ws, scale)
    else:
        rw, rh = int(scale[0]), int(scale[1])
    if rh < 1 or rw < 1:
        raise ValueError("Resize(%s) of a %dx%d frame is empty" % (scale, hs, ws))
    return rh, rw


def random_resized_crop_box(h, w, scale=(0.08, 1.0), ratio=(3. / 4., 4. / 3.), rng=random):
    """RandomResizedCrop.get_params + the box __call__ hands to mmcv.imcrop (augmentations.py:612-651), quirks kept: Python's `random`
    (`rng`: the module or a random.Random), 10 attempts of uniform, uniform, random [, randint, randint when the box fits]; the crop's
    width is tested against the image HEIGHT and its height against the WIDTH (shape[0] / shape[1]); the centre-square fallback; the box
    [x1, y1, x1 + crop_w - 1, y1 + crop_h - 1], which the axis swap can make overhang the frame, clipped to the image as mmcv.imcrop
    does.  -> the clipped patch (by, bx, bh, bw)."""
    for _ in range(10):
        area = h * w
        target_area = rng.uniform(*scale) * area
        aspect_ratio = rng.uniform(*ratio)
        cw = int(round(math.sqrt(target_area * aspect_ratio)))
        ch = int(round(math.sqrt(target_area / aspect_ratio)))
        if rng.random() < 0.5:
            cw, ch = ch, cw
        if cw <= h and ch <= w:
            x1 = rng.randint(0, w - ch)
            y1 = rng.randint(0, h - cw)
            break
    else:
        cw = ch = min(h, w)
        x1, y1 = (w - cw) // 2, (h - cw) // 2
    x2, y2 = x1 + cw - 1, y1 + ch - 1
    x1, x2 = (max(min(v, w - 1), 0) for v in (x1, x2))         # mmcv.bbox_clip
    y1, y2 = (max(min(v, h - 1), 0) for v in (y1, y2))
    if x2 < x1 or y2 < y1:
        raise ValueError("RandomResizedCrop drew an empty box on a %dx%d frame" % (h, w))
    return y1, x1, y2 - y1 + 1, x2 - x1 + 1


def _hw(size):
    """cfg sizes are (w, h) or an int -> (h, w)."""
    return (size, size) if isinstance(size, int) else (int(size[1]), int(size[0]))


def _table(rows):
    import numpy as np
    return np.asarray(rows, dtype=np.int32).reshape(-1, RESAMPLE_COLS)


def resize_rows(hs, ws, n_frames, scale, keep_ratio=True):
    """Rows for `Resize(scale, keep_ratio)` alone: every frame resized whole, the output is the whole resized image (crop = (rh, rw))."""
    rh, rw = resized_hw(hs, ws, scale, keep_ratio)
    return _table([(hs, ws, 0, 0, hs, ws, rh, rw, 0, 0, 0)] * n_frames)


def train_rows(hs, ws, n_frames, input_size=224, scale=(0.08, 1.0), ratio=(3. / 4., 4. / 3.), flip_ratio=0.5, rng=random, np_rng=None):
    """The shipped train recipe RandomResizedCrop(input_size) -> Flip(flip_ratio) for one clip of n_frames hs x ws frames, draws in the
    reference's order: get_params on `rng` (Python's random), then Flip's one np.random draw (`np_rng`, default the global numpy
    generator).  One box and one flip for the whole clip.  -> (n_frames, 11) int32."""
    by, bx, bh, bw = random_resized_crop_box(hs, ws, scale, ratio, rng)
    rh, rw = _hw(input_size)
    flip = int(flip_flag(flip_ratio, np_rng))
    return _table([(hs, ws, by, bx, bh, bw, rh, rw, 0, 0, flip)] * n_frames)


def val_rows(hs, ws, n_frames, scale=(float("inf"), 256), crop_size=224, keep_ratio=True):
    """The shipped val recipe Resize(scale, keep_ratio) -> CenterCrop(crop_size) (augmentations.py:445-452 offsets on the resized size).
    The recipe's Flip(flip_ratio=0) never mirrors (it still consumes one np.random draw in the reference; none is drawn here)."""
    rh, rw = resized_hw(hs, ws, scale, keep_ratio)
    ch, cw = _hw(crop_size)
    if ch > rh or cw > rw:
        raise ValueError("CenterCrop %dx%d larger than the resized %dx%d frame" % (ch, cw, rh, rw))
    return _table([(hs, ws, 0, 0, hs, ws, rh, rw, (rh - ch) // 2, (rw - cw) // 2, 0)] * n_frames)


def test_rows(hs, ws, n_frames, scale=(float("inf"), 256), crop_size=256, keep_ratio=True):
    """The shipped test recipe Resize(scale, keep_ratio) -> ThreeCrop(crop_size): 3 * n_frames rows, crop-major and frame-minor as
    ThreeCrop stacks its img_group (three_crop_windows); the caller repeats the clip's frames three times."""
    rh, rw = resized_hw(hs, ws, scale, keep_ratio)
    ch, cw = _hw(crop_size)
    if ch > rh or cw > rw:
        raise ValueError("ThreeCrop %dx%d larger than the resized %dx%d frame" % (ch, cw, rh, rw))
    return _table([(hs, ws, 0, 0, hs, ws, rh, rw, y0, x0, 0) for (y0, x0, _) in three_crop_windows(n_frames, rh, rw, ch, cw)])


test_rows.__test__ = False          # a row builder, not a pytest test


def collate_frames(groups, pad_to=None, cols=None):
    """groups: a list of (frames, rows) per clip -- frames (T, h_b, w_b, 3) uint8 (numpy or a CPU tensor), rows its (T, 11) table --
    -> (frames (B, T, Hs, Ws, 3) uint8, rows (B * T, 11) int32), CPU tensors.  Clips of different resolutions share one dense tensor,
    zero padded to the largest (or to `pad_to` = (Hs, Ws), so a prefetcher's persistent buffers keep their shape); every row keeps its
    own frame's (hs_i, ws_i).  `cols` (default 11) is the tables' column count: 23 for jitter_rows tables (collate_jitter_frames)."""
    import numpy as np
    cols = RESAMPLE_COLS if cols is None else int(cols)
    fr = [torch.as_tensor(np.asarray(f)) for f, _ in groups]
    rows = [torch.as_tensor(np.asarray(r, dtype=np.int32)).reshape(-1, cols) for _, r in groups]
    if not fr:
        raise ValueError("collate_frames: no clips")
    t = fr[0].shape[0]
    for f, r in zip(fr, rows):
        if f.dtype != torch.uint8 or f.dim() != 4 or f.shape[-1] != 3 or f.shape[0] != t:
            raise ValueError("collate_frames: every clip must be (T=%d, h, w, 3) uint8, got %s %s" % (t, f.dtype, tuple(f.shape)))
        if r.shape[0] != t or bool((r[:, 0] != f.shape[1]).any()) or bool((r[:, 1] != f.shape[2]).any()):
            raise ValueError("collate_frames: rows do not describe their %s frames" % (tuple(f.shape),))
    hs, ws = (max(f.shape[1] for f in fr), max(f.shape[2] for f in fr)) if pad_to is None else (int(pad_to[0]), int(pad_to[1]))
    if any(f.shape[1] > hs or f.shape[2] > ws for f in fr):
        raise ValueError("collate_frames: a clip is larger than pad_to=%s" % (pad_to,))
    out = torch.zeros(len(fr), t, hs, ws, 3, dtype=torch.uint8)
    for b, f in enumerate(fr):
        out[b, :, :f.shape[1], :f.shape[2]] = f
    return out, torch.cat(rows).contiguous()


class ResamplingFramePipeline(FramePipeline):
    """FramePipeline with the resize in front of the crop: per-frame int32 rows (hs_i, ws_i, by, bx, bh, bw, rh, rw, oy, ox, flip)
    (train_rows / val_rows / test_rows / resize_rows) instead of (y0, x0, flip) windows; same constructor, `crop_hw`, `to_nchw` and
    `to_stem` interface, so the engines take it through `input_pipeline` / `window=`.  The frames may be smaller than the crop.
    This class, JitterFramePipeline and GatherFramePipeline share one table parser and one export, mvf_frames_gather_resample_u8 with
    the colour and src pointers NULL where the table has no such columns; they differ in the column counts they take (_COLS)."""

    _COLS = (RESAMPLE_COLS,)

    def center_window(self, n, hs, ws, flip=False, device="cuda"):
        """Rows of CenterCrop without a resize (augmentations.py:447-452)."""
        h, w = self.crop_hw
        row = [hs, ws, 0, 0, hs, ws, hs, ws, (hs - h) // 2, (ws - w) // 2, int(bool(flip))]
        return torch.tensor([row] * n, dtype=torch.int32, device=device)

    def _as_table(self, table):
        """The table as a CUDA int32 (n, cols) tensor, cols one of _COLS."""
        name, takes = type(self).__name__, " / ".join(str(c) for c in self._COLS)
        if table is None:
            raise ValueError("%s needs one int32 row of %s columns per image: (hs_i, ws_i, by, bx, bh, bw, rh, rw, oy, ox, flip) [+ 12 colour] [+ src]" % (name, takes))
        t = torch.as_tensor(table).to(device="cuda", dtype=torch.int32)
        if t.dim() == 1 and len(self._COLS) == 1:                 # a flat table is unambiguous where one width is taken
            t = t.reshape(-1, self._COLS[0])
        cols = _ncols(t)
        if cols not in self._COLS:
            raise ValueError("%s rows must have %s columns, got %s" % (name, takes, tuple(t.shape)))
        return t.reshape(-1, cols)

    def _geometry(self, t, hs, ws):
        """(n, 11 or 23) -> (geo, color) checked: every patch in its frame (and the frame in the hs x ws padded extent, when the batch has
        one), every crop in its resized patch."""
        color = None
        if t.shape[1] == JITTER_COLS:
            t, color = t[:, :RESAMPLE_COLS], t[:, RESAMPLE_COLS:].contiguous().view(torch.float32)
        geo = t.contiguous()
        h, w = self.crop_hw
        fh, fw, by, bx, bh, bw, rh, rw, oy, ox, flip = geo.to(torch.int64).unbind(1)
        bad = ((fh < 1) | (fw < 1)
               | (by < 0) | (bx < 0) | (bh < 1) | (bw < 1) | (by + bh > fh) | (bx + bw > fw)
               | (oy < 0) | (ox < 0) | (oy + h > rh) | (ox + w > rw)
               | ((flip != 0) & (flip != 1)))
        if hs is not None:
            bad = bad | (fh > hs) | (fw > ws)                     # every frame shares the hs x ws padded extent: the check holds per src
        if bool(bad.any()):
            i = int(bad.nonzero()[0, 0])
            where = "its %dx%d-padded frame" % (hs, ws) if hs is not None else "its own hs_i x ws_i frame"
            raise ValueError("row %d %s: the patch must lie in %s and the %dx%d crop in the resized patch" % (i, geo[i].tolist(), where, h, w))
        if color is not None and not bool(torch.isfinite(color).all()):
            raise ValueError("%s: colour coefficients must be finite" % type(self).__name__)
        return geo, color

    def _parse(self, table, n_src, hs, ws):
        name = type(self).__name__
        t = self._as_table(table)
        src = None
        if t.shape[1] in (RESAMPLE_COLS + 1, JITTER_COLS + 1):    # one row per OUTPUT image, cut from frames[src]
            if t.shape[0] < 1:
                raise ValueError("%s: an empty table" % name)
            t, src = t[:, :-1], t[:, -1].contiguous()
            bad = (src < 0) | (src >= n_src)
            if bool(bad.any()):
                i = int(bad.nonzero()[0, 0])
                raise ValueError("row %d: source frame %d is not one of the %d frames" % (i, int(src[i]), n_src))
        elif t.shape[0] != n_src:
            raise ValueError("rows: %d rows for %d frames" % (t.shape[0], n_src))
        geo, color = self._geometry(t, hs, ws)
        return geo, color, src

    def _launch(self, f, n_src, hs, ws, geo, color, src, n, pad, wp, out_stem, out_nchw, dt):
        h, w = self.crop_hw
        check(lib.mvf_frames_gather_resample_u8(f.data_ptr(), n_src, hs, ws, _ptr(src), n, geo.data_ptr(), _ptr(color), h, w, self.mean, self.std,
                                                int(self.to_rgb), int(self.div_255), pad, wp, out_stem, out_nchw, dt,
                                                torch.cuda.current_stream().cuda_stream), "mvf_frames_gather_resample_u8")


# ---- TSN-style recipe (host side; reference augmentations.py:71-192 MultiScaleCrop, :238-339 ColorJitter, :544-596 TenCrop, ----------
# ---- :672-707 RandomRescaledCrop, :428-457 CenterCrop) ------------------------------------------------------------------------------
COLOR_COLS = 12             # M[0][0..2], M[1][0..2], M[2][0..2], b[0..2]: see include/mvfnet_hip.h mvf_frames_resample_color_u8
JITTER_COLS = RESAMPLE_COLS + COLOR_COLS


def fix_offsets(more_fix_crop, image_w, image_h, crop_w, crop_h):
    """MultiScaleCrop.fill_fix_offset (augmentations.py:160-183): (x, y) of the 5 fixed crops (corners, centre) or, with more_fix_crop,
    13 (plus the edge centres and the quarter points), in the reference's order; steps are floored quarters of the slack."""
    ws, hs = (image_w - crop_w) // 4, (image_h - crop_h) // 4
    ret = [(0, 0), (4 * ws, 0), (0, 4 * hs), (4 * ws, 4 * hs), (2 * ws, 2 * hs)]
    if more_fix_crop:
        ret += [(0, 2 * hs), (4 * ws, 2 * hs), (2 * ws, 4 * hs), (2 * ws, 0), (ws, hs), (3 * ws, hs), (ws, 3 * hs), (3 * ws, 3 * hs)]
    return ret


def multi_scale_crop_box(h, w, input_size, scales=None, max_distort=1, fix_crop=True, more_fix_crop=True, rng=random):
    """MultiScaleCrop._sample_crop_size + the box __call__ hands to mmcv.imcrop (augmentations.py:106-157) for an h x w frame, draws on
    Python's `random` (`rng`) in the reference's order: `choice` over the (crop_w, crop_h) pairs whose scale levels differ by at most
    max_distort -- sizes int(min(h, w) * scale), snapped to the input size when within 3 of it -- then `choice` over fix_offsets, or
    randint(0, w - crop_w), randint(0, h - crop_h) without fix_crop.  The box [x, y, x + crop_w - 1, y + crop_h - 1] is clipped to the
    image as mmcv.imcrop does (a snapped size can exceed the frame).  -> the clipped patch (by, bx, bh, bw)."""
    in_w, in_h = (input_size, input_size) if isinstance(input_size, int) else (int(input_size[0]), int(input_size[1]))
    base = min(w, h)
    sizes = [int(base * x) for x in (scales if scales is not None else [1, .875, .75, .66])]
    crop_h = [in_h if abs(x - in_h) < 3 else x for x in sizes]
    crop_w = [in_w if abs(x - in_w) < 3 else x for x in sizes]
    pairs = [(cw, ch) for i, ch in enumerate(crop_h) for j, cw in enumerate(crop_w) if abs(i - j) <= max_distort]
    cw, ch = rng.choice(pairs)
    if not fix_crop:
        x1 = rng.randint(0, w - cw)
        y1 = rng.randint(0, h - ch)
    else:
        x1, y1 = rng.choice(fix_offsets(more_fix_crop, w, h, cw, ch))
    x2, y2 = x1 + cw - 1, y1 + ch - 1
    x1, x2 = (max(min(v, w - 1), 0) for v in (x1, x2))         # mmcv.bbox_clip
    y1, y2 = (max(min(v, h - 1), 0) for v in (y1, y2))
    return y1, x1, y2 - y1 + 1, x2 - x1 + 1


def multi_scale_crop_rows(hs, ws, n_frames, input_size=224, scales=None, max_distort=1, fix_crop=True, more_fix_crop=True, flip_ratio=0.5,
                          rng=random, np_rng=None):
    """The TSN train recipe MultiScaleCrop(input_size, ...) -> Flip(flip_ratio) for one clip of n_frames hs x ws frames: the box on `rng`
    (Python's random), then Flip's one np.random draw (`np_rng`); one box and one flip per clip, the patch resized to input_size.
    -> (n_frames, 11) int32."""
    by, bx, bh, bw = multi_scale_crop_box(hs, ws, input_size, scales, max_distort, fix_crop, more_fix_crop, rng)
    rh, rw = _hw(input_size)
    flip = int(flip_flag(flip_ratio, np_rng))
    return _table([(hs, ws, by, bx, bh, bw, rh, rw, 0, 0, flip)] * n_frames)


def ten_crop_rows(hs, ws, n_frames, crop_size=224, scale=None, keep_ratio=True):
    """TenCrop(crop_size) (augmentations.py:563-591): 10 * n_frames rows -- for each of the five fix_offsets(False, ...) positions (four
    corners, centre) the clip's plain crops, then the same crops mirrored; no resize, or `Resize(scale, keep_ratio)` in front when
    `scale` is given (as test_rows).  The caller repeats the clip's frames ten times."""
    rh, rw = (hs, ws) if scale is None else resized_hw(hs, ws, scale, keep_ratio)
    ch, cw = _hw(crop_size)
    if ch > rh or cw > rw:
        raise ValueError("TenCrop %dx%d larger than the %dx%d frame" % (ch, cw, rh, rw))
    return _table([(hs, ws, 0, 0, hs, ws, rh, rw, y0, x0, flip) for (x0, y0) in fix_offsets(False, rw, rh, cw, ch)
                   for flip in (0, 1) for _ in range(n_frames)])


def random_rescaled_crop_rows(hs, ws, n_frames, input_size, scale=(256, 320), rng=random):
    """RandomRescaledCrop(input_size, scale) (augmentations.py:682-699), its axis naming kept: randint(*scale) is the short edge,
    imrescale by the float factor max(edge / hs, edge / ws); then `w, h, _ = img.shape` makes "w" the ROW count, so randint(0, rows -
    input_size[0]) offsets the rows and randint(0, cols - input_size[1]) the columns, and the output is input_size[0] rows by
    input_size[1] columns (build the pipeline with crop_size=(input_size[1], input_size[0]) when they differ).  Draws on `rng`."""
    n0, n1 = (input_size, input_size) if isinstance(input_size, int) else (int(input_size[0]), int(input_size[1]))
    edge = float(rng.randint(*scale))
    rw, rh = rescale_size(hs, ws, max(edge / hs, edge / ws))
    oy = rng.randint(0, rh - n0)
    ox = rng.randint(0, rw - n1)
    return _table([(hs, ws, 0, 0, hs, ws, rh, rw, oy, ox, 0)] * n_frames)


def center_crop_rows(hs, ws, n_frames, crop_size):
    """CenterCrop(crop_size) with no Resize in front (augmentations.py:445-452)."""
    ch, cw = _hw(crop_size)
    if ch > hs or cw > ws:
        raise ValueError("CenterCrop %dx%d larger than the %dx%d frame" % (ch, cw, hs, ws))
    return _table([(hs, ws, 0, 0, hs, ws, hs, ws, (hs - ch) // 2, (ws - cw) // 2, 0)] * n_frames)


_EIGVAL = (55.46, 4.794, 1.148)
_EIGVEC = ((-0.5675, 0.7192, 0.4009), (-0.5808, -0.0045, -0.8140), (-0.5836, -0.6948, 0.4203))
_TYIQ = ((0.299, 0.587, 0.114), (0.596, -0.274, -0.321), (0.211, -0.523, 0.311))
_ITYIQ = ((1.0, 0.956, 0.621), (1.0, -0.272, -0.647), (1.0, -1.107, 1.705))


def color_identity(n_frames):
    """(n_frames, 12) float32 rows of the identity colour transform: M = I, b = 0."""
    import numpy as np
    return np.tile(np.concatenate([np.eye(3).reshape(-1), np.zeros(3)]).astype(np.float32), (n_frames, 1))


def color_jitter_table(n_frames, color_space_aug=False, alphastd=0.1, eigval=None, eigvec=None, rng=random, np_rng=None):
    """ColorJitter(color_space_aug, alphastd, eigval, eigvec).__call__ (augmentations.py:306-333) for one clip of n_frames frames as one
    affine map q = M p + b per frame, p the (B, G, R) pixel in stored order -> (n_frames, 12) float32 rows M[0], M[1], M[2], b.
    Every step of the reference is affine and nothing clips:
      brightness  + float32(delta);  contrast  * float32(alpha);
      saturation  alpha * p + (1 - alpha) * (0.299 p0 + 0.587 p1 + 0.114 p2), the grey weights on the channels in STORED order;
      hue         p @ t, t = float32((ityiq @ bt @ tyiq).T), u, w = cos / sin(alpha * pi), alpha from (-18, 18) with no degree conversion;
      lighting    + float32(eigvec * alpha @ eigval)[::-1], always.
    Draws in the reference's order: with color_space_aug three `np.random.uniform` (`np_rng`) and one `random.uniform` (`rng`) per clip,
    then per frame on `rng` the brightness coin, the order coin and one coin per step in the chosen order (contrast, saturation, hue --
    or saturation, hue, contrast); last `np.random.normal(0, alphastd, size=3)`.  Composed in float64, rounded once to float32."""
    import numpy as np
    np_rng = np_rng if np_rng is not None else np.random
    eigval = np.asarray(_EIGVAL if eigval is None else eigval, dtype=np.float64)
    eigvec = np.asarray(_EIGVEC if eigvec is None else eigvec, dtype=np.float64)
    maps = [(np.eye(3), np.zeros(3)) for _ in range(n_frames)]
    if color_space_aug:
        delta = float(np.float32(np_rng.uniform(-32, 32)))
        c_alpha = float(np.float32(np_rng.uniform(0.6, 1.4)))
        s_alpha = float(np_rng.uniform(0.6, 1.4))
        h_alpha = rng.uniform(-18, 18)
        grey = np.array([0.299, 0.587, 0.114], dtype=np.float32).astype(np.float64)
        u, w = np.cos(h_alpha * np.pi), np.sin(h_alpha * np.pi)
        bt = np.array([[1.0, 0.0, 0.0], [0.0, u, -w], [0.0, w, u]])
        t = np.dot(np.dot(np.array(_ITYIQ), bt), np.array(_TYIQ)).T.astype(np.float32).astype(np.float64)
        steps = {"contrast": c_alpha * np.eye(3), "saturation": s_alpha * np.eye(3) + (1.0 - s_alpha) * np.outer(np.ones(3), grey),
                 "hue": t.T}                                   # (p @ t)[c] = sum_k t[k][c] p[k]
        for i in range(n_frames):
            m, b = maps[i]
            if rng.uniform(0, 1) > 0.5:
                b = b + delta
            order = ("contrast", "saturation", "hue") if rng.uniform(0, 1) > 0.5 else ("saturation", "hue", "contrast")
            for name in order:
                if rng.uniform(0, 1) > 0.5:
                    m, b = np.dot(steps[name], m), np.dot(steps[name], b)
            maps[i] = (m, b)
    alpha = np_rng.normal(0, alphastd, size=(3,))
    bgr = np.array(np.dot(eigvec * alpha, eigval)).astype(np.float32)[::-1].astype(np.float64)
    return np.stack([np.concatenate([m.reshape(-1), b + bgr]) for m, b in maps]).astype(np.float32)


def jitter_rows(rows, color=None):
    """(n, 11) int32 geometry rows + (n, 12) float32 colour rows (default: color_identity) -> ONE (n, 23) int32 table, the colour
    coefficients as their fp32 bit patterns, so that geometry and colour travel together through `window=` and `collate_jitter_frames`."""
    import numpy as np
    rows = _table(rows)
    color = color_identity(rows.shape[0]) if color is None else np.ascontiguousarray(np.asarray(color, dtype=np.float32)).reshape(-1, COLOR_COLS)
    if color.shape[0] != rows.shape[0]:
        raise ValueError("jitter_rows: %d colour rows for %d geometry rows" % (color.shape[0], rows.shape[0]))
    if not np.isfinite(color).all():
        raise ValueError("jitter_rows: colour coefficients must be finite")
    return np.concatenate([rows, color.view(np.int32)], axis=1)


def split_jitter_rows(table):
    """The inverse of jitter_rows on the host: (n, 23) int32 -> ((n, 11) int32, (n, 12) float32), bit for bit."""
    import numpy as np
    table = np.ascontiguousarray(np.asarray(table, dtype=np.int32)).reshape(-1, JITTER_COLS)
    return table[:, :RESAMPLE_COLS].copy(), table[:, RESAMPLE_COLS:].copy().view(np.float32)


def collate_jitter_frames(groups, pad_to=None):
    """collate_frames for jitter_rows tables: groups of (frames, (T, 23) table); an (T, 11) table is taken as "no jitter".
    -> (frames (B, T, Hs, Ws, 3) uint8, rows (B * T, 23) int32), CPU tensors."""
    import numpy as np
    full = []
    for f, r in groups:
        r = np.asarray(r, dtype=np.int32)
        full.append((f, jitter_rows(r) if r.shape[-1] == RESAMPLE_COLS else r))
    return collate_frames(full, pad_to, cols=JITTER_COLS)


class JitterFramePipeline(ResamplingFramePipeline):
    """ResamplingFramePipeline with ColorJitter between the resample and Normalize: rows are ONE int32
    table of 23 columns per frame, the 11 geometry columns followed by the 12 colour coefficients' fp32 bit patterns (jitter_rows), so
    the engines carry it through `input_pipeline` / `window=` as they carry the 11-column table.  11-column rows mean "no jitter" and
    give ResamplingFramePipeline's output bit for bit.  Same constructor, `crop_hw`, `to_nchw` and `to_stem`."""

    _COLS = (RESAMPLE_COLS, JITTER_COLS)


# ---- whole-video testing: several output images per decoded frame --------------------------------------------------------------------
def gather_rows(rows, src):
    """(n, 11) or (n, 23) int32 rows + (n,) source-frame numbers -> ONE (n, 12) or (n, 24) int32 table, `src` as the trailing column:
    output image i is cut from frame src[i] of the frames handed to GatherFramePipeline (row i describes THAT frame: its hs_i, ws_i)."""
    import numpy as np
    rows = np.asarray(rows, dtype=np.int32)
    if rows.ndim != 2 or rows.shape[1] not in (RESAMPLE_COLS, JITTER_COLS):
        raise ValueError("gather_rows: rows must have %d or %d columns, got %s" % (RESAMPLE_COLS, JITTER_COLS, rows.shape))
    src = np.asarray(src).reshape(-1)
    if src.shape[0] != rows.shape[0]:
        raise ValueError("gather_rows: %d source indices for %d rows" % (src.shape[0], rows.shape[0]))
    if src.size and (src.min() < 0 or src.max() > np.iinfo(np.int32).max):
        raise ValueError("gather_rows: source indices must be non-negative int32")
    return np.concatenate([rows, src.astype(np.int32)[:, None]], axis=1)


def split_gather_rows(table):
    """The inverse of gather_rows on the host: (n, 12) or (n, 24) int32 -> ((n, 11) or (n, 23) int32, (n,) int32 src)."""
    import numpy as np
    table = np.asarray(table, dtype=np.int32)
    if table.ndim != 2 or table.shape[1] not in (RESAMPLE_COLS + 1, JITTER_COLS + 1):
        raise ValueError("split_gather_rows: the table must have %d or %d columns, got %s" % (RESAMPLE_COLS + 1, JITTER_COLS + 1, table.shape))
    return table[:, :-1].copy(), table[:, -1].copy()


def video_test_table(frame_inds, hs, ws, rows_fn=test_rows, **recipe):
    """One video's test-time input from its DISTINCT frames.  frame_inds: what sample_frame_inds(..., test_mode=True) returned (clip-major,
    frame-minor; clips may share frames, clamped indices repeat); hs x ws: the decoded frame size; rows_fn(hs, ws, n_frames, **recipe):
    the geometry of the recipe over the whole sampled list -- test_rows (Resize + ThreeCrop, the shipped test recipe), val_rows (Resize +
    CenterCrop), ten_crop_rows, center_crop_rows, resize_rows.
    -> (the sorted distinct frame numbers to decode, the (crops * len(frame_inds), 12) gather table).  Oversampling crops are crop-major
    over the WHOLE sampled list and frame-minor inside it (augmentations.py:512-530, :544-596), so image k * len(frame_inds) + j is crop k
    of sampled frame j and reshaping the outputs to (-1, n_segment) yields the reference's clips; its src is the position of
    frame_inds[j] among the distinct frames."""
    import numpy as np
    frame_inds = np.asarray(frame_inds).reshape(-1)
    if frame_inds.size == 0:
        raise ValueError("video_test_table: no frame indices")
    distinct, inverse = np.unique(frame_inds, return_inverse=True)
    rows = rows_fn(hs, ws, frame_inds.size, **recipe)
    if rows.shape[0] % frame_inds.size:
        raise ValueError("video_test_table: %d rows for %d sampled frames" % (rows.shape[0], frame_inds.size))
    return distinct, gather_rows(rows, np.tile(inverse.reshape(-1), rows.shape[0] // frame_inds.size))


class GatherFramePipeline(JitterFramePipeline):
    """JitterFramePipeline whose output images name their source frame: the table is the 11- or 23-column
    table plus one trailing `src` column (gather_rows, video_test_table), one row per OUTPUT image, and `frames` are the n_src distinct
    decoded frames; image i is cut from frames[src_i].  An 11- or 23-column table means "no gather" (one image per frame) and gives
    JitterFramePipeline's output bit for bit.  Same constructor, `crop_hw`, `to_nchw` and `to_stem`; `n_out` tells the engines how many
    images a (frames, table) pair makes."""

    _COLS = (RESAMPLE_COLS, JITTER_COLS, RESAMPLE_COLS + 1, JITTER_COLS + 1)

    def gathers(self, rows):
        """True when `rows` carries the src column (12 or 24 columns)."""
        return _ncols(rows) in (RESAMPLE_COLS + 1, JITTER_COLS + 1)

    def n_out(self, frames, rows):
        """The number of images (frames, rows) produce: the table's row count with a src column, the frame count otherwise."""
        if self.gathers(rows):
            return int(rows.reshape(-1, rows.shape[-1]).shape[0])
        return math.prod(int(d) for d in frames.shape[:-self.frame_dims])


# ---- decoder-native YUV 4:2:0 frames ---------------------------------------------------------------------------------------------------
YUV_LAYOUTS = {"i420": 0, "nv12": 1}
YUV_STANDARDS = {"bt601": 0, "bt601-full": 1, "bt709": 2}
YUV_ORDERS = {"bgr": 0, "rgb": 1}


def _enum(name, value, table):
    """A name of `table` or its number -> the number."""
    if isinstance(value, str):
        if value.lower() not in table:
            raise ValueError("%s must be one of %s (or %s), got %r" % (name, sorted(table), sorted(table.values()), value))
        return table[value.lower()]
    if isinstance(value, bool) or int(value) != value or int(value) not in table.values():
        raise ValueError("%s must be one of %s (or %s), got %r" % (name, sorted(table), sorted(table.values()), value))
    return int(value)


def _yuv_planes(frames, who):
    """One clip's frames as (Y (T, h, w), U, V (T, ceil(h / 2), ceil(w / 2))) uint8 CPU tensors: the three planes as given, or cut from a
    (T, 3 * h / 2, w) I420 array (what `frame.to_ndarray(format='yuv420p')` returns, stacked; h and w even)."""
    import numpy as np
    if isinstance(frames, (tuple, list)):
        if len(frames) != 3:
            raise ValueError("%s: a clip is (Y, U, V) planes or one (T, 3 * h / 2, w) I420 array" % who)
        y, u, v = (torch.as_tensor(np.asarray(p)) for p in frames)
    else:
        f = torch.as_tensor(np.asarray(frames))
        if f.dim() != 3 or f.shape[1] % 3 or f.shape[2] % 2:
            raise ValueError("%s: an I420 clip must be (T, 3 * h / 2, w) with h and w even, got %s" % (who, tuple(f.shape)))
        t, h, w = f.shape[0], f.shape[1] // 3 * 2, f.shape[2]
        flat, q = f.reshape(t, -1), (h // 2) * (w // 2)
        y = flat[:, :h * w].reshape(t, h, w)
        u = flat[:, h * w:h * w + q].reshape(t, h // 2, w // 2)
        v = flat[:, h * w + q:].reshape(t, h // 2, w // 2)
    if y.dim() != 3 or any(p.dtype != torch.uint8 for p in (y, u, v)):
        raise ValueError("%s: planes must be uint8 (T, h, w) / (T, ceil(h / 2), ceil(w / 2))" % who)
    t, h, w = y.shape
    chroma = (t, (h + 1) // 2, (w + 1) // 2)
    if tuple(u.shape) != chroma or tuple(v.shape) != chroma:
        raise ValueError("%s: a %dx%d luma plane needs %s chroma planes, got %s and %s" % (who, h, w, chroma, tuple(u.shape), tuple(v.shape)))
    return y, u, v


def collate_yuv_frames(groups, layout, pad_to=None, cols=None):
    """collate_frames for YUV 4:2:0 clips.  groups: a list of (frames, rows) per clip -- frames the clip's (Y (T, h_b, w_b), U, V (T,
    ceil(h_b / 2), ceil(w_b / 2))) uint8 planes (numpy or CPU tensors; h_b, w_b may be odd) or one (T, 3 * h_b / 2, w_b) I420 array, rows its
    (T, cols) table -- -> (frames (B, T, 3 * Hs / 2, Ws) uint8 in `layout` ('i420' | 'nv12') at pitch Ws, rows (B * T, cols) int32), CPU
    tensors for Yuv420FramePipeline.  Hs x Ws is the largest clip (or `pad_to` = (Hs, Ws)) rounded up to even; every clip's planes are
    copied into the zero padded planes at the padded pitch and every row keeps its own frame's (hs_i, ws_i).  `cols` defaults to 11."""
    import numpy as np
    lay = _enum("layout", layout, YUV_LAYOUTS)
    cols = RESAMPLE_COLS if cols is None else int(cols)
    if not groups:
        raise ValueError("collate_yuv_frames: no clips")
    planes = [_yuv_planes(f, "collate_yuv_frames") for f, _ in groups]
    rows = [torch.as_tensor(np.asarray(r, dtype=np.int32)).reshape(-1, cols) for _, r in groups]
    t = planes[0][0].shape[0]
    for (y, _, _), r in zip(planes, rows):
        if y.shape[0] != t:
            raise ValueError("collate_yuv_frames: every clip must have T=%d frames, got %d" % (t, y.shape[0]))
        if r.shape[0] != t or bool((r[:, 0] != y.shape[1]).any()) or bool((r[:, 1] != y.shape[2]).any()):
            raise ValueError("collate_yuv_frames: rows do not describe their %s luma planes" % (tuple(y.shape),))
    hs, ws = (max(y.shape[1] for y, _, _ in planes), max(y.shape[2] for y, _, _ in planes)) if pad_to is None else (int(pad_to[0]), int(pad_to[1]))
    if any(y.shape[1] > hs or y.shape[2] > ws for y, _, _ in planes):
        raise ValueError("collate_yuv_frames: a clip is larger than pad_to=%s" % (pad_to,))
    hs, ws = hs + hs % 2, ws + ws % 2
    out = torch.zeros(len(planes), t, hs * 3 // 2, ws, dtype=torch.uint8)
    luma = out[:, :, :hs]
    chroma, q = out.view(len(planes), t, -1)[:, :, hs * ws:], (hs // 2) * (ws // 2)      # views of `out`: chroma rows are pitch / 2 samples
    if lay == 0:
        cu, cv = (c.view(len(planes), t, hs // 2, ws // 2) for c in (chroma[:, :, :q], chroma[:, :, q:]))
    else:
        uv = chroma.view(len(planes), t, hs // 2, ws // 2, 2)
        cu, cv = uv[..., 0], uv[..., 1]
    for b, (y, u, v) in enumerate(planes):
        luma[b, :, :y.shape[1], :y.shape[2]] = y
        cu[b, :, :u.shape[1], :u.shape[2]] = u
        cv[b, :, :v.shape[1], :v.shape[2]] = v
    return out, torch.cat(rows).contiguous()


class Yuv420FramePipeline(GatherFramePipeline):
    """GatherFramePipeline for decoder-native YUV 4:2:0 frames (mvf_frames_yuv420_gather_resample_u8): `frames` is a CUDA uint8 tensor
    (..., 3 * Hs / 2, pitch), one I420 or NV12 image per frame (include/mvfnet_hip.h; collate_yuv_frames builds it), half the bytes of the
    packed frames; the colour conversion runs in the kernel, in front of the resample's taps.  Constructor extras: `layout` 'i420' | 'nv12';
    `standard` 'bt601' (limited range, the default) | 'bt601-full' (yuvj420p) | 'bt709' or 0 / 1 / 2; `order` 'bgr' (default: what the
    raw-frame path stores) | 'rgb', the stored channel order the frames stand for -- ColorJitter's map and `to_rgb` apply to it as they do
    to packed frames; `pitch` = the row length in bytes when it exceeds the frame width (a decoder's aligned surfaces: the tensor's last
    dimension must then be `pitch`, and `width` names the true frame width Ws; default: both are the tensor's last dimension).
    Takes the 11-, 23-, 12- and 24-column tables (without the src column: one image per frame) and gives, bit for bit, GatherFramePipeline's
    output for the converted packed frames.  Same `crop_hw`, `to_nchw`, `to_stem`, `n_out`, `gathers` and `center_window`."""

    frame_dims = 2

    def __init__(self, *args, layout="i420", standard=0, order="bgr", pitch=None, width=None, **kwargs):
        super().__init__(*args, **kwargs)
        self.layout, self.standard, self.order = _enum("layout", layout, YUV_LAYOUTS), _enum("standard", standard, YUV_STANDARDS), _enum("order", order, YUV_ORDERS)
        self.pitch = None if pitch is None else int(pitch)
        self.width = None if width is None else int(width)
        if self.pitch is not None and (self.pitch < 2 or self.pitch % 2):
            raise ValueError("Yuv420FramePipeline: pitch=%d must be even" % self.pitch)
        if self.width is not None and (self.width < 1 or (self.pitch is not None and self.width > self.pitch)):
            raise ValueError("Yuv420FramePipeline: width=%d must lie in [1, pitch]" % self.width)

    def _source(self, frames):
        """-> (the frames flattened to (n_src, 3 * Hs / 2, pitch) contiguous, n_src, Hs, Ws)."""
        if frames.dtype != torch.uint8 or frames.dim() < 2 or not frames.is_cuda:
            raise TypeError("Yuv420FramePipeline expects a CUDA uint8 tensor (..., 3 * Hs / 2, pitch) of YUV 4:2:0 frames, got %s %s"
                            % (frames.dtype, tuple(frames.shape)))
        rows3, pitch = int(frames.shape[-2]), int(frames.shape[-1])
        if rows3 < 3 or rows3 % 3 or pitch % 2:
            raise ValueError("Yuv420FramePipeline: a frame is 3 * Hs / 2 rows of an even pitch, Hs even; got %d x %d" % (rows3, pitch))
        if self.pitch is not None and pitch != self.pitch:
            raise ValueError("Yuv420FramePipeline: the frames' rows are %d bytes, not pitch=%d" % (pitch, self.pitch))
        ws = pitch if self.width is None else self.width
        if ws > pitch:
            raise ValueError("Yuv420FramePipeline: width=%d exceeds the frames' %d-byte rows" % (ws, pitch))
        f = frames.reshape(-1, rows3, pitch).contiguous()
        return f, f.shape[0], rows3 // 3 * 2, ws

    def _launch(self, f, n_src, hs, ws, geo, color, src, n, pad, wp, out_stem, out_nchw, dt):
        h, w = self.crop_hw
        check(lib.mvf_frames_yuv420_gather_resample_u8(f.data_ptr(), n_src, hs, ws, f.shape[2], self.layout, self.standard, self.order, _ptr(src), n,
                                                       geo.data_ptr(), _ptr(color), h, w, self.mean, self.std, int(self.to_rgb), int(self.div_255),
                                                       pad, wp, out_stem, out_nchw, dt, torch.cuda.current_stream().cuda_stream),
              "mvf_frames_yuv420_gather_resample_u8")


# ---- addressed frames: every image carries the offsets and pitches of its planes --------------------------------------------------------
ADDR_COLS = 5               # (o0, p0, o1, o2, p1): see include/mvfnet_hip.h mvf_frames_addressed_resample_u8
FRAME_FORMATS = {"packed": 0, "i420": 1, "nv12": 2}


def address_rows(rows, addr):
    """(n, 11) or (n, 23) int32 rows + (n, 5) int32 address rows (o0, p0, o1, o2, p1) -> ONE (n, 16) or (n, 28) int32 table, the address
    as the trailing columns: output image i is cut from the planes at those byte offsets and pitches of the buffer handed to
    AddressedFramePipeline.  A (n, 12) or (n, 24) gather table (gather_rows, video_test_table) is taken with ONE address row per SOURCE
    frame, (n_src, 5): its `src` column is replaced by addr[src]."""
    import numpy as np
    rows, addr = np.asarray(rows, dtype=np.int32), np.asarray(addr)
    if rows.ndim != 2 or rows.shape[1] not in (RESAMPLE_COLS, JITTER_COLS, RESAMPLE_COLS + 1, JITTER_COLS + 1):
        raise ValueError("address_rows: rows must have %d, %d, %d or %d columns, got %s"
                         % (RESAMPLE_COLS, JITTER_COLS, RESAMPLE_COLS + 1, JITTER_COLS + 1, rows.shape))
    if addr.ndim != 2 or addr.shape[1] != ADDR_COLS:
        raise ValueError("address_rows: addr must be (n, %d), got %s" % (ADDR_COLS, addr.shape))
    if addr.size and (addr.min() < np.iinfo(np.int32).min or addr.max() > np.iinfo(np.int32).max):
        raise ValueError("address_rows: offsets and pitches must fit int32")
    addr = addr.astype(np.int32)
    if rows.shape[1] in (RESAMPLE_COLS + 1, JITTER_COLS + 1):
        rows, src = rows[:, :-1], rows[:, -1]
        if src.size and (src.min() < 0 or src.max() >= addr.shape[0]):
            raise ValueError("address_rows: a source frame is not one of the %d addressed frames" % addr.shape[0])
        addr = addr[src]
    elif addr.shape[0] != rows.shape[0]:
        raise ValueError("address_rows: %d address rows for %d rows" % (addr.shape[0], rows.shape[0]))
    return np.concatenate([rows, addr], axis=1)


def split_address_rows(table):
    """The inverse of address_rows on the host: (n, 16) or (n, 28) int32 -> ((n, 11) or (n, 23) int32, (n, 5) int32 addr)."""
    import numpy as np
    table = np.asarray(table, dtype=np.int32)
    if table.ndim != 2 or table.shape[1] not in (RESAMPLE_COLS + ADDR_COLS, JITTER_COLS + ADDR_COLS):
        raise ValueError("split_address_rows: the table must have %d or %d columns, got %s"
                         % (RESAMPLE_COLS + ADDR_COLS, JITTER_COLS + ADDR_COLS, table.shape))
    return table[:, :-ADDR_COLS].copy(), table[:, -ADDR_COLS:].copy()


def check_addresses(rows, addr, format, frames_bytes):
    """The address rows (n, 5) of images whose geometry rows (n, >= 2: hs_i, ws_i lead) are `rows`, against a buffer of frames_bytes bytes
    in `format` ('packed' | 'i420' | 'nv12' or 0 / 1 / 2).  Returns silently, or raises ValueError naming the first bad row.  Required:
    offsets >= 0; pitches >= the plane's row bytes (3 ws_i packed; ws_i luma; ceil(ws_i / 2) I420 chroma, 2 ceil(ws_i / 2) NV12 chroma);
    the last byte of every plane < frames_bytes; the columns the format does not use 0; 1 <= frames_bytes < 2^31.
    numpy arrays or tensors; the arithmetic is int64 torch on the tensors' own device (AddressedFramePipeline runs it on the GPU)."""
    import numpy as np
    fmt, frames_bytes = _enum("format", format, FRAME_FORMATS), int(frames_bytes)
    if frames_bytes < 1 or frames_bytes >= (1 << 31):
        raise ValueError("check_addresses: frames_bytes=%d must lie in [1, 2^31): offsets are int32" % frames_bytes)
    rows = rows if isinstance(rows, torch.Tensor) else torch.as_tensor(np.asarray(rows))
    addr = addr if isinstance(addr, torch.Tensor) else torch.as_tensor(np.asarray(addr))
    if addr.dim() != 2 or addr.shape[1] != ADDR_COLS or rows.dim() != 2 or rows.shape[1] < 2 or rows.shape[0] != addr.shape[0]:
        raise ValueError("check_addresses: (n, >= 2) geometry rows and (n, %d) address rows, got %s and %s" % (ADDR_COLS, tuple(rows.shape), tuple(addr.shape)))
    hs, ws = rows[:, 0].to(torch.int64), rows[:, 1].to(torch.int64)
    o0, p0, o1, o2, p1 = addr.to(device=rows.device, dtype=torch.int64).unbind(1)
    ch, cw = (hs + 1) // 2, (ws + 1) // 2
    # (offset, pitch, rows, row bytes) of every plane, and the columns that must be 0
    if fmt == 0:
        planes, unused = [(o0, p0, hs, 3 * ws)], (o1, o2, p1)
    elif fmt == 1:
        planes, unused = [(o0, p0, hs, ws), (o1, p1, ch, cw), (o2, p1, ch, cw)], ()
    else:
        planes, unused = [(o0, p0, hs, ws), (o1, p1, ch, 2 * cw)], (o2,)
    def any_of(masks):
        out = torch.zeros_like(hs, dtype=torch.bool)
        for m in masks:
            out = out | m
        return out
    faults = {"a frame size below 1": (hs < 1) | (ws < 1),
              "a negative offset": any_of(o < 0 for o, _, _, _ in planes),
              "a pitch below the plane's row bytes": any_of(p < rb for _, p, _, rb in planes),
              "a plane that ends past frames_bytes=%d" % frames_bytes: any_of(o + (n - 1) * p + rb > frames_bytes for o, p, n, rb in planes),
              "a non-zero column the format does not use": any_of(u != 0 for u in unused)}
    bad = any_of(faults.values())
    if bool(bad.any()):
        i = int(bad.nonzero()[0, 0])
        why = [k for k, v in faults.items() if bool(v[i])]
        raise ValueError("check_addresses: row %d, a %dx%d %s frame at (o0, p0, o1, o2, p1) = %s: %s"
                         % (i, int(hs[i]), int(ws[i]), sorted(FRAME_FORMATS, key=FRAME_FORMATS.get)[fmt], addr[i].tolist(), "; ".join(why)))


def _round_up(v, a):
    return (v + a - 1) // a * a


def collate_addressed_frames(groups, format, slot_bytes=None, pitch_align=1, plane_align=64, fill=0, cols=None):
    """collate_frames / collate_yuv_frames without the padding to a bounding box.  groups: a list of (frames, rows) per clip -- for
    format 'packed' frames (T, h_b, w_b, 3) uint8, for 'i420' / 'nv12' the clip's (Y, U, V) planes or one (T, 3 * h_b / 2, w_b) I420 array
    (as collate_yuv_frames), rows its (T, cols) table, cols 11 (default) or 23 -- -> (frames (B, T, S) uint8, table (B * T, cols + 5)
    int32), CPU tensors for AddressedFramePipeline.  Every frame lies in its own slot of S bytes at its OWN size and pitch: row pitches
    are the row bytes rounded up to `pitch_align`, every plane starts at a multiple of `plane_align` in its slot, and S is the largest
    frame's byte count rounded up to `plane_align` -- or `slot_bytes`, so a prefetcher's pinned buffers keep their shape (ValueError when a
    frame does not fit).  The table's offsets count from the start of the whole tensor, which stays dense (B, T, S) so that the engines'
    B, T logic and the stream split work on it unchanged.  Two orientations of one resolution cost no padding; frames of different areas
    waste only the difference in area.  Bytes no plane owns are `fill`."""
    import numpy as np
    fmt = _enum("format", format, FRAME_FORMATS)
    cols = RESAMPLE_COLS if cols is None else int(cols)
    pitch_align, plane_align = int(pitch_align), int(plane_align)
    if cols not in (RESAMPLE_COLS, JITTER_COLS) or pitch_align < 1 or plane_align < 1:
        raise ValueError("collate_addressed_frames: cols must be %d or %d and the alignments positive" % (RESAMPLE_COLS, JITTER_COLS))
    if not groups:
        raise ValueError("collate_addressed_frames: no clips")
    clips = []                                                    # per clip: [(plane (T, n, row bytes) uint8, pitch)], ...
    for f, _ in groups:
        if fmt == 0:
            f = torch.as_tensor(np.asarray(f))
            if f.dtype != torch.uint8 or f.dim() != 4 or f.shape[-1] != 3:
                raise ValueError("collate_addressed_frames: a packed clip must be (T, h, w, 3) uint8, got %s %s" % (f.dtype, tuple(f.shape)))
            clips.append((f.shape[1], f.shape[2], [f.reshape(f.shape[0], f.shape[1], -1)]))
        else:
            y, u, v = _yuv_planes(f, "collate_addressed_frames")
            clips.append((y.shape[1], y.shape[2], [y, u, v] if fmt == 1 else [y, torch.stack((u, v), dim=-1).reshape(u.shape[0], u.shape[1], -1)]))
    rows = [torch.as_tensor(np.asarray(r, dtype=np.int32)).reshape(-1, cols) for _, r in groups]
    t = clips[0][2][0].shape[0]
    layouts = []                                                  # per clip: [(offset in the slot, pitch)] per plane, and the frame's bytes
    for (h, w, planes), r in zip(clips, rows):
        if planes[0].shape[0] != t:
            raise ValueError("collate_addressed_frames: every clip must have T=%d frames, got %d" % (t, planes[0].shape[0]))
        if r.shape[0] != t or bool((r[:, 0] != h).any()) or bool((r[:, 1] != w).any()):
            raise ValueError("collate_addressed_frames: rows do not describe their %dx%d frames" % (h, w))
        at, lay = 0, []
        for pl in planes:
            pitch = _round_up(pl.shape[2], pitch_align)
            at = _round_up(at, plane_align)
            lay.append((at, pitch))
            at += pl.shape[1] * pitch
        layouts.append((lay, at))
    need = _round_up(max(n for _, n in layouts), plane_align)
    slot = need if slot_bytes is None else int(slot_bytes)
    if slot < max(n for _, n in layouts):
        raise ValueError("collate_addressed_frames: a frame of %d bytes does not fit slot_bytes=%d" % (max(n for _, n in layouts), slot))
    if len(clips) * t * slot >= (1 << 31):
        raise ValueError("collate_addressed_frames: %d x %d slots of %d bytes exceed the 2^31 bytes int32 offsets address" % (len(clips), t, slot))
    out = torch.full((len(clips), t, slot), int(fill), dtype=torch.uint8)
    addr = np.zeros((len(clips), t, ADDR_COLS), dtype=np.int64)
    base = (np.arange(len(clips) * t, dtype=np.int64) * slot).reshape(len(clips), t)
    for b, ((h, w, planes), (lay, _)) in enumerate(zip(clips, layouts)):
        for pl, (at, pitch) in zip(planes, lay):
            out[b, :, at:at + pl.shape[1] * pitch].view(t, pl.shape[1], pitch)[:, :, :pl.shape[2]] = pl
        addr[b, :, 0], addr[b, :, 1] = base[b] + lay[0][0], lay[0][1]
        if fmt != 0:
            addr[b, :, 2], addr[b, :, 4] = base[b] + lay[1][0], lay[1][1]
        if fmt == 1:
            addr[b, :, 3] = base[b] + lay[2][0]
    table = torch.cat([torch.cat(rows), torch.from_numpy(addr.reshape(-1, ADDR_COLS).astype(np.int32))], dim=1).contiguous()
    return out, table


class AddressedFramePipeline(GatherFramePipeline):
    """GatherFramePipeline over frames where and how the decoder left them (mvf_frames_addressed_resample_u8): `frames` is ANY contiguous
    CUDA uint8 tensor, taken as one flat byte buffer (collate_addressed_frames builds a (B, T, S) one), and the table is the 11- or 23-column
    table plus five trailing address columns (address_rows): (o0, p0, o1, o2, p1), the byte offsets and row pitches of the planes output
    image i is cut from (include/mvfnet_hip.h).  One row per OUTPUT image; rows may name the same planes (a video's clips and crops), and
    the frames of one launch may differ in size, pitch and plane placement.  Constructor extras: `format` 'packed' (3-byte pixels in stored
    channel order, what GatherFramePipeline takes) | 'i420' | 'nv12' or 0 / 1 / 2; `standard` and `order` as Yuv420FramePipeline ('packed'
    ignores both).  Gives, bit for bit, GatherFramePipeline's (Yuv420FramePipeline's) output on the dense batch that holds the same frames.
    Every table is checked before the launch: the geometry against each row's own (hs_i, ws_i), the addresses with check_addresses.
    Same `crop_hw`, `to_nchw`, `to_stem` and `n_out`; `gathers` is true for its tables: they name their source, so the engines hand every
    stream's chain the whole buffer and a slice of the table."""

    frame_dims = 1
    _COLS = (RESAMPLE_COLS + ADDR_COLS, JITTER_COLS + ADDR_COLS)

    def __init__(self, *args, format="packed", standard=0, order="bgr", **kwargs):
        super().__init__(*args, **kwargs)
        self.format, self.standard, self.order = _enum("format", format, FRAME_FORMATS), _enum("standard", standard, YUV_STANDARDS), _enum("order", order, YUV_ORDERS)

    def gathers(self, rows):
        """True when `rows` carries the address columns (16 or 28 columns)."""
        return _ncols(rows) in self._COLS

    def _source(self, frames):
        """-> (the frames as one flat byte buffer, its byte count, None, None): there is no shared frame extent."""
        if frames.dtype != torch.uint8 or not frames.is_cuda:
            raise TypeError("AddressedFramePipeline expects a CUDA uint8 tensor (any shape: one flat byte buffer), got %s %s" % (frames.dtype, tuple(frames.shape)))
        f = frames.contiguous().reshape(-1)
        return f, f.numel(), None, None

    def _parse(self, table, frames_bytes, hs, ws):
        t = self._as_table(table)
        if t.shape[0] < 1:
            raise ValueError("AddressedFramePipeline: an empty table")
        t, addr = t[:, :-ADDR_COLS], t[:, -ADDR_COLS:].contiguous()
        geo, color = self._geometry(t, None, None)
        check_addresses(geo, addr, self.format, frames_bytes)
        return geo, color, addr

    def _launch(self, f, frames_bytes, hs, ws, geo, color, addr, n, pad, wp, out_stem, out_nchw, dt):
        h, w = self.crop_hw
        check(lib.mvf_frames_addressed_resample_u8(f.data_ptr(), frames_bytes, self.format, self.standard, self.order, n, geo.data_ptr(), addr.data_ptr(),
                                                   _ptr(color), h, w, self.mean, self.std, int(self.to_rgb), int(self.div_255), pad, wp, out_stem, out_nchw,
                                                   dt, torch.cuda.current_stream().cuda_stream), "mvf_frames_addressed_resample_u8")


# ---- frame-index arithmetic (host side; reference codes/datasets/pipelines/loading.py:11-131) ------------------------------------
def _train_offsets(total_frames, span, num_clips, rng):
    """SampleFrames._sample_clips (loading.py:35-60): start offsets of `num_clips` training clips of `span = clip_len * frame_interval`
    source frames.  Three cases, in the reference's order: equal segments with one random shift each; sorted random starts when the
    segments would be empty but the video is longer than max(num_clips, span); otherwise every clip starts at frame 0.
    Draws: ONE `randint(high, size=num_clips)` call in the first two cases, none in the third."""
    import numpy as np
    room = total_frames - span + 1
    seg = room // num_clips
    if seg > 0:
        return np.arange(num_clips, dtype=np.int64) * seg + np.asarray(rng.randint(seg, size=num_clips), dtype=np.int64)
    if total_frames > max(num_clips, span):
        return np.sort(np.asarray(rng.randint(room, size=num_clips), dtype=np.int64))
    return np.zeros(num_clips, dtype=np.int64)


def _test_offsets(total_frames, span, num_clips, sth_samples, rng):
    """SampleFrames._test_sample_clips (loading.py:62-94).  sth_samples 1: segment centres int(tick / 2 + tick * k) (zeros when
    tick <= 0); 2: the centres followed by the segment starts int(tick * k), no tick test; 10: ten training draws in a row; any other
    value s: the centres, then s - 1 rows of k * floor(room / num_clips) + randint(floor(room / num_clips))."""
    import numpy as np
    room = total_frames - span + 1
    tick = room / float(num_clips)
    centres = [int(tick / 2.0 + tick * k) for k in range(num_clips)]
    if sth_samples == 1:
        return np.array(centres, dtype=np.int64) if tick > 0 else np.zeros(num_clips, dtype=np.int64)
    if sth_samples == 2:
        return np.array(centres + [int(tick * k) for k in range(num_clips)], dtype=np.int64)
    if sth_samples == 10:
        return np.concatenate([_train_offsets(total_frames, span, num_clips, rng) for _ in range(10)])
    seg = room // num_clips                                   # the reference's `// float(num_clips)`: same value, as a float
    rows = [np.array(centres, dtype=np.int64)]
    for _ in range(sth_samples - 1):
        rows.append(np.arange(num_clips, dtype=np.int64) * seg + np.asarray(rng.randint(float(seg), size=num_clips), dtype=np.int64))
    return np.concatenate(rows)


def sample_frame_inds(total_frames, clip_len, frame_interval=1, num_clips=1, test_mode=False, temporal_jitter=False, sth_samples=1, rng=None):
    """The frame indices `SampleFrames(clip_len, frame_interval, num_clips, temporal_jitter, sth_samples)` writes to
    results['frame_inds'] (loading.py:96-116): clip-major, frame-minor int64 array of len(offsets) * clip_len entries --
    offset + frame * frame_interval (+ ONE jitter draw `randint(frame_interval, size=clip_len)` shared by all clips when
    temporal_jitter), clamped to total_frames - 1.  `rng`: numpy.random (default, the reference's global generator) or a RandomState."""
    import numpy as np
    rng = rng if rng is not None else np.random
    span = clip_len * frame_interval
    if test_mode:
        offs = _test_offsets(total_frames, span, num_clips, sth_samples, rng)
    else:
        offs = _train_offsets(total_frames, span, num_clips, rng)
    inds = offs[:, None] + np.arange(clip_len, dtype=np.int64)[None, :] * frame_interval
    if temporal_jitter:
        inds = inds + np.asarray(rng.randint(frame_interval, size=clip_len), dtype=np.int64)[None, :]
    return np.minimum(inds.reshape(-1), total_frames - 1).astype(np.int64)


class SampleFrames(object):
    """Pipeline step with the reference's name, constructor and result keys (loading.py:11-131); `total_frames` must be in `results`
    (the reference's fallback opens the video with mmcv.VideoReader: decoding stays on the host, out of this repo's scope)."""

    def __init__(self, clip_len, frame_interval=1, num_clips=1, temporal_jitter=False, sth_samples=1):
        self.clip_len, self.frame_interval, self.num_clips = clip_len, frame_interval, num_clips
        self.temporal_jitter, self.sth_samples = temporal_jitter, sth_samples

    def __call__(self, results):
        if "total_frames" not in results:
            raise KeyError("SampleFrames: results['total_frames'] is required (video probing is not part of this build)")
        results["frame_inds"] = sample_frame_inds(results["total_frames"], self.clip_len, self.frame_interval, self.num_clips,
                                                  bool(results["test_mode"]), self.temporal_jitter, self.sth_samples)
        results["clip_len"], results["frame_interval"] = self.clip_len, self.frame_interval
        results["num_clips"], results["sth_samples"] = self.num_clips, self.sth_samples
        return results


class Normalize(object):
    """Pipeline step with the reference's name, constructor and result keys (augmentations.py:343-376) over the device kernel: here
    `img_group` is a CUDA uint8 tensor (..., H, W, 3) of decoded frames and the result is the (n, 3, H, W) fp32 tensor the reference's
    Normalize + FormatShape('NCHW') produce -- float32(img) [/ 255] -> channel swap when to_rgb -> subtract float32(mean) -> multiply by
    float32(1 / float64(std)), each a single rounded fp32 operation (mvf_frames_prep_u8)."""

    def __init__(self, mean, std, div_255=False, to_rgb=False):
        import numpy as np
        self.mean, self.std = np.array(mean, dtype=np.float32), np.array(std, dtype=np.float32)
        self.div_255, self.to_rgb = div_255, to_rgb

    def __call__(self, results):
        f = results["img_group"]
        pipe = FramePipeline(self.mean.tolist(), self.std.tolist(), to_rgb=self.to_rgb, div_255=self.div_255, crop_size=(f.shape[-2], f.shape[-3]))
        results["img_group"] = pipe.to_nchw(f)
        results["img_norm_cfg"] = dict(mean=self.mean, std=self.std, div_255=self.div_255, to_rgb=self.to_rgb)
        return results
