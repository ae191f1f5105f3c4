#!/usr/bin/env python3
"""Golden vectors for whole-video testing from a video's distinct frames, produced by the REFERENCE's own classes
(codes/datasets/pipelines/loading.py SampleFrames :11-131; augmentations.py Resize :13-68, CenterCrop :428-457, ThreeCrop :465-540,
TenCrop :544-596) imported with the mmcv / cv2 placeholders of make_golden.py.  As in make_jitter_golden.py the images are INDEX-CODED --
every pixel holds (row, column, frame number) -- and `mmcv.imcrop` / `imresize` / `imrescale` / `imflip` are stand-ins that apply the
documented mmcv 0.4.3 geometry without resampling: a resized image holds its own (row, column) indices and keeps its frame number, so what
a test recipe returns says, for every output image, which sampled frame it was cut from, where, and whether it was mirrored.

Each case runs SampleFrames(clip_len, frame_interval, num_clips, sth_samples=...) in test mode, "decodes" frame_inds into index images,
and applies one recipe: 0 = Resize((inf, short)) + ThreeCrop (the shipped test recipe), 1 = Resize + CenterCrop (the val recipe),
2 = TenCrop alone, 3 = Resize + TenCrop, 4 = CenterCrop alone.

What this pins (stored arrays = data only), cases stacked:
  gc_args   (case, 11) total_frames, clip_len, frame_interval, num_clips, sth_samples, H, W, recipe, short (0 = no Resize), crop_w, crop_h
  gc_inds   every case's frame_inds, concatenated; gc_inds_off (case + 1,) the offsets
  gc_out    every case's output images in the order the recipe returned them, concatenated, 9 columns per image: the frame number, the
            (row, column) of its top-left pixel in the resized image, the column of its top-right pixel (smaller than the left one =
            mirrored), the row of its bottom-left pixel, its (h, w), and the (rh, rw) of the image the crops were cut from
  gc_out_off (case + 1,) the offsets

Run in the build container: python tests/golden/make_gather_golden.py"""
import io
import os
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

mg._install_stubs()
import mmcv  # noqa: E402  (the placeholder module)

if not hasattr(np, "int"):
    np.int = int          # loading.py:112 `.astype(np.int)`


def index_image(h, w, frame):
    out = np.empty((h, w, 3), dtype=np.int32)
    out[..., 0], out[..., 1], out[..., 2] = np.arange(h)[:, None], np.arange(w)[None, :], frame
    return out


def imcrop(img, bboxes, scale=1.0, pad_fill=None):
    x1, y1, x2, y2 = (int(v) for v in np.asarray(bboxes).reshape(-1).astype(np.int32))
    x1, x2 = (max(min(v, img.shape[1] - 1), 0) for v in (x1, x2))
    y1, y2 = (max(min(v, img.shape[0] - 1), 0) for v in (y1, y2))
    return img[y1:y2 + 1, x1:x2 + 1]


def imresize(img, size, return_scale=False, interpolation="bilinear"):
    w, h = int(size[0]), int(size[1])
    out = index_image(h, w, img[0, 0, 2])
    if not return_scale:
        return out
    return out, w / img.shape[1], h / img.shape[0]


def imrescale(img, scale, return_scale=False, interpolation="bilinear"):
    h, w = img.shape[:2]
    if isinstance(scale, (float, int)):
        f = scale
    else:
        f = min(max(scale) / max(h, w), min(scale) / min(h, w))
    out = imresize(img, (int(w * float(f) + 0.5), int(h * float(f) + 0.5)))
    return (out, f) if return_scale else out


mmcv.imcrop, mmcv.imresize, mmcv.imrescale = imcrop, imresize, imrescale
mmcv.imflip = lambda img, direction="horizontal": img[:, ::-1]
mmcv.iminvert = lambda img: 255 - img
mmcv.is_tuple_of = lambda seq, t: isinstance(seq, tuple) and all(isinstance(v, t) for v in seq)
mmcv.is_list_of = lambda seq, t: isinstance(seq, list) and all(isinstance(v, t) for v in seq)
mmcv.impad_to_multiple = None
mmcv.rescale_size = None

sys.path.insert(0, mg.REF)
from codes.datasets.pipelines.augmentations import CenterCrop, Resize, TenCrop, ThreeCrop  # noqa: E402
from codes.datasets.pipelines.loading import SampleFrames  # noqa: E402

# (total_frames, clip_len, frame_interval, num_clips, sth_samples, H, W, recipe, short, crop (w, h))
CASES = [
    (300, 8, 8, 10, 1, 256, 340, 0, 256, (256, 256)),     # the shipped test recipe: 80 frames, 240 images
    (250, 8, 8, 10, 1, 340, 256, 0, 256, (256, 256)),     # portrait: ThreeCrop's crop_w == img_w branch
    (40, 8, 2, 4, 1, 48, 64, 0, 32, (32, 32)),            # clips SHARE frames: offsets 3, 9, 15, 21, each clip spans 15 frames
    (40, 8, 8, 10, 1, 48, 64, 0, 32, (32, 32)),           # total_frames < span: zero offsets, the clamped index 39 repeats
    (63, 8, 8, 10, 1, 30, 40, 0, 36, (28, 24)),           # tick = 0: ten identical clips; upscaling Resize, ThreeCrop's quarter-step branch
    (80, 8, 2, 2, 2, 48, 64, 0, 32, (32, 32)),            # sth_samples = 2: centres then segment starts
    (12, 8, 2, 2, 2, 64, 48, 0, 40, (40, 40)),            # sth_samples = 2 on a short video (negative tick, clamp)
    (300, 8, 8, 1, 1, 256, 340, 1, 256, (224, 224)),      # the shipped val recipe
    (40, 4, 4, 3, 1, 37, 53, 1, 30, (20, 24)),            # val recipe, non-square crop
    (40, 8, 2, 4, 1, 48, 64, 2, 0, (32, 32)),             # TenCrop, shared frames
    (30, 4, 8, 5, 2, 37, 53, 2, 0, (20, 30)),             # TenCrop, sth_samples = 2, clamped repeats
    (100, 8, 4, 3, 1, 60, 80, 3, 48, (40, 40)),           # Resize + TenCrop
    (40, 8, 8, 10, 1, 48, 64, 4, 0, (32, 32)),            # a bare CenterCrop over repeated frames
]

args, inds, outs = [], [], []
shared = clamped = 0
for (total, clip_len, interval, num_clips, sth, H, W, recipe, short, crop) in CASES:
    res = SampleFrames(clip_len, interval, num_clips, False, sth)(dict(total_frames=total, test_mode=True))
    fi = np.asarray(res["frame_inds"])
    assert fi.dtype == np.int64 and fi.size == num_clips * clip_len * (2 if sth == 2 else 1)
    shared += int(np.unique(fi).size < fi.size)
    clamped += int((fi == total - 1).sum() > 1)
    res["img_group"] = [index_image(H, W, f) for f in fi]           # "decoding": one image per sampled index, repeats included
    res["modality"] = "RGB"
    if short:
        res = Resize((float("inf"), short), keep_ratio=True)(res)
    rh, rw = res["img_group"][0].shape[:2]
    step = {0: ThreeCrop, 1: CenterCrop, 2: TenCrop, 3: TenCrop, 4: CenterCrop}[recipe](crop)
    res = step(res)
    imgs = res["img_group"]
    assert len(imgs) == fi.size * {0: 3, 1: 1, 2: 10, 3: 10, 4: 1}[recipe]
    args.append((total, clip_len, interval, num_clips, sth, H, W, recipe, short, crop[0], crop[1]))
    inds.append(fi)
    outs.append(np.array([(im[0, 0, 2], im[0, 0, 0], im[0, 0, 1], im[0, -1, 1], im[-1, 0, 0], im.shape[0], im.shape[1], rh, rw) for im in imgs],
                         dtype=np.int64))
assert shared >= 3 and clamped >= 2, "the cases must include shared and clamped-repeat frame indices"

out = {"gc_args": np.array(args, dtype=np.int64),
       "gc_inds": np.concatenate(inds), "gc_inds_off": np.cumsum([0] + [len(v) for v in inds]).astype(np.int64),
       "gc_out": np.concatenate(outs), "gc_out_off": np.cumsum([0] + [len(v) for v in outs]).astype(np.int64)}

# an .npz (a zip of .npy members) with fixed member timestamps, so that a re-run reproduces the file byte for byte
path = os.path.join(HERE, "gather_cases.npz")
with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
    for k in sorted(out):
        buf = io.BytesIO()
        np.lib.format.write_array(buf, np.asanyarray(out[k]), allow_pickle=False)
        info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
        info.compress_type = zipfile.ZIP_DEFLATED
        info.external_attr = 0o644 << 16
        z.writestr(info, buf.getvalue())
print("wrote gather_cases.npz: %d cases, %d output images, %d bytes (%d cases with shared frames, %d with clamped repeats)"
      % (len(CASES), len(out["gc_out"]), os.path.getsize(path), shared, clamped))
