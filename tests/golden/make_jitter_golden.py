#!/usr/bin/env python3
"""Golden vectors for the TSN-style augmentations of the input pipeline, produced by the REFERENCE's own classes
(codes/datasets/pipelines/augmentations.py: MultiScaleCrop :71-192, ColorJitter :238-339, Normalize :343-396, TenCrop :544-596,
RandomRescaledCrop :672-707) imported with the mmcv / cv2 placeholders of make_golden.py.  As in make_resize_golden.py,
`mmcv.imcrop` / `imresize` / `imrescale` / `imflip` are RECORDING stand-ins that log what the reference hands them and apply the
documented mmcv 0.4.3 geometry (pixels are not resampled: a resized image holds its own (row, column) indices, so later slicing shows
in the output); as in make_normalize_golden.py, cv2.cvtColor / subtract / multiply are numpy stand-ins with OpenCV's documented CV_32F
semantics (what that maker pins and does not pin about third-party arithmetic applies here unchanged).

What this pins (stored arrays = data only), one row per case:
  msc_hw_seed (H, W, seed)   msc_args (in_w, in_h, max_distort, fix_crop, more_fix_crop)   msc_scales (NaN-padded; all NaN = default)
  msc_box     [x1, y1, x2, y2] handed to imcrop (before clipping)   msc_patch (h, w) of the clipped patch
  msc_size    (w, h) handed to imresize   msc_next a follow-up random.random(): pins HOW MANY draws were made
  tc_case     (H, W, crop_w, crop_h, n_frames)
  tc_boxes    (case, 5 * n_frames, 4) boxes in imcrop call order
  tc_out      (case, 10 * n_frames, 5) per returned image: the (row, column, frame) its top-left pixel came from, the column of its
              top-right pixel (smaller than the left one = mirrored) and the row of its bottom-left pixel; tc_shape (case, 2) its (h, w)
  rsc_hw_seed (H, W, seed)   rsc_args (input_size[0], input_size[1], scale[0], scale[1])   rsc_factor the float handed to imrescale
  rsc_resized (rows, cols) of the rescaled image   rsc_slice (row0, col0, rows, cols) of the slice returned   rsc_next follow-up draw
  cj_seed, cj_aug (color_space_aug), cj_frames (case, 4, 6, 5, 3) uint8, cj_out (case, 4, 6, 5, 3) float32 = ColorJitter then
  Normalize(K400 mean / std, to_rgb=True); cj_dtype the dtype NAME of ColorJitter's own output per case (the reference leans on
  numpy's promotion of uint8 + float32; numpy_version says which numpy decided); cj_coins (case, 4, 5) the per-frame coin results
  (brightness, order, then the three step coins in the order taken; all zero without colour-space augmentation);
  cj_next (random.random(), np.random.rand()) follow-up draws
  cj_rel_err  over the color_space_aug cases, max |restatement - reference| / (S_c / std_c) with S_c = sum_k |M[c][k]| * 255 + |b[c]| + 255
              (tests/jitter_numpy.py fed with mvfnet_amd.preprocess.color_jitter_table under the same seeds)

Run in the build container: python tests/golden/make_jitter_golden.py"""
import io
import os
import random
import sys
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402

mg._install_stubs()
import cv2  # noqa: E402  (the placeholder modules)
import mmcv  # noqa: E402

LOG = []


def imcrop(img, bboxes, scale=1.0, pad_fill=None):
    b = np.asarray(bboxes)
    LOG.append(("crop", tuple(float(v) for v in b.reshape(-1))))
    x1, y1, x2, y2 = (int(v) for v in b.reshape(-1).astype(np.int32))
    x1, x2 = (max(min(v, img.shape[1] - 1), 0) for v in (x1, x2))
    y1, y2 = (max(min(v, img.shape[0] - 1), 0) for v in (y1, y2))
    return img[y1:y2 + 1, x1:x2 + 1]


def index_image(h, w, frame=0):
    out = np.empty((h, w, 3), dtype=np.int32)
    out[..., 0], out[..., 1], out[..., 2] = np.arange(h)[:, None], np.arange(w)[None, :], frame
    return out


def imresize(img, size, return_scale=False, interpolation="bilinear"):
    LOG.append(("resize", tuple(size), img.shape[:2]))
    w, h = int(size[0]), int(size[1])
    out = index_image(h, w)
    if not return_scale:
        return out
    return out, w / img.shape[1], h / img.shape[0]


def imrescale(img, scale, return_scale=False, interpolation="bilinear"):
    LOG.append(("rescale", scale, type(scale).__name__))
    h, w = img.shape[:2]
    if isinstance(scale, (float, int)):
        f = scale
    else:
        f = min(max(scale) / max(h, w), min(scale) / min(h, w))
    out = imresize(img, (int(w * float(f) + 0.5), int(h * float(f) + 0.5)))
    return (out, f) if return_scale else out


def cvtColor(src, code, dst=None):
    out = src[..., ::-1].copy()
    if dst is not None:
        dst[...] = out
        return dst
    return out


def subtract(src1, src2, dst=None):
    out = (src1 - np.float32(np.asarray(src2).reshape(-1))).astype(np.float32)      # the scalar converted to the CV_32F working type
    if dst is not None:
        dst[...] = out
        return dst
    return out


def multiply(src1, src2, dst=None):
    out = (src1 * np.float32(np.asarray(src2).reshape(-1))).astype(np.float32)
    if dst is not None:
        dst[...] = out
        return dst
    return out


mmcv.imcrop, mmcv.imresize, mmcv.imrescale = imcrop, imresize, imrescale
mmcv.imflip = lambda img, direction="horizontal": img[:, ::-1]
mmcv.iminvert = lambda img: 255 - img
mmcv.is_tuple_of = lambda seq, t: isinstance(seq, tuple) and all(isinstance(v, t) for v in seq)
mmcv.is_list_of = lambda seq, t: isinstance(seq, list) and all(isinstance(v, t) for v in seq)
mmcv.impad_to_multiple = None
mmcv.rescale_size = None
cv2.COLOR_BGR2RGB = 4
cv2.cvtColor, cv2.subtract, cv2.multiply = cvtColor, subtract, multiply

sys.path.insert(0, mg.REF)
from codes.datasets.pipelines import augmentations as aug  # noqa: E402

out = {}

# ---- MultiScaleCrop ------------------------------------------------------------------------------------------------------------------
# (H, W, input_size): the K400 / UCF frame shapes, a portrait one, 258 rows (int(258 * .875) = 225 snaps to 224), 226 rows (the full
# size snaps), 128 x 171 with a 112 input (int(128 * .875) = 112) and with a non-square (w, h) input
MSC_FRAMES = [(256, 340, 224), (240, 320, 224), (128, 171, 224), (340, 256, 224), (258, 344, 224), (226, 300, 224), (128, 171, 112),
              (128, 171, (112, 96))]
# (fix_crop, more_fix_crop, max_distort, scales)
MSC_CFG = [(True, True, 1, None), (True, False, 1, None), (False, True, 1, None), (False, False, 0, None), (True, True, 0, None),
           (True, True, 2, None), (False, False, 2, [1, .8, .5])]
rows = {k: [] for k in ("msc_hw_seed", "msc_args", "msc_scales", "msc_box", "msc_patch", "msc_size", "msc_next")}
snaps = 0


def run_msc(H, W, size, fix, more, md, scales, seed):
    img = np.zeros((H, W, 3), dtype=np.uint8)
    random.seed(seed)
    del LOG[:]
    step = aug.MultiScaleCrop(size, scales=scales, max_distort=md, fix_crop=fix, more_fix_crop=more)
    res = step(dict(img_group=[img, img], modality="RGB"))
    nxt = random.random()
    crops = [e[1] for e in LOG if e[0] == "crop"]
    sizes = [e for e in LOG if e[0] == "resize"]
    assert len(crops) == 2 and crops[0] == crops[1] and len(sizes) == 2 and sizes[0] == sizes[1]
    in_w, in_h = step.input_size
    assert res["img_group"][0].shape[:2] == (in_h, in_w)
    rows["msc_hw_seed"].append((H, W, seed))
    rows["msc_args"].append((in_w, in_h, md, int(fix), int(more)))
    rows["msc_scales"].append(tuple(scales) + (np.nan,) * (4 - len(scales)) if scales is not None else (np.nan,) * 4)
    rows["msc_box"].append(crops[0])
    rows["msc_patch"].append(sizes[0][2])
    rows["msc_size"].append(sizes[0][1])
    rows["msc_next"].append(nxt)
    raw = [int(min(H, W) * x) for x in step.scales]
    return int((crops[0][2] - crops[0][0] + 1 == in_w and in_w not in raw) or (crops[0][3] - crops[0][1] + 1 == in_h and in_h not in raw))


for (H, W, size) in MSC_FRAMES:
    for (fix, more, md, scales) in MSC_CFG:
        for seed in (0, 5):
            snaps += run_msc(H, W, size, fix, more, md, scales, seed)
for seed in range(1, 7):             # more draws on the two frames with a size within 3 of the input: the snapped pair gets chosen
    snaps += run_msc(258, 344, 224, True, True, 1, None, seed) + run_msc(226, 300, 224, False, True, 1, None, seed)
for seed in range(6):                # 222 rows: the full size snaps UP to 224, past the frame; the fixed offsets go negative, imcrop clips
    snaps += run_msc(222, 300, 224, True, True, 1, None, seed)
assert snaps >= 4, "no case took a crop size that was snapped to the input size"
assert any(p[0] < 224 and b[3] - b[1] + 1 == 224 for p, b in zip(rows["msc_patch"], rows["msc_box"])), "no clipped box"
for k, v in rows.items():
    out[k] = np.array(v, dtype=np.int64 if k in ("msc_hw_seed", "msc_args", "msc_patch", "msc_size") else np.float64)
n_msc = len(rows["msc_next"])

# ---- TenCrop -------------------------------------------------------------------------------------------------------------------------
TC = [(256, 340, 224), (240, 320, 224), (128, 171, 112), (340, 256, (200, 224)), (224, 224, 224), (37, 53, (20, 30))]
NF = 2
tc_case, tc_boxes, tc_out, tc_shape = [], [], [], []
for (H, W, size) in TC:
    del LOG[:]
    step = aug.TenCrop(size)
    res = step(dict(img_group=[index_image(H, W, f) for f in range(NF)], modality="RGB"))
    cw, ch = step.crop_size
    boxes = [e[1] for e in LOG if e[0] == "crop"]
    assert len(boxes) == 5 * NF and len(res["img_group"]) == 10 * NF
    assert all(im.shape[:2] == (ch, cw) for im in res["img_group"])
    tc_case.append((H, W, cw, ch, NF))
    tc_boxes.append(boxes)
    tc_out.append([(im[0, 0, 0], im[0, 0, 1], im[0, 0, 2], im[0, -1, 1], im[-1, 0, 0]) for im in res["img_group"]])
    tc_shape.append((ch, cw))
out["tc_case"], out["tc_shape"] = np.array(tc_case, dtype=np.int64), np.array(tc_shape, dtype=np.int64)
out["tc_boxes"], out["tc_out"] = np.array(tc_boxes, dtype=np.float64), np.array(tc_out, dtype=np.int64)

# ---- RandomRescaledCrop --------------------------------------------------------------------------------------------------------------
RSC = [(256, 340, 224, (256, 320)), (340, 256, 224, (256, 320)), (240, 320, (224, 200), (256, 320)), (128, 171, (100, 120), (128, 160)),
       (480, 640, 224, (256, 320)), (300, 300, (200, 224), (224, 256))]
rows = {k: [] for k in ("rsc_hw_seed", "rsc_args", "rsc_factor", "rsc_resized", "rsc_slice", "rsc_next")}
for (H, W, size, scale) in RSC:
    for seed in (0, 3):
        random.seed(seed)
        del LOG[:]
        step = aug.RandomRescaledCrop(size, scale=scale)
        res = step(dict(img_group=[index_image(H, W, f) for f in range(2)], modality="RGB"))
        nxt = random.random()
        calls = [e for e in LOG if e[0] == "rescale"]
        assert len(calls) == 2 and calls[0] == calls[1] and calls[0][2] == "float"
        resized = [e[1] for e in LOG if e[0] == "resize"][0]
        im = res["img_group"][0]
        assert np.array_equal(im, res["img_group"][1]) and np.array_equal(im[..., :2], index_image(resized[1], resized[0])[
            im[0, 0, 0]:im[0, 0, 0] + im.shape[0], im[0, 0, 1]:im[0, 0, 1] + im.shape[1], :2])
        rows["rsc_hw_seed"].append((H, W, seed))
        rows["rsc_args"].append(tuple(step.input_size) + tuple(scale))
        rows["rsc_factor"].append(calls[0][1])
        rows["rsc_resized"].append((resized[1], resized[0]))
        rows["rsc_slice"].append((im[0, 0, 0], im[0, 0, 1], im.shape[0], im.shape[1]))
        rows["rsc_next"].append(nxt)
for k, v in rows.items():
    out[k] = np.array(v, dtype=np.float64 if k in ("rsc_factor", "rsc_next") else np.int64)

# ---- ColorJitter + Normalize -----------------------------------------------------------------------------------------------------------
MEAN, STD = [123.675, 116.28, 103.53], [58.395, 57.12, 57.375]          # configs/MVFNet/K400/*.py img_norm_cfg, to_rgb=True
T, FH, FW = 4, 6, 5


class RecordingRandom(object):
    """Python's `random` as the reference module sees it, with every uniform(0, 1) coin logged."""

    def __init__(self):
        self.coins = []

    def uniform(self, a, b):
        v = random.uniform(a, b)
        if (a, b) == (0, 1):
            self.coins.append(v > 0.5)
        return v

    def __getattr__(self, name):
        return getattr(random, name)


def cj_frames(seed):
    if seed < 0:                                                        # the corner values only
        return (np.random.RandomState(77).randint(0, 2, size=(T, FH, FW, 3)) * 255).astype(np.uint8)
    return np.random.RandomState(1000 + seed).randint(0, 256, size=(T, FH, FW, 3)).astype(np.uint8)


CJ = [(s, False) for s in range(8)] + [(s, True) for s in range(48)] + [(-1, True), (-1, False)]
rows = {k: [] for k in ("cj_seed", "cj_aug", "cj_frames", "cj_out", "cj_dtype", "cj_coins", "cj_next")}
for seed, space in CJ:
    fr = cj_frames(seed)
    random.seed(abs(seed))
    np.random.seed(abs(seed))
    rec = RecordingRandom()
    aug.random = rec
    try:
        res = aug.ColorJitter(color_space_aug=space)(dict(img_group=[f for f in fr], modality="RGB"))
    finally:
        aug.random = random
    dtypes = sorted(set(str(im.dtype) for im in res["img_group"]))
    res = aug.Normalize(MEAN, STD, to_rgb=True)(res)
    imgs = np.stack(res["img_group"])
    assert imgs.dtype == np.float32 and imgs.shape == fr.shape
    assert len(rec.coins) == (5 * T if space else 0)
    rows["cj_seed"].append(seed)
    rows["cj_aug"].append(int(space))
    rows["cj_frames"].append(fr)
    rows["cj_out"].append(imgs)
    rows["cj_dtype"].append("/".join(dtypes))
    rows["cj_coins"].append(np.array(rec.coins, dtype=np.int64).reshape(T, 5) if space else np.zeros((T, 5), dtype=np.int64))
    rows["cj_next"].append((random.random(), np.random.rand()))
coins = np.stack(rows["cj_coins"])[[i for i, (s, sp) in enumerate(CJ) if sp and s >= 0]].reshape(-1, 5)
for bright in (0, 1):
    assert (coins[:, 0] == bright).any(), "brightness %d never drawn" % bright
for order in (0, 1):                                                    # 1: contrast, saturation, hue   0: saturation, hue, contrast
    sel = coins[coins[:, 1] == order]
    assert len(sel), "order %d never drawn" % order
    for step in range(3):
        for on in (0, 1):
            assert (sel[:, 2 + step] == on).any(), "order %d step %d never %d" % (order, step, on)
out["cj_seed"], out["cj_aug"] = np.array(rows["cj_seed"], dtype=np.int64), np.array(rows["cj_aug"], dtype=np.int64)
out["cj_frames"], out["cj_out"] = np.stack(rows["cj_frames"]), np.stack(rows["cj_out"])
out["cj_dtype"] = np.array(rows["cj_dtype"])
out["cj_coins"], out["cj_next"] = np.stack(rows["cj_coins"]), np.array(rows["cj_next"], dtype=np.float64)
out["numpy_version"] = np.array(np.__version__)

# the distance between the kernel's arithmetic (one float64 composition, applied in fp32) and the reference's chain of fp32 steps
import jitter_numpy as J  # noqa: E402
from mvfnet_amd.preprocess import color_jitter_table  # noqa: E402

worst = 0.0
for i, (seed, space) in enumerate(CJ):
    if not space:
        continue
    random.seed(abs(seed))
    np.random.seed(abs(seed))
    table = color_jitter_table(T, color_space_aug=True)
    got = J.color_normalize(out["cj_frames"][i], table, MEAN, STD, to_rgb=True)
    worst = max(worst, J.scaled_error(got, out["cj_out"][i].transpose(0, 3, 1, 2), table, STD, to_rgb=True))
out["cj_rel_err"] = np.array(worst, dtype=np.float64)

# an .npz (a zip of .npy members) with fixed member timestamps, so that a re-run reproduces the file byte for byte
path = os.path.join(HERE, "jitter_cases.npz")
with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
    for k in sorted(out):
        buf = io.BytesIO()
        np.lib.format.write_array(buf, np.asanyarray(out[k]), allow_pickle=False)
        info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
        info.compress_type = zipfile.ZIP_DEFLATED
        info.external_attr = 0o644 << 16
        z.writestr(info, buf.getvalue())
print("wrote jitter_cases.npz: %d arrays, %d bytes (%d MultiScaleCrop cases, %d snapped; %d ColorJitter cases, dtypes %s; cj_rel_err %.3g)"
      % (len(out), os.path.getsize(path), n_msc, snaps, len(CJ), sorted(set(rows["cj_dtype"])), worst))
