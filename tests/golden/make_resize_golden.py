#!/usr/bin/env python3
"""Golden vectors for the resize GEOMETRY of the input pipeline, produced by the REFERENCE's own classes
(codes/datasets/pipelines/augmentations.py: RandomResizedCrop :600-661, Resize :13-68) imported with the mmcv / cv2 placeholders of
make_golden.py -- except that `mmcv.imcrop`, `mmcv.imresize` and `mmcv.imrescale` are RECORDING stand-ins here: they log what the
reference's code hands them and apply the documented mmcv 0.4.3 geometry (imcrop: the box cast to int32 and clipped to the image, then
img[y1:y2+1, x1:x2+1]; imresize(img, (w, h)) -> an h x w image; imrescale: rescale_size's factor and int(x * f + 0.5) rounding) so that
the classes run to completion.  The pixels are not resampled: only shapes travel.

What this pins (stored arrays = data only):
one row per case, cases stacked:
  * rrc_hw_seed       (H, W, random.seed) of the RandomResizedCrop(224) case
  * rrc_box           the [x1, y1, x2, y2] box it hands to imcrop (before mmcv's clipping; the axis-swap quirk can make it overhang)
  * rrc_patch         (h, w) of the clipped patch imcrop returns
  * rrc_size          the (w, h) size handed to imresize
  * rrc_next          a follow-up random.random() draw: pins HOW MANY draws get_params made (10 attempts, the fallback, two randint)
  * resize_hw         (H, W) of the Resize case; resize_scale = the scale handed on (a lone float in column 0, NaN in column 1);
    resize_keep       keep_ratio; resize_call = 0 when it went to imrescale, 1 for imresize; resize_out = the output (h, w)
What it does NOT pin: cv2.resize's pixel arithmetic (INTER_LINEAR) -- third-party code that is not in the build container; the restatement
in tests/resample_numpy.py is the contract for it.

Run in the build container: python tests/golden/make_resize_golden.py"""
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402

mg._install_stubs()
import mmcv  # noqa: E402  (the placeholder module)

LOG = []


def imcrop(img, bboxes, scale=1.0, pad_fill=None):
    b = np.asarray(bboxes)
    LOG.append(("crop", tuple(float(v) for v in b.reshape(-1))))
    x1, y1, x2, y2 = (int(v) for v in b.reshape(-1).astype(np.int32))
    x1, x2 = (max(min(v, img.shape[1] - 1), 0) for v in (x1, x2))
    y1, y2 = (max(min(v, img.shape[0] - 1), 0) for v in (y1, y2))
    return img[y1:y2 + 1, x1:x2 + 1]


def imresize(img, size, return_scale=False, interpolation="bilinear"):
    LOG.append(("resize", tuple(size)))
    w, h = int(size[0]), int(size[1])
    out = np.zeros((h, w) + img.shape[2:], dtype=img.dtype)
    if not return_scale:
        return out
    return out, w / img.shape[1], h / img.shape[0]


def imrescale(img, scale, return_scale=False, interpolation="bilinear"):
    LOG.append(("rescale", scale))
    h, w = img.shape[:2]
    if isinstance(scale, (float, int)):
        f = scale
    else:
        f = min(max(scale) / max(h, w), min(scale) / min(h, w))
    new = (int(w * float(f) + 0.5), int(h * float(f) + 0.5))
    out = imresize(img, new)
    return (out, f) if return_scale else out


mmcv.imcrop = imcrop
mmcv.imresize = imresize
mmcv.imrescale = imrescale
mmcv.imflip = lambda img, direction="horizontal": img[:, ::-1]
mmcv.iminvert = lambda img: 255 - img
mmcv.is_tuple_of = lambda seq, t: isinstance(seq, tuple) and all(isinstance(v, t) for v in seq)
mmcv.is_list_of = lambda seq, t: isinstance(seq, list) and all(isinstance(v, t) for v in seq)
mmcv.impad_to_multiple = None
mmcv.rescale_size = None

sys.path.insert(0, mg.REF)
from codes.datasets.pipelines.augmentations import RandomResizedCrop, Resize  # noqa: E402

# (H, W): the K400 frame shapes (340 x 256 landscape, its portrait twin), odd and small frames, and strongly elongated frames whose ten
# attempts all fail (the centre-square fallback)
SHAPES = [(256, 340), (340, 256), (256, 341), (240, 320), (257, 455), (128, 171), (37, 53), (300, 16), (16, 300), (9, 400), (224, 224), (31, 30)]
SEEDS = [0, 1, 2, 3, 7]

rows = {k: [] for k in ("rrc_hw_seed", "rrc_box", "rrc_patch", "rrc_size", "rrc_next", "resize_hw", "resize_scale", "resize_keep",
                         "resize_call", "resize_out")}
fallbacks = overhangs = 0
for (H, W) in SHAPES:
    for s in SEEDS:
        img = np.zeros((H, W, 3), dtype=np.uint8)
        random.seed(s)
        del LOG[:]
        res = RandomResizedCrop(224)(dict(img_group=[img, img], modality="RGB"))
        nxt = random.random()
        crops = [e[1] for e in LOG if e[0] == "crop"]
        sizes = [e[1] for e in LOG if e[0] == "resize"]
        assert len(crops) == 2 and crops[0] == crops[1] and len(sizes) == 2 and sizes[0] == sizes[1]
        x1, y1, x2, y2 = (int(v) for v in crops[0])
        patch = imcrop(img, np.array(crops[0]))
        del LOG[-1]
        overhangs += int(x2 > W - 1 or y2 > H - 1)
        side = min(H, W)
        fallbacks += int(x2 - x1 + 1 == side and y2 - y1 + 1 == side and x1 == (W - side) // 2 and y1 == (H - side) // 2)
        assert res["img_group"][0].shape[:2] == (sizes[0][1], sizes[0][0])
        rows["rrc_hw_seed"].append((H, W, s))
        rows["rrc_box"].append(crops[0])
        rows["rrc_patch"].append(patch.shape[:2])
        rows["rrc_size"].append(sizes[0])
        rows["rrc_next"].append(nxt)

# Resize: the val / test recipe (np.Inf, 256) keep_ratio, a finite tuple, a float factor, and the exact-size form keep_ratio=False
RESIZE = [((np.inf, 256), True), ((340, 256), True), ((512, 128), True), (0.5, True), ((200, 150), False)]
for (H, W) in [(256, 340), (340, 256), (240, 320), (37, 53), (480, 640), (720, 1280)]:
    for scale, keep in RESIZE:
        img = np.zeros((H, W, 3), dtype=np.uint8)
        del LOG[:]
        res = Resize(scale, keep_ratio=keep)(dict(img_group=[img], modality="RGB"))
        calls = [e for e in LOG if e[0] in ("rescale", "resize")]
        sc = calls[0][1]
        rows["resize_hw"].append((H, W))
        rows["resize_scale"].append(tuple(sc) if isinstance(sc, tuple) else (sc, np.nan))
        rows["resize_keep"].append(int(keep))
        rows["resize_call"].append(0 if calls[0][0] == "rescale" else 1)
        rows["resize_out"].append(res["img_shape"][:2])
out = {k: np.array(v, dtype=np.float64 if k in ("rrc_box", "rrc_next", "resize_scale") else np.int64) for k, v in rows.items()}
np.savez_compressed(os.path.join(HERE, "resize_cases.npz"), **out)
print("wrote resize_cases.npz: %d arrays (%d rrc cases: %d fallbacks, %d overhanging boxes)" % (len(out), len(SHAPES) * len(SEEDS), fallbacks, overhangs))
