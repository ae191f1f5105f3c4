"""numpy restatement of the resample in front of the crop (mvf_frames_resample_u8): cv2.resize(INTER_LINEAR) on a CV_8U image, as the
reference's Resize / RandomResizedCrop call it through mmcv.imresize / imrescale (augmentations.py:13-68, 600-661), then
oracle/frames_numpy.py's crop -> flip -> Normalize -> FormatShape.

PARITY STATUS: third-party pixel arithmetic, parity unpinned.  This restates OpenCV resize.cpp (INTER_LINEAR, CV_8U: the fixed-point
coefficients, HResizeLinear, the vectorised VResizeLinear row blend; the INTER_AREA switch for exactly 2x down) from its documented
behaviour; neither cv2 nor mmcv is installed in the build container, so nothing here is checked against cv2 itself.  The resize
GEOMETRY (which box, which output size, how many random draws) is the reference's own code and is pinned by
tests/golden/make_resize_golden.py.  This module is the contract the kernel is tested against, bit for bit.

TEST INFRASTRUCTURE ONLY -- never imported by mvfnet_amd."""
import numpy as np

from oracle import frames_numpy as F

COLS = 11          # (hs_i, ws_i, by, bx, bh, bw, rh, rw, oy, ox, flip)


def _coords(dst, src):
    """Per destination index: (s0, s1, w0, w1, fx zeroed?) of the fp64 -> fp32 source coordinate (dx + 0.5) * scale - 0.5 with
    scale = 1 / (dst / src), the floor, the fp32 fraction and the two 11-bit weights, each rounded on its own (saturate_cast<short>)."""
    scale = 1.0 / (float(dst) / src)
    d = np.arange(dst, dtype=np.float64)
    f = ((d + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(np.float32)).astype(np.float32)
    return s, f


def _weights(f):
    w0 = np.rint((np.float32(1.0) - f).astype(np.float32) * np.float32(2048)).astype(np.int64)
    w1 = np.rint(f * np.float32(2048)).astype(np.int64)
    return w0, w1


def resize_linear_u8(img, rh, rw):
    """cv2.resize(img, (rw, rh), interpolation=INTER_LINEAR) for an (h, w, 3) uint8 image, as restated in the module docstring."""
    img = np.asarray(img)
    bh, bw = img.shape[:2]
    src = img.astype(np.int64)
    if bh == 2 * rh and bw == 2 * rw:                       # cv2 switches to INTER_AREA: the rounded 2x2 mean
        s = src[0::2, 0::2] + src[0::2, 1::2] + src[1::2, 0::2] + src[1::2, 1::2]
        return ((s + 2) >> 2).astype(np.uint8)
    sx, fx = _coords(rw, bw)
    lo, hi = sx < 0, sx >= bw - 1                           # x taps: clamped, the fraction zeroed
    sx = np.where(lo, 0, np.where(hi, bw - 1, sx))
    fx = np.where(lo | hi, np.float32(0), fx).astype(np.float32)
    a0, a1 = _weights(fx)
    sx1 = np.minimum(sx + 1, bw - 1)
    hsum = src[:, sx] * a0[None, :, None] + src[:, sx1] * a1[None, :, None]       # (bh, rw, 3) HResizeLinear
    sy, fy = _coords(rh, bh)                                # y: fraction kept, the two rows clamped
    b0, b1 = _weights(fy)
    r0, r1 = np.clip(sy, 0, bh - 1), np.clip(sy + 1, 0, bh - 1)
    v = ((hsum[r0] >> 4) * b0[:, None, None] >> 16) + ((hsum[r1] >> 4) * b1[:, None, None] >> 16)
    return np.clip((v + 2) >> 2, 0, 255).astype(np.uint8)


def resample_frame(frame, row, h, w):
    """One row (hs_i, ws_i, by, bx, bh, bw, rh, rw, oy, ox, flip) -> the (h, w, 3) uint8 crop: resize the patch, cut, mirror."""
    _, _, by, bx, bh, bw, rh, rw, oy, ox, flip = (int(v) for v in row)
    out = resize_linear_u8(frame[by:by + bh, bx:bx + bw], rh, rw)[oy:oy + h, ox:ox + w]
    return out[:, ::-1] if flip else out


def frames_to_nchw(frames_u8, rows, h, w, mean, std, to_rgb=True, div_255=False):
    """frames_u8 (n, Hs, Ws, 3) uint8, rows (n, 11) -> (n, 3, h, w) float32, what mvf_frames_resample_u8 writes to out_nchw."""
    crops = np.stack([resample_frame(frames_u8[i], rows[i], h, w) for i in range(frames_u8.shape[0])])
    return F.frames_to_nchw(crops, None, h, w, mean, std, to_rgb=to_rgb, div_255=div_255)
