"""numpy restatement of mvf_frames_resample_color_u8's colour arithmetic, float32 op by op, on top of tests/resample_numpy.py's resample:

    p[k] = float32(px[k])                                              k = 0..2, the resampled uint8 value, stored channel order
    q[c] = ((M[c][0]*p[0] + M[c][1]*p[1]) + M[c][2]*p[2]) + b[c]       every * and + rounded to float32 on its own
    f    = q[2 - k if to_rgb else k];  f = f / 255 when div_255;  v[k] = (f - mean[k]) * stdinv[k]        as oracle/frames_numpy.py

`color` is the (n, 12) float32 table of preprocess.color_jitter_table: M[0][0..2], M[1][0..2], M[2][0..2], b[0..2].  With M = I this is
float32(p + b), what the reference's ColorJitter(color_space_aug=False) computes (`img + bgr`, uint8 + float32); with colour-space
augmentation the reference chains up to four rounded steps where this applies their float64 composition once, so the two agree to a
few fp32 roundings, not bit for bit (tests/golden/make_jitter_golden.py records the distance).

TEST INFRASTRUCTURE ONLY -- never imported by mvfnet_amd."""
import numpy as np

import resample_numpy as R

F32 = np.float32


def apply_color(crops_u8, color):
    """crops (n, h, w, 3) uint8, color (n, 12) float32 or None -> (n, h, w, 3) float32 q, stored channel order."""
    p = crops_u8.astype(F32)
    if color is None:
        return p
    color = np.asarray(color, dtype=F32).reshape(-1, 12)
    out = np.empty_like(p)
    for i in range(p.shape[0]):
        m, b = color[i, :9].reshape(3, 3), color[i, 9:]
        for c in range(3):
            acc = (m[c, 0] * p[i, ..., 0]).astype(F32) + (m[c, 1] * p[i, ..., 1]).astype(F32)
            acc = acc.astype(F32) + (m[c, 2] * p[i, ..., 2]).astype(F32)
            out[i, ..., c] = acc.astype(F32) + b[c]
    return out


def normalize(q, mean, std, to_rgb=True, div_255=False):
    """(n, h, w, 3) float32 in stored order -> (n, 3, h, w) float32: oracle/frames_numpy.py imnormalize from the float value on."""
    if div_255:
        q = (q / F32(255)).astype(F32)
    if to_rgb:
        q = q[..., ::-1]
    mean32 = F32(np.float64(np.asarray(mean, dtype=F32)))
    stdinv32 = F32(1.0 / np.float64(np.asarray(std, dtype=F32)))
    out = (q - mean32).astype(F32)
    return np.ascontiguousarray((out * stdinv32).astype(F32).transpose(0, 3, 1, 2))


def color_normalize(crops_u8, color, mean, std, to_rgb=True, div_255=False):
    """crops (n, h, w, 3) uint8 -> (n, 3, h, w) float32: the kernel's arithmetic from the resampled pixel on."""
    return normalize(apply_color(np.asarray(crops_u8), color), mean, std, to_rgb, div_255)


def frames_to_nchw(frames_u8, rows, color, h, w, mean, std, to_rgb=True, div_255=False):
    """frames_u8 (n, Hs, Ws, 3) uint8, rows (n, 11), color (n, 12) or None -> (n, 3, h, w) float32, what mvf_frames_resample_color_u8
    writes to out_nchw."""
    crops = np.stack([R.resample_frame(frames_u8[i], rows[i], h, w) for i in range(frames_u8.shape[0])])
    return color_normalize(crops, color, mean, std, to_rgb, div_255)


def scaled_error(got, want, color, std, to_rgb=True):
    """max over everything of |got - want| / (S_c / std_k), S_c = sum_j |M[c][j]| * 255 + |b[c]| + 255 for the stored channel c behind
    output channel k: the error in units of the largest magnitude the frame's affine map can reach.  got / want (n, 3, h, w)."""
    color = np.asarray(color, dtype=np.float64).reshape(-1, 12)
    s = np.abs(color[:, :9]).reshape(-1, 3, 3).sum(2) * 255.0 + np.abs(color[:, 9:]) + 255.0          # (n, 3) stored order
    if to_rgb:
        s = s[:, ::-1]
    denom = s / np.asarray(std, dtype=np.float64)[None, :]
    return float((np.abs(got.astype(np.float64) - want.astype(np.float64)) / denom[:, :, None, None]).max())
