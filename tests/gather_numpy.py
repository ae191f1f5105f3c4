"""numpy restatement of mvf_frames_gather_resample_u8: the gather `frames[src]`, then tests/jitter_numpy.py (which sits on
tests/resample_numpy.py) unchanged -- the index adds no arithmetic of its own.

TEST INFRASTRUCTURE ONLY -- never imported by mvfnet_amd."""
import numpy as np

import jitter_numpy as J


def frames_to_nchw(frames_u8, src, rows, color, h, w, mean, std, to_rgb=True, div_255=False):
    """frames_u8 (n_src, Hs, Ws, 3) uint8, src (n_out,) or None (= i -> i), rows (n_out, 11), color (n_out, 12) or None
    -> (n_out, 3, h, w) float32, what mvf_frames_gather_resample_u8 writes to out_nchw."""
    frames_u8 = np.asarray(frames_u8)
    if src is not None:
        frames_u8 = frames_u8[np.asarray(src, dtype=np.int64)]
    return J.frames_to_nchw(frames_u8, np.asarray(rows), color, h, w, mean, std, to_rgb, div_255)
