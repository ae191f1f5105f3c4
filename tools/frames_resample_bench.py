"""mvf_frames_resample_u8 and mvf_frames_resample_color_u8 against mvf_frames_prep_u8 at the C3 shape: 256 decoded 340 x 256 frames -> the
224 x 224 bf16 stem operand (pad 3, the engines' wp), timed with HIP events, the kernels alternated in rounds.  Resample cases: the val
recipe (Resize(inf, 256) is the identity size here, CenterCrop 224: the bilinear path at scale 1), the train recipe (RandomResizedCrop(224)
boxes, Flip) and an exact Resize to 224 x 224 (a 0.66 x 0.875 downscale of the whole frame).  Colour cases: the train rows again with
ColorJitter's default table (the lighting term) and with the full colour-space table, and the TSN train recipe (MultiScaleCrop(224) boxes,
Flip, full table); each is also reported against "resample train", the same geometry without the colour step.
usage: python tools/frames_resample_bench.py [iters] [rounds]"""
import os
import random
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mvfnet_amd._lib import check, lib  # noqa: E402
from mvfnet_amd.preprocess import (FramePipeline, JitterFramePipeline, ResamplingFramePipeline, color_jitter_table, jitter_rows,  # noqa: E402
                                   multi_scale_crop_rows, resize_rows, train_rows, val_rows)

n, hs, ws, c, pad = 256, 256, 340, 224, 3
iters = int(sys.argv[1]) if len(sys.argv) > 1 else 50
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 5
wp = (c + 2 * pad + 2 + 1) // 2 * 2
fr = torch.from_numpy(np.random.RandomState(0).randint(0, 256, size=(n, hs, ws, 3)).astype(np.uint8)).cuda()
out = torch.empty(n, c + 2 * pad, wp, 4, dtype=torch.bfloat16, device="cuda")
prep, rs = FramePipeline(crop_size=c), ResamplingFramePipeline(crop_size=c)
win = prep.center_window(n, hs, ws)
random.seed(0)
np.random.seed(0)
cases = {
    "resample val": torch.from_numpy(val_rows(hs, ws, n)).cuda(),
    "resample train": torch.from_numpy(np.concatenate([train_rows(hs, ws, 8) for _ in range(n // 8)])).cuda(),
    "resample resize224": torch.from_numpy(resize_rows(hs, ws, n, (c, c), keep_ratio=False)).cuda(),
}
msc = np.concatenate([multi_scale_crop_rows(hs, ws, 8) for _ in range(n // 8)])
tables = {"default": np.concatenate([color_jitter_table(8) for _ in range(n // 8)]),
          "full": np.concatenate([color_jitter_table(8, color_space_aug=True) for _ in range(n // 8)])}
color_cases = {                                  # name -> (geometry rows, colour table), both on the device
    "color train default": (cases["resample train"], torch.from_numpy(tables["default"]).cuda()),
    "color train full": (cases["resample train"], torch.from_numpy(tables["full"]).cuda()),
    "color msc full": (torch.from_numpy(msc).cuda(), torch.from_numpy(tables["full"]).cuda()),
}
for k, rows in cases.items():                    # the rows are validated once, through the pipeline; the timed calls go straight to the C ABI
    rs.to_stem(fr, rows, pad, wp, torch.bfloat16, out=out)
jt = JitterFramePipeline(crop_size=c)
for k, (rows, color) in color_cases.items():
    jt.to_stem(fr, torch.from_numpy(jitter_rows(rows.cpu().numpy(), color.cpu().numpy())).cuda(), pad, wp, torch.bfloat16, out=out)
prep.to_stem(fr, win, pad, wp, torch.bfloat16, out=out)
st = torch.cuda.current_stream().cuda_stream


def call(fn, table):
    return lambda: check(fn(fr.data_ptr(), n, hs, ws, table.data_ptr(), c, c, prep.mean, prep.std, 1, 0, pad, wp, out.data_ptr(), None, 1, st))


runs = {"prep_u8 window": call(lib.mvf_frames_prep_u8, win)}
for k, rows in cases.items():
    runs[k] = call(lib.mvf_frames_resample_u8, rows)


def call_color(rows, color):
    return lambda: check(lib.mvf_frames_resample_color_u8(fr.data_ptr(), n, hs, ws, rows.data_ptr(), color.data_ptr(), c, c, prep.mean, prep.std, 1, 0,
                                                          pad, wp, out.data_ptr(), None, 1, st))


for k, (rows, color) in color_cases.items():
    runs[k] = call_color(rows, color)
times = {k: [] for k in runs}
for k, go in runs.items():                       # warm up every case
    for _ in range(3):
        go()
torch.cuda.synchronize()
for _ in range(rounds):
    for k, go in runs.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            go()
        e1.record()
        torch.cuda.synchronize()
        times[k].append(e0.elapsed_time(e1) * 1e3 / iters)
out_bytes = out.numel() * out.element_size()
base = float(np.median(times["prep_u8 window"]))
train = float(np.median(times["resample train"]))
print("C3 shape: %d frames %dx%d -> %dx%d bf16 stem operand (%.1f MB written per call); %d rounds x %d calls" % (n, ws, hs, c, c, out_bytes / 1e6, rounds, iters))
for k, t in times.items():
    med = float(np.median(t))
    print("%-20s median %7.1f us  (min %7.1f, max %7.1f)  %5.2f TB/s of output  %.2fx prep_u8%s"
          % (k, med, min(t), max(t), out_bytes / med / 1e6, med / base, "  %.3fx resample train" % (med / train) if k.startswith("color") else ""))
