"""mvf_frames_yuv420_gather_resample_u8 (I420 and NV12 frames) against the unchanged mvf_frames_gather_resample_u8 (packed frames) on identical
geometry, bf16 stem operand, and the host-to-device copy of each source tensor from pinned memory:

  C3  256 decoded 340 x 256 frames -> 224 x 224 via train_rows (one RandomResizedCrop box and flip per 8-frame clip);
  C5  one video of the shipped test recipe: 80 sampled frames (the distinct ones uploaded) of 340 x 256 -> 240 images of 256 x 256 via
      video_test_table (Resize((inf, 256)) -> ThreeCrop(256)).

The YUV frames are random planes and the packed frames their numpy conversion (tests/yuv_numpy.py), so the three kernels compute the same
stem operand: compared bit for bit before anything is timed.  Kernel = device events around `iters` back-to-back launches, the three
kernels alternating inside every round; copy = device events around one copy; median (min, max) over the rounds, after a warm-up.
usage: python tools/yuv_input_bench.py [iters] [rounds]"""
import os
import random
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import yuv_numpy as Y  # noqa: E402
from mvfnet_amd._lib import check, lib  # noqa: E402
from mvfnet_amd.preprocess import (GatherFramePipeline, Yuv420FramePipeline, gather_rows, sample_frame_inds, split_gather_rows, test_rows,  # noqa: E402
                                   train_rows, video_test_table)

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 20
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 15
hs, ws, pad = 256, 340, 3
if not torch.cuda.is_available():
    raise SystemExit("yuv_input_bench: no GPU -- nothing is measured without one")
st = torch.cuda.current_stream().cuda_stream


def events(go, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        go()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def case(name, n_src, table, c):
    rows, src = split_gather_rows(table)
    n_out = rows.shape[0]
    wp = (c + 2 * pad + 2 + 1) // 2 * 2
    planes = Y.random_planes(n_src, hs, ws, 0)
    host = {"packed": torch.from_numpy(Y.planes_to_packed(*planes, 0, Y.BGR)).pin_memory(),
            "i420": torch.from_numpy(Y.pack(*planes, Y.I420)).pin_memory(), "nv12": torch.from_numpy(Y.pack(*planes, Y.NV12)).pin_memory()}
    dev = {k: torch.empty(v.shape, dtype=torch.uint8, device="cuda") for k, v in host.items()}
    copies = {k: (lambda k=k: dev[k].copy_(host[k], non_blocking=True)) for k in host}
    for go in copies.values():
        go()
    rows_d, src_d = torch.from_numpy(rows).cuda(), torch.from_numpy(src).cuda()
    out = {k: torch.empty(n_out, c + 2 * pad, wp, 4, dtype=torch.bfloat16, device="cuda") for k in host}
    prep = GatherFramePipeline(crop_size=c)

    def packed():
        check(lib.mvf_frames_gather_resample_u8(dev["packed"].data_ptr(), n_src, hs, ws, src_d.data_ptr(), n_out, rows_d.data_ptr(), None, c, c,
                                                prep.mean, prep.std, 1, 0, pad, wp, out["packed"].data_ptr(), None, 1, st))

    def yuv(k, layout):
        check(lib.mvf_frames_yuv420_gather_resample_u8(dev[k].data_ptr(), n_src, hs, ws, ws, layout, 0, 0, src_d.data_ptr(), n_out, rows_d.data_ptr(),
                                                       None, c, c, prep.mean, prep.std, 1, 0, pad, wp, out[k].data_ptr(), None, 1, st))
    kernels = {"packed": packed, "i420": lambda: yuv("i420", 0), "nv12": lambda: yuv("nv12", 1)}
    # validate the table once through the pipelines, then compare the three operands bit for bit
    tab_d = torch.from_numpy(table).cuda()
    want = prep.to_stem(dev["packed"], tab_d, pad, wp, torch.bfloat16)
    for k, go in kernels.items():
        go()
    torch.cuda.synchronize()
    for k in kernels:
        assert torch.equal(out[k].view(torch.int16), want.view(torch.int16)), k
    assert torch.equal(Yuv420FramePipeline(crop_size=c, layout="nv12").to_stem(dev["nv12"], tab_d, pad, wp, torch.bfloat16).view(torch.int16), want.view(torch.int16))
    for go in list(kernels.values()) + list(copies.values()):     # warm up
        for _ in range(5):
            go()
    torch.cuda.synchronize()
    tk, tc = {k: [] for k in kernels}, {k: [] for k in copies}
    for _ in range(rounds):
        for k, go in kernels.items():
            tk[k].append(events(go, iters))
        for k, go in copies.items():
            tc[k].append(events(go, 1))
    print("%s: %d source frames of %dx%d -> %d images of %dx%d, bf16 stem operand (%.1f MB written); %d rounds x %d launches"
          % (name, n_src, ws, hs, n_out, c, c, out["packed"].numel() * 2 / 1e6, rounds, iters))
    med = {}
    for k in kernels:
        med[k] = float(np.median(tk[k]))
        print("  kernel %-6s median %8.1f us  (min %8.1f, max %8.1f)  source %6.1f MB" % (k, med[k], min(tk[k]), max(tk[k]), host[k].numel() / 1e6))
    cm = {}
    for k in copies:
        cm[k] = float(np.median(tc[k]))
        print("  copy   %-6s median %8.1f us  (min %8.1f, max %8.1f)  %6.1f MB pinned -> device, %.1f GB/s"
              % (k, cm[k], min(tc[k]), max(tc[k]), host[k].numel() / 1e6, host[k].numel() / cm[k] / 1e3))
    for k in ("i420", "nv12"):
        print("  %s - packed: kernel %+8.1f us (%.3fx), copy %+8.1f us (%.3fx), kernel + copy %+8.1f us"
              % (k, med[k] - med["packed"], med[k] / med["packed"], cm[k] - cm["packed"], cm[k] / cm["packed"],
                 med[k] + cm[k] - med["packed"] - cm["packed"]))


random.seed(0)
np.random.seed(0)
c3 = np.concatenate([train_rows(hs, ws, 8, input_size=224) for _ in range(32)])
case("C3 train_rows", 256, gather_rows(c3, np.arange(256)), 224)
inds = sample_frame_inds(300, 8, 8, 10, test_mode=True)
distinct, table = video_test_table(inds, hs, ws, test_rows)
case("C5 video_test_table", len(distinct), table, 256)
