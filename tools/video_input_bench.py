"""Input of ONE video of the shipped test recipe (configs/MVFNet/K400 test pipeline: SampleFrames(8 x 8, num_clips=10) -> 80 sampled frames
of 340 x 256 -> Resize((inf, 256)) -> ThreeCrop(256) -> 240 images = 30 clips), bf16 stem operand, two ways in one process:

  parent  the host builds the 240-frame uint8 tensor out of the 80 decoded frames (numpy take into pinned memory), one host-to-device
          copy, mvf_frames_resample_u8 with test_rows;
  gather  host-to-device copy of the distinct frames from pinned memory, mvf_frames_gather_resample_u8 with video_test_table's index.

End to end = a host clock from the decoded frames in host memory to the stem operand on the device, ending in a device synchronise; the
kernel alone = device events around `iters` back-to-back launches.  The two paths alternate inside every round; median (min, max) over
the rounds.  The two stem operands are compared bit for bit before anything is timed.
usage: python tools/video_input_bench.py [iters] [rounds] [total_frames]"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from mvfnet_amd._lib import check, lib  # noqa: E402
from mvfnet_amd.preprocess import (GatherFramePipeline, ResamplingFramePipeline, sample_frame_inds, split_gather_rows, test_rows,  # noqa: E402
                                   video_test_table)

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 50
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 7
total = int(sys.argv[3]) if len(sys.argv) > 3 else 300
hs, ws, c, pad = 256, 340, 256, 3
wp = (c + 2 * pad + 2 + 1) // 2 * 2
if not torch.cuda.is_available():
    raise SystemExit("video_input_bench: no GPU -- nothing is measured without one")

inds = sample_frame_inds(total, 8, 8, 10, test_mode=True)
distinct, table = video_test_table(inds, hs, ws, test_rows)
rows, src = split_gather_rows(table)
n_out, n_src = rows.shape[0], len(distinct)
assert np.array_equal(rows, test_rows(hs, ws, len(inds)))
decoded = np.random.RandomState(0).randint(0, 256, size=(n_src, hs, ws, 3)).astype(np.uint8)      # the video's distinct frames, as decoded

rows_d, src_d = torch.from_numpy(rows).cuda(), torch.from_numpy(src).cuda()
pin_rep = torch.empty(n_out, hs, ws, 3, dtype=torch.uint8).pin_memory()
pin_dec = torch.empty(n_src, hs, ws, 3, dtype=torch.uint8).pin_memory()
dev_rep, dev_dec = torch.empty(pin_rep.shape, dtype=torch.uint8, device="cuda"), torch.empty(pin_dec.shape, dtype=torch.uint8, device="cuda")
out_a = torch.empty(n_out, c + 2 * pad, wp, 4, dtype=torch.bfloat16, device="cuda")
out_b = torch.empty_like(out_a)
prep = ResamplingFramePipeline(crop_size=c)
st = torch.cuda.current_stream().cuda_stream


def kernel_parent():
    check(lib.mvf_frames_resample_u8(dev_rep.data_ptr(), n_out, hs, ws, rows_d.data_ptr(), c, c, prep.mean, prep.std, 1, 0, pad, wp, out_a.data_ptr(),
                                     None, 1, st))


def kernel_gather():
    check(lib.mvf_frames_gather_resample_u8(dev_dec.data_ptr(), n_src, hs, ws, src_d.data_ptr(), n_out, rows_d.data_ptr(), None, c, c, prep.mean,
                                            prep.std, 1, 0, pad, wp, out_b.data_ptr(), None, 1, st))


def path_parent():
    np.take(decoded, src, axis=0, out=pin_rep.numpy())           # the host's replication: 240 frames out of the distinct ones
    dev_rep.copy_(pin_rep, non_blocking=True)
    kernel_parent()


def path_gather():
    pin_dec.numpy()[...] = decoded                               # the same staging into pinned memory, of the distinct frames only
    dev_dec.copy_(pin_dec, non_blocking=True)
    kernel_gather()


# validate the tables once through the pipelines, then compare the two paths' outputs bit for bit
path_parent(), path_gather()
torch.cuda.synchronize()
ResamplingFramePipeline(crop_size=c).to_stem(dev_rep, rows_d, pad, wp, torch.bfloat16, out=out_a)
got = GatherFramePipeline(crop_size=c).to_stem(dev_dec, torch.from_numpy(table).cuda(), pad, wp, torch.bfloat16)
torch.cuda.synchronize()
assert torch.equal(got.view(torch.int16), out_a.view(torch.int16)) and torch.equal(out_b.view(torch.int16), out_a.view(torch.int16))

paths = {"parent end to end": path_parent, "gather end to end": path_gather}
kernels = {"parent kernel": kernel_parent, "gather kernel": kernel_gather}
times = {k: [] for k in list(paths) + list(kernels)}
for go in list(paths.values()) + list(kernels.values()):         # warm up
    for _ in range(3):
        go()
torch.cuda.synchronize()
for _ in range(rounds):
    for k, go in paths.items():
        reps = max(iters // 10, 3)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(reps):
            go()
            torch.cuda.synchronize()
        times[k].append((time.perf_counter() - t0) * 1e6 / reps)
    for k, go in kernels.items():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            go()
        e1.record()
        torch.cuda.synchronize()
        times[k].append(e0.elapsed_time(e1) * 1e3 / iters)
frame_mb = hs * ws * 3 / 1e6
print("one video, shipped test recipe: %d sampled frames (%d distinct) of %dx%d -> %d images of %dx%d, bf16 stem operand (%.1f MB written); "
      "uint8 shipped: parent %.1f MB, gather %.1f MB; %d rounds x %d kernel launches"
      % (len(inds), n_src, ws, hs, n_out, c, c, out_a.numel() * 2 / 1e6, n_out * frame_mb, n_src * frame_mb, rounds, iters))
for k, t in times.items():
    print("%-18s median %9.1f us  (min %9.1f, max %9.1f)" % (k, float(np.median(t)), min(t), max(t)))
pk, gk = float(np.median(times["parent kernel"])), float(np.median(times["gather kernel"]))
pe, ge = float(np.median(times["parent end to end"])), float(np.median(times["gather end to end"]))
print("gather / parent: kernel %.3fx (parent kernel spread %.3fx of its median), end to end %.3fx"
      % (gk / pk, (max(times["parent kernel"]) - min(times["parent kernel"])) / pk, ge / pe))
