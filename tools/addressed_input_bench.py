"""mvf_frames_addressed_resample_u8 (per-image plane offsets and pitches) against the unchanged dense exports, packed and NV12:

  TRAIN  a 32 x 8 training batch, half 256 x 454 and half 454 x 256 clips -> 224 x 224 via train_rows;
  VIDEO  one test video of the shipped recipe: 30 clips of 8 sampled frames (the distinct ones uploaded) of 256 x 340 -> 256 x 256 via
         video_test_table (Resize((inf, 256)) -> ThreeCrop(256)).

Printed per case and format:
  upload bytes, dense collate against addressed collate (computed from the tensors' shapes: needs no GPU);
  CPU collate time of each (median of `rounds` runs);
  on a GPU, the kernel time of the addressed export against the dense export ON SAME-SIZE FRAMES in the same run (TRAIN: 256 landscape
  frames, so that both kernels read the same bytes and only the address step differs), bf16 stem operand, the outputs compared bit for bit
  before anything is timed; device events around `iters` back-to-back launches, the kernels alternating inside every round; median (min,
  max) over the rounds after a warm-up, and the spread of the dense kernel's own repeated timings to judge the difference by.
usage: python tools/addressed_input_bench.py [iters] [rounds]"""
import os
import random
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
import yuv_numpy as Y  # noqa: E402
from mvfnet_amd import preprocess as P  # noqa: E402
from mvfnet_amd._lib import check, lib  # noqa: E402

iters = int(sys.argv[1]) if len(sys.argv) > 1 else 20
rounds = int(sys.argv[2]) if len(sys.argv) > 2 else 15
gpu = torch.cuda.is_available()
pad = 3


def median_ms(fn, n):
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), min(ts), max(ts)


def clips_of(fmt, shapes, t, seed):
    """One clip per shape: packed (t, h, w, 3) random bytes, or random (Y, U, V) planes."""
    rng = np.random.RandomState(seed)
    if fmt == "packed":
        return [rng.randint(0, 256, size=(t, h, w, 3)).astype(np.uint8) for h, w in shapes]
    return [Y.random_planes(t, h, w, seed + k) for k, (h, w) in enumerate(shapes)]


def collate_pair(fmt, clips, tables):
    groups = list(zip(clips, tables))
    dense = (lambda: P.collate_frames(groups)) if fmt == "packed" else (lambda: P.collate_yuv_frames(groups, fmt))
    return dense, (lambda: P.collate_addressed_frames(groups, fmt))


def upload_and_collate(name, fmt, clips, tables):
    dense, addressed = collate_pair(fmt, clips, tables)
    d, a = dense()[0], addressed()[0]
    n = max(3, rounds // 3)
    td, ta = median_ms(dense, n), median_ms(addressed, n)
    print("%s %-6s upload: dense %s = %.1f MB, addressed %s = %.1f MB (%.2fx less)" % (name, fmt, tuple(d.shape), d.numel() / 1e6, tuple(a.shape), a.numel() / 1e6,
                                                                                      d.numel() / a.numel()))
    print("%s %-6s CPU collate: dense median %.1f ms (min %.1f, max %.1f), addressed median %.1f ms (min %.1f, max %.1f)" % ((name, fmt) + td + ta))


def events(go, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        go()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def kernels(name, fmt, planes_or_frames, table, hs, ws, c):
    """Same-size frames: the dense export on the dense batch, the addressed export on the very same device buffer (tight pitch: the
    address row of frame i is what the dense kernel computes from i), `table` a 12-column gather table."""
    st = torch.cuda.current_stream().cuda_stream
    rows, src = P.split_gather_rows(table)
    n_out, wp = rows.shape[0], (c + 2 * pad + 2 + 1) // 2 * 2
    if fmt == "packed":
        host = torch.from_numpy(planes_or_frames)
        fb = hs * ws * 3
        per_src = np.array([(i * fb, ws * 3, 0, 0, 0) for i in range(host.shape[0])], dtype=np.int64)
    else:
        host = torch.from_numpy(Y.pack(*planes_or_frames, Y.NV12))
        fb = hs * ws * 3 // 2
        per_src = np.array([(i * fb, ws, i * fb + hs * ws, 0, ws) for i in range(host.shape[0])], dtype=np.int64)
    n_src = host.shape[0]
    dev = host.cuda()
    atab = P.address_rows(table, per_src)
    geo, addr = P.split_address_rows(atab)
    P.check_addresses(geo, addr, fmt, dev.numel())
    rows_d, src_d, addr_d = torch.from_numpy(rows).cuda(), torch.from_numpy(src).cuda(), torch.from_numpy(addr).cuda()
    out = {k: torch.empty(n_out, c + 2 * pad, wp, 4, dtype=torch.bfloat16, device="cuda") for k in ("dense", "addressed")}
    prep = P.GatherFramePipeline(crop_size=c)

    def dense():
        if fmt == "packed":
            check(lib.mvf_frames_gather_resample_u8(dev.data_ptr(), n_src, hs, ws, src_d.data_ptr(), n_out, rows_d.data_ptr(), None, c, c, prep.mean, prep.std,
                                                    1, 0, pad, wp, out["dense"].data_ptr(), None, 1, st))
        else:
            check(lib.mvf_frames_yuv420_gather_resample_u8(dev.data_ptr(), n_src, hs, ws, ws, 1, 0, 0, src_d.data_ptr(), n_out, rows_d.data_ptr(), None, c, c,
                                                           prep.mean, prep.std, 1, 0, pad, wp, out["dense"].data_ptr(), None, 1, st))

    def addressed():
        check(lib.mvf_frames_addressed_resample_u8(dev.data_ptr(), dev.numel(), P.FRAME_FORMATS[fmt], 0, 0, n_out, rows_d.data_ptr(), addr_d.data_ptr(), None, c,
                                                   c, prep.mean, prep.std, 1, 0, pad, wp, out["addressed"].data_ptr(), None, 1, st))
    runs = {"dense": dense, "addressed": addressed}
    for go in runs.values():
        go()
    torch.cuda.synchronize()
    assert torch.equal(out["dense"].view(torch.int16), out["addressed"].view(torch.int16)), (name, fmt)
    pipe = P.AddressedFramePipeline(crop_size=c, format=fmt)
    assert torch.equal(pipe.to_stem(dev, torch.from_numpy(atab).cuda(), pad, wp, torch.bfloat16).view(torch.int16), out["dense"].view(torch.int16))
    for go in runs.values():
        for _ in range(5):
            go()
    torch.cuda.synchronize()
    tk = {k: [] for k in runs}
    for _ in range(rounds):
        for k, go in runs.items():
            tk[k].append(events(go, iters))
    med = {k: float(np.median(v)) for k, v in tk.items()}
    for k in runs:
        print("%s %-6s kernel %-9s median %8.1f us  (min %8.1f, max %8.1f)" % (name, fmt, k, med[k], min(tk[k]), max(tk[k])))
    spread = max(tk["dense"]) - min(tk["dense"])
    diff = med["addressed"] - med["dense"]
    print("%s %-6s addressed - dense: %+.1f us (%.3fx); run-to-run spread of the dense kernel %.1f us -> %s"
          % (name, fmt, diff, med["addressed"] / med["dense"], spread,
             "ADDRESSED IS SLOWER BY MORE THAN THE SPREAD" if diff > spread else "within the spread (or faster)"))


random.seed(0)
np.random.seed(0)
print("addressed_input_bench: %d rounds x %d launches%s" % (rounds, iters, "" if gpu else "; no GPU: upload bytes and CPU collate only"))
# TRAIN: 32 clips of 8 frames, half 256 x 454 and half 454 x 256
shapes = [(256, 454), (454, 256)] * 16
tables = [P.train_rows(h, w, 8, input_size=224) for h, w in shapes]
for fmt in ("packed", "nv12"):
    upload_and_collate("TRAIN", fmt, clips_of(fmt, shapes, 8, 1), tables)
# VIDEO: 30 clips of 8 frames of one 256 x 340 video
hs, ws = 256, 340
inds = P.sample_frame_inds(300, 8, 8, 30, test_mode=True)
distinct, vtable = P.video_test_table(inds, hs, ws, P.test_rows)
vrows = P.resize_rows(hs, ws, len(distinct), (8, 8), keep_ratio=False)
for fmt in ("packed", "nv12"):
    upload_and_collate("VIDEO", fmt, clips_of(fmt, [(hs, ws)], len(distinct), 2), [vrows])
if gpu:
    same = np.concatenate([P.train_rows(256, 454, 8, input_size=224) for _ in range(32)])
    ttable = P.gather_rows(same, np.arange(256))
    for fmt in ("packed", "nv12"):
        kernels("TRAIN", fmt, clips_of(fmt, [(256, 454)], 256, 3)[0], ttable, 256, 454, 224)
        kernels("VIDEO", fmt, clips_of(fmt, [(hs, ws)], len(distinct), 4)[0], vtable, hs, ws, 256)
