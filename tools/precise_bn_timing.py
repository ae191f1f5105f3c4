"""What precise BatchNorm (TrainEngine.precise_bn, csrc/precise_bn.hip) costs on the MI355X (R50, 8 frames, 224 x 224, bf16 storage), in one run on one box:

  (a) the plain training-mode forward  -- engine.forward on one batch, what the engine could do before, the floor of a calibration batch
  (b) precise_bn per batch             -- the same forward with momentum 1 + ONE mvf_bn_stats_accumulate; the gather on entry and the finalize are in the
                                          window and divided over its batches; weights='live' and weights='ema' (two parameter swaps and a scatter more per call)
  (c) the three kernels alone          -- mvf_bn_stats_accumulate / _finalize (through the table) / _exchange (swap) over the engine's own table

    python tools/precise_bn_timing.py [--clips 12,32] [--batches 20] [--reps 7] [--iters 50]

(a), (b): windows of --batches batches bracketed by a device synchronisation, --reps windows each after one warm-up window, the variants alternating inside
every repeat so that they share whatever else the box is doing; median / min / max per batch.  (c): HIP events around --iters back-to-back calls (this includes
the host-side table check of every call, which is part of the entry point), --reps times; median / min / max per call.  One JSON line per figure on stdout.
Needs the GPU: there is no fallback."""
import argparse
import json
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--clips", default="12,32")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--batches", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    import mvfnet_amd
    from mvfnet_amd import synth
    from mvfnet_amd import train_engine as te
    if not torch.cuda.is_available():
        raise SystemExit("precise_bn_timing: no GPU")
    gen = torch.Generator(device="cuda").manual_seed(0)

    def engine():
        m = mvfnet_amd.build_recognizer(mvfnet_amd.mvfnet_config(50, args.frames), None, dict(average_clips=None))
        sd = m.state_dict()
        vals = synth.synth_state_dict({"r50/" + k: tuple(v.shape) for k, v in sd.items()})
        m.load_state_dict({k: torch.from_numpy(vals["r50/" + k]) for k in sd}, strict=True)
        return m.cuda().train().train_engine(dtype=torch.bfloat16)

    def stats(v, unit):
        v = sorted(v)
        return {"median_" + unit: round(v[len(v) // 2], 3), "min_" + unit: round(v[0], 3), "max_" + unit: round(v[-1], 3)}

    def emit(name, d):
        print(json.dumps(dict(dict(what=name, frames=args.frames, size=args.size), **d)), flush=True)

    eng = engine()
    eng.enable_ema(momentum=2e-4)
    for clips in [int(c) for c in args.clips.split(",")]:
        data = [(torch.randn(clips, args.frames, 3, args.size, args.size, device="cuda", generator=gen),
                 torch.randint(0, 400, (clips, 1), device="cuda", generator=gen)) for _ in range(2)]
        feed = [data[i % 2] for i in range(args.batches)]

        def forwards():
            for imgs, labels in feed:
                eng.forward(imgs, labels)
        variants = (("a_forward", forwards), ("b_precise_bn_live", lambda: eng.precise_bn(feed, num_iters=args.batches)),
                    ("b_precise_bn_ema", lambda: eng.precise_bn(feed, num_iters=args.batches, weights="ema")))
        times = {name: [] for name, _ in variants}
        for rep in range(args.reps + 1):                          # the first repeat is the warm-up of all three
            for name, fn in variants:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                if rep:
                    times[name].append((time.perf_counter() - t0) * 1e3 / args.batches)
        for name, _ in variants:
            emit(name, dict(dict(clips=clips, batches_per_window=args.batches, windows=args.reps), **stats(times[name], "ms_per_batch")))
    # (c) the kernels alone, over the table precise_bn built
    tab = eng._stat_table([b for b in eng._all_bns() if not b.frozen])
    spare = torch.zeros_like(tab.shadow)
    calls = (("c_accumulate", tab.accumulate), ("c_finalize_through_table", lambda: tab.finalize(3)), ("c_exchange_swap", lambda: tab.exchange(spare, 2)))
    times = {name: [] for name, _ in calls}
    tab.exchange(tab.shadow, 0)
    with te._on_stream(torch.cuda.current_stream(), main=True):
        for rep in range(args.reps + 1):
            for name, fn in calls:
                tab.acc.zero_()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.iters):
                    fn()
                e1.record()
                e1.synchronize()
                if rep:
                    times[name].append(e0.elapsed_time(e1) * 1e3 / args.iters)
        tab.exchange(tab.shadow, 1)
    for name, _ in calls:
        emit(name, dict(dict(segments=tab.nseg, elements=tab.n, calls_per_window=args.iters, windows=args.reps), **stats(times[name], "us_per_call")))


if __name__ == "__main__":
    main()
