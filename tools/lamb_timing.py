"""What the fused LAMB step costs on the MI355X beside the SGD and AdamW steps (R50, 8 frames, 224 x 224, bf16 storage), in one run on one box:

  (a) the SGD optimizer sequence   -- norm partials + finalize + SGD kernel on the flat buffers (mvf_sgd_nesterov_step)
  (b) the AdamW sequence           -- norm partials + finalize (+ step count, bias corrections) + AdamW kernel (mvf_adamw_step)
  (c) the LAMB sequence            -- norm partials + finalize + moments pass + ratio pass + apply pass (mvf_lamb_step), one table segment per parameter
  (d) LAMB with the average        -- the same launches, the averaged weights updated inside the apply pass
  (e) LAMB guarded                 -- the same launches behind the non-finite guard (flag read per workgroup, counters in the finalize lane)
  (f) the whole train step at 12 and at 32 clips under SGD, AdamW and LAMB

Bytes per element, by count: the norm reads the gradient once (4); the SGD update moves 5 floats (20), the AdamW update 7 (28); LAMB's moments pass reads
parameter, gradient, exp_avg, exp_avg_sq and writes the last two (24), its apply pass reads exp_avg, exp_avg_sq, parameter and writes the parameter (16): 40;
the average adds one read and one write (8).  Per sequence: SGD 24, AdamW 32, LAMB 44, LAMB with the average 52, LAMB guarded 44.  The ratio pass and the
per-(chunk, segment) partials are a few hundred KB and are not counted.

    python tools/lamb_timing.py [--what abcde,f] [--clips 12,32] [--steps 40] [--reps 7] [--iters 20]

(a)-(e): HIP events around --iters optimizer calls (the engines' own _apply_sgd / _apply_adamw / _apply_lamb, nothing else between the events), --reps times,
the variants alternating inside every repeat so that they share whatever else the box is doing; median / min / max per call and the bandwidth the byte count
implies.  (f): windows of --steps train steps bracketed by device synchronisation, the three engines alternating, after a warm-up that takes them past their
two eager and two recorded steps (launch plans; the optimizer runs outside them).  One JSON line per figure on stdout.  Needs the GPU: there is no fallback."""
import argparse
import json
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="abcde,f")
    ap.add_argument("--clips", default="12,32")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    import mvfnet_amd
    from mvfnet_amd import synth
    if not torch.cuda.is_available():
        raise SystemExit("lamb_timing: no GPU")
    what = set(args.what.split(","))
    clip_counts = [int(c) for c in args.clips.split(",")]
    gen = torch.Generator(device="cuda").manual_seed(0)

    def engine(**opt):
        m = mvfnet_amd.build_recognizer(mvfnet_amd.mvfnet_config(50, args.frames), None, dict(average_clips=None))
        sd = m.state_dict()
        vals = synth.synth_state_dict({"r50/" + k: tuple(v.shape) for k, v in sd.items()})
        m.load_state_dict({k: torch.from_numpy(vals["r50/" + k]) for k in sd}, strict=True)
        return m.cuda().train().train_engine(dtype=torch.bfloat16, **opt)

    def batches(clips):
        return [(torch.randn(clips, args.frames, 3, args.size, args.size, device="cuda", generator=gen),
                 torch.randint(0, 400, (clips, 1), device="cuda", generator=gen)) for _ in range(2)]

    def stats(v, unit):
        v = sorted(v)
        return {"median_" + unit: round(v[len(v) // 2], 3), "min_" + unit: round(v[0], 3), "max_" + unit: round(v[-1], 3)}

    def emit(name, d):
        print(json.dumps(dict(dict(what=name, frames=args.frames, size=args.size), **d)), flush=True)

    sgd = engine()
    adam = engine(optimizer="adamw", lr=1e-3, weight_decay=0.05)
    lamb = engine(optimizer="lamb", lr=5e-3, weight_decay=0.02)
    if "abcde" in what:
        data = batches(clip_counts[0])
        for i in range(3):
            for eng in (sgd, adam, lamb):
                eng.train_step(*data[i % 2])                      # a real gradient in flat_grads
        n = sgd.flat_params.numel() - sgd.trainable_offset()
        lr = 1e-6                                                 # hundreds of steps on one gradient: the weights stay where they are
        run_sgd = lambda: sgd._apply_sgd(sgd.flat_grads, 1.0, lr)           # noqa: E731
        run_adam = lambda: adam._apply_adamw(adam.flat_grads, 1.0, lr)      # noqa: E731
        run_lamb = lambda: lamb._apply_lamb(lamb.flat_grads, 1.0, lr)       # noqa: E731
        variants = (("a_sgd_step", run_sgd, 24, False, False), ("b_adamw_step", run_adam, 32, False, False), ("c_lamb_step", run_lamb, 44, False, False),
                    ("d_lamb_step_ema", run_lamb, 52, True, False), ("e_lamb_step_guarded", run_lamb, 44, False, True))
        times = {v[0]: [] for v in variants}
        for rep in range(args.reps + 1):                          # the first repeat is the warm-up of all five
            for name, fn, _, ema, guard in variants:
                if ema:
                    lamb.enable_ema()
                elif lamb.flat_ema is not None:
                    lamb.disable_ema()
                if guard:
                    lamb.enable_step_guard()
                else:
                    lamb.disable_step_guard()
                fn()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(args.iters):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                if rep:
                    times[name].append(e0.elapsed_time(e1) / args.iters * 1e3)
        if lamb.flat_ema is not None:
            lamb.disable_ema()
        lamb.disable_step_guard()
        nseg = len(lamb.trust_ratios())
        for name, _, per, _, _ in variants:
            d = stats(times[name], "us")
            emit(name, dict(d, elements=n, segments=nseg if "lamb" in name else None, bytes=n * per, bytes_per_element=per,
                            gb_per_s=round(n * per / d["median_us"] * 1e-3, 1), calls_per_repeat=args.iters, reps=args.reps))
        del data
    if "f" in what:
        for clips in clip_counts:
            data = batches(clips)
            engines = (("sgd", sgd), ("adamw", adam), ("lamb", lamb))
            for i in range(10):
                for _, eng in engines:
                    eng.train_step(*data[i % 2])
            times = {name: [] for name, _ in engines}
            for rep in range(args.reps):
                for name, eng in engines:
                    eng.train_step(*data[0])
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for i in range(args.steps):
                        eng.train_step(*data[i % 2])
                    torch.cuda.synchronize()
                    times[name].append((time.perf_counter() - t0) / args.steps * 1e3)
            for name, eng in engines:
                emit("f_train_step_%s" % name, dict(stats(times[name], "ms"), clips=clips, steps_per_window=args.steps, reps=args.reps,
                                                    plan=[s["plan"] is not None for s in getattr(eng, "_plans", {}).values()]))
            del data


if __name__ == "__main__":
    main()
