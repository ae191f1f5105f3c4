"""What gradient accumulation costs on the MI355X, at the reference's own per-GPU batch (R50, 8 frames, 224 x 224, 12 clips, bf16 storage):

  (a) train_step                          -- gains no launch from the feature; --repo DIR times another checkout's (the parent commit's) package the same way
  (b) one optimizer step of k = 8 micro-steps (accumulate_step x 8 + apply_accumulated)
  (c) the accumulate launch alone (mvf_grad_accumulate over the engine's flat gradient, HIP events), first = 1 (8 bytes / element) and first = 0
      (12 bytes / element), as achieved GB/s

    python tools/grad_accum_timing.py [--what a,b,c] [--repo DIR] [--clips 12] [--k 8] [--steps 40] [--reps 5]

Every figure is the median of --reps windows of --steps steps, each window bracketed by device synchronisation, after a warm-up that takes the engine past its
two eager and two recorded steps (launch plans).  One JSON line per figure on stdout.  Needs the GPU: there is no fallback."""
import argparse
import json
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="a,b,c")
    ap.add_argument("--repo", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="checkout whose mvfnet_amd package is timed")
    ap.add_argument("--clips", type=int, default=12)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--k", type=int, default=8)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--label", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.repo))
    import torch
    import mvfnet_amd
    from mvfnet_amd import _lib, synth
    if not torch.cuda.is_available():
        raise SystemExit("grad_accum_timing: no GPU")
    what = set(args.what.split(","))
    label = args.label or os.path.abspath(args.repo)

    def engine():
        m = mvfnet_amd.build_recognizer(mvfnet_amd.mvfnet_config(50, args.frames), None, dict(average_clips=None))
        sd = m.state_dict()
        vals = synth.synth_state_dict({"r50/" + k: tuple(v.shape) for k, v in sd.items()})
        m.load_state_dict({k: torch.from_numpy(vals["r50/" + k]) for k in sd}, strict=True)
        return m.cuda().train().train_engine(dtype=torch.bfloat16)

    gen = torch.Generator(device="cuda").manual_seed(0)
    batches = [(torch.randn(args.clips, args.frames, 3, args.size, args.size, device="cuda", generator=gen),
                torch.randint(0, 400, (args.clips, 1), device="cuda", generator=gen)) for _ in range(2)]

    def windows(fn, per_window):
        """median / min / max over --reps windows of ms per call of fn()."""
        out = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(per_window):
                fn(i)
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) / per_window * 1e3)
        out.sort()
        return dict(median_ms=round(out[len(out) // 2], 4), min_ms=round(out[0], 4), max_ms=round(out[-1], 4))

    def emit(name, d):
        print(json.dumps(dict(dict(what=name, label=label, clips=args.clips, frames=args.frames, size=args.size), **d)), flush=True)

    if "a" in what:
        eng = engine()
        step = lambda i: eng.train_step(*batches[i % 2])          # noqa: E731
        for i in range(10):
            step(i)
        emit("a_train_step", dict(windows(step, args.steps), steps_per_window=args.steps, reps=args.reps,
                                  plan=[s["plan"] is not None for s in getattr(eng, "_plans", {}).values()]))
        del eng
    if "b" in what or "c" in what:
        eng = engine()
        opt_step = lambda i: eng.train_step_accumulated([batches[(i + j) % 2] for j in range(args.k)])          # noqa: E731
        for i in range(2):
            opt_step(i)                                           # 2 k micro-steps: past the plan's recordings for k >= 2
        if "b" in what:
            per = max(1, args.steps // args.k)
            micro = lambda i: eng.accumulate_step(*batches[i % 2])          # noqa: E731
            d = windows(opt_step, per)
            m_ = windows(micro, args.steps)
            eng.apply_accumulated()
            emit("b_optimizer_step_of_k_micro_steps", dict(d, k=args.k, optimizer_steps_per_window=per, reps=args.reps, micro_step_median_ms=m_["median_ms"],
                                                           plan=[s["plan"] is not None for s in getattr(eng, "_plans", {}).values()]))
        if "c" in what:
            n = eng.flat_grads.numel()
            lib = _lib.lib
            stream = torch.cuda.current_stream().cuda_stream
            for first in (1, 0):
                launch = lambda: lib.mvf_grad_accumulate(eng.flat_acc.data_ptr(), eng.flat_grads.data_ptr(), n, first, stream)          # noqa: E731
                for _ in range(10):
                    assert launch() == 0
                times = []
                for _ in range(args.reps):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    iters = 50
                    e0.record()
                    for _ in range(iters):
                        launch()
                    e1.record()
                    torch.cuda.synchronize()
                    times.append(e0.elapsed_time(e1) / iters * 1e3)
                times.sort()
                us = times[len(times) // 2]
                nbytes = n * (8 if first else 12)
                emit("c_accumulate_launch_first%d" % first, dict(elements=n, bytes=nbytes, median_us=round(us, 2), min_us=round(times[0], 2), max_us=round(times[-1], 2),
                                                                 gb_per_s=round(nbytes / us * 1e-3, 1), launches_per_window=50, reps=args.reps))


if __name__ == "__main__":
    main()
