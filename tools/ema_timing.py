"""What the averaged weights (EMA) cost on the MI355X (R50, 8 frames, 224 x 224, bf16 storage), in one run on one box:

  (a) the plain optimizer step        -- norm partials + finalize + SGD kernel on the flat buffers (mvf_sgd_nesterov_step), 24 bytes / element
  (b) the _ema optimizer step         -- the same launches, the average updated inside the SGD kernel (mvf_sgd_nesterov_step_ema), 32 bytes / element
  (c) the plain step + mvf_ema_update -- the average as a launch of its own, 36 bytes / element
  (d) the whole train step at 12 and at 32 clips with the average off and on

    python tools/ema_timing.py [--what abc,d] [--clips 12,32] [--steps 40] [--reps 7] [--iters 20]

(a)-(c): HIP events around --iters optimizer calls (the engine's own _apply_sgd, nothing else between the events), --reps times, the three variants
alternating inside every repeat so that they share whatever else the box is doing; median / min / max per call and the bandwidth the byte count implies.
(d): windows of --steps train steps bracketed by device synchronisation, off / on alternating, after a warm-up that takes the engine past its two eager and
two recorded steps (launch plans).  One JSON line per figure on stdout.  Needs the GPU: there is no fallback."""
import argparse
import json
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="abc,d")
    ap.add_argument("--clips", default="12,32")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import ctypes as C
    import torch
    import mvfnet_amd
    from mvfnet_amd import _lib, synth
    if not torch.cuda.is_available():
        raise SystemExit("ema_timing: no GPU")
    what = set(args.what.split(","))
    clip_counts = [int(c) for c in args.clips.split(",")]
    gen = torch.Generator(device="cuda").manual_seed(0)

    def engine():
        m = mvfnet_amd.build_recognizer(mvfnet_amd.mvfnet_config(50, args.frames), None, dict(average_clips=None))
        sd = m.state_dict()
        vals = synth.synth_state_dict({"r50/" + k: tuple(v.shape) for k, v in sd.items()})
        m.load_state_dict({k: torch.from_numpy(vals["r50/" + k]) for k in sd}, strict=True)
        return m.cuda().train().train_engine(dtype=torch.bfloat16)

    def batches(clips):
        return [(torch.randn(clips, args.frames, 3, args.size, args.size, device="cuda", generator=gen),
                 torch.randint(0, 400, (clips, 1), device="cuda", generator=gen)) for _ in range(2)]

    def stats(v, unit):
        v = sorted(v)
        return {"median_" + unit: round(v[len(v) // 2], 3), "min_" + unit: round(v[0], 3), "max_" + unit: round(v[-1], 3)}

    def emit(name, d):
        print(json.dumps(dict(dict(what=name, frames=args.frames, size=args.size), **d)), flush=True)

    eng = engine()
    if "abc" in what:
        data = batches(clip_counts[0])
        for i in range(3):
            eng.train_step(*data[i % 2])                          # a real gradient in flat_grads
        off = eng.trainable_offset()
        n = eng.flat_params.numel() - off
        own = eng.flat_params.clone()                             # (c)'s averaged copy
        lib = _lib.lib
        lr = 1e-6                                                 # hundreds of steps on one gradient: the weights stay where they are
        plain = lambda: eng._apply_sgd(eng.flat_grads, 1.0, lr)          # noqa: E731

        def unfused():
            plain()
            assert lib.mvf_ema_update(own.data_ptr() + 4 * off, eng.flat_params.data_ptr() + 4 * off, n, C.c_float(2e-4), torch.cuda.current_stream().cuda_stream) == 0
        variants = (("a_plain_sgd_step", plain, 24, False), ("b_sgd_step_ema", plain, 32, True), ("c_plain_sgd_step_then_ema_update", unfused, 36, False))
        times = {name: [] for name, _, _, _ in variants}
        for rep in range(args.reps + 1):                          # the first repeat is the warm-up of all three
            for name, fn, _, on in variants:
                if on:
                    eng.enable_ema()
                elif eng.flat_ema is not None:
                    eng.disable_ema()
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
        if eng.flat_ema is not None:
            eng.disable_ema()
        for name, _, per, _ in variants:
            d = stats(times[name], "us")
            emit(name, dict(d, elements=n, bytes=n * per, bytes_per_element=per, gb_per_s=round(n * per / d["median_us"] * 1e-3, 1), calls_per_repeat=args.iters,
                            reps=args.reps))
        del own
    if "d" in what:
        for clips in clip_counts:
            data = batches(clips)
            step = lambda i: eng.train_step(*data[i % 2])          # noqa: E731
            for i in range(10):
                step(i)
            times = {False: [], True: []}
            for rep in range(args.reps):
                for on in (False, True):
                    if on:
                        eng.enable_ema()
                    elif eng.flat_ema is not None:
                        eng.disable_ema()
                    step(0)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for i in range(args.steps):
                        step(i)
                    torch.cuda.synchronize()
                    times[on].append((time.perf_counter() - t0) / args.steps * 1e3)
            if eng.flat_ema is not None:
                eng.disable_ema()
            for on in (False, True):
                emit("d_train_step_ema_%s" % ("on" if on else "off"), dict(stats(times[on], "ms"), clips=clips, steps_per_window=args.steps, reps=args.reps,
                                                                           plan=[s["plan"] is not None for s in getattr(eng, "_plans", {}).values()]))
            del data


if __name__ == "__main__":
    main()
