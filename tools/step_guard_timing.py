"""What the non-finite step guard costs on the MI355X (R50, 8 frames, 224 x 224, bf16 storage), in one run on one box:

  (a) the plain optimizer sequence    -- norm partials + finalize + SGD kernel on the flat buffers (mvf_sgd_nesterov_step)
  (b) the guarded optimizer sequence  -- the same three launches with the flag decided in finalize and read by every workgroup of the SGD kernel
                                         (mvf_sgd_step_guarded), then the conditional restore of the BatchNorm statistics (mvf_bn_stats_restore)
  (c) the snapshot                    -- one launch over the ~60 k statistics words and the num_batches_tracked counters (mvf_bn_stats_snapshot)
  (d) the whole train step at 12 and at 32 clips with the guard off and on

    python tools/step_guard_timing.py [--what abc,d] [--clips 12,32] [--steps 40] [--reps 7] [--iters 20] [--out profiles/step_guard.txt]

(a)-(c): HIP events around --iters calls (the engine's own _apply_sgd / _guard_snapshot, nothing else between the events), --reps times, the variants
alternating inside every repeat so that they share whatever else the box is doing; median / min / max per call.
(d): windows of --steps train steps bracketed by device synchronisation, off / on alternating, after a warm-up that takes the engine past its two eager and
two recorded steps (launch plans).  One JSON line per figure on stdout, and the same lines under a short header in --out.  Needs the GPU: there is no
fallback."""
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
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import torch
    import mvfnet_amd
    from mvfnet_amd import synth
    if not torch.cuda.is_available():
        raise SystemExit("step_guard_timing: no GPU")
    what = set(args.what.split(","))
    clip_counts = [int(c) for c in args.clips.split(",")]
    gen = torch.Generator(device="cuda").manual_seed(0)
    lines = []

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
        lines.append(json.dumps(dict(dict(what=name, frames=args.frames, size=args.size), **d)))
        print(lines[-1], flush=True)

    eng = engine()
    if "abc" in what:
        data = batches(clip_counts[0])
        for i in range(3):
            eng.train_step(*data[i % 2])                          # a real gradient in flat_grads
        n = eng.flat_params.numel() - eng.trainable_offset()
        lr = 1e-6                                                 # hundreds of steps on one gradient: the weights stay where they are
        sgd = lambda: eng._apply_sgd(eng.flat_grads, 1.0, lr)          # noqa: E731

        eng.enable_step_guard()
        guard = eng._guard
        eng._guard_snapshot()                                     # builds and validates the table
        snap = guard["snap"]
        words, counters = snap[0].n, eng._nbt_flat.numel()

        def guarded():
            guard["snap"] = snap                                  # as after a forward: the restore is launched (and stores nothing)
            sgd()

        def snapshot():
            guard["snap"] = None
            eng._guard_snapshot()
        variants = (("a_plain_sgd_sequence", sgd, None), ("b_guarded_sgd_sequence_and_restore", guarded, guard), ("c_statistics_snapshot", snapshot, guard))
        times = {name: [] for name, _, _ in variants}
        for rep in range(args.reps + 1):                          # the first repeat is the warm-up of all three
            for name, fn, g in variants:
                eng._guard = g                                    # None: exactly the launches of an engine that never enabled the guard
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
        eng._guard = guard
        state = eng.guard_state()
        eng.disable_step_guard()
        for name, _, _ in variants:
            emit(name, dict(stats(times[name], "us"), elements=n, statistics_words=words, counters=counters, calls_per_repeat=args.iters, reps=args.reps))
        emit("guard_state_after_abc", state)
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
                        eng.enable_step_guard()
                    else:
                        eng.disable_step_guard()
                    step(0)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for i in range(args.steps):
                        step(i)
                    torch.cuda.synchronize()
                    times[on].append((time.perf_counter() - t0) / args.steps * 1e3)
            state = eng.guard_state()
            eng.disable_step_guard()
            for on in (False, True):
                emit("d_train_step_guard_%s" % ("on" if on else "off"), dict(stats(times[on], "ms"), clips=clips, steps_per_window=args.steps, reps=args.reps,
                                                                             plan=[s["plan"] is not None for s in getattr(eng, "_plans", {}).values()]))
            off_ms, on_ms = sorted(times[False])[len(times[False]) // 2], sorted(times[True])[len(times[True]) // 2]
            emit("d_guard_cost", dict(clips=clips, median_delta_ms=round(on_ms - off_ms, 3), median_delta_percent=round((on_ms / off_ms - 1.0) * 100.0, 2),
                                      skipped_in_last_window=state["skipped"]))
            del data
    if args.out:
        with open(args.out, "w") as f:
            f.write("Non-finite step guard: cost on one MI355X, one run, one box (tools/step_guard_timing.py %s)\n" % " ".join(sys.argv[1:]))
            f.write("R50, %d frames, %d x %d, bf16 storage.  (a)-(c): HIP events around %d calls, %d repeats, variants alternating.  (d): windows of %d train steps,\n"
                    % (args.frames, args.size, args.size, args.iters, args.reps, args.steps))
            f.write("guard off / on alternating in the same process, so both sides of every comparison ran on the same box within seconds of each other.\n\n")
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
