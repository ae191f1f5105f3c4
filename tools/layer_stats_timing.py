"""What the per-parameter statistics cost on the MI355X (R50, 8 frames, 224 x 224, bf16 storage), in one run on one box:

  (a) one measured step's reductions  -- mvf_flat_segment_stats on the gradient, on the parameters and on parameters - copy (two launches each), and the
                                         copy of flat_params between them: what measure_layer_stats() adds to ONE step per log interval
  (b) the predicated pair             -- mvf_flat_segment_stats + mvf_bn_stats_nonfinite with the guard's flag clear: what on_skip adds to EVERY step
  (c) the whole train step at 12 and at 32 clips: option never enabled (guard off), guard on, guard on + on_skip

    python tools/layer_stats_timing.py [--what ab,c] [--clips 12,32] [--steps 40] [--reps 7] [--iters 20] [--out profiles/layer_stats.txt]

(a), (b): HIP events around --iters calls of the engine's own hooks, --reps times, the variants alternating inside every repeat; median / min / max per call.
(c): windows of --steps train steps bracketed by device synchronisation, the three variants alternating in one process, after a warm-up that takes the engine
past its two eager and two recorded steps (launch plans).  One JSON line per figure on stdout, and the same lines under a short header in --out.  The figure
against the PARENT commit is bench.py's (same command on both trees); this tool's `off` variant runs the code of an engine that never enabled the option.
Needs the GPU: there is no fallback."""
import argparse
import json
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="ab,c")
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
        raise SystemExit("layer_stats_timing: no GPU")
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
    if "ab" in what:
        data = batches(clip_counts[0])
        for i in range(3):
            eng.train_step(*data[i % 2])                          # a real gradient in flat_grads
        eng.enable_step_guard()
        eng.enable_layer_stats(on_skip=True)
        eng.train_step(*data[0])                                  # builds the statistics table (snapshot) and the on_skip buffers
        ls, guard = eng._lstats, eng._guard
        eng._guard_snapshot()
        tab = guard["snap"][0]
        guard["snap"] = None

        def measured():
            ls["armed"] = True
            eng._layer_stats_before(eng.flat_grads)
            eng._layer_stats_after()

        def predicated():
            ls["grads"] = eng.flat_grads
            eng._layer_stats_on_skip(tab)
        variants = (("a_measured_step_three_reductions_and_copy", measured), ("b_predicated_pair_flag_clear", predicated))
        times = {name: [] for name, _ in variants}
        for rep in range(args.reps + 1):                      # the first repeat is the warm-up
            for name, fn in variants:
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
        n = eng.flat_params.numel()
        for name, _ in variants:
            emit(name, dict(stats(times[name], "us"), elements=n, parameters=ls["nseg"], statistics_segments=tab.nseg, megabytes_read_by_byte_count=round(
                (4 * n * 4 if name[0] == "a" else 0) / 1e6, 1), megabytes_written_by_byte_count=round((n * 4 if name[0] == "a" else 0) / 1e6, 1),
                calls_per_repeat=args.iters, reps=args.reps))
        emit("last_skip_after_ab", dict(record=eng.last_skip(), guard=eng.guard_state()))
        eng.disable_layer_stats()
        eng.disable_step_guard()
    if "c" in what:
        variants = ("off", "guard", "guard_on_skip")
        for clips in clip_counts:
            data = batches(clips)
            step = lambda i: eng.train_step(*data[i % 2])          # noqa: E731
            for i in range(10):
                step(i)
            times = {v: [] for v in variants}
            for rep in range(args.reps):
                for v in variants:
                    eng.disable_layer_stats()
                    eng.disable_step_guard()
                    if v != "off":
                        eng.enable_step_guard()
                    if v == "guard_on_skip":
                        eng.enable_layer_stats(on_skip=True)
                    step(0)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for i in range(args.steps):
                        step(i)
                    torch.cuda.synchronize()
                    times[v].append((time.perf_counter() - t0) / args.steps * 1e3)
            skipped = eng.guard_state()["skipped"]
            eng.disable_layer_stats()
            eng.disable_step_guard()
            med = {v: sorted(times[v])[len(times[v]) // 2] for v in variants}
            for v in variants:
                emit("c_train_step_%s" % v, dict(stats(times[v], "ms"), clips=clips, steps_per_window=args.steps, reps=args.reps,
                                                 plan=[s["plan"] is not None for s in getattr(eng, "_plans", {}).values()]))
            emit("c_on_skip_cost", dict(clips=clips, median_delta_ms_against_guard=round(med["guard_on_skip"] - med["guard"], 3),
                                        median_delta_percent_against_guard=round((med["guard_on_skip"] / med["guard"] - 1.0) * 100.0, 2),
                                        median_delta_percent_against_off=round((med["guard_on_skip"] / med["off"] - 1.0) * 100.0, 2), skipped_in_last_window=skipped))
            del data
    if args.out:
        with open(args.out, "w") as f:
            f.write("Per-parameter statistics: cost on one MI355X, one run, one box (tools/layer_stats_timing.py %s)\n" % " ".join(sys.argv[1:]))
            f.write("R50, %d frames, %d x %d, bf16 storage.  (a), (b): HIP events around %d calls, %d repeats, variants alternating.  (c): windows of %d train steps,\n"
                    % (args.frames, args.size, args.size, args.iters, args.reps, args.steps))
            f.write("off / guard / guard + on_skip alternating in the same process, so all sides of every comparison ran on the same box within seconds of each other.\n\n")
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
