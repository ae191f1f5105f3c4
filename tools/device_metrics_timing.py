"""What the device-side accuracy costs, or saves, on the MI355X (R50, 8 frames, bf16 storage), in one run on one box:

  (a) validation throughput -- videos/s of a validation pass over synthetic videos (one video = --clips clips x 8 frames of --size^2, average_clips='prob',
      inputs resident on the device) through the host path (runner.single_gpu_test: one readback per video, then evaluation.top_k_accuracy in numpy) and
      through the device path (runner.device_test + DeviceMetrics.compute(): one readback per pass).  Same model, same videos, passes alternating.
  (b) training step time -- the bf16 R50 8x8 train step at 12 and at 32 clips with the training accuracy off and on (TrainEngine.enable_train_accuracy):
      windows of --steps train steps bracketed by a device synchronisation, off / on alternating, after a warm-up that takes the engine past its two eager
      and two recorded steps (every timed step replays a launch plan; the accuracy launch sits behind the replay).

    python tools/device_metrics_timing.py [--what a,b] [--videos 40] [--clips 10] [--size 224] [--train-clips 12,32] [--steps 40] [--reps 7] [--out FILE]

Median (min ... max) over --reps repeats.  Writes the figures to --out (default profiles/device_metrics.txt) and one JSON line per figure to stdout.
Needs the GPU: there is no fallback."""
import argparse
import json
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--what", default="a,b")
    ap.add_argument("--videos", type=int, default=40)
    ap.add_argument("--clips", type=int, default=10)
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--train-clips", default="12,32")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, repo)
    out_path = args.out or os.path.join(repo, "profiles", "device_metrics.txt")
    import numpy as np
    import torch
    import mvfnet_amd
    from mvfnet_amd import synth
    from mvfnet_amd.evaluation import top_k_accuracy
    from mvfnet_amd.metrics import DeviceMetrics
    from mvfnet_amd.runner import device_test, single_gpu_test
    if not torch.cuda.is_available():
        raise SystemExit("device_metrics_timing: no GPU")
    what = set(args.what.split(","))
    gen = torch.Generator(device="cuda").manual_seed(0)
    lines, records = [], []

    def model(test_cfg):
        m = mvfnet_amd.build_recognizer(mvfnet_amd.mvfnet_config(50, args.frames), None, test_cfg)
        sd = m.state_dict()
        vals = synth.synth_state_dict({"r50/" + k: tuple(v.shape) for k, v in sd.items()})
        m.load_state_dict({k: torch.from_numpy(vals["r50/" + k]) for k in sd}, strict=True)
        return m.cuda()

    def stats(v):
        v = sorted(v)
        return v[len(v) // 2], v[0], v[-1]

    def emit(name, d):
        records.append(dict(dict(what=name, frames=args.frames), **d))
        print(json.dumps(records[-1]), flush=True)

    lines += ["Device-side accuracy (mvf_metrics_update, metrics.DeviceMetrics, runner.device_test, TrainEngine.enable_train_accuracy): cost on the MI355X",
              "=" * 140, "",
              "Method (tools/device_metrics_timing.py; R50, %d frames, bf16 storage; ONE process on one box, so every comparison below is inside one run;" % args.frames,
              "median (min ... max) over %d repeats, the two sides of a comparison alternating inside every repeat):" % args.reps, ""]
    if "a" in what:
        m = model(dict(average_clips="prob")).eval()
        m.backbone.engine_dtype = torch.bfloat16
        distinct = [torch.randn(1, args.clips * args.frames, 3, args.size, args.size, device="cuda", generator=gen) for _ in range(2)]
        loader = [dict(img_group=distinct[i % 2]) for i in range(args.videos)]
        labels = [int(v) for v in np.random.RandomState(0).randint(0, 400, size=args.videos)]
        metrics = DeviceMetrics(400, k=(1, 5))

        def host_pass():
            rows = single_gpu_test(m, loader)
            return top_k_accuracy([np.asarray(r).squeeze() for r in rows], labels, k=(1, 5))

        def device_pass():
            metrics.reset()
            device_test(m, loader, labels, metrics)
            fig = metrics.compute()
            return [fig["top1"], fig["top5"]]
        passes = (("host", host_pass), ("device", device_pass))
        times = {name: [] for name, _ in passes}
        figures = {}
        for rep in range(args.reps + 1):                         # the first repeat warms both paths up
            for name, fn in passes:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                figures[name] = [float(a) for a in fn()]
                torch.cuda.synchronize()
                if rep:
                    times[name].append(args.videos / (time.perf_counter() - t0))
        lines += ["  (a) validation pass over %d synthetic videos (one video = %d clips x %d frames of %d x %d, average_clips='prob', k = (1, 5), inputs on the device)"
                  % (args.videos, args.clips, args.frames, args.size, args.size),
                  "      host path = single_gpu_test (one readback per video) + evaluation.top_k_accuracy; device path = device_test + DeviceMetrics.compute() (one readback per pass)",
                  "", "                                              videos / s"]
        for name, _ in passes:
            med, lo, hi = stats(times[name])
            emit("a_validation_%s_path" % name, dict(median_videos_per_s=round(med, 2), min_videos_per_s=round(lo, 2), max_videos_per_s=round(hi, 2), videos=args.videos,
                                                      clips=args.clips, size=args.size, reps=args.reps, top1=figures[name][0], top5=figures[name][1]))
            lines.append("      %-38s  %8.2f  (%.2f ... %.2f)" % (name + " path", med, lo, hi))
        h, d = stats(times["host"])[0], stats(times["device"])[0]
        lines += ["      device / host = %.4f; both paths report the same figures: %s" % (d / h, figures["host"] == figures["device"]), ""]
        del m, distinct, loader
        torch.cuda.empty_cache()
    if "b" in what:
        eng = model(dict(average_clips=None)).train().train_engine(dtype=torch.bfloat16)
        lines += ["  (b) the whole bf16 train step with the training accuracy off and on: windows of %d steps bracketed by a device synchronisation, off / on alternating,"
                  % args.steps, "      after a warm-up past the launch plan's two eager and two recorded steps", "", "                                              per step, ms"]
        for clips in [int(c) for c in args.train_clips.split(",")]:
            data = [(torch.randn(clips, args.frames, 3, args.size, args.size, device="cuda", generator=gen),
                     torch.randint(0, 400, (clips, 1), device="cuda", generator=gen)) for _ in range(2)]
            step = lambda i: eng.train_step(*data[i % 2])          # noqa: E731
            for i in range(10):
                step(i)
            times = {False: [], True: []}
            for rep in range(args.reps):
                for on in (False, True):
                    if on:
                        eng.enable_train_accuracy()
                    else:
                        eng.disable_train_accuracy()
                    step(0)
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for i in range(args.steps):
                        step(i)
                    torch.cuda.synchronize()
                    times[on].append((time.perf_counter() - t0) / args.steps * 1e3)
            counted = eng.train_accuracy()["count"]
            eng.disable_train_accuracy()
            plan = [s["plan"] is not None for s in getattr(eng, "_plans", {}).values()]
            off = stats(times[False])
            for on in (False, True):
                med, lo, hi = stats(times[on])
                emit("b_train_step_accuracy_%s" % ("on" if on else "off"), dict(median_ms=round(med, 3), min_ms=round(lo, 3), max_ms=round(hi, 3), clips=clips, size=args.size,
                                                                                steps_per_window=args.steps, reps=args.reps, plan=plan))
                note = "" if not on else "      %+.3f ms = %+.2f %%" % (med - off[0], (med / off[0] - 1.0) * 100.0)
                lines.append("      %2d clips, accuracy %-3s                    %7.3f  (%.3f ... %.3f)%s" % (clips, "on" if on else "off", med, lo, hi, note))
            assert counted == clips * (args.steps + 1), counted    # the last window counted every step
            del data
        lines.append("")
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", out_path)


if __name__ == "__main__":
    main()
