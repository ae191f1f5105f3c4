"""What the focal / asymmetric losses cost in the training step, and what the sample-wise AP, the F1 counts and the best-F1 thresholds cost on the device, on
the MI355X:

  parent   train_step of another checkout's package (--repo DIR: the parent commit), which has none of this              (R50, 8 frames, 224 x 224, bf16 storage)
  default  train_step of this tree with the default loss: must issue the launches the parent issues (the plan's op count is printed) and agree in time
           within the run-to-run spread of the medians measured in the same session
  bce      train_step with loss_cls = BCELossWithLogits against a multi-hot (clips, 400) label matrix
  focal    the same with loss_cls = SigmoidFocalLoss (gamma 2, alpha 0.25): mvf_head_train_fwd_focal in the place of mvf_head_train_fwd_bce
  asl      the same with loss_cls = AsymmetricLossMultiLabel (gamma- 4, gamma+ 1, clip 0.05)
  eval     metrics.DeviceMultiLabelMetrics.compute() with no option, sample_ap=True, threshold=0.5, best_f1=True and all three, each with its reads, at
           1 863 x 157 (Charades validation) and 19 796 x 400, beside the host functions of evaluation.py on the same data (the matrix read back + numpy)

    python tools/focal_timing.py --config default,bce,focal,asl,eval [--clips 12,32] [--steps 40] [--reps 5] [--rounds 2] [--json FILE]
    python tools/focal_timing.py --config parent --repo <parent checkout> [--first-round 1] [--json FILE]
    python tools/focal_timing.py --report profiles/focal.txt --json FILE

Every step figure is the median of --reps windows of --steps steps, each window bracketed by device synchronisation, after a warm-up that takes the engine
past its two eager and two recorded steps (launch plans).  Every eval figure is the median of --reps calls, each ended by its own read.  One JSON line per
figure on stdout, appended to --json FILE when given; --report OUT writes the text of profiles/focal.txt (method, counts, and the table of whatever FILE
holds) and needs no GPU.  Timing needs the GPU: there is no fallback."""
import argparse
import json
import os
import sys
import time

CONFIGS = ("parent", "default", "bce", "focal", "asl", "eval")
LOSSES = {"bce": dict(type="BCELossWithLogits"), "focal": dict(type="SigmoidFocalLoss", gamma=2.0, alpha=0.25), "asl": dict(type="AsymmetricLossMultiLabel")}
EVAL_SHAPES = ((1863, 157, 0.04), (19796, 400, 0.005))    # rows, classes, label density
EVAL_OPTIONS = (("none", dict()), ("sample_ap", dict(sample_ap=True)), ("threshold", dict(threshold=0.5)), ("best_f1", dict(best_f1=True)),
                ("all", dict(sample_ap=True, threshold=0.5, best_f1=True)))

METHOD = """Focal / asymmetric losses (mvf_focal_loss / mvf_head_train_fwd_focal) and sample AP / F1 / best-F1 (csrc/multilabel_f1.hip): cost on the MI355X
====================================================================================================================================================

Method (tools/focal_timing.py).  Training step: R50, 8 frames, 224 x 224, bf16 storage, 12 and 32 clips; medians of --reps windows of --steps train_steps,
every window bracketed by a device synchronisation, after a warm-up past the launch plan's two eager and two recorded steps.  One MI355X, one session,
alternating processes (parent, this tree, parent, ...):

  parent   the parent commit's package (--repo <parent checkout>), which has none of this
  default  this tree, default loss: the accepted plan must have as many ops as the parent's, and the step time is judged against the run-to-run spread of
           a configuration's medians over the rounds of this same session.  Nothing in the default path changes
  bce / focal / asl   this tree, multi-hot (clips, 400) fp32 labels under BCELossWithLogits / SigmoidFocalLoss / AsymmetricLossMultiLabel: reported, not gated

Evaluation: metrics.DeviceMultiLabelMetrics.compute() on a filled record (sigmoid of gaussian scores, random labels at the stated density) with each
option, its launches and its reads, beside the host path on the same data: the (videos, classes) matrix read back + the numpy functions of evaluation.py
(mean_average_precision; + mmit_mean_average_precision; + precision_recall_f1; + best_f1_thresholds).  Medians of --reps calls.

By count (from shapes, no device needed).  The focal head replaces the BCE head's launch pair by another of the same grids over clips x 400 elements; per
element it adds two pow, one log and a dozen fp64 multiplies to BCE's exp and log1p: 4 800 elements at 12 clips.  The step's launch count and plan op count
do not change.  Sample AP: one launch, sum_i |P_i| x classes comparisons to (64-row x 64-class chunk) granularity -- at 19 796 x 400 at most 19 796 x 400^2
= 3.2e9 LDS broadcast reads if every chunk of every row holds a positive; the record is read ceil(classes / 64) + 1 times at most (32 MB each at that
size).  prf: one launch, one pass over the record.  best F1: one launch, one pass over tp / nn and the scores.
"""


def report(path, json_path):
    rows = []
    if json_path and os.path.exists(json_path):
        rows = [json.loads(line) for line in open(json_path) if line.strip().startswith("{")]
    text = METHOD + "\n"
    steps, evals = [r for r in rows if r["config"] != "eval"], [r for r in rows if r["config"] == "eval"]
    if not rows:
        text += ("Figures: NOT MEASURED.  No MI355X run of tools/focal_timing.py has been recorded yet.  No statement about speed rests on anything but the\n"
                 "counts above.\n")
    if steps:
        text += "Training step (one MI355X, one session; ms per train_step, median [min .. max] of the windows; plan_ops = ops of the accepted launch plan):\n\n"
        text += "  %-8s %5s %5s  %-32s %s\n" % ("config", "clips", "round", "ms / step", "plan_ops")
        for r in steps:
            ops = ",".join("-" if v is None else str(v) for v in r.get("plan_ops", [])) or "-"
            text += "  %-8s %5d %5d  %-32s %s\n" % (r["config"], r["clips"], r.get("round", 0), "%.3f [%.3f .. %.3f]" % (r["median_ms"], r["min_ms"], r["max_ms"]), ops)
        by = {}
        for r in steps:
            by.setdefault((r["config"], r["clips"]), []).append(r["median_ms"])
        mean = {k: sum(v) / len(v) for k, v in by.items()}
        text += "\n"
        for clips in sorted(set(k[1] for k in mean)):
            spread = [max(v) / min(v) - 1.0 for k, v in by.items() if k[1] == clips and len(v) > 1]
            if ("parent", clips) in mean and ("default", clips) in mean:
                p, o = mean[("parent", clips)], mean[("default", clips)]
                text += "  %d clips: default %.3f ms against parent %.3f ms = %+.2f %%\n" % (clips, o, p, (o / p - 1.0) * 100.0)
            if spread:
                text += "  %d clips: run-to-run spread of a configuration's medians over the rounds: up to %.2f %%\n" % (clips, max(spread) * 100.0)
            for name in ("bce", "focal", "asl"):
                if (name, clips) in mean and ("default", clips) in mean:
                    text += "  %d clips: %s %.3f ms = default %+.3f ms (reported, not gated)\n" % (clips, name, mean[(name, clips)], mean[(name, clips)] - mean[("default", clips)])
        text += "\n"
    if evals:
        text += "Evaluation (ms per call, median [min .. max]; device = compute(option) with its reads; host = the matrix read back + numpy):\n\n"
        text += "  %6s %7s %8s %-10s %5s  %-30s %-32s %s\n" % ("rows", "classes", "density", "option", "round", "device ms", "host ms", "agreement")
        for r in evals:
            text += "  %6d %7d %8.3f %-10s %5d  %-30s %-32s %s\n" % (r["rows"], r["classes"], r["density"], r["option"], r.get("round", 0),
                                                                    "%.3f [%.3f .. %.3f]" % (r["device_ms"], r["device_min_ms"], r["device_max_ms"]),
                                                                    "%.3f [%.3f .. %.3f]" % (r["host_ms"], r["host_min_ms"], r["host_max_ms"]), r["agreement"])
    with open(path, "w") as f:
        f.write(text)
    print("wrote %s (%d figures)" % (path, len(rows)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="default,bce,focal,asl,eval")
    ap.add_argument("--repo", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="checkout whose mvfnet_amd package is timed")
    ap.add_argument("--clips", default="12,32")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--first-round", type=int, default=0, help="the round number the first round is labelled with (alternating processes: parent, this tree, parent, ...)")
    ap.add_argument("--json", default=None, help="append every figure's JSON line to this file")
    ap.add_argument("--report", default=None, help="write the text of profiles/focal.txt from --json's figures and exit (no GPU)")
    args = ap.parse_args()
    if args.report:
        return report(args.report, args.json)
    configs = args.config.split(",")
    for config in configs:
        if config not in CONFIGS:
            raise SystemExit("focal_timing: --config takes %s" % ", ".join(CONFIGS))
    sys.path.insert(0, os.path.abspath(args.repo))
    import numpy as np
    import torch
    import mvfnet_amd
    from mvfnet_amd import synth
    if not torch.cuda.is_available():
        raise SystemExit("focal_timing: no GPU")

    def emit(**fig):
        line = json.dumps(fig)
        print(line, flush=True)
        if args.json:
            with open(args.json, "a") as f:
                f.write(line + "\n")

    def model(loss_cls):
        cfg = mvfnet_amd.mvfnet_config(50, args.frames)
        if loss_cls is not None:
            cfg["cls_head"]["loss_cls"] = loss_cls
        m = mvfnet_amd.build_recognizer(cfg, None, dict(average_clips=None))
        sd = m.state_dict()
        vals = synth.synth_state_dict({"r50/" + k: tuple(v.shape) for k, v in sd.items()}, seed=0)
        m.load_state_dict({k: torch.from_numpy(vals["r50/" + k]) for k in sd}, strict=True)
        return m.cuda()

    def time_step(config, clips, rnd):
        gen = torch.Generator(device="cuda").manual_seed(0)
        batches = []
        for _ in range(2):
            imgs = torch.randn(clips, args.frames, 3, args.size, args.size, device="cuda", generator=gen)
            labels = torch.randint(0, 400, (clips, 1), device="cuda", generator=gen)
            if config in LOSSES:
                labels = (torch.rand(clips, 400, device="cuda", generator=gen) < 0.02).float()
            batches.append((imgs, labels))
        eng = model(LOSSES.get(config)).train().train_engine(dtype=torch.bfloat16)
        for i in range(10):
            eng.train_step(*batches[i % 2])
        out = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(args.steps):
                eng.train_step(*batches[i % 2])
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) / args.steps * 1e3)
        out.sort()
        plans = [s["plan"] for s in getattr(eng, "_plans", {}).values()]
        emit(config=config, round=rnd, repo=os.path.abspath(args.repo), clips=clips, frames=args.frames, size=args.size, median_ms=round(out[len(out) // 2], 4),
             min_ms=round(out[0], 4), max_ms=round(out[-1], 4), steps_per_window=args.steps, reps=args.reps,
             plan_ops=[p.n_ops if p is not None else None for p in plans])
        del eng, batches
        torch.cuda.empty_cache()

    def time_eval(rows, classes, density, rnd):
        from mvfnet_amd import evaluation as ev
        from mvfnet_amd.metrics import DeviceMultiLabelMetrics
        gen = torch.Generator(device="cuda").manual_seed(rows + classes)
        scores = torch.sigmoid(torch.randn(rows, classes, device="cuda", generator=gen))
        labels = (torch.rand(rows, classes, device="cuda", generator=gen) < density).to(torch.uint8)
        m = DeviceMultiLabelMetrics(classes, capacity=rows)
        for i in range(0, rows, 256):
            m.update(scores[i:i + 256].contiguous(), labels[i:i + 256].contiguous())

        def host(option):
            s, y = scores.cpu().numpy(), labels.cpu().numpy()
            out = dict(mAP=ev.mean_average_precision(s, y))
            if option in ("sample_ap", "all"):
                out["sample_mAP"] = ev.mmit_mean_average_precision(s, y)
            if option in ("threshold", "all"):
                out.update(ev.precision_recall_f1(s, y, threshold=0.5))
            if option in ("best_f1", "all"):
                out.update(ev.best_f1_thresholds(s, y))
            return out
        for option, kw in EVAL_OPTIONS:
            dev, hst, fig, want = [], [], None, None
            m.compute(**kw)                              # warm-up: the code objects' first launch
            for _ in range(args.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fig = m.compute(**kw)
                dev.append((time.perf_counter() - t0) * 1e3)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                want = host(option)
                hst.append((time.perf_counter() - t0) * 1e3)
            dev.sort()
            hst.sort()
            agree = ["|mAP diff| %.1e" % abs(fig["mAP"] - want["mAP"])]
            if "sample_mAP" in fig:
                agree.append("|sample mAP diff| %.1e" % abs(fig["sample_mAP"] - want["sample_mAP"]))
            if "counts" in fig:
                agree.append("counts equal" if np.array_equal(fig["counts"], want["counts"]) else "COUNTS DIFFER")
            if "best_threshold" in fig:
                same = np.array_equal(fig["best_threshold"].astype(np.float64), want["best_threshold"], equal_nan=True) and np.array_equal(fig["best_f1"], want["best_f1"], equal_nan=True)
                agree.append("best F1 / thresholds equal" if same else "BEST F1 DIFFERS")
            emit(config="eval", option=option, round=rnd, rows=rows, classes=classes, density=density, reps=args.reps, device_ms=round(dev[len(dev) // 2], 4),
                 device_min_ms=round(dev[0], 4), device_max_ms=round(dev[-1], 4), host_ms=round(hst[len(hst) // 2], 4), host_min_ms=round(hst[0], 4),
                 host_max_ms=round(hst[-1], 4), agreement=", ".join(agree))

    for rnd in range(args.first_round, args.first_round + args.rounds):
        for config in configs:
            if config == "eval":
                for rows, classes, density in EVAL_SHAPES:
                    time_eval(rows, classes, density, rnd)
            else:
                for clips in (int(c) for c in args.clips.split(",")):
                    time_step(config, clips, rnd)


if __name__ == "__main__":
    main()
