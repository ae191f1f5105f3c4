"""What the binary cross-entropy head costs in the training step, and what mean average precision costs on the device, on the MI355X:

  parent   train_step of another checkout's package (--repo DIR: the parent commit), which has no BCE head          (R50, 8 frames, 224 x 224, bf16 storage)
  default  train_step of this tree with the default loss: must issue the launches the parent issues (the plan's op count is printed) and agree in time
           within the +-2.5 % box-to-box spread the README records
  bce      train_step of this tree with loss_cls = BCELossWithLogits against a multi-hot (clips, 400) label matrix: mvf_head_train_fwd_bce in the place of
           mvf_head_train_fwd, the same op count
  ap       mvf_multilabel_ap (metrics.DeviceMultiLabelMetrics.compute, its two launches and the read of ap / positives / state) at 1 863 x 157 (Charades
           validation) and 19 796 x 400, beside the host path: the read-back of the (videos, classes) matrix + evaluation.mean_average_precision

    python tools/multilabel_timing.py --config default,bce,ap [--clips 12,32] [--steps 40] [--reps 5] [--rounds 2] [--json FILE]
    python tools/multilabel_timing.py --config parent --repo <parent checkout> [--first-round 1] [--json FILE]
    python tools/multilabel_timing.py --report profiles/multilabel.txt --json FILE

Every step figure is the median of --reps windows of --steps steps, each window bracketed by device synchronisation, after a warm-up that takes the engine
past its two eager and two recorded steps (launch plans).  Every ap figure is the median of --reps calls, each ended by its own read.  One JSON line per figure
on stdout, appended to --json FILE when given; --report OUT writes the text of profiles/multilabel.txt (method, counts, and the table of whatever FILE holds)
and needs no GPU.  Timing needs the GPU: there is no fallback."""
import argparse
import json
import os
import sys
import time

CONFIGS = ("parent", "default", "bce", "ap")
AP_SHAPES = ((1863, 157, 0.04), (19796, 400, 0.005))      # rows, classes, label density (Charades: 6.8 actions per video; one label in 400 twice over)

METHOD = """Multi-label recognition (mvf_bce_loss / mvf_head_train_fwd_bce, mvf_multilabel_record / mvf_multilabel_ap): cost on the MI355X
====================================================================================================================================

Method (tools/multilabel_timing.py).  Training step: R50, 8 frames, 224 x 224, bf16 storage, 12 and 32 clips; medians of --reps windows of --steps
train_steps, every window bracketed by a device synchronisation, after a warm-up past the launch plan's two eager and two recorded steps:

  parent   the parent commit's package (--repo <parent checkout>), which has no BCE head
  default  this tree, default loss: the accepted plan must have as many ops as the parent's, and the step time must agree with the parent's within the
           +-2.5 % box-to-box spread the README records.  Nothing in the default path changes
  bce      this tree, loss_cls = BCELossWithLogits, multi-hot (clips, 400) fp32 labels: reported, not gated

AP evaluation: metrics.DeviceMultiLabelMetrics.compute() on a filled record (gaussian scores, random labels at the stated density) -- two launches and the
read of 2 x classes + 8 words -- beside the host path on the same data: the (videos, classes) score matrix read back + evaluation.mean_average_precision
(one numpy sort per class).  Medians of --reps calls.

By count (from shapes, no device needed).  The BCE head replaces one launch pair of the head (ce_loss_kernel + mean_reduce_kernel) by another
(bce_clip_kernel + bce_mean_kernel) over clips x 400 elements, 19 KB of scores at 12 clips: the step's launch count and plan op count do not change for a
label matrix, and integer labels add the one mvf_soft_targets launch smoothing already adds.  AP: the first launch makes sum_c |P_c| x n comparisons to
workgroup granularity -- at 1 863 x 157 and 4 % density at most 157 x 1 863^2 = 5.4e8, at 19 796 x 400 at most 400 x 19 796^2 = 1.6e11 if every 256-row
workgroup holds a positive -- each one LDS broadcast read, a compare and two integer adds per lane; the record is 1.2 MB / 31.7 MB of scores.
"""


def report(path, json_path):
    rows = []
    if json_path and os.path.exists(json_path):
        rows = [json.loads(line) for line in open(json_path) if line.strip().startswith("{")]
    text = METHOD + "\n"
    steps, aps = [r for r in rows if r["config"] != "ap"], [r for r in rows if r["config"] == "ap"]
    if not rows:
        text += ("Figures: NOT MEASURED.  No MI355X run of tools/multilabel_timing.py has been recorded yet.  Open: (1) 'default' against 'parent', plan op counts equal\n"
                 "and step time within +-2.5 %; (2) the cost of 'bce'; (3) the AP figures.  No statement about speed rests on anything but the counts above.\n")
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
            if ("parent", clips) in mean and ("default", clips) in mean:
                p, o = mean[("parent", clips)], mean[("default", clips)]
                text += "  %d clips: default %.3f ms against parent %.3f ms = %+.2f %% (to agree within +-2.5 %%)\n" % (clips, o, p, (o / p - 1.0) * 100.0)
            if ("bce", clips) in mean and ("default", clips) in mean:
                text += "  %d clips: bce %.3f ms = default %+.3f ms (reported, not gated)\n" % (clips, mean[("bce", clips)], mean[("bce", clips)] - mean[("default", clips)])
            spread = [max(v) / min(v) - 1.0 for k, v in by.items() if k[1] == clips and len(v) > 1]
            if spread:
                text += "  %d clips: run-to-run spread of a configuration's medians over the rounds: up to %.2f %%\n" % (clips, max(spread) * 100.0)
        text += "\n"
    if aps:
        text += "AP evaluation (ms per call, median [min .. max]; device = compute() with its read; host = the matrix read back + numpy):\n\n"
        text += "  %6s %7s %8s %5s  %-30s %-30s %s\n" % ("rows", "classes", "density", "round", "device ms", "host ms", "|mAP difference|")
        for r in aps:
            text += "  %6d %7d %8.3f %5d  %-30s %-30s %.2e\n" % (r["rows"], r["classes"], r["density"], r.get("round", 0),
                                                               "%.3f [%.3f .. %.3f]" % (r["device_ms"], r["device_min_ms"], r["device_max_ms"]),
                                                               "%.3f [%.3f .. %.3f]" % (r["host_ms"], r["host_min_ms"], r["host_max_ms"]), r["map_diff"])
    with open(path, "w") as f:
        f.write(text)
    print("wrote %s (%d figures)" % (path, len(rows)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="default,bce,ap")
    ap.add_argument("--repo", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="checkout whose mvfnet_amd package is timed")
    ap.add_argument("--clips", default="12,32")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--first-round", type=int, default=0, help="the round number the first round is labelled with (alternating processes: parent, this tree, parent, ...)")
    ap.add_argument("--json", default=None, help="append every figure's JSON line to this file")
    ap.add_argument("--report", default=None, help="write the text of profiles/multilabel.txt from --json's figures and exit (no GPU)")
    args = ap.parse_args()
    if args.report:
        return report(args.report, args.json)
    configs = args.config.split(",")
    for config in configs:
        if config not in CONFIGS:
            raise SystemExit("multilabel_timing: --config takes %s" % ", ".join(CONFIGS))
    sys.path.insert(0, os.path.abspath(args.repo))
    import numpy as np
    import torch
    import mvfnet_amd
    from mvfnet_amd import synth
    if not torch.cuda.is_available():
        raise SystemExit("multilabel_timing: no GPU")

    def emit(**fig):
        line = json.dumps(fig)
        print(line, flush=True)
        if args.json:
            with open(args.json, "a") as f:
                f.write(line + "\n")

    def model(bce):
        cfg = mvfnet_amd.mvfnet_config(50, args.frames)
        if bce:
            cfg["cls_head"]["loss_cls"] = dict(type="BCELossWithLogits")
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
            if config == "bce":
                labels = (torch.rand(clips, 400, device="cuda", generator=gen) < 0.02).float()
            batches.append((imgs, labels))
        eng = model(config == "bce").train().train_engine(dtype=torch.bfloat16)
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

    def time_ap(rows, classes, density, rnd):
        from mvfnet_amd.evaluation import mean_average_precision
        from mvfnet_amd.metrics import DeviceMultiLabelMetrics
        gen = torch.Generator(device="cuda").manual_seed(rows + classes)
        scores = torch.randn(rows, classes, device="cuda", generator=gen)
        labels = (torch.rand(rows, classes, device="cuda", generator=gen) < density).to(torch.uint8)
        m = DeviceMultiLabelMetrics(classes, capacity=rows)
        for i in range(0, rows, 256):
            m.update(scores[i:i + 256].contiguous(), labels[i:i + 256].contiguous())
        dev, host, fig, want = [], [], None, None
        m.compute()                                  # warm-up: the code objects' first launch
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fig = m.compute()
            dev.append((time.perf_counter() - t0) * 1e3)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            want = mean_average_precision(scores.cpu().numpy(), labels.cpu().numpy())
            host.append((time.perf_counter() - t0) * 1e3)
        dev.sort()
        host.sort()
        emit(config="ap", round=rnd, rows=rows, classes=classes, density=density, reps=args.reps, device_ms=round(dev[len(dev) // 2], 4),
             device_min_ms=round(dev[0], 4), device_max_ms=round(dev[-1], 4), host_ms=round(host[len(host) // 2], 4), host_min_ms=round(host[0], 4),
             host_max_ms=round(host[-1], 4), mAP=fig["mAP"], map_diff=abs(fig["mAP"] - want), positives=int(np.sum(fig["positives"])))

    for rnd in range(args.first_round, args.first_round + args.rounds):
        for config in configs:
            if config == "ap":
                for rows, classes, density in AP_SHAPES:
                    time_ap(rows, classes, density, rnd)
            else:
                for clips in (int(c) for c in args.clips.split(",")):
                    time_step(config, clips, rnd)


if __name__ == "__main__":
    main()
