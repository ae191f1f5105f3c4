"""What knowledge distillation costs in the training step on the MI355X (student R50, 8 frames, 224 x 224, bf16 storage), at 12 and 32 clips:

  parent   train_step of another checkout's package (--repo DIR: the parent commit), which has no distillation
  off      train_step of this tree with distill off: must issue the launches the parent issues (the plan's op count is printed) and agree in time within the
           +-2.5 % box-to-box spread the README records
  r50      train_step of this tree with KnowledgeDistillation(<an R50 teacher>, temperature=4, alpha=0.5) on the engine: + the teacher's eval-mode chain on the
           step's stem operand and mvf_distill_loss; such steps run eagerly (no launch plan)
  r101     the same with an R101 teacher

    python tools/distill_timing.py --config off,r50,r101 [--clips 12,32] [--steps 40] [--reps 5] [--rounds 2] [--json FILE]
    python tools/distill_timing.py --config parent --repo <parent checkout> [--first-round 1] [--json FILE]
    python tools/distill_timing.py --report profiles/distill.txt --json FILE

Every figure is the median of --reps windows of --steps steps, each window bracketed by device synchronisation, after a warm-up that takes the engine past its
two eager and two recorded steps (launch plans).  --rounds N runs the whole list of configurations N times, one after another, so that two configurations are
compared within one process on one box.  One JSON line per figure on stdout, appended to --json FILE when given; --report OUT writes the text of
profiles/distill.txt (method, counts, and the table of whatever FILE holds) and needs no GPU.  Timing needs the GPU: there is no fallback."""
import argparse
import json
import os
import sys
import time

CONFIGS = ("parent", "off", "r50", "r101")

METHOD = """Knowledge distillation (mvf_distill_loss, BackboneEngine.forward_stem; TrainEngine.distill): cost on the MI355X
=================================================================================================================

Method (tools/distill_timing.py; student R50, 8 frames, 224 x 224, bf16 storage, 12 and 32 clips; medians of --reps windows of --steps train_steps, every
window bracketed by a device synchronisation, after a warm-up past the launch plan's two eager and two recorded steps), four configurations:

  parent   the parent commit's package (--repo <parent checkout>), which has no distillation
  off      this tree, distill off: the accepted plan must have as many ops as the parent's, and the step time must agree with the parent's within the
           +-2.5 % box-to-box spread the README records.  Nothing in the off path changes
  r50      this tree, KnowledgeDistillation(R50 teacher, temperature = 4, alpha = 0.5) on the engine: reported, not gated
  r101     the same with an R101 teacher: reported, not gated

By count (from shapes, no device needed).  The teacher reads the stem operand the student's own stem reads -- one frame is 230 x 232 x 4 elements =
426 880 bytes in bf16, 41.0 MB at 12 clips (96 frames), 109.3 MB at 32 (256 frames) -- so no pixel is uploaded, cropped or normalised a second time.  Per
step with distill on: + the teacher's eval-mode launch chain (stem conv, max-pool, 16 / 33 bottleneck blocks with BatchNorm folded, the head's pool + fc:
the chain BackboneEngine.forward runs without its stem-prep launch) + 3 launches of mvf_distill_loss over clips x 400 scores (19 KB at 12 clips) + one
(clips, 400) fp32 buffer and 2 floats.  The step runs eagerly: the student's launches are issued from Python instead of from its recorded plan,
which is part of the measured difference.  From the recorded bf16 inference rate (about 7.9 k clips/s for R50, README) one would guess +1.5 ms at 12
clips for an R50 teacher and about twice that for R101 -- a guess from the byte and rate figures, not a result.
"""


def report(path, json_path):
    rows = []
    if json_path and os.path.exists(json_path):
        rows = [json.loads(line) for line in open(json_path) if line.strip().startswith("{")]
    text = METHOD + "\n"
    if not rows:
        text += ("Figures: NOT MEASURED.  No MI355X run of tools/distill_timing.py has been recorded yet.  Open: (1) 'off' against 'parent', plan op counts equal and step\n"
                 "time within +-2.5 %; (2) the cost of 'r50' and 'r101'.  No statement about the speed of this path rests on anything but the counts above.\n")
    else:
        text += "Figures (one MI355X, one session; ms per train_step, median [min .. max] of the windows; plan_ops = ops of the accepted launch plan, - = eager):\n\n"
        text += "  %-7s %5s %5s  %-32s %s\n" % ("config", "clips", "round", "ms / step", "plan_ops")
        for r in rows:
            ops = ",".join("-" if v is None else str(v) for v in r.get("plan_ops", [])) or "-"
            text += "  %-7s %5d %5d  %-32s %s\n" % (r["config"], r["clips"], r.get("round", 0), "%.3f [%.3f .. %.3f]" % (r["median_ms"], r["min_ms"], r["max_ms"]), ops)
        by = {}
        for r in rows:
            by.setdefault((r["config"], r["clips"]), []).append(r["median_ms"])
        mean = {k: sum(v) / len(v) for k, v in by.items()}
        text += "\n"
        for clips in sorted(set(k[1] for k in mean)):
            if ("parent", clips) in mean and ("off", clips) in mean:
                p, o = mean[("parent", clips)], mean[("off", clips)]
                text += "  %d clips: off %.3f ms against parent %.3f ms = %+.2f %% (to agree within +-2.5 %%)\n" % (clips, o, p, (o / p - 1.0) * 100.0)
            for cfg in ("r50", "r101"):
                if (cfg, clips) in mean and ("off", clips) in mean:
                    text += "  %d clips: %s teacher %.3f ms = off %+.3f ms (reported, not gated)\n" % (clips, cfg, mean[(cfg, clips)], mean[(cfg, clips)] - mean[("off", clips)])
    with open(path, "w") as f:
        f.write(text)
    print("wrote %s (%d figures)" % (path, len(rows)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="off,r50,r101")
    ap.add_argument("--repo", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="checkout whose mvfnet_amd package is timed")
    ap.add_argument("--clips", default="12,32")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--first-round", type=int, default=0, help="the round number the first round is labelled with (alternating processes: parent, this tree, parent, ...)")
    ap.add_argument("--json", default=None, help="append every figure's JSON line to this file")
    ap.add_argument("--report", default=None, help="write the text of profiles/distill.txt from --json's figures and exit (no GPU)")
    args = ap.parse_args()
    if args.report:
        return report(args.report, args.json)
    configs = args.config.split(",")
    for config in configs:
        if config not in CONFIGS:
            raise SystemExit("distill_timing: --config takes %s" % ", ".join(CONFIGS))
    sys.path.insert(0, os.path.abspath(args.repo))
    import torch
    import mvfnet_amd
    from mvfnet_amd import synth
    if not torch.cuda.is_available():
        raise SystemExit("distill_timing: no GPU")

    def model(depth, seed):
        m = mvfnet_amd.build_recognizer(mvfnet_amd.mvfnet_config(depth, args.frames), None, dict(average_clips=None))
        sd = m.state_dict()
        vals = synth.synth_state_dict({"r%d/" % depth + k: tuple(v.shape) for k, v in sd.items()}, seed=seed)
        m.load_state_dict({k: torch.from_numpy(vals["r%d/" % depth + k]) for k in sd}, strict=True)
        return m.cuda()

    for rnd in range(args.first_round, args.first_round + args.rounds):
        for config in configs:
            for clips in (int(c) for c in args.clips.split(",")):
                gen = torch.Generator(device="cuda").manual_seed(0)
                batches = [(torch.randn(clips, args.frames, 3, args.size, args.size, device="cuda", generator=gen),
                            torch.randint(0, 400, (clips, 1), device="cuda", generator=gen)) for _ in range(2)]
                eng = model(50, 0).train().train_engine(dtype=torch.bfloat16)
                if config in ("r50", "r101"):
                    from mvfnet_amd.distill import KnowledgeDistillation
                    eng.distill = KnowledgeDistillation(model(50 if config == "r50" else 101, 1), temperature=4.0, alpha=0.5)
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
                line = json.dumps(dict(config=config, round=rnd, repo=os.path.abspath(args.repo), clips=clips, frames=args.frames, size=args.size,
                                       median_ms=round(out[len(out) // 2], 4), min_ms=round(out[0], 4), max_ms=round(out[-1], 4), steps_per_window=args.steps,
                                       reps=args.reps, plan_ops=[p.n_ops if p is not None else None for p in plans]))
                print(line, flush=True)
                if args.json:
                    with open(args.json, "a") as f:
                        f.write(line + "\n")
                del eng, batches
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
