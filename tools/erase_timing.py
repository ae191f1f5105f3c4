"""What RandomErasing costs in the training step on the MI355X (R50, 8 frames, 224 x 224, bf16 storage), at 12 and 32 clips:

  parent   train_step of another checkout's package (--repo DIR: the parent commit), which has no erasing
  off      train_step of this tree with erasing off: must issue the launches the parent issues (the plan's op count is printed) and agree in time within the
           +-2.5 % box-to-box spread the README records
  pixel    train_step of this tree with RandomErasing(probability=0.25, mode='pixel') on the engine: + mvf_stem_erase, and the table's one non-blocking
           host-to-device copy per step
  worst    the same with probability=1 and min_area = max_area = 1/3: every clip erased at the largest area, the most the kernel ever writes

    python tools/erase_timing.py --config off,pixel,worst [--clips 12,32] [--steps 40] [--reps 5] [--rounds 2]
    python tools/erase_timing.py --config parent --repo <parent checkout>

Every figure is the median of --reps windows of --steps steps, each window bracketed by device synchronisation, after a warm-up that takes the engine past its
two eager and two recorded steps (launch plans).  --rounds N runs the whole list of configurations N times, one after another, so that two configurations are
compared within one process on one box.  One JSON line per figure on stdout.  Needs the GPU: there is no fallback."""
import argparse
import json
import os
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="off,pixel")
    ap.add_argument("--repo", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="checkout whose mvfnet_amd package is timed")
    ap.add_argument("--clips", default="12,32")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=1)
    args = ap.parse_args()
    configs = args.config.split(",")
    for config in configs:
        if config not in ("parent", "off", "pixel", "worst"):
            raise SystemExit("erase_timing: --config takes parent, off, pixel, worst")
    sys.path.insert(0, os.path.abspath(args.repo))
    import torch
    import mvfnet_amd
    from mvfnet_amd import synth
    if not torch.cuda.is_available():
        raise SystemExit("erase_timing: no GPU")

    def engine():
        m = mvfnet_amd.build_recognizer(mvfnet_amd.mvfnet_config(50, args.frames), None, dict(average_clips=None))
        sd = m.state_dict()
        vals = synth.synth_state_dict({"r50/" + k: tuple(v.shape) for k, v in sd.items()})
        m.load_state_dict({k: torch.from_numpy(vals["r50/" + k]) for k in sd}, strict=True)
        return m.cuda().train().train_engine(dtype=torch.bfloat16)

    for rnd in range(args.rounds):
        for config in configs:
            for clips in (int(c) for c in args.clips.split(",")):
                gen = torch.Generator(device="cuda").manual_seed(0)
                batches = [(torch.randn(clips, args.frames, 3, args.size, args.size, device="cuda", generator=gen),
                            torch.randint(0, 400, (clips, 1), device="cuda", generator=gen)) for _ in range(2)]
                eng = engine()
                if config in ("pixel", "worst"):
                    from mvfnet_amd.erasing import RandomErasing
                    kw = dict(probability=1.0, min_area=1.0 / 3.0, max_area=1.0 / 3.0) if config == "worst" else dict(probability=0.25)
                    eng.erasing = RandomErasing(mode="pixel", seed=0, **kw)
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
                print(json.dumps(dict(config=config, round=rnd, repo=os.path.abspath(args.repo), clips=clips, frames=args.frames, size=args.size,
                                      median_ms=round(out[len(out) // 2], 4), min_ms=round(out[0], 4), max_ms=round(out[-1], 4), steps_per_window=args.steps,
                                      reps=args.reps, plan_ops=[p.n_ops if p is not None else None for p in plans])), flush=True)
                del eng, batches
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
