"""What RandAugment costs in the training step on the MI355X (R50, 8 frames, bf16 storage) from uint8 256 x 340 frames cropped to 224 x 224 by a
FramePipeline, at 12 and 32 clips:

  parent   train_step of another checkout's package (--repo DIR: the parent commit), which has no RandAugment
  off      train_step of this tree with randaug off: issues the launches the parent issues; must agree in time within the +-2.5 % box-to-box spread the
           README records
  on       train_step of this tree with RandAugment('rand-m7-n4-mstd0.5-inc1') on the engine: the host's draw, the table's one non-blocking host-to-device
           copy, and mvf_frames_randaug_u8 (four apply passes, and a statistics pass for every layer in which some clip drew autocontrast, equalize or
           contrast) in front of the frame kernel
  stats    the same with ops = Equalize only and prob = 1: four statistics passes and four table-lookup passes, the most passes a table can ask for
  affine   the same with ops = Rotate only and prob = 1: four passes of the fp64 bilinear map, the most arithmetic a table can ask for

    python tools/randaug_timing.py --config off,on,stats,affine [--clips 12,32] [--steps 40] [--reps 5] [--rounds 2]
    python tools/randaug_timing.py --config parent --repo <parent checkout>

The uint8 path never runs from a launch plan, so every step is an eager one.  Every figure is the median of --reps windows of --steps steps, each window
bracketed by device synchronisation, after a warm-up of 10 steps.  --rounds N runs the whole list of configurations N times, one after another, so that two
configurations are compared within one process on one box.  One JSON line per figure on stdout.  Needs the GPU: there is no fallback."""
import argparse
import json
import os
import random
import sys
import time

CONFIGS = ("parent", "off", "on", "stats", "affine")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="off,on")
    ap.add_argument("--repo", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="checkout whose mvfnet_amd package is timed")
    ap.add_argument("--clips", default="12,32")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--source", default="256x340", help="HxW of the uploaded frames")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=1)
    args = ap.parse_args()
    configs = args.config.split(",")
    for config in configs:
        if config not in CONFIGS:
            raise SystemExit("randaug_timing: --config takes %s" % ", ".join(CONFIGS))
    hs, ws = (int(v) for v in args.source.split("x"))
    sys.path.insert(0, os.path.abspath(args.repo))
    import numpy as np
    import torch
    import mvfnet_amd
    from mvfnet_amd import synth
    from mvfnet_amd.preprocess import FramePipeline
    if not torch.cuda.is_available():
        raise SystemExit("randaug_timing: no GPU")

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
                batches = [(torch.randint(0, 256, (clips, args.frames, hs, ws, 3), device="cuda", generator=gen, dtype=torch.uint8),
                            torch.randint(0, 400, (clips, 1), device="cuda", generator=gen)) for _ in range(2)]
                eng = engine()
                pipe = FramePipeline(crop_size=args.size)
                eng.input_pipeline = pipe
                eng.input_window = pipe.center_window(clips * args.frames, hs, ws)
                if config in ("on", "stats", "affine"):
                    from mvfnet_amd.randaug import RandAugment
                    random.seed(0)
                    np.random.seed(0)
                    kw = dict(on={}, stats=dict(ops=["Equalize"], prob=1.0), affine=dict(ops=["Rotate"], prob=1.0))[config]
                    eng.randaug = RandAugment("rand-m7-n4-mstd0.5-inc1", **kw)
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
                print(json.dumps(dict(config=config, round=rnd, repo=os.path.abspath(args.repo), clips=clips, frames=args.frames, size=args.size,
                                      source=[hs, ws], median_ms=round(out[len(out) // 2], 4), min_ms=round(out[0], 4), max_ms=round(out[-1], 4),
                                      steps_per_window=args.steps, reps=args.reps)), flush=True)
                del eng, batches
                torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
