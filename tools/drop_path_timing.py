"""What drop path (stochastic depth) costs in the training step on the MI355X (R50, 8 frames, 224 x 224, bf16 storage, fp32 clips through the launch
plans) at 12 and 32 clips, and what its forward kernel costs beside mvf_bn_apply_bits.  Writes profiles/drop_path.txt.

  parent   train_step of another checkout's package (--parent DIR: the parent commit), which has no drop path
  off      train_step of this tree with drop_path unset: issues the launches the parent issues -- the same plan op count, and a time equal within the
           run-to-run spread of the two configurations' medians in this session
  r005     train_step with DropPath(0.05) on the engine (the A1 / A2 recipes): the 15 blocks behind block 0 take the stored-z3 path and the two kernels
  r02      the same with DropPath(0.2)
  kernels  mvf_bn_apply_bits_rowscale against mvf_bn_apply_bits, timed in one run on the four stages' bn3 shapes at 32 clips (256 images)

    python tools/drop_path_timing.py --parent <parent checkout> [--out profiles/drop_path.txt] [--clips 12,32] [--rounds 3] [--steps 30] [--reps 5]
    python tools/drop_path_timing.py --child off --clips 12          (one configuration in this process: one JSON line per figure)

The driver starts every configuration in a fresh child process, parent and off alternating, one at a time, each under a time limit; a child that fails ends
the run.  Every step figure is the median of --reps windows of --steps steps, each window bracketed by device synchronisation, after 12 warm-up steps (two
eager, two recorded, the rest replayed).  Needs the GPU: there is no fallback."""
import argparse
import json
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
CONFIGS = ("parent", "off", "r005", "r02", "kernels")
KEEP_MARKER = "---- errors printed by tests/test_drop_path_gpu.py"
BN3_SHAPES = ((56, 256), (28, 512), (14, 1024), (7, 2048))          # (h = w, c) of the four stages' bn3 at 224 x 224


def child_step(args, config, clips):
    import torch
    import mvfnet_amd
    from mvfnet_amd import synth
    m = mvfnet_amd.build_recognizer(mvfnet_amd.mvfnet_config(50, args.frames), None, dict(average_clips=None))
    sd = m.state_dict()
    vals = synth.synth_state_dict({"r50/" + k: tuple(v.shape) for k, v in sd.items()})
    m.load_state_dict({k: torch.from_numpy(vals["r50/" + k]) for k in sd}, strict=True)
    eng = m.cuda().train().train_engine(dtype=torch.bfloat16)
    if config in ("r005", "r02"):
        from mvfnet_amd.droppath import DropPath
        eng.drop_path = DropPath(0.05 if config == "r005" else 0.2, seed=0)
    gen = torch.Generator(device="cuda").manual_seed(0)
    batches = [(torch.randn(clips, args.frames, 3, args.size, args.size, device="cuda", generator=gen), torch.randint(0, 400, (clips, 1), device="cuda", generator=gen))
               for _ in range(2)]
    for i in range(12):
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
    plans = [s["plan"] for s in getattr(eng, "_plans", {}).values() if s["plan"] is not None]
    print(json.dumps(dict(config=config, clips=clips, median_ms=round(out[len(out) // 2], 4), min_ms=round(out[0], 4), max_ms=round(out[-1], 4),
                          plan_ops=plans[0].n_ops if plans else 0, steps_per_window=args.steps, reps=args.reps)), flush=True)


def child_kernels(args):
    import ctypes as C
    import torch
    from mvfnet_amd import _lib
    lib = _lib.lib
    n = 32 * args.frames

    def p(t):
        return C.c_void_p(t.data_ptr())
    for hw, c in BN3_SHAPES:
        m = n * hw * hw
        z, r = torch.randn(m, c, device="cuda").bfloat16(), torch.randn(m, c, device="cuda").relu_().bfloat16()
        sc, sh = torch.rand(c, device="cuda") + 0.5, torch.randn(c, device="cuda") * 0.1
        tab = (torch.rand(n, device="cuda") > 0.1).float() / 0.9
        out, bits = torch.empty_like(z), torch.empty(m, c // 4, dtype=torch.uint8, device="cuda")

        def old():
            _lib.check(lib.mvf_bn_apply_bits(p(z), m, c, p(sc), p(sh), p(r), None, None, 1, p(out), p(bits), 1, None))

        def new():
            _lib.check(lib.mvf_bn_apply_bits_rowscale(p(z), m, c, p(sc), p(sh), p(r), None, None, p(tab), hw * hw, 1, p(out), p(bits), 1, None))
        t = dict(old=[], new=[])
        for fn in (old, new):
            for _ in range(10):
                fn()
        for _ in range(args.reps):
            for name, fn in (("old", old), ("new", new)):            # alternating windows in one run
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.kernel_iters):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                t[name].append(e0.elapsed_time(e1) / args.kernel_iters * 1e3)
        for v in t.values():
            v.sort()
        old_us, new_us = t["old"][len(t["old"]) // 2], t["new"][len(t["new"]) // 2]
        gbytes = (3 * m * c * 2 + m * c // 4) / 1e9
        print(json.dumps(dict(config="kernels", m=m, c=c, rows_per_image=hw * hw, old_us=round(old_us, 2), new_us=round(new_us, 2), ratio=round(new_us / old_us, 4),
                              old_tbps=round(gbytes / old_us * 1e3, 3), new_tbps=round(gbytes / new_us * 1e3, 3))), flush=True)


def run_child(args, config, clips, repo):
    cmd = [sys.executable, os.path.abspath(__file__), "--child", config, "--clips", str(clips), "--steps", str(args.steps), "--reps", str(args.reps),
           "--frames", str(args.frames), "--size", str(args.size), "--kernel-iters", str(args.kernel_iters), "--repo", repo]
    res = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=args.child_timeout, cwd=repo)
    if res.returncode != 0:
        sys.stderr.write(res.stderr.decode("utf-8", "replace")[-4000:])
        raise SystemExit("drop_path_timing: the %s child ended with status %d; nothing more is started" % (config, res.returncode))
    rows = [json.loads(line) for line in res.stdout.decode().splitlines() if line.startswith("{")]
    for row in rows:
        print(json.dumps(row), flush=True)
    return rows


def driver(args):
    clips = [int(c) for c in args.clips.split(",")]
    rows = []
    for rnd in range(args.rounds):                                   # parent and off alternate; the two rates ride along in every round
        for c in clips:
            for config in ("parent", "off", "r005", "r02"):
                if config == "parent" and not args.parent:
                    continue
                for row in run_child(args, config, c, os.path.abspath(args.parent) if config == "parent" else REPO):
                    row["round"] = rnd
                    rows.append(row)
    kern = run_child(args, "kernels", 32, REPO)
    lines = ["Drop path (stochastic depth): cost on one MI355X, one session, one configuration per process, alternating (tools/drop_path_timing.py).",
             "R50, 8 frames, 224 x 224, bf16 storage, fp32 clips replayed from launch plans; medians of %d windows of %d steps, ms per step." % (args.reps, args.steps), ""]
    med = {}
    for c in clips:
        lines.append("%d clips" % c)
        for config in ("parent", "off", "r005", "r02"):
            mine = [r for r in rows if r["clips"] == c and r["config"] == config]
            if not mine:
                continue
            ms = [r["median_ms"] for r in mine]
            med[(c, config)] = ms
            lines.append("  %-7s medians per round %s   spread %.3f   plan ops %s" % (config, " ".join("%.3f" % v for v in ms), max(ms) - min(ms),
                                                                                    sorted(set(r["plan_ops"] for r in mine))))
        lines.append("")
    lines.append("(a) drop_path unset against the parent commit: equal when the difference of the mean medians is within the larger run-to-run spread")
    for c in clips:
        if (c, "parent") in med:
            p_, o_ = med[(c, "parent")], med[(c, "off")]
            diff = sum(o_) / len(o_) - sum(p_) / len(p_)
            spread = max(max(p_) - min(p_), max(o_) - min(o_))
            lines.append("  %d clips: off - parent = %+.3f ms (%+.2f %%), spread %.3f ms -> %s" % (c, diff, 100.0 * diff / (sum(p_) / len(p_)), spread,
                                                                                                 "equal within the spread" if abs(diff) <= spread else "OUTSIDE the spread"))
    lines += ["", "(b) the step with drop path on (no bound was set in advance: the 15 blocks behind block 0 leave the fused paths)"]
    for c in clips:
        o_ = sum(med[(c, "off")]) / len(med[(c, "off")])
        for config in ("r005", "r02"):
            v = sum(med[(c, config)]) / len(med[(c, config)])
            lines.append("  %d clips: %s %.3f ms against off %.3f ms: %+.3f ms (%+.1f %%)" % (c, config, v, o_, v - o_, 100.0 * (v - o_) / o_))
    lines += ["", "(c) mvf_bn_apply_bits_rowscale against mvf_bn_apply_bits, bf16, plain residual, ReLU, 256 images, one run (expected: at most 1.1 x)"]
    for r in kern:
        lines.append("  m %7d c %4d rows/image %4d: old %8.2f us (%.2f TB/s)  new %8.2f us (%.2f TB/s)  ratio %.3f%s" % (
            r["m"], r["c"], r["rows_per_image"], r["old_us"], r["old_tbps"], r["new_us"], r["new_tbps"], r["ratio"], "" if r["ratio"] <= 1.1 else "   ABOVE 1.1"))
    text = "\n".join(lines) + "\n"
    if os.path.exists(args.out):                                      # the section below the marker (the tests' printed errors) is kept as it is
        old = open(args.out).read()
        if KEEP_MARKER in old:
            text += "\n" + old[old.index(KEEP_MARKER):]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    sys.stdout.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", default=None, help="run one configuration in this process: %s" % ", ".join(CONFIGS))
    ap.add_argument("--repo", default=REPO, help="(child) checkout whose mvfnet_amd package is timed")
    ap.add_argument("--parent", default=None, help="checkout of the parent commit, built")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "drop_path.txt"))
    ap.add_argument("--clips", default="12,32")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--kernel-iters", type=int, default=50)
    ap.add_argument("--child-timeout", type=int, default=240)
    args = ap.parse_args()
    if args.child is None:
        return driver(args)
    if args.child not in CONFIGS:
        raise SystemExit("drop_path_timing: --child takes %s" % ", ".join(CONFIGS))
    sys.path.insert(0, os.path.abspath(args.repo))
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("drop_path_timing: no GPU")
    if args.child == "kernels":
        return child_kernels(args)
    for c in (int(v) for v in args.clips.split(",")):
        child_step(args, args.child, c)


if __name__ == "__main__":
    main()
