"""What the temporal-relation head (TSNClsHead consensus 'TRN' / 'TRNmultiscale'; csrc/trn_head.hip) costs on the MI355X:

  parent   train_step of another checkout's package (--repo DIR: the parent commit), which has none of this              (R50, 8 frames, 224 x 224, bf16 storage)
  default  train_step of this tree with the default (average) head: must issue the launches the parent issues (the plan's op count is printed) and agree
           in time within the run-to-run spread of the medians measured in the same session
  trn      train_step with consensus_cfg = dict(type='TRN', num_frames=8): eager steps (no launch plan)
  trnms    the same with 'TRNmultiscale' (19 relation rows per step)
  head     mvf_trn_head_fwd + mvf_trn_head_bwd alone (bf16 features, 7 x 7 x 2048, 400 classes) beside a torch-eager fp32 autograd restatement of the same
           head on the same device in the same process, both types, with the launch counts of the HIP head from its launch record

    python tools/trn_head_timing.py --config default,trn,trnms,head [--clips 12,32] [--steps 40] [--reps 5] [--rounds 2] [--json FILE]
    python tools/trn_head_timing.py --config parent --repo <parent checkout> [--first-round 1] [--json FILE]
    python tools/trn_head_timing.py --report profiles/trn_head.txt --json FILE [--errors TEST_LOG]

Every step figure is the median of --reps windows of --steps steps, each window bracketed by device synchronisation, after a warm-up that takes the engine
past its two eager and two recorded steps (launch plans).  Every head figure is the median of --reps windows of --steps forward + backward pairs.  One JSON
line per figure on stdout, appended to --json FILE when given; --report OUT writes the text of profiles/trn_head.txt (method, and the tables of whatever FILE
holds; --errors: the 'end to end' lines of a tests/test_trn_head_gpu.py -s log) and needs no GPU.  Timing needs the GPU: there is no fallback."""
import argparse
import ctypes as C
import json
import os
import sys
import time

CONFIGS = ("parent", "default", "trn", "trnms", "head")
KINDS = {"trn": "TRN", "trnms": "TRNmultiscale"}

METHOD = """Temporal-relation head (TSNClsHead consensus 'TRN' / 'TRNmultiscale'; mvf_trn_head_fwd / mvf_trn_head_bwd, csrc/trn_head.hip): cost on the MI355X
=================================================================================================================================================

Method (tools/trn_head_timing.py).  Training step: R50, 8 frames, 224 x 224, bf16 storage, 400 classes, 12 and 32 clips; medians of --reps windows of --steps
train_steps, every window bracketed by a device synchronisation, after a warm-up past the launch plan's two eager and two recorded steps.  One MI355X, one
session, alternating processes (parent, this tree, parent, ...):

  parent   the parent commit's package (--repo <parent checkout>), which has none of this
  default  this tree, default head: the accepted plan must have as many ops as the parent's, and the step time is judged against the run-to-run spread of
           a configuration's medians over the rounds of this same session.  Nothing in the default path changes
  trn / trnms   this tree with the relation head: these steps run EAGERLY (no launch plan: the per-scale operands are a host array built per call), so the
           figure holds the Python launch sequence of the whole step, not only the head.  Reported, not gated

Head alone: mvf_trn_head_fwd + mvf_trn_head_bwd through the C ABI on bf16 features (clips x 8, 7 x 7, 2048), 400 classes, a drawn table (1 row for TRN,
19 for TRNmultiscale), beside the same head restated with torch modules in fp32 (mean, Linear, ReLU, index, sum; autograd backward of sum(scores * dscores),
the bf16 -> fp32 cast of the features included) on the same device in the same process.  The HIP head's launch count is its launch record's
(mvf_trn_head_last_launch); the torch restatement's launches were not counted.

By count (from shapes, no device needed).  The relation head holds 256 x 2048 + 512 x 2048 + 400 x 512 = 1.8 M parameters ('TRN', T = 8) or 256 x 2048 +
35 x 65 536 + 7 x 400 x 256 = 3.5 M ('TRNmultiscale', T = 8); it launches 5 kernels forward and 7 backward whatever the number of relation rows, plus the
2 launches of the stand-alone loss, against the average head's 4 + 4.
"""


def report(path, json_path, errors_path):
    rows = []
    if json_path and os.path.exists(json_path):
        rows = [json.loads(line) for line in open(json_path) if line.strip().startswith("{")]
    text = METHOD + "\n"
    steps, heads = [r for r in rows if r["config"] != "head"], [r for r in rows if r["config"] == "head"]
    if not rows:
        text += ("Figures: NOT MEASURED.  No MI355X run of tools/trn_head_timing.py has been recorded yet.  No statement about speed rests on anything but the\n"
                 "counts above.\n")
    if steps:
        text += "Training step (one MI355X, one session; ms per train_step, median [min .. max] of the windows; plan_ops = ops of the accepted launch plan):\n\n"
        text += "  %-8s %5s %5s  %-32s %s\n" % ("config", "clips", "round", "ms / step", "plan_ops")
        for r in steps:
            ops = ",".join("-" if v is None else str(v) for v in r.get("plan_ops", [])) or "- (eager)"
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
            for name in ("trn", "trnms"):
                if (name, clips) in mean and ("default", clips) in mean:
                    text += "  %d clips: %s %.3f ms = default %+.3f ms (eager step against a planned one; reported, not gated)\n" % (
                        clips, name, mean[(name, clips)], mean[(name, clips)] - mean[("default", clips)])
        text += "\n"
    if heads:
        text += "Head alone (ms per forward + backward, median [min .. max]; launches = the HIP head's launch record, forward + backward):\n\n"
        text += "  %-14s %5s %5s %5s  %-30s %-32s %s\n" % ("type", "clips", "rows", "round", "HIP ms", "torch eager fp32 ms", "launches")
        for r in heads:
            text += "  %-14s %5d %5d %5d  %-30s %-32s %d + %d\n" % (r["kind"], r["clips"], r["rows"], r.get("round", 0),
                                                                   "%.4f [%.4f .. %.4f]" % (r["hip_ms"], r["hip_min_ms"], r["hip_max_ms"]),
                                                                   "%.4f [%.4f .. %.4f]" % (r["torch_ms"], r["torch_min_ms"], r["torch_max_ms"]), r["launches_fwd"], r["launches_bwd"])
        text += "\n"
    if errors_path and os.path.exists(errors_path):
        lines = [ln.strip() for ln in open(errors_path) if "end to end" in ln]
        if lines:
            text += ("End-to-end errors observed on the MI355X (tests/test_trn_head_gpu.py: device forward + mvf_ce_loss + backward against the fp64 chain from the\n"
                     "inputs; max-norm relative to each tensor's largest magnitude; dfeat of the bf16 cases holds its one bf16 rounding):\n\n")
            text += "".join("  " + ln.lstrip(".F") + "\n" for ln in lines) + "\n"
    with open(path, "w") as f:
        f.write(text)
    print("wrote %s (%d figures)" % (path, len(rows)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="default,trn,trnms,head")
    ap.add_argument("--repo", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="checkout whose mvfnet_amd package is timed")
    ap.add_argument("--clips", default="12,32")
    ap.add_argument("--frames", type=int, default=8)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--first-round", type=int, default=0, help="the round number the first round is labelled with (alternating processes: parent, this tree, parent, ...)")
    ap.add_argument("--json", default=None, help="append every figure's JSON line to this file")
    ap.add_argument("--report", default=None, help="write the text of profiles/trn_head.txt from --json's figures and exit (no GPU)")
    ap.add_argument("--errors", default=None, help="with --report: a tests/test_trn_head_gpu.py -s log whose 'end to end' lines are quoted")
    args = ap.parse_args()
    if args.report:
        return report(args.report, args.json, args.errors)
    configs = args.config.split(",")
    for config in configs:
        if config not in CONFIGS:
            raise SystemExit("trn_head_timing: --config takes %s" % ", ".join(CONFIGS))
    sys.path.insert(0, os.path.abspath(args.repo))
    import numpy as np
    import torch
    import mvfnet_amd
    from mvfnet_amd import synth
    if not torch.cuda.is_available():
        raise SystemExit("trn_head_timing: no GPU")

    def emit(**fig):
        line = json.dumps(fig)
        print(line, flush=True)
        if args.json:
            with open(args.json, "a") as f:
                f.write(line + "\n")

    def model(kind):
        cfg = mvfnet_amd.mvfnet_config(50, args.frames)
        if kind is not None:
            cfg["cls_head"]["consensus_cfg"] = dict(type=kind, num_frames=args.frames)
        m = mvfnet_amd.build_recognizer(cfg, None, dict(average_clips=None))
        sd = m.state_dict()
        vals = synth.synth_state_dict({"r50/" + k: tuple(v.shape) for k, v in sd.items()}, seed=0)
        m.load_state_dict({k: torch.from_numpy(vals["r50/" + k]) for k in sd}, strict=True)
        return m.cuda()

    def windows(fn):
        out = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for i in range(args.steps):
                fn(i)
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t0) / args.steps * 1e3)
        out.sort()
        return out

    def time_step(config, clips, rnd):
        gen = torch.Generator(device="cuda").manual_seed(0)
        batches = []
        for _ in range(2):
            imgs = torch.randn(clips, args.frames, 3, args.size, args.size, device="cuda", generator=gen)
            batches.append((imgs, torch.randint(0, 400, (clips, 1), device="cuda", generator=gen)))
        eng = model(KINDS.get(config)).train().train_engine(dtype=torch.bfloat16)
        np.random.seed(0)
        for i in range(10):
            eng.train_step(*batches[i % 2])
        out = windows(lambda i: eng.train_step(*batches[i % 2]))
        plans = [s["plan"] for s in getattr(eng, "_plans", {}).values()]
        emit(config=config, round=rnd, repo=os.path.abspath(args.repo), clips=clips, frames=args.frames, size=args.size, median_ms=round(out[len(out) // 2], 4),
             min_ms=round(out[0], 4), max_ms=round(out[-1], 4), steps_per_window=args.steps, reps=args.reps,
             plan_ops=[p.n_ops if p is not None else None for p in plans])
        del eng, batches
        torch.cuda.empty_cache()

    def time_head(kind, clips, rnd):
        from mvfnet_amd import _lib as L
        from mvfnet_amd.heads import relation as rel
        T, hw, c, classes, fdim = args.frames, 49, 2048, 400, rel.IMG_FEATURE_DIM
        torch.manual_seed(clips)
        np.random.seed(clips)
        fc = torch.nn.Linear(c, fdim).cuda()
        mod = rel.return_TRN(kind, fdim, T, classes).cuda()
        hidden = mod.num_bottleneck
        table = rel.draw_relation_table(kind, T)
        rows = int(table.shape[0])
        table_d = torch.from_numpy(table).cuda()
        feat = (torch.randn(clips * T, hw, c, device="cuda") + 0.5).to(torch.bfloat16)
        dscores = torch.randn(clips, classes, device="cuda") / clips
        layers = mod.scale_layers()
        params = [p for pair in layers for lin in pair for p in (lin.weight, lin.bias)]
        grads = [torch.empty_like(p) for p in params]
        arr = (L.TrnScale * len(layers))()
        for i in range(len(layers)):
            for j, name in enumerate(("w1", "b1", "w2", "b2")):
                setattr(arr[i], name, params[4 * i + j].data_ptr())
                setattr(arr[i], "d" + name, grads[4 * i + j].data_ptr())
        e = lambda *s: torch.empty(s, device="cuda")  # noqa: E731
        pooled, f, h, scores = e(clips * T, c), e(clips * T, fdim), e(rows, clips, hidden), e(clips, classes)
        hpart = e(L.TRN_KSPLIT_MAX, rows, clips, hidden)
        dfw, dfb, dh, df, dpool, dfeat = e(fdim, c), e(fdim), e(rows, clips, hidden), e(clips * T, fdim), e(clips * T, c), torch.empty_like(feat)
        P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        info, counts = L.TrnLaunchInfo(), []

        def hip(i):
            L.check(L.lib.mvf_trn_head_fwd(P(feat), clips, T, hw, c, P(fc.weight), P(fc.bias), fdim, arr, len(arr), hidden, classes, P(table_d), rows, None, P(pooled),
                                           P(f), P(h), P(hpart), P(scores), L.MVF_BF16, st), "mvf_trn_head_fwd")
            if i == 0:
                L.lib.mvf_trn_head_last_launch(C.byref(info))
                counts.append(info.launches)
            L.check(L.lib.mvf_trn_head_bwd(P(dscores), P(pooled), P(f), P(h), P(fc.weight), arr, len(arr), hidden, classes, P(table_d), rows, None, clips, T, hw, c,
                                           fdim, P(dfw), P(dfb), P(dh), P(df), P(dpool), P(dfeat), L.MVF_BF16, st), "mvf_trn_head_bwd")
            if i == 0:
                L.lib.mvf_trn_head_last_launch(C.byref(info))
                counts.append(info.launches)
        relations = [(int(r[0]), [int(v) for v in r[1:1 + T - int(r[0])]]) for r in table.tolist()]
        seqs = [mod.classifier] if kind == "TRN" else list(mod.fc_fusion_scales)
        x = feat.clone().requires_grad_(True)

        def eager(i):
            for p in [x, fc.weight, fc.bias] + params:
                p.grad = None
            fr = fc(x.float().mean(1)).reshape(clips, T, fdim)
            out = None
            for si, frames in relations:
                act = seqs[si](fr[:, frames, :].reshape(clips, -1))
                out = act if out is None else out + act
            (out * dscores).sum().backward()
        for i in range(3):
            hip(i)
            eager(i)
        torch.cuda.synchronize()
        err = float((scores - torch.stack([seqs[si](fc(feat.float().mean(1)).reshape(clips, T, fdim)[:, fr_, :].reshape(clips, -1)) for si, fr_ in relations]).sum(0)).abs().max()
                    / scores.abs().max())
        a, b = windows(hip), windows(eager)
        emit(config="head", kind=kind, round=rnd, clips=clips, rows=rows, classes=classes, reps=args.reps, steps_per_window=args.steps, hip_ms=round(a[len(a) // 2], 5),
             hip_min_ms=round(a[0], 5), hip_max_ms=round(a[-1], 5), torch_ms=round(b[len(b) // 2], 5), torch_min_ms=round(b[0], 5), torch_max_ms=round(b[-1], 5),
             launches_fwd=counts[0], launches_bwd=counts[1], scores_rel_diff=err)

    for rnd in range(args.first_round, args.first_round + args.rounds):
        for config in configs:
            for clips in (int(c) for c in args.clips.split(",")):
                if config == "head":
                    for kind in ("TRN", "TRNmultiscale"):
                        time_head(kind, clips, rnd)
                else:
                    time_step(config, clips, rnd)


if __name__ == "__main__":
    main()
