#!/usr/bin/env python3
"""bench.py -- MVFNet-R50 8x8 hot path on MI355X.

    python bench.py [--mode train|infer] [--gpus N] [--steps K] [--warmup W] [--dtype f32|bf16] [--clips B] [--full] [--dump-outputs DIR]
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

A plain call sets up, runs W warm-up steps, times K steps and prints one JSON line (`metric`, `value`, `unit`, `higher_is_better`, `dtype`,
`ms_per_step` = milliseconds per timed step, ...).  `--full` adds everything else, after the timed region: the roofline passes, the CPU
baseline with the eager comparators, `other_configs` and, with more than one rank, the replica self-check.  `--dump-outputs DIR` writes what
the last timed step computed as DIR/<name>.npy (see dump_outputs()).

BASELINE.json's metric is "clips/sec (fwd+bwd) MVFNet-R50 8x8 224^2".  One "step" (default --mode train) = one full
training iteration of the reference's hot path over one batch of synthetic clips already resident in HBM:
forward with batch-statistics BatchNorm + MVF + head + cross-entropy, backward, [all-reduce of the flat gradient / world
over RCCL when N > 1], clip_grad_norm_(40), SGD-nesterov update -- 32 clips of 8 x 3 x 224 x 224 per GPU.
Default dtype bf16 = BASELINE.json configs[2] ("batch 32/GPU bf16, DDP train step"): activations and packed weights are
stored in bf16; accumulation, BatchNorm statistics, every parameter gradient, the master weights and the optimizer are
fp32 (what the reference's own fp16 mode keeps in fp32).  `--dtype f32` runs the reference's shipped precision.
`--mode infer` is BASELINE configs[1] (eval-BN forward only, fp32 by default).

Clips are independent units: N GPUs hold N replicas and N disjoint batches (weak scaling); the only collective is the
gradient all-reduce of the training step.  The timed region is bracketed by barrier + synchronize, MAX over ranks.

Extra objects in the JSON line (--full)
  roofline      dominant kernel (implicit-GEMM conv `conv_igemm_kernel`: forward convs + data-gradient convs):
                algorithmic FLOP of its launches in one step / their summed HIP-event durations (instrumented passes on
                the launch stream, outside the timed region) vs the dense MFMA peak of the dtype; `wgrad` sub-object
                for the weight-gradient kernel
  cpu_baseline  the CPU restatement (oracle/net_torch.py, kind "port") of the same step on this box's host cores, bounded
                sample; plus the same restatement run by PyTorch-ROCm eager on this GPU (the ">= 1.5x" comparator)
"""
import argparse
import json
import os
import sys
import time

# (GPU_MAX_HW_QUEUES is deliberately left at ROCm's default of 4: with a torch.distributed process group up, 8 hardware queues
# made the same step 46 % slower -- 34.4 vs 23.6 ms on one MI355X, BENCH_FORCE_DIST=1 -- although it is neutral without one.
# Side streams are picked by measurement instead, mvfnet_amd/streams.py.)

import torch

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, REPO)

PEAK_TFLOPS = {"f32": 157.3, "bf16": 2500.0}     # MI355X_MICROARCH.md: dense MFMA peaks (fp32-in / bf16)
# fp32 convs run on the BF16 matrix cores as six bf16 partial products per fp32 product (conv_tile X3, the default; MVF_POLICY=f32_x3=0 = the fp32
# MFMA): their ceiling in fp32-EQUIVALENT flops is the bf16 peak / 6.  The fp32 weight gradients keep the fp32 MFMA (157.3).
def _policy(name, default):           # MVF_POLICY="name=value,..." (mvfnet_amd/policy.py; parsed here without importing torch)
    for item in os.environ.get("MVF_POLICY", "").replace(";", ",").split(","):
        if item.split("=")[0].strip().lower() == name and "=" in item:
            return int(item.split("=", 1)[1])
    return default


F32_X3 = _policy("f32_x3", 1) != 0
F32_CONV_PEAK = PEAK_TFLOPS["bf16"] / 6.0 if F32_X3 else PEAK_TFLOPS["f32"]
# the fp32 weight gradients likewise ([r4] wgrad_x3_kernel; MVF_POLICY=wgrad_x3=0 = the fp32 MFMA kernel)
F32_WGRAD_PEAK = PEAK_TFLOPS["bf16"] / 6.0 if (F32_X3 and _policy("wgrad_x3", 1) != 0) else PEAK_TFLOPS["f32"]
VIDEO = False
T_FRAMES, SIZE = 8, 224     # overwritten from --frames / --mode video in main()


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=["train", "infer", "video"], default="train",
                    help="train = fwd+bwd+update (default, configs[2]); infer = eval forward (configs[1]); video = configs[4]: "
                         "10 clips x 3 crops of 256^2 per video, fcn_testing head, average_clips='prob', one video per step")
    ap.add_argument("--frames", type=int, default=8, help="frames per clip (T); 16 with --depth 101 --clips 16 is configs[3]")
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10, help="timed steps (>= 1)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps, also run the roofline passes, the CPU baseline + eager comparators, other_configs and (multi-rank) "
                         "the replica self-check; the --no-* switches below still drop parts of it")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed as DIR/<name>.npy (float32, < 64 MB in all; rank 0)")
    ap.add_argument("--dtype", choices=["f32", "bf16"], default=None,
                    help="activation / packed-weight storage (fp32 accumulate, statistics, gradients, master weights). Default: bf16 for "
                         "--mode train (BASELINE.json configs[2]), f32 for --mode infer (configs[1])")
    ap.add_argument("--clips", type=int, default=32, help="clips per GPU per step")
    ap.add_argument("--depth", type=int, default=50)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-seconds", type=float, default=30.0)
    ap.add_argument("--no-overlap", action="store_true",
                    help="train mode: keep the weight-gradient GEMMs on the launch stream (profiling: every kernel runs alone, as in "
                         "the roofline pass)")
    ap.add_argument("--no-eager-compare", action="store_true",
                    help="skip the PyTorch-ROCm eager comparators (tools/eager_compare.py: the same train step under eager fp32 and under "
                         "autocast(bf16)+channels_last on this GPU, cudnn.benchmark=False; ~70 s each on a fresh box, bounded by --eager-seconds)")
    ap.add_argument("--eager-seconds", type=float, default=150.0, help="wall-clock bound per eager comparator run")
    ap.add_argument("--streams", type=int, default=2, help="infer: independent clip-group launch chains (HIP streams)")
    ap.add_argument("--per-layer", action="store_true", help="print a per-launch timing table to stderr (from the roofline passes of --full)")
    ap.add_argument("--host-input", action="store_true",
                    help="train mode: every step's batch starts in (pinned) HOST memory and is uploaded by runner.DevicePrefetcher one batch ahead "
                         "on a copy stream, as a data-loader-fed run does (reference: MMDistributedDataParallel.scatter, parallel/distributed.py:40-62); "
                         "the JSON line then carries `host_input` with the H2D bytes per step.  `value` of the default run stays the HBM-resident one")
    ap.add_argument("--no-other-configs", action="store_true",
                    help="--full 1-GPU train run at the headline shape only: skip the short runs of BASELINE.json's other configurations (configs[1] fp32 inference, "
                         "configs[3] R101 16x4 bf16 train, configs[4] 30-clip video) that are appended as `other_configs` AFTER the timed region")
    ap.add_argument("--other-seconds", type=float, default=150.0, help="wall-clock bound for each of those runs")
    ap.add_argument("--cpu-child", type=int, default=0, help=argparse.SUPPRESS)      # cpu_baseline's bounded os.cpu_count()-thread measurement (own process)
    return ap.parse_args()


def build_model(depth, dtype, train):
    import mvfnet_amd
    from mvfnet_amd import synth
    m = mvfnet_amd.build_recognizer(mvfnet_amd.mvfnet_config(depth, T_FRAMES, fcn_testing=VIDEO), None,
                                    dict(average_clips="prob" if VIDEO else None))
    sd = m.state_dict()
    pre = "r%d/" % depth
    vals = synth.synth_state_dict({pre + k: tuple(v.shape) for k, v in sd.items()})
    m.load_state_dict({k: torch.from_numpy(vals[pre + k]) for k in sd}, strict=True)
    m.backbone.engine_dtype = torch.float32 if dtype == "f32" else torch.bfloat16
    m = m.cuda()
    return m.train() if train else m.eval()


class _Timer(object):
    """HIP-event bracket around every call of a bound method; events go on torch's current stream = the launch stream."""

    def __init__(self):
        self.rec = []

    def wrap(self, cls, name, describe):
        orig = getattr(cls, name)
        timer = self

        def timed(obj, *a, **kw):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = orig(obj, *a, **kw)
            e1.record()
            timer.rec.append((e0, e1) + describe(obj, out, *a, **kw))
            return out

        setattr(cls, name, timed)
        return lambda: setattr(cls, name, orig)


def event_pair_overhead_ms(n=64):
    """What an EMPTY HIP-event bracket reads on the launch stream (record, record, elapsed): the two event packets themselves
    cost a few microseconds of queue time, which matters against ~100 us bf16 launches.  Median of n pairs."""
    import torch
    torch.cuda.synchronize()
    pairs = []
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        e1.record()
        pairs.append((e0, e1))
    torch.cuda.synchronize()
    v = sorted(a.elapsed_time(b) for a, b in pairs)
    return v[len(v) // 2]


def _summ(rec, per_layer, tag, peak_tf=2500.0):
    ms = sum(r[0].elapsed_time(r[1]) for r in rec)
    fl = sum(r[2] for r in rec)
    by = sum(r[4] for r in rec)
    if per_layer:
        agg = {}
        for r in rec:
            a = agg.setdefault(r[3], [0, 0.0, 0.0, 0.0])
            a[0] += 1
            a[1] += r[0].elapsed_time(r[1])
            a[2] += r[2]
            a[3] += r[4]
        # "bound" = the larger of bytes / 6.3 TB/s (measured HBM ceiling) and flops / the dtype's dense MFMA peak; "over" = time above it
        rows = [(k, cnt, t, f, b, max(b / 6.3e9, f / (peak_tf * 1e9))) for k, (cnt, t, f, b) in agg.items()]
        for k, cnt, t, f, b, lo in sorted(rows, key=lambda r: -(r[2] - r[5]))[:48]:
            print("  %-6s %-40s x%-2d %7.3f ms %6.1f TF/s %5.2f TB/s  bound %6.3f  over %6.3f" % (tag, k, cnt, t, f / t / 1e9, b / t / 1e9, lo, t - lo),
                  file=sys.stderr)
    return ms, fl, by, len(rec)


def roofline_infer(model, imgs, dtype, per_layer):
    from mvfnet_amd import engine as E
    t = _Timer()
    esz = 4 if dtype == "f32" else 2

    def desc(self, ret, x, n, h, w, c_total, **kw):
        y, ho, wo = ret
        stem = self.kw == 1 and self.cin == 32 and self.kh == 7
        k_alg = 147 if stem else self.kh * self.kw * self.cin
        st = kw.get("stride") or self.stride
        in_px = n * ho * wo if (self.kh == 1 and self.kw == 1 and st > 1) else n * h * w
        nbytes = esz * (in_px * (c_total if stem else self.cin) + n * ho * wo * self.cout * (2 if kw.get("residual") is not None else 1) + self.wp.numel())
        return (2.0 * n * ho * wo * self.cout * k_alg, "M%d N%d K%d k%dx%d s%d" % (n * ho * wo, self.cout, k_alg, self.kh, self.kw, st), nbytes)

    undo = t.wrap(E._Conv, "run", desc)
    streams = model.backbone.engine().streams
    model.backbone.engine().streams = 1
    try:
        tot = [0.0, 0.0, 0.0, 0]
        reps = 3
        for i in range(reps):
            del t.rec[:]
            model(imgs, None, return_loss=False, return_numpy=False)
            torch.cuda.synchronize()
            r = _summ(t.rec, per_layer and i == reps - 1, "conv", F32_CONV_PEAK if dtype == "f32" else PEAK_TFLOPS[dtype])
            tot = [a + b for a, b in zip(tot, r)]
    finally:
        undo()
        model.backbone.engine().streams = streams
    return _roof(tot, reps, dtype, event_pair_overhead_ms(), dtype + "_infer", pmc_group="conv", peak_tf=(F32_CONV_PEAK if dtype == "f32" else None), kernel="conv_igemm_* (conv_tile instantiations, csrc/conv_nhwc.hip) + conv3x3_c64 / stem_direct (the direct kernels of layer1's 3x3 and the stem)")


def roofline_train(eng, imgs, labels, dtype, per_layer, ms_step):
    """Instrumented passes (weight gradients on the launch stream, every launch alone): HIP-event brackets around every launch of
    the four kernel groups of the step -- implicit-GEMM convs (forward + data gradients), weight gradients, BatchNorm streaming
    kernels, MVF stencils -- with each launch's ALGORITHMIC bytes / flops from its shapes."""
    from mvfnet_amd import train_engine as TE
    tc, tw, tb, tm, tf = _Timer(), _Timer(), _Timer(), _Timer(), _Timer()
    esz = 4 if dtype == "f32" else 2

    def dfwd(self, out, d, x, x2, z, ws, part, shift):
        n, h, w, ho, wo = d.n, d.h, d.w, d.ho, d.wo
        k_alg = 147 if self.stem else self.kh * self.kw * self.cin
        in_px = n * ho * wo if (self.kh == 1 and self.stride > 1) else n * h * w
        nbytes = esz * (in_px * (4 if self.stem else self.cin) + (n * ho * wo * self.cout if z is not None else 0) + self.w.numel())
        return (2.0 * n * ho * wo * self.cout * k_alg, "fwd%s M%d N%d K%d s%d" % ("   " if z is not None else "(s)", n * ho * wo, self.cout, k_alg, self.stride), nbytes)

    def dfap(self, out, d, x, bn, residual, rbn, o, bits, ws):      # conv3 again + bn3 apply + residual + ReLU + sign bits (no z3 read)
        m = d.n * d.ho * d.wo
        nbytes = esz * (m * self.cin + 2 * m * self.cout + self.w.numel()) + m * self.cout // 4
        return (2.0 * m * self.cout * self.cin, "fwd+bn M%d N%d K%d s%d" % (m, self.cout, self.cin, self.stride), nbytes)

    def dbws(self, out, d, a_in, g, bits, bn, part, ws):            # conv3 again + bn3 backward sums (reads a2, g, bits; stores nothing)
        m = d.n * d.ho * d.wo
        return (2.0 * m * self.cout * self.cin, "bwd-sums M%d N%d K%d" % (m, self.cout, self.cin), esz * (m * self.cin + m * self.cout + self.w.numel()) + m * self.cout // 4)

    def dbwa(self, out, d, a_in, g, bits, bn, dz, ws):              # conv3 again + bn3 backward apply (reads a2, g, bits; writes dz3)
        m = d.n * d.ho * d.wo
        return (2.0 * m * self.cout * self.cin, "bwd-apply M%d N%d K%d" % (m, self.cout, self.cin), esz * (m * self.cin + 2 * m * self.cout + self.w.numel()) + m * self.cout // 4)

    def dbwf(self, out, m, a_in, g, bits, bn, bn_in, z_in, dx, spart, ns, slabs, a_pitch=None):      # [r4] conv again + BatchNorm backward apply + data gradient (+ bn_in sums) + weight gradient, dz on chip
        nbytes = esz * ((3 if bn_in is not None else 2) * m * self.cin + m * self.cout + self.w.numel()) + m * self.cout // 4 + 4 * self.w.numel()      # a2, (z2,) dx, g, bits, W, dW
        return (3 * 2.0 * m * self.cout * self.cin, "bwd-fused M%d N%d K%d (apply + dgrad + wgrad)" % (m, self.cout, self.cin), nbytes)

    def dbsp(self, out, a2, x, x_pitch, g, bits, m, eng_):      # [r4] bn3's and bn_d's backward sums of a z3-free downsample block: both convs again, g and the bits once
        c3 = self.c3
        nbytes = esz * (2 * m * c3.cin + m * c3.cout + 2 * c3.w.numel()) + m * c3.cout // 4
        return (2 * 2.0 * m * c3.cout * c3.cin, "bwd-sums(pair) M%d N%d K%d" % (m, c3.cout, c3.cin), nbytes)

    def dbs1(self, out, m, a_in, a_pitch, g, bits, bn, part, ns):      # [r4] conv3 again + bn3 backward sums on the one-branch form of pw_sums_pair
        return (2.0 * m * self.cout * self.cin, "bwd-sums M%d N%d K%d" % (m, self.cout, self.cin), esz * (m * self.cin + m * self.cout + self.w.numel()) + m * self.cout // 4)

    def ddgr(self, out, dz, n, ho, wo, h, w, residual=None, res_c0=0, res_bits=None, out_gate=None, gsum=None):
        fl = 2.0 * n * ho * wo * self.cout * self.kh * self.kw * self.cin          # algorithmic = the forward conv's MACs
        nbytes = esz * (n * ho * wo * self.cout + n * h * w * self.cin * (2 if residual is not None else 1) + self.w.numel())
        return (fl, "dgrad M%d N%d K%d s%d" % (n * h * w, self.cin, self.kh * self.kw * self.cout, self.stride), nbytes)

    def ddgb(self, out, d, dz, dx, z, bn, part, ws):          # stride-1 data gradient + BN-backward sums (reads z as well)
        n, ho, wo, h, w = d.n, d.h, d.w, d.ho, d.wo
        fl = 2.0 * n * ho * wo * self.cout * self.kh * self.kw * self.cin
        nbytes = esz * (n * ho * wo * self.cout + n * h * w * self.cin * 2 + self.w.numel())
        return (fl, "dgrad M%d N%d K%d s%d +bn" % (n * h * w, self.cin, self.kh * self.kw * self.cout, self.stride), nbytes)

    def ddzf(self, out, d, a_in, gm, bd, bias, dx, z_in, bn_in, part, ws):      # [r5] conv3's data gradient + bn2 sums taken on [gm | a2] (no dz3 tensor): algorithmic work = the data gradient's
        m, c, k = d.n * d.h * d.w, self.cout, self.cin
        nbytes = esz * (m * c + 3 * m * k + self.w.numel())          # gm, a2, z2, da2, W
        return (2.0 * m * c * k, "dgrad M%d N%d K%d s1 +bn (no dz3)" % (m, k, c), nbytes)

    def dwgr(self, out, dz, x, n, h, w, ho, wo, eng_, x_pitch=None, x2=None, split_c=0, on_main=False):
        k_alg = 147 if self.stem else self.kh * self.kw * self.cin
        nbytes = esz * (n * ho * wo * self.cout + n * h * w * (4 if self.stem else self.cin)) + 4 * self.w.numel()
        return (2.0 * n * ho * wo * self.cout * k_alg, "wgrad M%d N%d K%d s%d" % (n * ho * wo, self.cout, k_alg, self.stride), nbytes)

    def dwgq(self, out, d, gm, a_in, ws, wgs, slabs=False):      # [r5] conv3's weight-gradient GEMM Q = gm^T a2 taken on the launch stream (it also yields bn3's dgamma: dzfree_q)
        m, c, k = d.n * d.h * d.w, self.cout, self.cin
        return (2.0 * m * c * k, "wgrad M%d N%d K%d s1 (launch stream)" % (m, c, k), esz * m * (c + k) + 4 * self.w.numel())

    def dwgg(self, out, d, a_in, gram, ws, wgs):      # [r5] the Gram matrix a2^T a2 of conv3's input on the launch stream: bn3's batch statistics without a conv3 pass (gram_stats)
        m, k = d.n * d.h * d.w, self.cin
        return (2.0 * m * k * k, "gram  M%d K%d (launch stream, bn3 statistics)" % (m, k), esz * m * k + 4 * k * k)

    # BatchNorm streaming kernels: tensors read + written (the sign-bit byte per 4 channels where it is used)
    def dbap(self, out, z, m, act, residual=None, rbn=None, bits=False):
        nb = esz * m * self.c * (3 if residual is not None else 2) + (m * self.c // 4 if bits else 0)
        return (0.0, "bn apply%s M%d C%d" % ("+res" if residual is not None else "", m, self.c), nb)

    def dbre(self, out, g, g_pitch, z, m, eng_, mask_mode, ymask, gm_out):
        nb = esz * m * self.c * 2 + (m * self.c // 4 if mask_mode == 4 else 0)
        return (0.0, "bn bwd reduce<%d> M%d C%d" % (mask_mode, m, self.c), nb)

    def dbab(self, out, g, g_pitch, z, m, eng_, mask_mode, ymask, gm_out):
        nb = esz * m * self.c * 3 + (m * self.c // 4 if mask_mode == 4 else 0)
        return (0.0, "bn bwd apply<%d> M%d C%d" % (mask_mode, m, self.c), nb)

    def dbpr(self, out, b, g, g_pitch, za, zb, m, eng_, bits):          # bn3 + downsample BN -- reduce: g, z3, zd, bits; apply: the same + dz3, dzd
        return (0.0, "bn bwd pair M%d C%d" % (m, self.c), esz * m * self.c * 8 + 2 * (m * self.c // 4))

    # [r4] BatchNorm backward apply + the pointwise conv's weight gradient in one pass: g, z, dz (+ bits) + the conv input + dW
    def dbaw(self, out, g, g_pitch, z, m, eng_, mask_mode, ymask, conv, x, x_pitch):
        nb = esz * m * self.c * 3 + (m * self.c // 4 if mask_mode == 4 else 0) + esz * m * conv.cin + 4 * conv.w.numel()
        return (2.0 * m * self.c * conv.cin, "bn bwd apply<%d> + wgrad M%d C%d K%d" % (mask_mode, m, self.c, conv.cin), nb)

    def dbpw(self, out, b, g, g_pitch, za, zb, m, eng_, bits, conv_a, xa, xa_pitch, conv_b, xb, xb_pitch):
        nx = 2 if xb is not None else 1
        nb = esz * m * self.c * 8 + 2 * (m * self.c // 4) + nx * (esz * m * conv_a.cin + 4 * conv_a.w.numel())
        return (2.0 * nx * m * self.c * conv_a.cin, "bn bwd pair + %d wgrad M%d C%d K%d" % (nx, m, self.c, conv_a.cin), nb)

    def dmvf(self, out, d, src, src_c, dst, dst_c, flip, addend, addend_c, addend_bits, out_gate=None, gsum=None):
        m = d.nt * d.h * d.w
        nb = esz * m * d.cs * (3 if addend is not None else 2)          # slice read + slice write (+ the gated skip-connection slice)
        taps = 3 * bin(d.mode).count("1")
        return (2.0 * m * d.cs * taps, "mvf stencil%s M%d Cs%d" % ("^T" if flip else "", m, d.cs), nb)

    def dmvs(self, out, d, x, c, y, part):          # [r5] the forward stencil that also takes the BatchNorm statistics
        m = d.nt * d.h * d.w
        return (2.0 * m * d.cs * 3 * bin(d.mode).count("1"), "mvf stencil+stats M%d Cs%d" % (m, d.cs), esz * m * d.cs * 2)

    undo = [tc.wrap(TE._TConv, "launch_fwd", dfwd), tm.wrap(TE._TMvf, "launch_stencil_stats", dmvs), tc.wrap(TE._TConv, "launch_fwd_apply", dfap), tc.wrap(TE._TConv, "launch_bwd_sums", dbws), tc.wrap(TE._TConv, "launch_bwd_apply", dbwa),
            tc.wrap(TE._TConv, "dgrad", ddgr), tc.wrap(TE._TConv, "launch_dgrad_bnsums", ddgb), tc.wrap(TE._TConv, "launch_dzfree_dgrad", ddzf), tc.wrap(TE._TConv, "launch_bwd_fused", dbwf), tc.wrap(TE._TBlock, "launch_sums_pair", dbsp), tc.wrap(TE._TConv, "launch_bwd_sums1", dbs1),
            tw.wrap(TE._TConv, "wgrad", dwgr), tw.wrap(TE._TConv, "launch_q", dwgq), tw.wrap(TE._TConv, "launch_gram", dwgg), tb.wrap(TE._BN, "apply", dbap), tb.wrap(TE._BN, "_reduce", dbre), tb.wrap(TE._BN, "_apply_bwd", dbab),
            tb.wrap(TE._BN, "backward_pair", dbpr),
            tm.wrap(TE._TMvf, "launch_stencil", dmvf), tf.wrap(TE._BN, "_apply_bwd_wgrad", dbaw), tf.wrap(TE._BN, "backward_pair_wgrad", dbpw)]
    overlap = eng.overlap_wgrad
    eng.overlap_wgrad = False          # time every kernel alone on the launch stream (the timed steps overlap wgrad on a side stream)
    timers = (("igemm", tc), ("wgrad", tw), ("bn", tb), ("mvf", tm), ("bnwg", tf))
    try:
        tot = {k: [0.0, 0.0, 0.0, 0] for k, _ in timers}
        tot["igemm_required"], tot["igemm_recompute"] = [0.0, 0.0, 0.0, 0], [0.0, 0.0, 0.0, 0]
        reps = 2
        for i in range(reps):
            for _, t in timers:
                del t.rec[:]
            eng.forward(imgs, labels)
            eng.backward()
            torch.cuda.synchronize()
            for k, t in timers:
                tot[k] = [a + b for a, b in zip(tot[k], _summ(t.rec, per_layer and i == reps - 1, k, (F32_CONV_PEAK if k == "igemm" else F32_WGRAD_PEAK if k == "wgrad" else PEAK_TFLOPS[dtype]) if dtype == "f32" else PEAK_TFLOPS[dtype]))]
            rec = [r_ for r_ in tc.rec if r_[3].startswith(RECOMPUTE_TAGS)]
            req = [r_ for r_ in tc.rec if not r_[3].startswith(RECOMPUTE_TAGS)]
            tot["igemm_recompute"] = [a + b for a, b in zip(tot["igemm_recompute"], _summ(rec, False, "", PEAK_TFLOPS[dtype]))]
            tot["igemm_required"] = [a + b for a, b in zip(tot["igemm_required"], _summ(req, False, "", PEAK_TFLOPS[dtype]))]
    finally:
        for u in undo:
            u()
        eng.overlap_wgrad = overlap
    ovh = event_pair_overhead_ms()
    key = dtype + "_train"
    conv_kernels = ("conv_igemm_* (conv_tile instantiations: lowk / glds / p4 / streamk, csrc/conv_nhwc.hip) + conv3x3_c64 / stem_direct / pw_sums / pw_bwd_fused (the direct "
                    "kernels of layer1's 3x3 + its data gradient, of the stem, the sum-only passes of layer1's conv3 and its one-pass backward)")
    cpeak = F32_CONV_PEAK if dtype == "f32" else None
    fam = _roof(tot["igemm"], reps, dtype, ovh, key, conv_kernels, "conv", peak_tf=cpeak)
    # [r5] HEADLINE = the REQUIRED launches (one forward + one data gradient per conv): the recompute passes' bytes are not algorithmic work of the
    # network, they replace BatchNorm passes (reported beside it as `recompute`, the whole kernel family incl. them as `family`).  The counter traffic
    # cannot be split by launch kind (same kernels), so `traffic*` stay the FAMILY's figures, labelled so.
    r = _roof(tot["igemm_required"], reps, dtype, ovh, kernel=conv_kernels, peak_tf=cpeak)
    for k_ in ("traffic", "traffic_per_step", "traffic_source"):
        r[k_] = fam[k_]
    r["traffic_over_algorithmic"] = fam["traffic_over_algorithmic"]
    r["traffic_scope"] = "whole conv family incl. the recompute passes (counters cannot tell them apart); the ratio is against the family's algorithmic bytes"
    r["family"] = fam
    # the family with and without the RECOMPUTE passes (conv3 run again instead of re-reading z3: bn3's apply, backward sums, backward
    # apply as epilogues of a second / third / fourth pass).  Their bytes / flops are booked as algorithmic above because they replace
    # BatchNorm passes that moved MORE bytes; `required` is the like-for-like family (one forward + one data gradient per conv).
    r["required"] = "= this object (the headline figures)"
    r["recompute"] = _roof(tot["igemm_recompute"], reps, dtype, ovh, kernel="conv3 second passes: fwd+bn (bn3 apply + residual + ReLU), bwd-sums, bwd-apply (z3-free blocks)", peak_tf=cpeak)
    groups = {"wgrad": _roof(tot["wgrad"], reps, dtype, ovh, key, "wgrad_*_kernel + wgrad_reduce_kernel (csrc/wgrad_nhwc.hip) [+ the fused BatchNorm-backward-apply + weight-gradient kernels, csrc/bnbwd_wgrad.hip, where the step uses them]", "wgrad",
                              peak_tf=(F32_WGRAD_PEAK if dtype == "f32" else None)),
              "bn": _roof(tot["bn"], reps, dtype, ovh, key, "bn_apply / bn_bwd_reduce / bn_bwd_apply kernels (csrc/train_ops.hip)", "bn"),
              "mvf": _roof(tot["mvf"], reps, dtype, ovh, key, "mvf_nhwc_apply (stencil and transposed stencil, csrc/mvf_nhwc.hip)", "mvf")}
    if tot["bnwg"][3]:
        groups["bn_wgrad"] = _roof(tot["bnwg"], reps, dtype, ovh, key, "bnbwd_wgrad_kernel (csrc/bnbwd_wgrad.hip): BatchNorm backward apply (or the paired form incl. its reduce pass) "
                                   "+ the pointwise conv's weight gradient in one pass; the slab reduces run on the side stream", "bn_wgrad")
    mv = groups["mvf"]
    # [r5] the MVF slice (12.8 MB per layer3 launch) never leaves L2 / the 256 MB memory-side cache between its producer and this kernel
    # (tools/kbench.py mvf: a plain copy of the slice takes 3.8 us back to back), so an HBM-priced fraction says nothing about the kernel: it is a
    # latency-bound small launch (~5 us of launch + one dependent round trip of 42 loads per thread).  Priced as launches x latency instead.
    mv["bound"] = "latency"
    mv["frac_note"] = ("hbm_frac is NOT a roofline fraction here: the slice is cache-resident (L2 / MALL), the launch is latency-bound; "
                       "latency_floor_us = launch (~5 us) + one dependent memory round trip (~4 us) per launch")
    mv["latency_floor_us"] = 9.0
    mv["frac"] = round(9.0 / max(mv["avg_launch_us"], 1e-6), 4)
    mv["achieved"], mv["peak"], mv["unit"] = mv["avg_launch_us"], 9.0, "us per launch (lower is better; frac = floor / achieved)"
    for k, g in groups.items():
        r[k] = g
    if "bn_wgrad" in groups:
        # the paired fused launches run their reduce pass (bn_bwd_reduce2_kernel) inside the bracket, so their algorithmic bytes sit under bn_wgrad
        # while the counters file that kernel under bn: the two groups together are the comparable pair
        tb, tf_ = groups["bn"].get("traffic_per_step"), groups["bn_wgrad"].get("traffic_per_step")
        ab = groups["bn"]["alg_bytes_per_step"] + groups["bn_wgrad"]["alg_bytes_per_step"]
        r["bn_and_bn_wgrad"] = {"alg_bytes_per_step": ab, "traffic_per_step": (tb + tf_) if (tb and tf_) else None,
                                "traffic_over_algorithmic": round((tb + tf_) / ab, 3) if (tb and tf_ and ab) else None,
                                "ms_per_step": round(groups["bn"]["ms_per_step"] + groups["bn_wgrad"]["ms_per_step"], 3)}
    # whole step against the fully fused floor: every conv input / output read / written exactly once, forward + two backward GEMMs
    from mvfnet_amd.arch import fused_activation_elems_per_image
    clips, t = imgs.shape[0], imgs.shape[1]
    floor = 3.0 * fused_activation_elems_per_image(eng_depth(eng), imgs.shape[-1]) * t * clips * esz
    moved = sum(tot[k][2] for k, _ in timers) / reps
    counter, csrc = _pmc_traffic(key, "step_total")
    r["step"] = {"ms_per_step": round(ms_step, 3), "fused_floor_bytes": int(floor), "fused_floor_ms_at_peak": round(floor / PEAK_HBM_GBS / 1e6, 3),
                 "step_hbm_frac": round(floor / (ms_step * 1e-3) / 1e9 / PEAK_HBM_GBS, 4),
                 "alg_bytes_of_timed_groups": int(moved), "alg_bytes_frac_of_peak": round(moved / (ms_step * 1e-3) / 1e9 / PEAK_HBM_GBS, 4),
                 "counter_bytes": counter, "counter_bytes_over_fused_floor": (round(counter / floor, 3) if counter else None),
                 "counter_hbm_frac": (round(counter / (ms_step * 1e-3) / 1e9 / PEAK_HBM_GBS, 4) if counter else None),
                 "counter_source": ("STATIC, not measured in this run: " + csrc) if (counter and csrc) else None,
                 "note": "fused_floor = 3 x (conv-in + conv-out elements) x esz x frames (SURVEY 8d: 348 MB bf16 per R50 8-frame clip and pass); "
                         "alg_bytes_of_timed_groups = what the un-fused launches of the four groups move by their shapes"}
    return r


def eng_depth(eng):
    return eng.model.backbone.depth


def pmc_key(dtype, mode, depth, frames, size, clips, video=False):
    """Key of this run's workload in profiles/pmc_traffic_per_step.json: "<dtype>_<train|infer>" for the headline shapes (R50, 8 x 224^2 frames, 32 clips),
    suffixed "_r<depth>_t<frames>_s<size>_c<clips>" for every other configuration (C4: bf16_train_r101_t16_s224_c16, C5: f32_infer_r50_t8_s256_c30)."""
    base = "%s_%s" % (dtype, "train" if mode == "train" else "infer")
    if depth == 50 and frames == 8 and size == 224 and clips == 32 and not video:
        return base
    return "%s_r%d_t%d_s%d_c%d" % (base, depth, frames, size, clips)


PMC_KEY = None            # main(): this run's key (above)
RECOMPUTE_TAGS = ("fwd+bn", "bwd-sums", "bwd-apply")     # launch tags (roofline_train) of the conv3 passes that recompute z3
PMC_MATCHES_RUN = True    # the counters are static, per step of the workload named by the key: a key that is not in the file prints traffic: null
PEAK_HBM_GBS = 8000.0     # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec (6.3 TB/s measured ceiling)


def _pmc_traffic(pmc_key, group):
    """HBM bytes PER STEP of a kernel group from the PMC counters (profiles/pmc_traffic_per_step.json, written by tools/derive_traffic.py
    from separate --pmc FETCH_SIZE / WRITE_SIZE passes with the gfx950 x2 FETCH correction).  STATIC: collected once per round on the
    round's final kernels, not in this run."""
    pmc = os.path.join(REPO, "profiles", "pmc_traffic_per_step.json")
    if not (pmc_key and os.path.exists(pmc) and PMC_MATCHES_RUN):
        return None, None
    try:
        d = json.load(open(pmc)).get(PMC_KEY or pmc_key) or {}
        return d.get("bytes_per_step", {}).get(group), d.get("source")
    except Exception:
        return None, None


def _roof(tot, reps, dtype, event_overhead_ms=0.0, pmc_key=None, kernel=None, pmc_group=None, peak_tf=None):
    """One kernel group's roofline object.  Time = the GROSS sum of the HIP-event brackets (no overhead subtraction: rocprofv3's kernel
    durations agree with the gross figure, profiles/README.md); `event_pair_overhead_us` is printed for information only.
    fp32: the conv GEMMs are MFMA-bound (94 FLOP/B fused vs ~20 machine balance).  bf16: the same network is HBM-bound even when
    perfectly fused (188 FLOP/B vs ~310), so `frac` is algorithmic bytes/s over the HBM peak; both fractions
    are always printed (`hbm_frac`, `mfma_frac`).  `traffic` (counter HBM bytes) is per LAUNCH like `alg_bytes_per_launch`;
    `traffic_per_step` / `alg_bytes_per_step` are the same two figures per step and `traffic_over_algorithmic` their ratio."""
    ms, fl, by, n = tot
    ms = max(ms, 1e-6)
    n = max(n, 1)
    tflops = fl / (ms * 1e-3) / 1e12
    gbs = by / (ms * 1e-3) / 1e9
    peak = peak_tf or PEAK_TFLOPS[dtype]
    per_step, source = _pmc_traffic(pmc_key, pmc_group)
    launches = max(n // reps, 1)
    alg_step = by / reps
    common = {"kernel": kernel, "traffic": (round(per_step / launches) if per_step else None),
              "traffic_per_step": per_step, "alg_bytes_per_step": round(alg_step),
              "traffic_over_algorithmic": (round(per_step / alg_step, 3) if (per_step and alg_step) else None),
              "traffic_source": ("STATIC, not measured in this run: " + source) if (per_step and source) else None,
              "alg_bytes_per_launch": round(by / n), "launches_per_step": n // reps, "avg_launch_us": round(ms * 1e3 / n, 2),
              "event_pair_overhead_us": round(event_overhead_ms * 1e3, 2), "flop_per_launch": round(fl / n),
              "ms_per_step": round(ms / reps, 3), "tflops": round(tflops, 2), "mfma_frac": round(tflops / peak, 4),
              "hbm_gbs": round(gbs, 1), "hbm_frac": round(gbs / PEAK_HBM_GBS, 4)}
    if dtype == "bf16" or fl == 0.0:
        common.update({"bound": "hbm", "achieved": round(gbs, 1), "peak": PEAK_HBM_GBS, "unit": "GB/s", "frac": round(gbs / PEAK_HBM_GBS, 4)})
    else:
        common.update({"bound": "mfma", "achieved": round(tflops, 2), "peak": round(peak, 1), "unit": "TFLOP/s", "frac": round(tflops / peak, 4)})
        if peak_tf and abs(peak_tf - PEAK_TFLOPS["f32"]) > 1.0:
            common["peak_note"] = ("fp32-equivalent flops on the bf16 matrix cores: six bf16 partial products per fp32 product (exact three-term split), "
                                   "peak = 2500 / 6 TF/s; MVF_POLICY=f32_x3=0 runs the fp32 MFMA (157.3)")
    return common


_T_START = time.time()
WALL_BUDGET = 420.0        # [r6] seconds: the default call's optional parts (fp32 eager comparator, other_configs) are dropped, labelled, when a slow host has used it up


def _elapsed():
    return time.time() - _T_START


def usable_cpus():
    """(CPUs this process may actually use, why): os.cpu_count() capped by the affinity mask and by the container's CFS quota (cgroup v2 cpu.max / v1
    cpu.cfs_quota_us).  On the gpurun boxes os.cpu_count() = 256 while cpu.max = "1600000 100000": 16 CPUs' worth of time -- 256 runnable oneDNN threads on that
    quota are throttled into minutes per step, which is what `all_hw_threads` used to time out on."""
    n = os.cpu_count() or 1
    why = "os.cpu_count()"
    try:
        a = len(os.sched_getaffinity(0))
        if a < n:
            n, why = a, "affinity mask"
    except (AttributeError, OSError):
        pass
    quota = None
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if q != "max":
            quota = float(q) / float(per)
    except (OSError, ValueError):
        try:
            q = float(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
            per = float(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
            if q > 0:
                quota = q / per
        except (OSError, ValueError):
            pass
    if quota is not None and quota < n:
        n, why = max(1, int(quota)), "cgroup CPU quota (%.4g CPUs)" % quota
    return n, why


def cpu_baseline(depth, seconds, mode, gpu_clips, eager_compare=None):
    """The CPU restatement of the same step (oracle/net_torch.py) on the host cores, bounded sample; `eager_compare` = the results
    of eager_comparators() (the same restatement executed by PyTorch-ROCm eager on this GPU), attached to the object."""
    from mvfnet_amd import synth
    from mvfnet_amd.arch import state_dict_shapes
    from oracle import net_torch
    cores = os.cpu_count()
    shp = state_dict_shapes(depth)
    pre = "r%d/" % depth
    vals = synth.synth_state_dict({pre + k: v for k, v in shp.items()})
    train = mode == "train"

    def make_sd(dev):
        sd = {}
        for k in shp:
            t = torch.from_numpy(vals[pre + k]).to(dev)
            if train and t.dtype == torch.float32 and "running" not in k:
                t.requires_grad_(True)
            sd[k] = t
        return sd

    def one_step(sd, imgs, labels, mom):
        if not train:
            with torch.no_grad():
                return net_torch.forward_test(imgs, sd, depth, T_FRAMES, None)
        params = {k: v for k, v in sd.items() if v.requires_grad}
        for p in params.values():
            p.grad = None
        nb = {}
        loss = net_torch.forward_train(imgs, labels, sd, depth, new_buffers=nb, dropout_ratio=0.5)
        loss.backward()
        with torch.no_grad():
            net_torch.sgd_nesterov_step(params, {k: v.grad for k, v in params.items()}, mom)
            for k, v in nb.items():
                sd[k] = v
        return loss

    def cpu_model():
        try:
            for line in open("/proc/cpuinfo"):
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
        except Exception:
            pass
        return "unknown"

    def median_rate(fn, clips_, budget):
        """median of 5 after 2 warm-ups (fewer when the wall-clock budget runs out); -> (clips/s, timed runs)."""
        t_start = time.perf_counter()
        for _ in range(2):
            fn()
            if time.perf_counter() - t_start > budget:
                break
        ts = []
        while len(ts) < 5 and (len(ts) < 3 or time.perf_counter() - t_start < budget):
            t0 = time.perf_counter()
            fn()
            ts.append(time.perf_counter() - t0)
        ts.sort()
        return clips_ / ts[len(ts) // 2], len(ts)

    # C1 exact (BASELINE configs[0]: R50 4x16, 2 clips of 224^2, forward), the C2 shape at N = 2 (R50 8x8 forward), and the
    # metric's own step (C3 shape at N = 2: fwd+bwd+clip+SGD, fp32 -- the CPU has no bf16 path worth timing) -- every one at every candidate
    # thread count.  torch.set_num_threads(os.cpu_count()) as the survey wrote it thrashes oneDNN for minutes on this 256-thread host
    # (measured in round 1), so the candidates are 8 / 16 / 32 and the best per entry is reported with its thread count.
    entries = {"C1 configs[0]: R50 4x16, 2 clips, 224^2, fp32 forward": dict(t=4, clips=2, train=False),
               "C2 shape at N=2: R50 8x8, 2 clips, 224^2, fp32 forward": dict(t=8, clips=2, train=False),
               "C3 shape at N=2: R50 8x8, 2 clips, 224^2, fp32 train step (fwd+bwd+clip+SGD)": dict(t=8, clips=2, train=True)}
    if mode != "train":
        entries.pop("C3 shape at N=2: R50 8x8, 2 clips, 224^2, fp32 train step (fwd+bwd+clip+SGD)")
    usable, usable_why = usable_cpus()
    cands = sorted(set(t for t in (8, 16, 32) if t <= cores) | ({usable} if usable <= 64 else set()) or {cores})
    results = {k: None for k in entries}
    per_entry_budget = seconds / max(len(entries) * len(cands), 1)
    global T_FRAMES
    t_keep = T_FRAMES
    try:
        for thr in cands:
            torch.set_num_threads(thr)
            for name, e in entries.items():
                T_FRAMES = e["t"]
                sd, mom = make_sd("cpu") if e["train"] else {k: torch.from_numpy(vals[pre + k]) for k in shp}, {}
                imgs = torch.from_numpy(synth.synth_clip_batch(e["clips"], e["t"], SIZE, SIZE, seed=7))
                labels = torch.from_numpy(synth.synth_labels(e["clips"]))
                if e["train"]:
                    fn = lambda: one_step(sd, imgs, labels, mom)                                   # noqa: E731
                else:
                    def fn():
                        with torch.no_grad():
                            return net_torch.forward_test(imgs, sd, depth, e["t"], None)
                rate, n = median_rate(fn, e["clips"], per_entry_budget)
                by = dict((results[name] or {}).get("by_threads", {}))
                by[str(thr)] = round(rate, 2)
                if results[name] is None or rate > results[name]["value"]:
                    results[name] = {"value": round(rate, 2), "unit": "clips/s", "threads": thr, "timed_runs": n,
                                     "ms_per_clip": round(1e3 / rate, 1)}
                results[name]["by_threads"] = by
    finally:
        T_FRAMES = t_keep
    eager = eager_compare if isinstance(eager_compare, dict) else None
    head_key = [k for k in entries if k.startswith("C3" if train else "C2")][0]
    head = results[head_key]
    # [r6] ... and the same entry at os.cpu_count() threads, as SURVEY 8(d) literally specifies, in a bounded child process (it may not finish: oneDNN thrashes)
    all_threads = {"threads": cores, "value": None, "unit": "clips/s", "note": None}
    if usable < cores and usable in cands:
        # the container may use `usable` CPUs: THAT is the whole allotment, and it is one of the timed candidates
        all_threads.update(threads=usable, value=results[head_key].get("by_threads", {}).get(str(usable)), timed_at="usable CPUs",
                           note="os.cpu_count() = %d, usable = %d (%s): %d threads is the whole allotment; %d runnable threads on it are throttled into minutes per step"
                                % (cores, usable, usable_why, usable, cores))
    elif cores not in cands:
        import subprocess
        bound = max(20.0, min(60.0, 1.5 * seconds))
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--cpu-child", str(cores), "--depth", str(depth), "--mode", "train" if train else "infer"],
                               capture_output=True, text=True, timeout=bound, env=dict(os.environ, BENCH_CHILD="1"))
            out = r.stdout
        except subprocess.TimeoutExpired as e:
            out = (e.stdout.decode() if isinstance(e.stdout, bytes) else (e.stdout or ""))
            all_threads["note"] = "stopped after %.0f s" % bound
        lines = [l for l in out.splitlines() if l.startswith("{")]
        if lines:
            got = json.loads(lines[-1])
            got["note"] = "; ".join(n_ for n_ in (got.get("note"), all_threads["note"]) if n_) or None
            all_threads.update(got)
        elif all_threads["note"] is None:
            all_threads["note"] = "no result"
    else:
        all_threads.update(value=[r_ for r_ in results.values()][-1]["value"], note="one of the candidates")
    return {"value": head["value"], "unit": "clips/s", "cores": head["threads"], "kind": "port", "host_hw_threads": cores, "usable_cpus": usable, "usable_cpus_limit": usable_why, "cpu_model": cpu_model(),
            "entries": results, "all_hw_threads": all_threads, "torch_eager_gpu": eager,
            "sample": "%s; median of <= 5 runs after 2 warm-ups per entry and thread count, oracle/net_torch.py on torch CPU (oneDNN), best of %s threads "
                      "(%d hardware threads on the host, %d usable: %s), %.0f s budget" % (head_key, cands, cores, usable, usable_why, seconds)}


def eager_comparators(depth, clips, frames, size, seconds, engine_value, dtype):
    """BASELINE.json's '>= 1.5x the reference PyTorch-ROCm clips/sec' comparator, measured in THIS run: tools/eager_compare.py runs
    the same train step (oracle/net_torch.py's restatement of the reference graph) under PyTorch-ROCm eager on this GPU, once in
    the reference's shipped precision (fp32) and once like-for-like with the bf16 engine (autocast(bfloat16) + channels_last).
    Each in its own process with a wall-clock bound (MIOpen compiles its kernels on first use: ~70 s on a fresh box;
    cudnn.benchmark=False -- the exhaustive search of benchmark=True takes 3-25 minutes and measured the same 234 clips/s in fp32)."""
    import subprocess
    out = {}
    for dt in ("bf16", "f32"):
        if dt != dtype and _elapsed() > 0.45 * WALL_BUDGET:      # the like-for-like comparator always runs; the other one only while the call is on schedule
            out[dt] = "skipped: %.0f s of the %.0f s wall budget used before it (slow host); last measured 230-232 clips/s fp32 / 451-453 bf16, DESIGN.md section 5" % (_elapsed(), WALL_BUDGET)
            continue
        cmd = [sys.executable, os.path.join(REPO, "tools", "eager_compare.py"), "--dtype", dt, "--clips", str(clips), "--frames", str(frames),
               "--size", str(size), "--depth", str(depth), "--steps", "3", "--warmup", "1"]
        try:
            p = subprocess.run(cmd, capture_output=True, text=True, timeout=seconds)
            line = [l for l in p.stdout.splitlines() if l.startswith("{")]
            out[dt] = json.loads(line[-1]) if line else "failed rc=%d: %s" % (p.returncode, (p.stderr or "")[-160:])
        except subprocess.TimeoutExpired:
            out[dt] = "no result within %.0f s (MIOpen kernel compilation)" % seconds
        except Exception as e:      # comparator only
            out[dt] = str(e)[:160]
    res = {"torch_eager_gpu_clips_per_s": {k: (v["eager_clips_per_s"] if isinstance(v, dict) else v) for k, v in out.items()},
           "detail": out}
    same = out.get(dtype)
    if isinstance(same, dict) and same.get("eager_clips_per_s"):
        res["engine_over_eager_same_dtype"] = round(engine_value / same["eager_clips_per_s"], 2)
    f32 = out.get("f32")
    if isinstance(f32, dict) and f32.get("eager_clips_per_s"):
        res["engine_over_eager_fp32_reference_precision"] = round(engine_value / f32["eager_clips_per_s"], 2)
    # HEADLINE ratio: against MIOpen's best (cudnn.benchmark=True: an exhaustive kernel search of 240 s for bf16, too long for a default bench
    # run).  STATIC figures measured once on an MI355X of this pool (profiles/r03_eager_bf16_cudnn_benchmark.txt: 479.9 clips/s bf16; fp32 234 after a
    # 3-25 minute search); the ratio uses the larger of that and this run's own eager number.
    best_known = {"bf16": 479.92, "f32": 234.0}
    if depth == 50 and clips == 32 and frames == 8 and size == 224 and dtype in best_known:
        here = same.get("eager_clips_per_s") if isinstance(same, dict) else None
        ref = max(best_known[dtype], here or 0.0)
        res["headline_engine_over_eager_miopen_best"] = {"ratio": round(engine_value / ref, 2), "eager_clips_per_s": ref,
                                                         "note": "eager with cudnn.benchmark=True, STATIC (measured offline, profiles/r03_eager_bf16_cudnn_benchmark.txt) unless this run's "
                                                                 "benchmark=False number is higher; `engine_over_eager_same_dtype` is the in-run benchmark=False ratio"}
    return res


def verify_replicas(dist, eng, step, world):
    """Self-check of the data-parallel run, AFTER the timed steps (every rank calls it): (1) the replicas started from the same
    formula-generated weights and applied the same all-reduced gradient, so their parameters must be BIT-identical -- an integer
    checksum of the fp32 bit patterns is all-gathered and compared; (2) how much of the gradient all-reduce is exposed: a few steps
    with the tail bucket overlapped with backward (default), with the single un-overlapped collective, and with no exchange at all
    (the replicas diverge after that one, so it comes last)."""
    bits = eng.flat_params.view(torch.int32).to(torch.int64)
    chk = torch.stack([bits.sum(), (bits * (torch.arange(bits.numel(), device=bits.device) % 8191 + 1)).sum()])
    allc = [torch.zeros_like(chk) for _ in range(world)]
    dist.all_gather(allc, chk)
    equal = all(torch.equal(allc[0], c) for c in allc)

    def timed(n=3):
        step()                                   # settle the new setting
        torch.cuda.synchronize()
        dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            step()
        torch.cuda.synchronize()
        dist.barrier()
        torch.cuda.synchronize()
        t = torch.tensor([(time.perf_counter() - t0) / n * 1e3], device="cuda", dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    on = timed()
    eng.overlap_allreduce = False
    off = timed()
    eng.overlap_allreduce = True
    eng.exchange_enabled = False
    none = timed()
    eng.exchange_enabled = True
    out = {"rccl_ranks": dist.get_world_size(), "backend": dist.get_backend(), "params_bit_identical_across_ranks": bool(equal),
           "gradient_bytes": int(eng.flat_grads.numel() * 4), "allreduce_ms": {"tail_bucket_overlapped_with_backward": round(on, 3),
                                                                               "single_collective_after_backward": round(off, 3),
                                                                               "no_exchange": round(none, 3), "exposed": round(on - none, 3)}}
    if not equal:
        raise SystemExit("bench.py: replicas hold DIFFERENT parameters after the timed steps: %s" % [c.tolist() for c in allc])
    return out


def other_configs(seconds):
    """BASELINE.json's other single-GPU configurations, each as a short run of THIS script in a child process (after the headline's timed
    region; same JSON contract, 5 timed steps): so that the driver's record carries them, not only the builder's notes."""
    import subprocess
    # (in the order they are dropped last when the wall budget runs out)
    runs = {"C3 at the reference's own recipe (videos_per_gpu=12, configs/MVFNet/K400/mvf_kinetics400_2d_rgb_r50_dense.py:121-123): R50 8x8, 12 clips/GPU, bf16 train step": ["--mode", "train", "--dtype", "bf16", "--clips", "12"],
            "C4 configs[3]: R101 16x4, 16 clips/GPU, bf16 train step": ["--mode", "train", "--dtype", "bf16", "--depth", "101", "--frames", "16", "--clips", "16"],
            "C3 in fp32 (the reference's shipped training precision): R50 8x8, 32 clips, fp32 train step": ["--mode", "train", "--dtype", "f32"],
            "C2 configs[1]: R50 8x8, 32 clips, fp32, forward only": ["--mode", "infer", "--dtype", "f32"],
            "C5 configs[4]: R50 8x8, one video = 10 clips x 3 crops of 256^2, fcn_testing, fp32": ["--mode", "video", "--dtype", "f32"],
            "C5 in bf16": ["--mode", "video", "--dtype", "bf16"]}
    out = {}
    for name, flags in runs.items():
        if _elapsed() > WALL_BUDGET - 25.0:
            out[name] = {"skipped": "%.0f s of the %.0f s wall budget used (slow host); profiles/r06_final_numbers.txt has this configuration" % (_elapsed(), WALL_BUDGET)}
            continue
        # ([r6] 5 warm-up steps: a train engine replays its launch plan from the fifth step on -- two eager steps, two recorded ones)
        cmd = [sys.executable, os.path.abspath(__file__), "--steps", "10" if "train" in flags else "5", "--warmup", "5" if "train" in flags else "2", "--full",
               "--no-cpu-baseline", "--no-eager-compare", "--no-other-configs"] + flags
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, timeout=seconds, env=dict(os.environ, BENCH_CHILD="1"))
            line = [l for l in r.stdout.strip().splitlines() if l.startswith("{")]
            if r.returncode != 0 or not line:
                out[name] = {"error": (r.stderr or r.stdout)[-300:]}
                continue
            d = json.loads(line[-1])
            rf = d.get("roofline", {})
            out[name] = {"metric": d["metric"], "value": d["value"], "unit": d["unit"], "ms_per_step": d["ms_per_step"], "steps": d["steps"], "dtype": d["dtype"],
                         "model_tflops": d.get("model_tflops"), "conv_ms_per_step": rf.get("ms_per_step"), "conv_hbm_frac": rf.get("hbm_frac"),
                         "conv_mfma_frac": rf.get("mfma_frac")}
            if "videos_per_s" in d:
                out[name]["videos_per_s"] = d["videos_per_s"]
            # [r6] every kernel group of this configuration (not only the conv family): time, roofline fraction, algorithmic and counter bytes per step
            keep = ("ms_per_step", "launches_per_step", "bound", "frac", "hbm_frac", "mfma_frac", "alg_bytes_per_step", "traffic_per_step", "traffic_over_algorithmic",
                    "counter_bytes", "counter_bytes_over_fused_floor", "fused_floor_bytes", "step_hbm_frac", "counter_hbm_frac")
            groups = {"conv_required": rf}
            groups.update({g: rf[g] for g in ("family", "wgrad", "bn", "bn_wgrad", "mvf", "step") if isinstance(rf.get(g), dict)})
            out[name]["roofline"] = {g: {k: v[k] for k in keep if k in v} for g, v in groups.items()}
            src = rf.get("traffic_source") or (rf.get("step") or {}).get("counter_source")
            if src:
                out[name]["roofline"]["counter_source"] = src[:160]
        except subprocess.TimeoutExpired:
            out[name] = {"error": "timed out after %.0f s" % seconds}
    return out


def cpu_child(depth, threads, train):
    """[r6] SURVEY 8(d) asks for torch.set_num_threads(os.cpu_count()): on a 256-thread host that thrashes oneDNN for minutes, so it runs here, in a child
    process the parent bounds with a timeout -- one warm-up + up to three timed runs of the headline entry (C3 / C2 shape at N = 2)."""
    from mvfnet_amd import synth
    from mvfnet_amd.arch import state_dict_shapes
    from oracle import net_torch
    torch.set_num_threads(threads)
    shp = state_dict_shapes(depth)
    pre = "r%d/" % depth
    vals = synth.synth_state_dict({pre + k: v for k, v in shp.items()})
    sd = {}
    for k in shp:
        t = torch.from_numpy(vals[pre + k])
        if train and t.dtype == torch.float32 and "running" not in k:
            t.requires_grad_(True)
        sd[k] = t
    imgs = torch.from_numpy(synth.synth_clip_batch(2, 8, SIZE, SIZE, seed=7))
    labels = torch.from_numpy(synth.synth_labels(2))
    mom = {}

    def step():
        if not train:
            with torch.no_grad():
                return net_torch.forward_test(imgs, sd, depth, 8, None)
        params = {k: v for k, v in sd.items() if v.requires_grad}
        for p_ in params.values():
            p_.grad = None
        nb = {}
        loss = net_torch.forward_train(imgs, labels, sd, depth, new_buffers=nb, dropout_ratio=0.5)
        loss.backward()
        with torch.no_grad():
            net_torch.sgd_nesterov_step(params, {k: v.grad for k, v in params.items()}, mom)
            for k, v in nb.items():
                sd[k] = v
        return loss
    t0 = time.perf_counter()
    step()
    # (the parent takes the last line it got: if the timed runs do not fit its bound, the warm-up run -- first-touch and oneDNN primitive creation included -- is the figure)
    print(json.dumps({"threads": threads, "value": round(2.0 / (time.perf_counter() - t0), 3), "timed_runs": 0, "note": "warm-up run only"}), flush=True)
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        step()
        ts.append(time.perf_counter() - t0)
        print(json.dumps({"threads": threads, "value": round(2.0 / sorted(ts)[len(ts) // 2], 3), "timed_runs": len(ts), "note": None}), flush=True)


DUMP_SAMPLE = 1 << 22        # elements of the fixed sample taken from each flat parameter-sized buffer (16 MB of fp32 each)
DUMP_LIMIT = 64 << 20        # bytes, all files together


def dump_outputs(outdir, out, eng):
    """What the last timed step handed its caller, as float32 .npy files in `outdir`.
    train: `loss` (the step's return value), `grad_norm` (eng.norm_out: total gradient norm, clip coefficient), and a fixed sample
    (numpy default_rng(0), DUMP_SAMPLE sorted indices of the flat buffers, the same for every run of one configuration) of the updated
    fp32 master weights `params_sample` and of the step's gradients `grads_sample` -- the whole flat buffers are ~97 MB each at R50.
    infer / video: `scores` (the class scores the forward returns)."""
    import numpy as np
    arrays = {}
    if eng is not None:
        arrays["loss"] = out
        arrays["grad_norm"] = eng.norm_out
        n = eng.flat_grads.numel()
        idx = np.sort(np.random.default_rng(0).choice(n, size=min(DUMP_SAMPLE, n), replace=False))
        idx = torch.from_numpy(idx).to(eng.flat_grads.device)
        if eng.flat_params is not None:
            arrays["params_sample"] = eng.flat_params.index_select(0, idx)
        arrays["grads_sample"] = eng.flat_grads.index_select(0, idx)
    else:
        arrays["scores"] = out
    arrays = {k: v.detach().float().cpu().numpy() for k, v in arrays.items()}
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_LIMIT:
        raise SystemExit("bench.py: --dump-outputs would write %d bytes (limit %d)" % (total, DUMP_LIMIT))
    os.makedirs(outdir, exist_ok=True)
    for k, a in arrays.items():
        np.save(os.path.join(outdir, k + ".npy"), a)
    return sorted(arrays)


def main():
    global T_FRAMES, SIZE, VIDEO
    args = parse()
    if args.cpu_child:
        return cpu_child(args.depth, args.cpu_child, args.mode == "train")
    if args.steps < 1:
        raise SystemExit("bench.py: --steps must be >= 1")
    if args.dtype is None:
        args.dtype = "bf16" if args.mode == "train" else "f32"
    T_FRAMES = args.frames
    video = args.mode == "video"
    if video:
        SIZE, args.clips, args.mode, VIDEO = 256, 30, "infer", True   # 3 crops x 10 clips, ThreeCrop of a 256-short-side frame
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world == 1 and args.gpus > 1:
        raise SystemExit("launch with: python -m torch.distributed.run --nnodes=1 --nproc-per-node %d --master-addr 127.0.0.1 "
                         "bench.py --gpus %d ..." % (args.gpus, args.gpus))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs an MI355X (no CPU fallback for the product path)")
    # BENCH_BACKEND=gloo (rehearsal only): the multi-rank path -- rank_ms_per_step, MAX over ranks, verify_replicas, the exposed-all-reduce triple --
    # with world > 1 on a ONE-GPU box: every rank on the same device, gloo carrying the CUDA tensors (RCCL refuses two ranks per device).  The
    # driver's runs use the default, nccl = RCCL over xGMI, one device per rank.
    backend = os.environ.get("BENCH_BACKEND", "nccl")
    local = local % torch.cuda.device_count() if backend != "nccl" else local
    torch.cuda.set_device(local)
    # the train step's dropout masks come from torch's default generators, and the CUDA one is seeded at random in every process: seeded
    # here, so that the same arguments give the same inputs and the same step in every run (--dump-outputs compares builds output for output)
    torch.manual_seed(1234 + rank)
    dist = None
    if world > 1 or os.environ.get("BENCH_FORCE_DIST") == "1":      # the env switch exercises the RCCL path on a 1-GPU box
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend)

    train = args.mode == "train"
    model = build_model(args.depth, args.dtype, train)
    gen = torch.Generator(device="cuda").manual_seed(1234 + rank)
    global PMC_KEY
    PMC_KEY = pmc_key(args.dtype, args.mode, args.depth, T_FRAMES, SIZE, args.clips, video)
    imgs = torch.randn(args.clips, T_FRAMES, 3, SIZE, SIZE, device="cuda", generator=gen)
    if video:
        imgs = imgs.reshape(1, args.clips * T_FRAMES, 3, SIZE, SIZE)      # [1, crops*clips*T, 3, 256, 256] as the test pipeline emits
    labels = torch.randint(0, 400, (args.clips, 1), device="cuda", generator=gen)
    if train:
        eng = model.train_engine(dtype=torch.float32 if args.dtype == "f32" else torch.bfloat16)   # lr .015, mom .9, wd 1e-4, clip 40
        if args.no_overlap:
            eng.overlap_wgrad = False
        eng.dropout = 0.5
        eng.force_allreduce = dist is not None

        def step():
            return eng.train_step(imgs, labels)

        if args.host_input:
            from mvfnet_amd.runner import DevicePrefetcher
            host = dict(img_group=imgs.cpu().pin_memory(), label=labels.cpu().pin_memory())

            class _Loader(object):              # the same host batch again and again: every step pays its own upload
                def __init__(self, n):
                    self.n = n

                def __len__(self):
                    return self.n

                def __iter__(self):
                    for _ in range(self.n):
                        yield host

            feed = iter(DevicePrefetcher(_Loader(10 ** 9)))           # (also feeds the extra steps of the replica verification)

            def step():                         # noqa: F811
                data = next(feed)
                return eng.train_step(data["img_group"], data["label"])
    else:
        model.backbone.engine().streams = args.streams

        def step():
            return model(imgs, None, return_loss=False, return_numpy=False)

    for _ in range(args.warmup):
        out = step()
    if args.warmup == 0:
        # --warmup 0: one untimed priming step all the same -- the first step of an engine allocates every persistent buffer, builds
        # the pack tables and measures which candidate side stream really runs beside the launch stream (mvfnet_amd/streams.py);
        # none of that is part of a training step
        out = step()
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        out = step()
    torch.cuda.synchronize()
    if dist is not None:
        dist.barrier()
    torch.cuda.synchronize()
    el = time.perf_counter() - t0
    assert torch.isfinite(out).all()
    rank_ms = None
    if dist is not None:
        t = torch.tensor([el], device="cuda", dtype=torch.float64)
        every = [torch.zeros_like(t) for _ in range(world)]
        dist.all_gather(every, t)
        rank_ms = [float(x.item()) / args.steps * 1e3 for x in every]
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        el = float(t.item())
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, out, eng if train else None)
    replicas = None
    if args.full and dist is not None and train:
        replicas = verify_replicas(dist, eng, step, world)

    if rank == 0:
        from mvfnet_amd.arch import conv_macs_per_image
        ms = el / args.steps * 1e3
        value = world * args.clips * args.steps / el
        flop_clip = 2.0 * conv_macs_per_image(args.depth, SIZE) * T_FRAMES * (3 if train else 1)
        what = ("train step: fwd (batch-stat BN) + loss + bwd + %sclip + SGD-nesterov" % ("RCCL all-reduce + " if world > 1 else "")) if train \
            else "eval-BN forward (BASELINE.json configs[1])"
        res = {
            "metric": "clips/sec (%s) MVFNet-R%d %dx%d %d^2%s" % ("fwd+bwd" if train else "fwd", args.depth, T_FRAMES, 64 // T_FRAMES, SIZE,
                                                                     " (30-clip videos, fcn_testing)" if video else ""),
            "value": round(value, 2), "unit": "clips/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(ms, 3), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": args.dtype, "data": "synthetic",
            "config": {"workload": "MVFNet-ResNet%d %dx%d, %d clips/GPU of %dx3x%dx%d, %s, %s; all through the HIP C ABI "
                                   "(stem + %s bottlenecks + MVF + TSN head)" % (
                                       args.depth, T_FRAMES, 64 // T_FRAMES, args.clips, T_FRAMES, SIZE, SIZE,
                                       "fp32" if args.dtype == "f32" else "bf16", what, {50: 16, 101: 33, 152: 50}[args.depth]),
                       "clips_per_gpu": args.clips, "frames_per_clip": T_FRAMES,
                       "parallelism": ("dp%d: replicas, one flat gradient all-reduce per step" % world) if train else
                                      ("replicas x%d (clips sharded, no collective)" % world)},
            "model_tflops": round(value * flop_clip / 1e12, 2),
        }
        if rank_ms is not None:
            res["rank_ms_per_step"] = {"min": round(min(rank_ms), 3), "max": round(max(rank_ms), 3), "all": [round(v, 3) for v in rank_ms]}
        if train and args.host_input:
            res["host_input"] = {"h2d_bytes_per_step": int(imgs.numel() * imgs.element_size() + labels.numel() * labels.element_size()),
                                 "path": "pinned host batch -> runner.DevicePrefetcher (copy stream, one batch ahead) -> train_step"}
        if replicas is not None:
            res["replicas"] = replicas
        if video:
            res["videos_per_s"] = round(value / 30.0, 2)
        if args.full and train:
            res["roofline"] = roofline_train(eng, imgs, labels, args.dtype, args.per_layer, ms)
        elif args.full:
            res["roofline"] = roofline_infer(model, imgs, args.dtype, args.per_layer)
        if args.full and world == 1 and not args.no_cpu_baseline:
            eager = None
            if train and not args.no_eager_compare:
                # (the engine's buffers stay allocated: 288 GB of HBM hold both; the timed region is long over)
                eager = eager_comparators(args.depth, args.clips, T_FRAMES, SIZE, args.eager_seconds, value, args.dtype)
            res["cpu_baseline"] = cpu_baseline(args.depth, args.cpu_seconds, args.mode, args.clips, eager)
        if args.full and world == 1 and train and args.depth == 50 and T_FRAMES == 8 and args.clips == 32 and not args.no_other_configs:
            res["other_configs"] = other_configs(args.other_seconds)
            # the fp32 engine against the eager fp32 comparator of THIS run (the reference's shipped precision, like for like)
            try:
                f32 = next(v for k, v in res["other_configs"].items() if k.startswith("C3 in fp32"))
                eag = res["cpu_baseline"]["torch_eager_gpu"]["torch_eager_gpu_clips_per_s"]["f32"]
                if isinstance(eag, (int, float)) and eag > 0 and "value" in f32:
                    f32["engine_over_eager_fp32"] = round(f32["value"] / eag, 2)
            except Exception:
                pass
        print(json.dumps(res))
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
