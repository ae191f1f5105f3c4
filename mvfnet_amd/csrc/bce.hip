// Binary cross-entropy with logits for the train head: mvf_bce_loss, and the loss launches of mvf_head_train_fwd_bce (the rules are in include/mvfnet_hip.h).
//
// The sigmoid head of multi-label recognition (Charades, Multi-Moments in Time, HVU: several actions per video, multi-hot targets) and of timm's "ResNet
// strikes back" recipe (BCE against the Mixup / CutMix targets of mvf_soft_targets, optionally thresholded).  It leaves dscores, loss_part and loss exactly
// where mvf_ce_loss_soft leaves them, so mvf_head_train_bwd, mvf_distill_loss, the step guard and accumulation run behind it unchanged.
// The work is clips x classes elements (12 x 400 in the shipped recipe): launch latency is the whole cost, so the arithmetic is chosen for its error alone.
//
// fp64 throughout, as csrc/distill.hip: inputs are widened on load, exp / log1p are the double ones, every output is rounded to fp32 once.  At |s| = 200
// exp(-|s|) is 1.4e-87: zero in fp32, a number in fp64.  Contraction into fused multiply-adds is switched off for this file: the operations are the ones
// written below, in the order written.
//
// Launches, both on the caller's stream, no atomics, no workspace:
//   1. bce_clip_kernel: one workgroup per clip, 256 threads, a strided loop over the classes (any classes >= 1): the element losses, their sum, loss_part[i]
//      and, when asked for, the clip's row of dscores.
//   2. loss_mean_kernel (loss_common.h): one wavefront, loss[0] = the mean of loss_part.
// Every reduction has a fixed order -- a shuffle tree inside the wavefront, then the wave partials from LDS in wave order, then clips in ascending order --
// and the grids depend on clips alone: bit-identical from run to run.
//
// A NaN score makes (1 - t) * s NaN, hence the element, loss_part[i] and loss[0]; its gradient is set to NaN explicitly (the library's exp may clamp its
// argument).  A non-finite pos_weight entry does the same through lw.  The non-finite step guard then skips the step.
#include <cfloat>
#include <cmath>

#include "common.h"

#pragma clang fp contract(off)

#include "loss_common.h"

namespace {

__global__ __launch_bounds__(kThreads) void bce_clip_kernel(const float* __restrict__ scores, const float* __restrict__ targets, int clips, int classes,
                                                            const float* __restrict__ pos_weight, float threshold, int sum_classes,
                                                            float* __restrict__ dscores, float* __restrict__ loss_part) {
    __shared__ double red[kWaves];
    const int cl = blockIdx.x, tid = threadIdx.x;
    const float* s_row = scores + (long)cl * classes;
    const float* t_row = targets + (long)cl * classes;
    const bool thr_on = threshold == threshold;                    // NaN = off
    const double D = sum_classes ? 1.0 : (double)classes;
    const double gdiv = (double)clips * D;
    double acc = 0.0;
    for (int k = tid; k < classes; k += kThreads) {
        const float tf = t_row[k];
        const double s = (double)s_row[k];
        const double t = thr_on ? (tf > threshold ? 1.0 : 0.0) : (double)tf;
        const double w = pos_weight ? (double)pos_weight[k] : 1.0;
        const double lw = 1.0 + (w - 1.0) * t;
        const double e = exp(-fabs(s));
        const double sp = fmax(-s, 0.0) + log1p(e);                // softplus(-s)
        acc += (1.0 - t) * s + lw * sp;
        if (dscores) {
            const double sig = s >= 0.0 ? e / (1.0 + e) : 1.0 / (1.0 + e);       // sigmoid(-s): e = exp(-|s|) <= 1 for either sign
            const double g = ((1.0 - t) - lw * sig) / gdiv;
            dscores[(long)cl * classes + k] = s != s ? NAN : (float)g;
        }
    }
    const double r = clip_sum(acc, red);
    if (tid == 0) loss_part[cl] = (float)(r / D);
}

}  // namespace

namespace mvf_internal {

int bce_check(const char* who, const float* scores, const float* targets, int clips, int classes, float threshold, int sum_classes, const float* loss_part,
              const float* loss) {
    MVF_REQUIRE(scores && targets && loss_part && loss, MVF_EINVAL, "%s: NULL %s", who, !scores ? "scores" : !targets ? "targets" : !loss_part ? "loss_part" : "loss");
    MVF_REQUIRE(clips >= 1 && classes >= 1, MVF_EINVAL, "%s: bad argument (clips=%d classes=%d)", who, clips, classes);
    MVF_REQUIRE(!std::isinf(threshold), MVF_EINVAL, "%s: target_threshold=%g must be finite (NaN = off)", who, (double)threshold);
    MVF_REQUIRE(sum_classes == 0 || sum_classes == 1, MVF_EINVAL, "%s: sum_classes=%d is neither 0 nor 1", who, sum_classes);
    return MVF_OK;
}

int bce_launch(const float* scores, const float* targets, int clips, int classes, const float* pos_weight, float threshold, int sum_classes, float* dscores,
               float* loss_part, float* loss, hipStream_t st) {
    hipLaunchKernelGGL(bce_clip_kernel, dim3(clips), dim3(kThreads), 0, st, scores, targets, clips, classes, pos_weight, threshold, sum_classes, dscores, loss_part);
    MVF_LAUNCH_CHECK();
    hipLaunchKernelGGL(loss_mean_kernel, dim3(1), dim3(kWave), 0, st, (const float*)loss_part, clips, loss);
    MVF_LAUNCH_CHECK();
    return MVF_OK;
}

}  // namespace mvf_internal

extern "C" {

int mvf_bce_loss(const float* scores, const float* targets, int clips, int classes, const float* pos_weight, float target_threshold, int sum_classes,
                 float* dscores, float* loss_part, float* loss, void* stream) {
    const int rc = mvf_internal::bce_check("bce_loss", scores, targets, clips, classes, target_threshold, sum_classes, loss_part, loss);
    if (rc != MVF_OK) return rc;
    return mvf_internal::bce_launch(scores, targets, clips, classes, pos_weight, target_threshold, sum_classes, dscores, loss_part, loss, (hipStream_t)stream);
}

}  // extern "C"
