// Focal / asymmetric sigmoid losses for the train head: mvf_focal_loss, and the loss launches of mvf_head_train_fwd_focal (the rules are in
// include/mvfnet_hip.h).
//
// Long-tailed multi-label data (Charades, Multi-Moments in Time, HVU: 0.5 - 4 % label density) drowns plain binary cross-entropy in easy negatives.  One
// element function covers the three recipes in use: the sigmoid focal loss, its class-balanced form (a per-class weight) and the asymmetric loss with its
// probability margin.  It is linear in the target, as bce.hip's is, and leaves dscores, loss_part and loss exactly where mvf_bce_loss leaves them, so
// mvf_head_train_bwd, mvf_distill_loss, the step guard and accumulation run behind it unchanged.
// The work is clips x classes elements (12 x 400 in the shipped recipe): launch latency is the whole cost, so the arithmetic is chosen for its error alone.
//
// fp64 throughout, as bce.hip: inputs are widened on load, pow / exp / log / log1p are the double ones, every output is rounded to fp32 once.  sigmoid(s)
// and sigmoid(-s) both come from e = exp(-|s|) <= 1 (e / (1 + e) and 1 / (1 + e) by the sign of s), never as one minus the other: at s = 40 the negative
// probability is 4e-18, below an ulp of 1.  Contraction into fused multiply-adds is switched off for this file: the operations are the ones written below,
// in the order written.
//
// Launches, both on the caller's stream, no atomics, no workspace:
//   1. focal_clip_kernel: one workgroup per clip, 256 threads, a strided loop over the classes (any classes >= 1): the element losses, their sum,
//      loss_part[i] and, when asked for, the clip's row of dscores.
//   2. loss_mean_kernel (loss_common.h): one wavefront, loss[0] = the mean of loss_part.
// Every reduction has a fixed order -- a shuffle tree inside the wavefront, then the wave partials from LDS in wave order, then clips in ascending order --
// and the grids depend on clips alone: bit-identical from run to run.
//
// The settings are read from the host struct at the call and travel by value.  With margin = 0 the two places where the general form would divide or take a
// logarithm of sigmoid(-s) -- zero in fp64 for s > 745 -- use their closed forms: log(1 - p) = -(max(s, 0) + log1p(e)) and (dpm/ds) / pn = p.
//
// A NaN score makes logp NaN, hence t * L+ (also for t = 0), the element, loss_part[i] and loss[0]; its gradient is set to NaN explicitly (pow(NaN, 0) is 1).
// A non-finite class_weight entry is taken as NaN and does the same.  The non-finite step guard then skips the step.
#include <cfloat>
#include <cmath>

#include "common.h"

#pragma clang fp contract(off)

#include "loss_common.h"

namespace {

struct FocalArgs {
    double gp, gn, m, ap, an;    // focusing exponents, margin, a+ / a-
    float threshold;
    int sum_classes;
};

__global__ __launch_bounds__(kThreads) void focal_clip_kernel(const float* __restrict__ scores, const float* __restrict__ targets, int clips, int classes,
                                                              const float* __restrict__ class_weight, FocalArgs a, float* __restrict__ dscores,
                                                              float* __restrict__ loss_part) {
    __shared__ double red[kWaves];
    const int cl = blockIdx.x, tid = threadIdx.x;
    const float* s_row = scores + (long)cl * classes;
    const float* t_row = targets + (long)cl * classes;
    const bool thr_on = a.threshold == a.threshold;                // NaN = off
    const double D = a.sum_classes ? 1.0 : (double)classes;
    const double gdiv = (double)clips * D;
    double acc = 0.0;
    for (int k = tid; k < classes; k += kThreads) {
        const float tf = t_row[k];
        const double s = (double)s_row[k];
        const double t = thr_on ? (tf > a.threshold ? 1.0 : 0.0) : (double)tf;
        double c = class_weight ? (double)class_weight[k] : 1.0;
        if (!(c - c == 0.0)) c = (double)NAN;                      // inf or NaN
        const double e = exp(-fabs(s));
        const double big = 1.0 / (1.0 + e), small = e / (1.0 + e);
        const double p = s >= 0.0 ? big : small;                   // sigmoid(s)
        const double pn = s >= 0.0 ? small : big;                  // sigmoid(-s)
        const double logp = -(fmax(-s, 0.0) + log1p(e));
        const double wp = a.gp == 0.0 ? 1.0 : pow(pn, a.gp);
        const double lpos = -wp * logp;
        const bool on = p > a.m;
        const double pm = on ? p - a.m : 0.0;
        const double log1m = !on ? 0.0 : a.m == 0.0 ? -(fmax(s, 0.0) + log1p(e)) : log(pn + a.m);
        const double wn = a.gn == 0.0 ? 1.0 : pow(pm, a.gn);
        const double lneg = -wn * log1m;
        acc += c * (a.ap * t * lpos + a.an * (1.0 - t) * lneg);
        if (dscores) {
            const double dpos = wp * (a.gp * p * logp - pn);
            const double dpm = on ? p * pn : 0.0;
            const double ratio = !on ? 0.0 : a.m == 0.0 ? p : dpm / (pn + a.m);
            double dneg = wn * ratio;
            if (a.gn != 0.0) dneg = -(a.gn * (a.gn == 1.0 ? 1.0 : pow(pm, a.gn - 1.0)) * dpm) * log1m + dneg;
            const double g = c * (a.ap * t * dpos + a.an * (1.0 - t) * dneg) / gdiv;
            dscores[(long)cl * classes + k] = s != s ? NAN : (float)g;
        }
    }
    const double r = clip_sum(acc, red);
    if (tid == 0) loss_part[cl] = (float)(r / D);
}

bool gamma_ok(float g) { return g == 0.0f || (g >= 1.0f && g <= 16.0f); }

}  // namespace

namespace mvf_internal {

int focal_check(const char* who, const float* scores, const float* targets, int clips, int classes, const mvf_focal_params_t* prm, const float* loss_part,
                const float* loss) {
    MVF_REQUIRE(scores && targets && prm && loss_part && loss, MVF_EINVAL, "%s: NULL %s", who,
                !scores ? "scores" : !targets ? "targets" : !prm ? "prm" : !loss_part ? "loss_part" : "loss");
    MVF_REQUIRE(clips >= 1 && classes >= 1, MVF_EINVAL, "%s: bad argument (clips=%d classes=%d)", who, clips, classes);
    MVF_REQUIRE(gamma_ok(prm->gamma_pos) && gamma_ok(prm->gamma_neg), MVF_EINVAL, "%s: gamma_pos=%g gamma_neg=%g: each must be 0 or lie in [1, 16]", who,
                (double)prm->gamma_pos, (double)prm->gamma_neg);
    MVF_REQUIRE(prm->margin >= 0.0f && prm->margin < 1.0f, MVF_EINVAL, "%s: margin=%g is outside [0, 1)", who, (double)prm->margin);
    MVF_REQUIRE(prm->alpha <= 1.0f, MVF_EINVAL, "%s: alpha=%g must be <= 1 (negative = off)", who, (double)prm->alpha);
    MVF_REQUIRE(!std::isinf(prm->target_threshold), MVF_EINVAL, "%s: target_threshold=%g must be finite (NaN = off)", who, (double)prm->target_threshold);
    MVF_REQUIRE(prm->sum_classes == 0 || prm->sum_classes == 1, MVF_EINVAL, "%s: sum_classes=%d is neither 0 nor 1", who, prm->sum_classes);
    return MVF_OK;
}

int focal_launch(const float* scores, const float* targets, int clips, int classes, const float* class_weight, const mvf_focal_params_t& prm, float* dscores,
                 float* loss_part, float* loss, hipStream_t st) {
    FocalArgs a;
    a.gp = (double)prm.gamma_pos;
    a.gn = (double)prm.gamma_neg;
    a.m = (double)prm.margin;
    a.ap = prm.alpha < 0.0f ? 1.0 : (double)prm.alpha;
    a.an = prm.alpha < 0.0f ? 1.0 : 1.0 - (double)prm.alpha;
    a.threshold = prm.target_threshold;
    a.sum_classes = prm.sum_classes;
    hipLaunchKernelGGL(focal_clip_kernel, dim3(clips), dim3(kThreads), 0, st, scores, targets, clips, classes, class_weight, a, dscores, loss_part);
    MVF_LAUNCH_CHECK();
    hipLaunchKernelGGL(loss_mean_kernel, dim3(1), dim3(kWave), 0, st, (const float*)loss_part, clips, loss);
    MVF_LAUNCH_CHECK();
    return MVF_OK;
}

}  // namespace mvf_internal

extern "C" {

int mvf_focal_loss(const float* scores, const float* targets, int clips, int classes, const float* class_weight, const mvf_focal_params_t* prm, float* dscores,
                   float* loss_part, float* loss, void* stream) {
    const int rc = mvf_internal::focal_check("focal_loss", scores, targets, clips, classes, prm, loss_part, loss);
    if (rc != MVF_OK) return rc;
    return mvf_internal::focal_launch(scores, targets, clips, classes, class_weight, *prm, dscores, loss_part, loss, (hipStream_t)stream);
}

}  // extern "C"
