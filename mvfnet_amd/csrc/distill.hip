// Knowledge distillation: mvf_distill_loss (the rules are in include/mvfnet_hip.h).
//
// Runs right behind mvf_head_train_fwd / mvf_head_train_fwd_soft, which leave the cross-entropy's dscores, loss_part and loss in device memory, and turns
// them into Hinton's combined loss (1 - a) * CE + a * T^2 * KL(softmax(z / T) || softmax(s / T)) and its gradient with respect to the student's scores.
// The work is clips x classes elements (12 x 400 in the shipped recipe): launch latency is the whole cost, so the arithmetic is chosen for its error alone.
//
// fp64 throughout: the KL term is a sum of differences of nearly equal numbers when teacher and student are close or T is large -- restated in fp32 it
// reached 2.4e-4 relative error in loss_part at 400 classes and T = 20, against the project's 1e-5 loss bound (csrc/layer_stats.hip is the precedent for fp64
// in a reduction this small).  Inputs are widened on load, exp / log are the double ones, every output is rounded to fp32 once.  Contraction into fused
// multiply-adds is switched off for this file: the operations are the ones written below, in the order written.
//
// Launches, all on the caller's stream, no atomics, no workspace:
//   1. distill_terms_kernel (only with terms != NULL; one workgroup): terms[0] = the mean of the INCOMING loss_part, so it runs before launch 2 overwrites
//      them, and terms[1] = the mean of T^2 * kd_i.  The entry point takes no workspace, so this launch computes kd_i itself, clip after clip, with the
//      same row function and the same reduction order as launch 2: the same bits.
//   2. distill_clip_kernel: one workgroup per clip, 256 threads, strided loops over the classes: kd_i, then loss_part[i] and the clip's row of dscores.
//   3. loss_mean_kernel (loss_common.h): one wavefront, loss[0] = the mean of the new loss_part.
// Every reduction has a fixed order -- a shuffle tree inside the wavefront, then the wave partials from LDS in wave order, then clips in ascending order --
// and the grids depend on clips alone: bit-identical from run to run.
//
// A NaN or inf in a teacher (or student) row is looked for explicitly, in the pass that takes the maxima: fmax drops a NaN and the library's exp clamps
// its argument, so arithmetic alone does not carry one to every output.  Such a row's kd_i, loss_part and dscores are NaN, and with them loss[0] and
// terms[1]: the non-finite step guard skips the step.
#include <cfloat>
#include <cmath>

#include "common.h"

#pragma clang fp contract(off)

#include "loss_common.h"

namespace {

__device__ __forceinline__ double wave_max(double v) {
    for (int off = kWave / 2; off > 0; off >>= 1) v = fmax(v, __shfl_xor(v, off, kWave));
    return v;
}

// the workgroup's sum / maximum, the same bits in every thread: shuffle tree, then the wave partials in wave order.  red: kWaves doubles of LDS.
template <bool MAX>
__device__ __forceinline__ double block_reduce(double v, double* red) {
    v = MAX ? wave_max(v) : wave_sum(v);
    __syncthreads();                               // the previous reduction's readers are done with red
    if ((threadIdx.x & (kWave - 1)) == 0) red[threadIdx.x / kWave] = v;
    __syncthreads();
    double r = red[0];
    for (int w = 1; w < kWaves; ++w) r = MAX ? fmax(r, red[w]) : r + red[w];
    return r;
}

struct RowKd {
    double lse_z, lse_s, kd;
    bool bad;                                      // a NaN or inf among the row's 2 * classes inputs: kd is NaN, and so is everything made of the row
};

// one clip, by one workgroup of kThreads: lse(z / T), lse(s / T) and kd = sum_k p_k * ((z_k / T - s_k / T) - (lse(z / T) - lse(s / T))), p = softmax(z / T).
// z_k / T and s_k / T are formed the same way everywhere, so equal bits in z and s give a zero in every term, and one class gives
// (z / T - s / T) - (z / T - s / T).
__device__ __forceinline__ RowKd row_kd(const float* s, const float* z, int classes, double T, double* red) {
    const int tid = threadIdx.x;
    double mz = -INFINITY, ms = -INFINITY, nonfinite = 0.0;
    for (int k = tid; k < classes; k += kThreads) {
        const double zt = (double)z[k] / T, st = (double)s[k] / T;
        mz = fmax(mz, zt);
        ms = fmax(ms, st);
        nonfinite += (fabs(zt) <= DBL_MAX && fabs(st) <= DBL_MAX) ? 0.0 : 1.0;      // (a NaN fails the comparison)
    }
    mz = block_reduce<true>(mz, red);
    ms = block_reduce<true>(ms, red);
    nonfinite = block_reduce<false>(nonfinite, red);
    double ez = 0.0, es = 0.0;
    for (int k = tid; k < classes; k += kThreads) {
        ez += exp((double)z[k] / T - mz);
        es += exp((double)s[k] / T - ms);
    }
    ez = block_reduce<false>(ez, red);
    es = block_reduce<false>(es, red);
    RowKd r;
    r.lse_z = log(ez) + mz;
    r.lse_s = log(es) + ms;
    const double dl = r.lse_z - r.lse_s;
    double acc = 0.0;
    for (int k = tid; k < classes; k += kThreads) {
        const double zt = (double)z[k] / T, st = (double)s[k] / T;
        acc += exp(zt - r.lse_z) * ((zt - st) - dl);
    }
    acc = block_reduce<false>(acc, red);
    r.bad = nonfinite > 0.0;
    r.kd = r.bad ? (double)NAN : acc;
    return r;
}

__global__ __launch_bounds__(kThreads) void distill_clip_kernel(const float* scores, const float* teacher, int clips, int classes, float temperature, float alpha,
                                                                float* dscores, float* loss_part) {
    __shared__ double red[kWaves];
    const int cl = blockIdx.x, tid = threadIdx.x;
    const float* s = scores + (long)cl * classes;
    const float* z = teacher + (long)cl * classes;
    float* d = dscores + (long)cl * classes;
    const double T = (double)temperature, a = (double)alpha, keep = 1.0 - a;
    const RowKd r = row_kd(s, z, classes, T, red);
    if (tid == 0) loss_part[cl] = (float)(keep * (double)loss_part[cl] + a * (T * T * r.kd));
    for (int k = tid; k < classes; k += kThreads) {
        const double q = exp((double)s[k] / T - r.lse_s), p = exp((double)z[k] / T - r.lse_z);
        d[k] = r.bad ? NAN : (float)(keep * (double)d[k] + a * T * (q - p) / (double)clips);
    }
}

__global__ __launch_bounds__(kThreads) void distill_terms_kernel(const float* scores, const float* teacher, int clips, int classes, float temperature,
                                                                 const float* loss_part, float* terms) {
    __shared__ double red[kWaves];
    const double T = (double)temperature;
    double kd_sum = 0.0;                           // every thread holds the same bits (block_reduce)
    for (int cl = 0; cl < clips; ++cl) kd_sum += T * T * row_kd(scores + (long)cl * classes, teacher + (long)cl * classes, classes, T, red).kd;
    if (threadIdx.x < kWave) {
        const double ce = wave_mean(loss_part, clips, threadIdx.x);
        if (threadIdx.x == 0) {
            terms[0] = (float)ce;
            terms[1] = (float)(kd_sum / (double)clips);
        }
    }
}

}  // namespace

extern "C" {

int mvf_distill_loss(const float* scores, const float* teacher_scores, int clips, int classes, float temperature, float alpha, float* dscores,
                     float* loss_part, float* loss, float* terms, void* stream) {
    MVF_REQUIRE(scores && teacher_scores && dscores && loss_part && loss, MVF_EINVAL, "distill_loss: NULL %s",
                !scores ? "scores" : !teacher_scores ? "teacher_scores" : !dscores ? "dscores" : !loss_part ? "loss_part" : "loss");
    MVF_REQUIRE(clips >= 1 && classes >= 1, MVF_EINVAL, "distill_loss: bad argument (clips=%d classes=%d)", clips, classes);
    MVF_REQUIRE(std::isfinite(temperature) && temperature > 0.f, MVF_EINVAL, "distill_loss: temperature=%g must be finite and positive", (double)temperature);
    MVF_REQUIRE(std::isfinite(alpha) && alpha > 0.f && alpha <= 1.f, MVF_EINVAL, "distill_loss: alpha=%g is outside (0, 1]", (double)alpha);
    hipStream_t st = (hipStream_t)stream;
    if (terms) {
        hipLaunchKernelGGL(distill_terms_kernel, dim3(1), dim3(kThreads), 0, st, scores, teacher_scores, clips, classes, temperature, (const float*)loss_part, terms);
        MVF_LAUNCH_CHECK();
    }
    hipLaunchKernelGGL(distill_clip_kernel, dim3(clips), dim3(kThreads), 0, st, scores, teacher_scores, clips, classes, temperature, alpha, dscores, loss_part);
    MVF_LAUNCH_CHECK();
    hipLaunchKernelGGL(loss_mean_kernel, dim3(1), dim3(kWave), 0, st, (const float*)loss_part, clips, loss);
    MVF_LAUNCH_CHECK();
    return MVF_OK;
}

}  // extern "C"
