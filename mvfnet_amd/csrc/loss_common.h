// The fixed-order fp64 reductions the train head's fp64 losses share (bce.hip, focal.hip, distill.hip): 256 threads per clip, one wavefront for the mean.
// Sums only -- nothing here can contract into a fused multiply-add, whichever side of the including file's `#pragma clang fp contract(off)` it lands on.
// (The cross-entropy path of head.hip ends in mean_reduce_kernel, one thread walking the clips: another order, other bits.)
#pragma once
#include "common.h"

namespace {

constexpr int kWave = 64;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;

__device__ __forceinline__ double wave_sum(double v) {
    for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
    return v;
}

// the workgroup's sum, on thread 0 only: a shuffle tree inside each wavefront, then the wave partials from LDS in wave order.  red: kWaves doubles of LDS.
__device__ __forceinline__ double clip_sum(double acc, double* red) {
    const int tid = threadIdx.x;
    acc = wave_sum(acc);
    if ((tid & (kWave - 1)) == 0) red[tid / kWave] = acc;
    __syncthreads();
    double r = red[0];
    if (tid == 0)
        for (int w = 1; w < kWaves; ++w) r += red[w];
    return r;
}

// lanes take clips l, l + 64, .. in ascending order, a shuffle tree adds the 64 lane sums
__device__ __forceinline__ double wave_mean(const float* v, int n, int lane) {
    double s = 0.0;
    for (int i = lane; i < n; i += kWave) s += (double)v[i];
    return wave_sum(s) / (double)n;
}

// one wavefront: loss[0] = the mean of loss_part
static __global__ __launch_bounds__(kWave) void loss_mean_kernel(const float* loss_part, int clips, float* loss) {
    const double m = wave_mean(loss_part, clips, threadIdx.x);
    if (threadIdx.x == 0) loss[0] = (float)m;
}

}  // namespace
