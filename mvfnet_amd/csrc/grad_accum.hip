// Gradient accumulation over micro-batches: mvf_grad_accumulate.
//
// The reference's recipe is 8 GPUs x 12 clips per optimizer step with per-GPU BatchNorm statistics (configs/MVFNet/K400/mvf_kinetics400_2d_rgb_r50_dense.py:121-123,
// codes/core/dist_utils.py:61-67).  One GPU reproduces that step by running the 8 micro-batches one after another and summing their flat fp32 gradients before the
// optimizer runs once on the sum (TrainEngine.accumulate_step / apply_accumulated).  This file is the sum: acc = g for the first micro-batch of a group (so the
// accumulator is never cleared), acc = acc + g for every later one -- one fp32 add per element in a fixed order, no atomics, bit-identical from run to run.
//
// Memory-bound: 12 bytes per element (8 for the first).  The body moves 16 bytes per lane; the operands are arbitrary 4-byte-aligned views of the flat
// buffers (apply_sgd hands kernels flat_*[off:] the same way), so up to three leading elements (until acc is 16-byte aligned) and up to three trailing ones go
// through a scalar path, and where g's alignment differs from acc's its loads are scalar while acc's stay vectors.
#include <algorithm>

#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 256 * 8;      // grid-stride beyond 8 workgroups per CU (cdna_hip_programming.md, Guideline 11)

template <bool GVEC>
__device__ __forceinline__ float4 load_g(const float* p) {
    if (GVEC) return ld4(p);
    return make_float4(p[0], p[1], p[2], p[3]);
}

template <bool FIRST>
__device__ __forceinline__ float4 combine(const float* acc, float4 b) {
    if (FIRST) return b;
    const float4 a = ld4(acc);
    return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}

// acc[0, n) (=|+=) g[0, n); [head, head + 4 * nvec) is the 16-byte body (acc + head is 16-byte aligned), the other <= 6 elements are scalar
template <bool FIRST, bool GVEC>
__global__ __launch_bounds__(kThreads) void grad_accum_kernel(float* __restrict__ acc, const float* __restrict__ g, long n, int head, long nvec) {
    const long stride = (long)gridDim.x * kThreads;
    float* av = acc + head;
    const float* gv = g + head;
    long i = (long)blockIdx.x * kThreads + threadIdx.x;
    // two vectors in flight per lane: both loads are issued before the first store
    for (; i + stride < nvec; i += 2 * stride) {
        const long j = i + stride;
        const float4 b0 = load_g<GVEC>(gv + 4 * i), b1 = load_g<GVEC>(gv + 4 * j);
        const float4 r0 = combine<FIRST>(av + 4 * i, b0), r1 = combine<FIRST>(av + 4 * j, b1);
        st4(av + 4 * i, r0);
        st4(av + 4 * j, r1);
    }
    if (i < nvec) st4(av + 4 * i, combine<FIRST>(av + 4 * i, load_g<GVEC>(gv + 4 * i)));
    if (blockIdx.x == 0) {
        const long tail0 = head + 4 * nvec;
        const int ntail = (int)(n - tail0);
        const int t = threadIdx.x;
        if (t < head + ntail) {
            const long k = t < head ? (long)t : tail0 + (t - head);
            acc[k] = FIRST ? g[k] : acc[k] + g[k];
        }
    }
}

}  // namespace

extern "C" {

int mvf_grad_accumulate(float* acc, const float* g, long n, int first, void* stream) {
    MVF_REQUIRE(n >= 0, MVF_EINVAL, "grad_accumulate: n=%ld is negative", n);
    if (n == 0) return MVF_OK;
    MVF_REQUIRE(acc && g, MVF_EINVAL, "grad_accumulate: NULL %s with n=%ld", acc ? "g" : "acc", n);
    const uintptr_t pa = (uintptr_t)acc, pg = (uintptr_t)g;
    MVF_REQUIRE(pa % 4 == 0 && pg % 4 == 0, MVF_EINVAL, "grad_accumulate: acc / g must be 4-byte aligned");
    MVF_REQUIRE(pa + (uintptr_t)n * 4 <= pg || pg + (uintptr_t)n * 4 <= pa, MVF_EINVAL, "grad_accumulate: acc and g overlap");
    const int head = (int)std::min<long>(n, (long)(((16 - pa % 16) % 16) / 4));
    const long nvec = (n - head) / 4;
    const bool gvec = (pg + (uintptr_t)head * 4) % 16 == 0;
    const int grid = (int)std::max<long>(1, std::min<long>((nvec + kThreads - 1) / kThreads, kMaxBlocks));
    hipStream_t st = (hipStream_t)stream;
    if (first) {
        if (gvec) hipLaunchKernelGGL((grad_accum_kernel<true, true>), dim3(grid), dim3(kThreads), 0, st, acc, g, n, head, nvec);
        else hipLaunchKernelGGL((grad_accum_kernel<true, false>), dim3(grid), dim3(kThreads), 0, st, acc, g, n, head, nvec);
    } else {
        if (gvec) hipLaunchKernelGGL((grad_accum_kernel<false, true>), dim3(grid), dim3(kThreads), 0, st, acc, g, n, head, nvec);
        else hipLaunchKernelGGL((grad_accum_kernel<false, false>), dim3(grid), dim3(kThreads), 0, st, acc, g, n, head, nvec);
    }
    MVF_LAUNCH_CHECK();
    return MVF_OK;
}

}  // extern "C"
