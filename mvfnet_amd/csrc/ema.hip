// Exponential moving average of the flat fp32 parameters as launches of their own: mvf_ema_update, mvf_ema_swap.
//
// The training recipes for small sets (UCF101, HMDB51, Something-Something: 96-clip steps, blended inputs, a few thousand optimizer steps) are evaluated on
// an average of the weights, not on the last iterate.  The fused optimizer kernels keep that average where the new parameter value is already in a register
// (optim.hip: the EMA instantiations of sgd_kernel / adamw_kernel, lamb_apply_kernel).  mvf_ema_update is the same arithmetic after an optimizer that is not ours (the
// attach_grads path) and the twin those kernels are tested against; mvf_ema_swap exchanges the averaged copy with the live parameters in place for
// evaluation (TrainEngine.averaged_weights): the model's parameters are views of the flat buffer, so the pointers cannot be swapped, and a third
// parameter-sized buffer is not wanted.
//
// ema_step (common.h) is the ONE statement of the arithmetic: e' = fmaf(m, p - e, e), and e' = p at m = 1.
//
// Memory-bound: 12 bytes per element for the update, 16 for the swap.  Written as grad_accum.hip is: the body moves 16 bytes per lane, the operands are
// arbitrary 4-byte-aligned views of the flat buffers, so up to three leading elements (until the first operand is 16-byte aligned) and up to three trailing
// ones go through a scalar path, and where the second operand's alignment differs from the first's its accesses are scalar while the first's stay vectors.
// The grid depends on n and the alignment only; every element is owned by one lane: no atomics, bit-identical from run to run.
#include <algorithm>

#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 256 * 8;      // grid-stride beyond 8 workgroups per CU (cdna_hip_programming.md, Guideline 11)

template <bool VEC>
__device__ __forceinline__ float4 load4(const float* p) {
    if (VEC) return ld4(p);
    return make_float4(p[0], p[1], p[2], p[3]);
}
template <bool VEC>
__device__ __forceinline__ void store4(float* p, float4 v) {
    if (VEC) { st4(p, v); return; }
    p[0] = v.x; p[1] = v.y; p[2] = v.z; p[3] = v.w;
}
__device__ __forceinline__ float4 ema_step4(float4 e, float4 p, float m) {
    return make_float4(ema_step(e.x, p.x, m), ema_step(e.y, p.y, m), ema_step(e.z, p.z, m), ema_step(e.w, p.w, m));
}

// ema[0, n) <- ema_step(ema, params, m); [head, head + 4 * nvec) is the 16-byte body (ema + head is 16-byte aligned), the other <= 6 elements are scalar
template <bool PVEC>
__global__ __launch_bounds__(kThreads) void ema_update_kernel(float* __restrict__ ema, const float* __restrict__ params, long n, int head, long nvec, float m) {
    const long stride = (long)gridDim.x * kThreads;
    float* ev = ema + head;
    const float* pv = params + head;
    long i = (long)blockIdx.x * kThreads + threadIdx.x;
    // two vectors in flight per lane: all four loads are issued before the first store
    for (; i + stride < nvec; i += 2 * stride) {
        const long j = i + stride;
        const float4 p0 = load4<PVEC>(pv + 4 * i), p1 = load4<PVEC>(pv + 4 * j);
        const float4 e0 = ld4(ev + 4 * i), e1 = ld4(ev + 4 * j);
        st4(ev + 4 * i, ema_step4(e0, p0, m));
        st4(ev + 4 * j, ema_step4(e1, p1, m));
    }
    if (i < nvec) st4(ev + 4 * i, ema_step4(ld4(ev + 4 * i), load4<PVEC>(pv + 4 * i), m));
    if (blockIdx.x == 0) {
        const long tail0 = head + 4 * nvec;
        const int ntail = (int)(n - tail0);
        const int t = threadIdx.x;
        if (t < head + ntail) {
            const long k = t < head ? (long)t : tail0 + (t - head);
            ema[k] = ema_step(ema[k], params[k], m);
        }
    }
}

// a[0, n) <-> b[0, n), the same split; a lane reads its elements of both buffers before it writes either
template <bool BVEC>
__global__ __launch_bounds__(kThreads) void ema_swap_kernel(float* __restrict__ a, float* __restrict__ b, long n, int head, long nvec) {
    const long stride = (long)gridDim.x * kThreads;
    float* av = a + head;
    float* bv = b + head;
    long i = (long)blockIdx.x * kThreads + threadIdx.x;
    for (; i + stride < nvec; i += 2 * stride) {
        const long j = i + stride;
        const float4 b0 = load4<BVEC>(bv + 4 * i), b1 = load4<BVEC>(bv + 4 * j);
        const float4 a0 = ld4(av + 4 * i), a1 = ld4(av + 4 * j);
        st4(av + 4 * i, b0);
        st4(av + 4 * j, b1);
        store4<BVEC>(bv + 4 * i, a0);
        store4<BVEC>(bv + 4 * j, a1);
    }
    if (i < nvec) {
        const float4 b0 = load4<BVEC>(bv + 4 * i);
        const float4 a0 = ld4(av + 4 * i);
        st4(av + 4 * i, b0);
        store4<BVEC>(bv + 4 * i, a0);
    }
    if (blockIdx.x == 0) {
        const long tail0 = head + 4 * nvec;
        const int ntail = (int)(n - tail0);
        const int t = threadIdx.x;
        if (t < head + ntail) {
            const long k = t < head ? (long)t : tail0 + (t - head);
            const float x = a[k], y = b[k];
            a[k] = y;
            b[k] = x;
        }
    }
}

struct Split {
    int head, grid;
    long nvec;
    bool vec2;       // the second operand is 16-byte aligned where the first one's body starts
};

Split split_for(uintptr_t p0, uintptr_t p1, long n) {
    Split s;
    s.head = (int)std::min<long>(n, (long)(((16 - p0 % 16) % 16) / 4));
    s.nvec = (n - s.head) / 4;
    s.vec2 = (p1 + (uintptr_t)s.head * 4) % 16 == 0;
    s.grid = (int)std::max<long>(1, std::min<long>((s.nvec + kThreads - 1) / kThreads, kMaxBlocks));
    return s;
}

}  // namespace

extern "C" {

int mvf_ema_update(float* ema, const float* params, long n, float momentum, void* stream) {
    MVF_REQUIRE(n >= 0, MVF_EINVAL, "ema_update: n=%ld is negative", n);
    MVF_REQUIRE(momentum >= 0.f && momentum <= 1.f, MVF_EINVAL, "ema_update: momentum=%g is outside [0, 1]", (double)momentum);      // (NaN fails both)
    if (n == 0) return MVF_OK;
    MVF_REQUIRE(ema && params, MVF_EINVAL, "ema_update: NULL %s with n=%ld", ema ? "params" : "ema", n);
    const uintptr_t pe = (uintptr_t)ema, pp = (uintptr_t)params;
    MVF_REQUIRE(pe % 4 == 0 && pp % 4 == 0, MVF_EINVAL, "ema_update: ema / params must be 4-byte aligned");
    MVF_REQUIRE(pe + (uintptr_t)n * 4 <= pp || pp + (uintptr_t)n * 4 <= pe, MVF_EINVAL, "ema_update: ema and params overlap");
    const Split s = split_for(pe, pp, n);
    hipStream_t st = (hipStream_t)stream;
    if (s.vec2) hipLaunchKernelGGL(ema_update_kernel<true>, dim3(s.grid), dim3(kThreads), 0, st, ema, params, n, s.head, s.nvec, momentum);
    else hipLaunchKernelGGL(ema_update_kernel<false>, dim3(s.grid), dim3(kThreads), 0, st, ema, params, n, s.head, s.nvec, momentum);
    MVF_LAUNCH_CHECK();
    return MVF_OK;
}

int mvf_ema_swap(float* a, float* b, long n, void* stream) {
    MVF_REQUIRE(n >= 0, MVF_EINVAL, "ema_swap: n=%ld is negative", n);
    if (n == 0) return MVF_OK;
    MVF_REQUIRE(a && b, MVF_EINVAL, "ema_swap: NULL %s with n=%ld", a ? "b" : "a", n);
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    MVF_REQUIRE(pa % 4 == 0 && pb % 4 == 0, MVF_EINVAL, "ema_swap: a / b must be 4-byte aligned");
    MVF_REQUIRE(pa + (uintptr_t)n * 4 <= pb || pb + (uintptr_t)n * 4 <= pa, MVF_EINVAL, "ema_swap: a and b overlap");
    const Split s = split_for(pa, pb, n);
    hipStream_t st = (hipStream_t)stream;
    if (s.vec2) hipLaunchKernelGGL(ema_swap_kernel<true>, dim3(s.grid), dim3(kThreads), 0, st, a, b, n, s.head, s.nvec);
    else hipLaunchKernelGGL(ema_swap_kernel<false>, dim3(s.grid), dim3(kThreads), 0, st, a, b, n, s.head, s.nvec);
    MVF_LAUNCH_CHECK();
    return MVF_OK;
}

}  // extern "C"
