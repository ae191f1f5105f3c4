// Per-parameter training statistics: mvf_flat_segment_stats, mvf_flat_stats_workspace_bytes, mvf_bn_stats_nonfinite (the rules are in include/mvfnet_hip.h).
//
// The log carries one global grad_norm, and a step the non-finite guard skips leaves only a counter behind.  Both questions -- is every layer learning, and
// which layer produced the first NaN -- are answered by the same pass: per SEGMENT of a flat fp32 array (one segment per parameter of flat_grads /
// flat_params, or of the difference of two such arrays), the sum of squares and the largest magnitude of the finite elements and the counts of NaN / inf.
// ~160 segments of 64 .. 2.36 M elements on ResNet-50, read once: bandwidth-bound, and the figures stay on the device until the host asks for them.
//
// Two launches, no host work list, no floating-point atomics, no "last workgroup" counter:
//   1. flat_chunk_kernel: workgroup c owns the fixed chunk [c * kChunk, (c + 1) * kChunk) of the flat range.  It finds the segment that holds the chunk's
//      first element by binary search in `first` and walks the segments that intersect the chunk; the whole workgroup reduces one (chunk, segment)
//      intersection -- lanes stride over it, dwordx4 loads on the 16-byte-aligned body, dword loads on the ragged head and tail --, a shuffle tree finishes each
//      wavefront, the four wave partials meet in LDS and lane 0 stores the intersection's partial to workspace slot c + s.  Along the intersections in
//      flat order either c or s grows by one, so c + s is unique, and there are at most nchunks + nseg slots.
//   2. flat_segment_kernel: one wavefront per segment adds that segment's slots (chunks first / kChunk .. (end - 1) / kChunk): lane l takes slots l, l + 64, ..
//      in ascending order, a shuffle tree adds the 64 lane sums, lane 0 stores out[s].
// Every partial is formed by a fixed lane in a fixed order, and the grids depend on n and nseg alone: bit-identical from run to run.
//
// fp64 throughout: the square of an fp32 value is exact in fp64 and a 2.36 M-element sum of them loses ~2e-10 relative at worst, a gradient of 1e20 does not
// overflow the figure that is meant to explain the overflow and one of 1e-30 does not vanish.  The fp64 VALU work (one multiply-add, one max per element)
// stays below the load rate.
//
// Predication (the non-finite guard's rule, mvf_bn_stats_restore): with a guard pointer every workgroup of BOTH launches reads guard[0] first and returns when
// it is 0 -- 4 bytes read per workgroup, not one byte of out / step_out / the workspace stored.
//
// mvf_bn_stats_nonfinite: the same question for the BatchNorm running statistics (the table of mvf_bn_stats_snapshot), asked BEFORE the conditional restore
// erases them: one launch, one wavefront per table segment with a strided loop over its 32-bit words, exponent all ones = not finite, one store per segment.
#include <climits>
#include <cfloat>

#include "common.h"

namespace {

constexpr int kWave = 64;
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / kWave;
constexpr long kChunk = 4096;                       // elements per workgroup of the first launch: 16 KB, 4 dwordx4 loads per lane

static_assert(sizeof(mvf_flat_stats_t) == 32, "mvf_flat_stats_t is four 8-byte words");

__device__ __forceinline__ long lmin(long a, long b) { return a < b ? a : b; }
__device__ __forceinline__ long lmax(long a, long b) { return a > b ? a : b; }

struct Acc {
    double sumsq, absmax;
    long long n_nan, n_inf;
};

__device__ __forceinline__ void take(Acc& a, double d) {
    const double m = fabs(d);
    const bool finite = m <= DBL_MAX, nan = d != d;
    a.sumsq += finite ? d * d : 0.0;
    a.absmax = finite ? fmax(a.absmax, m) : a.absmax;
    a.n_nan += nan ? 1 : 0;
    a.n_inf += (!finite && !nan) ? 1 : 0;
}

__device__ __forceinline__ void merge(Acc& a, const Acc& b) {
    a.sumsq += b.sumsq;
    a.absmax = fmax(a.absmax, b.absmax);
    a.n_nan += b.n_nan;
    a.n_inf += b.n_inf;
}

// butterfly: every lane ends with the same bits (a + b is commutative, so both partners of a pair form the same sum)
__device__ __forceinline__ void wave_merge(Acc& a) {
#pragma unroll
    for (int m = kWave / 2; m > 0; m >>= 1) {
        Acc b;
        b.sumsq = __shfl_xor(a.sumsq, m, kWave);
        b.absmax = __shfl_xor(a.absmax, m, kWave);
        b.n_nan = __shfl_xor(a.n_nan, m, kWave);
        b.n_inf = __shfl_xor(a.n_inf, m, kWave);
        merge(a, b);
    }
}

// the last s in [0, nseg) with first[s] <= i (first[0] == 0)
__device__ __forceinline__ int segment_of(const long long* __restrict__ first, int nseg, long i) {
    int lo = 0, hi = nseg - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (first[mid] <= (long long)i) lo = mid; else hi = mid - 1;
    }
    return lo;
}

template <bool DIFF>
__device__ __forceinline__ double value_at(const float* __restrict__ x, const float* __restrict__ y, long i) {
    return DIFF ? (double)x[i] - (double)y[i] : (double)x[i];
}

// this lane's share of [b, e): stride kThreads; dwordx4 on the 16-byte-aligned body when `vec` (x, and y when given, equally aligned modulo 16)
template <bool DIFF>
__device__ __forceinline__ void reduce_range(const float* __restrict__ x, const float* __restrict__ y, long b, long e, bool vec, Acc& a) {
    const int t = threadIdx.x;
    if (vec && e - b >= 8) {
        const long head = (long)((4 - (int)(((uintptr_t)(x + b) >> 2) & 3)) & 3);      // elements in front of the first aligned one
        const long vb = b + head, nv = (e - vb) >> 2, ve = vb + (nv << 2);
        if (t < head) take(a, value_at<DIFF>(x, y, b + t));
        for (long v = t; v < nv; v += kThreads) {
            const float4 p = *reinterpret_cast<const float4*>(x + vb + (v << 2));
            if (DIFF) {
                const float4 q = *reinterpret_cast<const float4*>(y + vb + (v << 2));
                take(a, (double)p.x - (double)q.x);
                take(a, (double)p.y - (double)q.y);
                take(a, (double)p.z - (double)q.z);
                take(a, (double)p.w - (double)q.w);
            } else {
                take(a, (double)p.x);
                take(a, (double)p.y);
                take(a, (double)p.z);
                take(a, (double)p.w);
            }
        }
        if (ve + t < e) take(a, value_at<DIFF>(x, y, ve + t));                          // (at most 3 elements)
    } else {
        for (long i = b + t; i < e; i += kThreads) take(a, value_at<DIFF>(x, y, i));
    }
}

template <bool DIFF>
__global__ __launch_bounds__(kThreads) void flat_chunk_kernel(const float* __restrict__ x, const float* __restrict__ y, long n, const long long* __restrict__ first,
                                                              int nseg, const int* __restrict__ guard, mvf_flat_stats_t* __restrict__ slots) {
    if (guard && guard[0] == 0) return;
    __shared__ Acc part[2][kWaves];
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    const long c = blockIdx.x, c0 = c * kChunk, c1 = lmin(c0 + kChunk, n);
    const bool vec = !DIFF || (((uintptr_t)x ^ (uintptr_t)y) & 15) == 0;
    int s = segment_of(first, nseg, c0);
    for (int turn = 0; s < nseg; ++s, turn ^= 1) {
        const long sb = s == 0 ? 0 : (long)first[s];                // (segment 0 starts at 0 whatever the table says: every element has an owner)
        const long se = s + 1 < nseg ? (long)first[s + 1] : n;
        const long b = lmax(sb, c0), e = lmin(se, c1);
        if (b >= e) break;                                           // (workgroup-uniform, and only under a table that breaks its contract)
        Acc a = {0.0, 0.0, 0, 0};
        reduce_range<DIFF>(x, y, b, e, vec, a);
        wave_merge(a);
        if (lane == 0) part[turn][wave] = a;
        __syncthreads();        // one barrier per intersection: the next turn writes the OTHER half, and the turn after it starts behind the next barrier
        if (threadIdx.x == 0) {
            Acc r = part[turn][0];
#pragma unroll
            for (int w = 1; w < kWaves; ++w) merge(r, part[turn][w]);
            mvf_flat_stats_t o;
            o.sumsq = r.sumsq;
            o.absmax = r.absmax;
            o.n_nan = r.n_nan;
            o.n_inf = r.n_inf;
            slots[c + s] = o;
        }
        if (se >= c1) break;
    }
}

__global__ __launch_bounds__(kWave) void flat_segment_kernel(long n, const long long* __restrict__ first, int nseg, long nchunks, const int* __restrict__ guard,
                                                             const mvf_flat_stats_t* __restrict__ slots, mvf_flat_stats_t* __restrict__ out,
                                                             long long* __restrict__ step_out) {
    if (guard && guard[0] == 0) return;
    const int s = blockIdx.x, lane = threadIdx.x;
    const long sb = s == 0 ? 0 : (long)first[s];
    const long se = s + 1 < nseg ? (long)first[s + 1] : n;
    Acc a = {0.0, 0.0, 0, 0};
    if (sb < se && sb >= 0 && se <= n) {                             // (a table that breaks its contract gives zeros, never an access outside the workspace)
        const long lo = sb / kChunk, hi = lmin((se - 1) / kChunk, nchunks - 1);
        for (long c = lo + lane; c <= hi; c += kWave) {
            const mvf_flat_stats_t p = slots[c + s];
            Acc b = {p.sumsq, p.absmax, p.n_nan, p.n_inf};
            merge(a, b);
        }
    }
    wave_merge(a);
    if (lane == 0) {
        mvf_flat_stats_t o;
        o.sumsq = a.sumsq;
        o.absmax = a.absmax;
        o.n_nan = a.n_nan;
        o.n_inf = a.n_inf;
        out[s] = o;
        if (s == 0 && step_out) *step_out = (long long)guard[3];
    }
}

__global__ __launch_bounds__(kThreads) void stats_nonfinite_kernel(const mvf_stat_segment_t* __restrict__ seg, int nseg, long n, long long* __restrict__ counts,
                                                                   const int* __restrict__ guard) {
    if (guard && guard[0] == 0) return;
    const int lane = threadIdx.x % kWave, k = blockIdx.x * kWaves + threadIdx.x / kWave;
    if (k >= nseg) return;                                           // wave-uniform
    const long len = (k + 1 < nseg ? seg[k + 1].first : n) - seg[k].first;
    const uint32_t* __restrict__ p = reinterpret_cast<const uint32_t*>(seg[k].ptr);
    int bad = 0;
    for (long j = lane; j < len; j += kWave) bad += (p[j] & 0x7f800000u) == 0x7f800000u ? 1 : 0;
    long long total = bad;
#pragma unroll
    for (int m = kWave / 2; m > 0; m >>= 1) total += __shfl_xor(total, m, kWave);
    if (lane == 0) counts[k] = total;
}

inline bool overlaps(const void* a, size_t a_bytes, const void* b, size_t b_bytes) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a && b && a0 < b0 + b_bytes && b0 < a0 + a_bytes;
}

inline long chunks_of(long n) { return (n + kChunk - 1) / kChunk; }

}  // namespace

extern "C" {

size_t mvf_flat_stats_workspace_bytes(long n, int nseg) {
    if (n <= 0 || nseg <= 0 || (long)nseg > n) return 0;
    return ((size_t)chunks_of(n) + (size_t)nseg) * sizeof(mvf_flat_stats_t);
}

int mvf_flat_segment_stats(const float* x, const float* y_or_null, long n, const long long* first, int nseg, mvf_flat_stats_t* out, const int* guard_or_null,
                           long long* step_out_or_null, void* ws, size_t ws_bytes, void* stream) {
    const char* who = "flat_segment_stats";
    const float* y = y_or_null;
    MVF_REQUIRE(x && first && out, MVF_EINVAL, "%s: NULL x / first / out", who);
    MVF_REQUIRE(n > 0, MVF_EINVAL, "%s: n=%ld must be positive", who, n);
    MVF_REQUIRE(nseg > 0 && (long)nseg <= n, MVF_EINVAL, "%s: nseg=%d must be in [1, n=%ld]", who, nseg, n);
    MVF_REQUIRE(chunks_of(n) <= (long)INT_MAX, MVF_EINVAL, "%s: n=%ld is beyond one launch", who, n);
    MVF_REQUIRE((uintptr_t)x % 4 == 0 && (uintptr_t)y % 4 == 0 && (uintptr_t)guard_or_null % 4 == 0, MVF_EINVAL, "%s: x / y / guard must be 4-byte aligned", who);
    MVF_REQUIRE((uintptr_t)first % 8 == 0 && (uintptr_t)out % 8 == 0 && (uintptr_t)step_out_or_null % 8 == 0 && (uintptr_t)ws % 8 == 0, MVF_EINVAL,
                "%s: first / out / step_out / ws must be 8-byte aligned", who);
    MVF_REQUIRE(!step_out_or_null || guard_or_null, MVF_EINVAL, "%s: step_out is the guard's step counter; it needs the guard", who);
    const size_t xb = (size_t)n * 4, ob = (size_t)nseg * sizeof(mvf_flat_stats_t), need = mvf_flat_stats_workspace_bytes(n, nseg);
    MVF_REQUIRE(!overlaps(out, ob, x, xb) && !overlaps(out, ob, y, xb), MVF_EINVAL, "%s: out overlaps x / y", who);
    MVF_REQUIRE(!overlaps(ws, need, x, xb) && !overlaps(ws, need, y, xb), MVF_EINVAL, "%s: the workspace overlaps x / y", who);
    MVF_REQUIRE(!overlaps(ws, need, out, ob), MVF_EINVAL, "%s: the workspace overlaps out", who);
    MVF_REQUIRE(!overlaps(guard_or_null, 16, out, ob) && !overlaps(guard_or_null, 16, ws, need) && !overlaps(guard_or_null, 16, step_out_or_null, 8), MVF_EINVAL,
                "%s: guard overlaps out / step_out / the workspace", who);
    MVF_REQUIRE(ws && ws_bytes >= need, MVF_EWS, "%s: workspace too small (%zu bytes, need %zu)", who, ws ? ws_bytes : (size_t)0, need);
    hipStream_t st = (hipStream_t)stream;
    const long nchunks = chunks_of(n);
    mvf_flat_stats_t* slots = static_cast<mvf_flat_stats_t*>(ws);
    if (y) hipLaunchKernelGGL(flat_chunk_kernel<true>, dim3((unsigned)nchunks), dim3(kThreads), 0, st, x, y, n, first, nseg, guard_or_null, slots);
    else hipLaunchKernelGGL(flat_chunk_kernel<false>, dim3((unsigned)nchunks), dim3(kThreads), 0, st, x, y, n, first, nseg, guard_or_null, slots);
    MVF_LAUNCH_CHECK();
    hipLaunchKernelGGL(flat_segment_kernel, dim3((unsigned)nseg), dim3(kWave), 0, st, n, first, nseg, nchunks, guard_or_null, slots, out, step_out_or_null);
    MVF_LAUNCH_CHECK();
    return MVF_OK;
}

int mvf_bn_stats_nonfinite(const mvf_stat_segment_t* seg, int nseg, long n, long long* counts, const int* guard_or_null, void* stream) {
    const char* who = "bn_stats_nonfinite";
    MVF_REQUIRE(seg && (uintptr_t)seg % 8 == 0, MVF_EINVAL, "%s: the segment table is NULL or not 8-byte aligned", who);
    MVF_REQUIRE(nseg > 0, MVF_EINVAL, "%s: nseg=%d must be positive", who, nseg);
    MVF_REQUIRE(n > 0, MVF_EINVAL, "%s: n=%ld must be positive", who, n);
    MVF_REQUIRE((long)nseg <= n, MVF_EINVAL, "%s: nseg=%d segments cannot share n=%ld elements", who, nseg, n);
    MVF_REQUIRE(counts && (uintptr_t)counts % 8 == 0, MVF_EINVAL, "%s: counts is NULL or not 8-byte aligned", who);
    MVF_REQUIRE((uintptr_t)guard_or_null % 4 == 0, MVF_EINVAL, "%s: guard is not 4-byte aligned", who);
    const size_t cb = (size_t)nseg * 8, tb = (size_t)nseg * sizeof(mvf_stat_segment_t);
    MVF_REQUIRE(!overlaps(counts, cb, seg, tb), MVF_EINVAL, "%s: counts overlaps the segment table", who);
    MVF_REQUIRE(!overlaps(guard_or_null, 16, counts, cb) && !overlaps(guard_or_null, 16, seg, tb), MVF_EINVAL, "%s: guard overlaps counts / the segment table", who);
    hipLaunchKernelGGL(stats_nonfinite_kernel, dim3((unsigned)((nseg + kWaves - 1) / kWaves)), dim3(kThreads), 0, (hipStream_t)stream, seg, nseg, n, counts,
                       guard_or_null);
    MVF_LAUNCH_CHECK();
    return MVF_OK;
}

}  // extern "C"
