// Precise BatchNorm: the running statistics of every calibrated BatchNorm averaged over a few hundred forward-only batches, one launch per batch:
// mvf_bn_stats_accumulate, mvf_bn_stats_finalize, mvf_bn_stats_exchange.
//
// The statistics are ~70 separate module buffers on ResNet-50 (53 BatchNorm2d + 16 MVF BatchNorm3d, a mean and a variance each, ~60 k floats in all), updated in
// place by four kernel families, so they stay where they are: a persistent device table of mvf_stat_segment_t {ptr, first} lays them out as ONE flat "shadow"
// range [0, n) -- segment k owns [first_k, first_{k+1}) -- and each entry point is one launch over that range.  During calibration every statistics kernel runs
// with momentum 1, i.e. stores the batch mean / unbiased batch variance themselves ((1 - m) r + m x at m = 1); accumulate adds them into an fp64 shadow array,
// finalize writes (float)(acc / count) back through the table or into a flat fp32 array (the averaged model's statistics, TrainEngine.flat_ema_stats), and
// exchange gathers / scatters / swaps the modules' buffers against such a flat array bit for bit.
//
// Latency-bound (60 k elements: the launch is the cost, which is why there is ONE): a thread per element, its segment found by binary search as
// sgd_kernel<SEG> does (optim.hip: ~7 dependent 16-byte table reads that hit L2 after the first wave), no grid-stride loop, no atomics, every
// element owned by one thread: bit-identical from run to run.  The fp64 sum is taken in call order, the division is one IEEE fp64 division and one rounding to
// fp32, so the result equals numpy's np.float32(sum(np.float64(x_j)) / np.float64(k)) bit for bit.
//
// The table is checked on the HOST before every launch (first_0 = 0, strictly ascending, below n; non-NULL 4-byte-aligned pointers): a table in device memory
// is read back through a private non-blocking stream (16 bytes per segment, ~2 KB), which waits for that copy alone and never for the work queued on the
// caller's stream.  The table's upload must have completed before the call (a torch .to(device) from pageable memory has); the entry points are not capturable
// into a HIP graph -- the engine calls them outside its launch plans.
//
// Non-finite step guard (mvf_bn_stats_snapshot, mvf_bn_stats_restore): the same table, every training step.  snapshot gathers the statistics into a flat
// array and copies the int64 num_batches_tracked array before the step's first forward; restore scatters both back when the optimizer's guard flag says the
// step was skipped, and stores nothing otherwise (every lane reads the flag first).  One launch each: lanes [0, n) move the 32-bit words, lanes
// [n, n + ncount) the counters.  These two do NOT read the table back -- a blocking copy per step is what the launch-ahead of the training loop cannot
// afford -- they check by-value arguments and alignment only; the table's content is validated once by the caller (any mvf_bn_stats_exchange call on it).
#include <climits>
#include <cstring>
#include <mutex>

#include "common.h"

namespace {

constexpr int kThreads = 256;

__device__ __forceinline__ uint32_t* element_of(const mvf_stat_segment_t* __restrict__ seg, int nseg, long i) {
    int lo = 0, hi = nseg - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (seg[mid].first <= i) lo = mid; else hi = mid - 1;
    }
    return reinterpret_cast<uint32_t*>(seg[lo].ptr) + (i - seg[lo].first);
}

__global__ __launch_bounds__(kThreads) void stats_accumulate_kernel(const mvf_stat_segment_t* __restrict__ seg, int nseg, long n, double* __restrict__ acc) {
    const long i = (long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    acc[i] += (double)__uint_as_float(*element_of(seg, nseg, i));
}

__global__ __launch_bounds__(kThreads) void stats_finalize_kernel(const mvf_stat_segment_t* __restrict__ seg, int nseg, long n, const double* __restrict__ acc,
                                                                   double count, float* __restrict__ dst) {
    const long i = (long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    const float v = (float)(acc[i] / count);
    if (dst) dst[i] = v;
    else *element_of(seg, nseg, i) = __float_as_uint(v);
}

// 32-bit words, no floating-point instruction touches them: NaN payloads and -0.0 travel unchanged
template <int MODE>
__global__ __launch_bounds__(kThreads) void stats_exchange_kernel(const mvf_stat_segment_t* __restrict__ seg, int nseg, long n, uint32_t* __restrict__ flat) {
    const long i = (long)blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    uint32_t* e = element_of(seg, nseg, i);
    if (MODE == 0) {
        flat[i] = *e;
    } else if (MODE == 1) {
        *e = flat[i];
    } else {
        const uint32_t a = *e, b = flat[i];
        *e = b;
        flat[i] = a;
    }
}

// RESTORE = false: flat / cnt_copy <- the segments / cnt; true: the other way round, and only when *guard != 0
template <bool RESTORE>
__global__ __launch_bounds__(kThreads) void stats_guard_kernel(const mvf_stat_segment_t* __restrict__ seg, int nseg, long n, uint32_t* flat, long long* cnt, long ncount,
                                                                long long* cnt_copy, const int* __restrict__ guard) {
    if (RESTORE) { if (guard[0] == 0) return; }
    const long i = (long)blockIdx.x * kThreads + threadIdx.x;
    if (i < n) {
        uint32_t* e = element_of(seg, nseg, i);
        if (RESTORE) *e = flat[i]; else flat[i] = *e;
    } else if (i - n < ncount) {
        if (RESTORE) cnt[i - n] = cnt_copy[i - n]; else cnt_copy[i - n] = cnt[i - n];
    }
}

// ---- host-side check of the table --------------------------------------------------------------------------------------------------------------------------
struct TableReader {
    std::mutex mu;
    int device = -1;
    hipStream_t stream = nullptr;
    void* staging = nullptr;          // pinned
    size_t cap = 0;
};
TableReader g_reader;

// Host-readable copy of the table: `seg` itself when it is host memory (the argument tests that run without a GPU), else a read-back into pinned staging.
// Returns NULL (error set) when the read-back fails.  Called with g_reader.mu held; the result is valid until it is released.
const mvf_stat_segment_t* host_view(const char* who, const mvf_stat_segment_t* seg, int nseg) {
    hipPointerAttribute_t at;
    std::memset(&at, 0, sizeof(at));
    const hipError_t e = hipPointerGetAttributes(&at, seg);
    if (e != hipSuccess) {
        (void)hipGetLastError();      // an address HIP does not know (or no device at all): ordinary host memory
        return seg;
    }
    if (at.type != hipMemoryTypeDevice) return seg;        // unregistered / pinned / managed: readable from here
    TableReader& r = g_reader;
    const size_t bytes = (size_t)nseg * sizeof(mvf_stat_segment_t);
    if (r.stream == nullptr || r.device != at.device) {
        int cur = 0;
        if (hipGetDevice(&cur) != hipSuccess || cur != at.device) {
            mvf_set_error("%s: the segment table lives on device %d, which is not the current device", who, at.device);
            (void)hipGetLastError();
            return nullptr;
        }
        if (r.stream) (void)hipStreamDestroy(r.stream);
        r.stream = nullptr;
        if (hipStreamCreateWithFlags(&r.stream, hipStreamNonBlocking) != hipSuccess) {
            mvf_set_error("%s: cannot create the table read-back stream", who);
            (void)hipGetLastError();
            return nullptr;
        }
        r.device = at.device;
    }
    if (r.cap < bytes) {
        if (r.staging) (void)hipHostFree(r.staging);
        r.staging = nullptr;
        r.cap = 0;
        const size_t want = std::max<size_t>(bytes, 16384);
        if (hipHostMalloc(&r.staging, want, hipHostMallocDefault) != hipSuccess) {
            mvf_set_error("%s: cannot allocate %zu bytes of pinned staging for the segment table", who, want);
            (void)hipGetLastError();
            return nullptr;
        }
        r.cap = want;
    }
    if (hipMemcpyAsync(r.staging, seg, bytes, hipMemcpyDeviceToHost, r.stream) != hipSuccess || hipStreamSynchronize(r.stream) != hipSuccess) {
        mvf_set_error("%s: reading the segment table back failed: %s", who, hipGetErrorString(hipGetLastError()));
        return nullptr;
    }
    return static_cast<const mvf_stat_segment_t*>(r.staging);
}

// `other` [0, other_bytes): the flat array the launch reads or writes beside the segments; no segment may overlap it
int check_table(const char* who, const mvf_stat_segment_t* seg, int nseg, long n, const void* other, size_t other_bytes) {
    MVF_REQUIRE(seg, MVF_EINVAL, "%s: NULL segment table", who);
    MVF_REQUIRE(nseg > 0, MVF_EINVAL, "%s: nseg=%d must be positive", who, nseg);
    MVF_REQUIRE(n > 0, MVF_EINVAL, "%s: n=%ld must be positive", who, n);
    MVF_REQUIRE((n + kThreads - 1) / kThreads <= (long)INT_MAX, MVF_EINVAL, "%s: n=%ld is beyond one launch", who, n);
    MVF_REQUIRE((long)nseg <= n, MVF_EINVAL, "%s: nseg=%d segments cannot share n=%ld elements", who, nseg, n);
    std::lock_guard<std::mutex> lock(g_reader.mu);
    const mvf_stat_segment_t* h = host_view(who, seg, nseg);
    if (!h) return MVF_EHIP;
    MVF_REQUIRE(h[0].first == 0, MVF_EINVAL, "%s: segment 0 starts at %ld, not at 0", who, h[0].first);
    for (int k = 0; k < nseg; ++k) {
        MVF_REQUIRE(h[k].ptr && (uintptr_t)h[k].ptr % 4 == 0, MVF_EINVAL, "%s: segment %d has a NULL or misaligned pointer", who, k);
        const long next = k + 1 < nseg ? h[k + 1].first : n;
        MVF_REQUIRE(h[k].first < next, MVF_EINVAL, "%s: segment offsets must ascend strictly and stay below n=%ld (segment %d starts at %ld, the next at %ld)", who,
                    n, k, h[k].first, next);
        const uintptr_t p0 = (uintptr_t)h[k].ptr, p1 = p0 + (uintptr_t)(next - h[k].first) * 4, o0 = (uintptr_t)other;
        MVF_REQUIRE(!other || p1 <= o0 || o0 + other_bytes <= p0, MVF_EINVAL, "%s: segment %d overlaps the flat array", who, k);
    }
    return MVF_OK;
}

inline int grid_of(long n) { return (int)((n + kThreads - 1) / kThreads); }

// what snapshot / restore can check without reading the table: by-value arguments, NULL, alignment, and (restore) the guard against the other operands
int check_guard_call(const char* who, const mvf_stat_segment_t* seg, int nseg, long n, const void* flat, const void* cnt, long ncount, const void* cnt_copy,
                     const int* guard, bool with_guard) {
    MVF_REQUIRE(seg && (uintptr_t)seg % 8 == 0, MVF_EINVAL, "%s: the segment table is NULL or not 8-byte aligned", who);
    MVF_REQUIRE(nseg > 0, MVF_EINVAL, "%s: nseg=%d must be positive", who, nseg);
    MVF_REQUIRE(n > 0, MVF_EINVAL, "%s: n=%ld must be positive", who, n);
    MVF_REQUIRE((long)nseg <= n, MVF_EINVAL, "%s: nseg=%d segments cannot share n=%ld elements", who, nseg, n);
    MVF_REQUIRE(ncount >= 0, MVF_EINVAL, "%s: ncount=%ld is negative", who, ncount);
    MVF_REQUIRE(n <= LONG_MAX - ncount && (n + ncount + kThreads - 1) / kThreads <= (long)INT_MAX, MVF_EINVAL, "%s: n=%ld + ncount=%ld is beyond one launch", who, n,
                ncount);
    MVF_REQUIRE(flat && (uintptr_t)flat % 4 == 0, MVF_EINVAL, "%s: flat is NULL or not 4-byte aligned", who);
    if (ncount > 0) {
        MVF_REQUIRE(cnt && cnt_copy && (uintptr_t)cnt % 8 == 0 && (uintptr_t)cnt_copy % 8 == 0, MVF_EINVAL, "%s: the counter arrays are NULL or not 8-byte aligned", who);
        const uintptr_t a = (uintptr_t)cnt, b = (uintptr_t)cnt_copy, len = (uintptr_t)ncount * 8;
        MVF_REQUIRE(a + len <= b || b + len <= a, MVF_EINVAL, "%s: the counters and their copy overlap", who);
    }
    if (with_guard) {
        MVF_REQUIRE(guard && (uintptr_t)guard % 4 == 0, MVF_EINVAL, "%s: guard is NULL or not 4-byte aligned", who);
        const uintptr_t pg = (uintptr_t)guard;
        const uintptr_t other[4] = {(uintptr_t)flat, (uintptr_t)cnt, (uintptr_t)cnt_copy, (uintptr_t)seg};
        const uintptr_t bytes[4] = {(uintptr_t)n * 4, (uintptr_t)ncount * 8, (uintptr_t)ncount * 8, (uintptr_t)nseg * sizeof(mvf_stat_segment_t)};
        const char* names[4] = {"flat", "the counters", "the counters' copy", "the segment table"};
        for (int k = 0; k < 4; ++k)
            MVF_REQUIRE(!other[k] || pg + 16 <= other[k] || other[k] + bytes[k] <= pg, MVF_EINVAL, "%s: guard and %s overlap", who, names[k]);
    }
    return MVF_OK;
}

}  // namespace

extern "C" {

int mvf_bn_stats_accumulate(const mvf_stat_segment_t* seg, int nseg, long n, double* acc, void* stream) {
    MVF_REQUIRE(acc && (uintptr_t)acc % 8 == 0, MVF_EINVAL, "bn_stats_accumulate: acc is NULL or not 8-byte aligned");
    const int rc = check_table("bn_stats_accumulate", seg, nseg, n, acc, (size_t)n * 8);
    if (rc != MVF_OK) return rc;
    hipLaunchKernelGGL(stats_accumulate_kernel, dim3(grid_of(n)), dim3(kThreads), 0, (hipStream_t)stream, seg, nseg, n, acc);
    MVF_LAUNCH_CHECK();
    return MVF_OK;
}

int mvf_bn_stats_finalize(const mvf_stat_segment_t* seg, int nseg, long n, const double* acc, long count, float* dst_flat_or_null, void* stream) {
    MVF_REQUIRE(acc && (uintptr_t)acc % 8 == 0, MVF_EINVAL, "bn_stats_finalize: acc is NULL or not 8-byte aligned");
    MVF_REQUIRE(count > 0, MVF_EINVAL, "bn_stats_finalize: count=%ld must be positive", count);
    MVF_REQUIRE((uintptr_t)dst_flat_or_null % 4 == 0, MVF_EINVAL, "bn_stats_finalize: the flat destination must be 4-byte aligned");
    const int rc = check_table("bn_stats_finalize", seg, nseg, n, dst_flat_or_null, (size_t)n * 4);
    if (rc != MVF_OK) return rc;
    hipLaunchKernelGGL(stats_finalize_kernel, dim3(grid_of(n)), dim3(kThreads), 0, (hipStream_t)stream, seg, nseg, n, acc, (double)count, dst_flat_or_null);
    MVF_LAUNCH_CHECK();
    return MVF_OK;
}

int mvf_bn_stats_exchange(const mvf_stat_segment_t* seg, int nseg, long n, float* flat, int mode, void* stream) {
    MVF_REQUIRE(flat && (uintptr_t)flat % 4 == 0, MVF_EINVAL, "bn_stats_exchange: flat is NULL or not 4-byte aligned");
    MVF_REQUIRE(mode >= 0 && mode <= 2, MVF_EINVAL, "bn_stats_exchange: mode=%d (0 gather, 1 scatter, 2 swap)", mode);
    const int rc = check_table("bn_stats_exchange", seg, nseg, n, flat, (size_t)n * 4);
    if (rc != MVF_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    uint32_t* f = reinterpret_cast<uint32_t*>(flat);
    if (mode == 0) hipLaunchKernelGGL(stats_exchange_kernel<0>, dim3(grid_of(n)), dim3(kThreads), 0, st, seg, nseg, n, f);
    else if (mode == 1) hipLaunchKernelGGL(stats_exchange_kernel<1>, dim3(grid_of(n)), dim3(kThreads), 0, st, seg, nseg, n, f);
    else hipLaunchKernelGGL(stats_exchange_kernel<2>, dim3(grid_of(n)), dim3(kThreads), 0, st, seg, nseg, n, f);
    MVF_LAUNCH_CHECK();
    return MVF_OK;
}

int mvf_bn_stats_snapshot(const mvf_stat_segment_t* seg, int nseg, long n, float* flat, const long long* counters, long ncount, long long* counters_copy,
                          void* stream) {
    const int rc = check_guard_call("bn_stats_snapshot", seg, nseg, n, flat, counters, ncount, counters_copy, nullptr, false);
    if (rc != MVF_OK) return rc;
    hipLaunchKernelGGL(stats_guard_kernel<false>, dim3(grid_of(n + ncount)), dim3(kThreads), 0, (hipStream_t)stream, seg, nseg, n, reinterpret_cast<uint32_t*>(flat),
                       const_cast<long long*>(counters), ncount, counters_copy, (const int*)nullptr);
    MVF_LAUNCH_CHECK();
    return MVF_OK;
}

int mvf_bn_stats_restore(const mvf_stat_segment_t* seg, int nseg, long n, const float* flat, long long* counters, long ncount,
                         const long long* counters_copy, const int* guard, void* stream) {
    const int rc = check_guard_call("bn_stats_restore", seg, nseg, n, flat, counters, ncount, counters_copy, guard, true);
    if (rc != MVF_OK) return rc;
    hipLaunchKernelGGL(stats_guard_kernel<true>, dim3(grid_of(n + ncount)), dim3(kThreads), 0, (hipStream_t)stream, seg, nseg, n,
                       reinterpret_cast<uint32_t*>(const_cast<float*>(flat)), counters, ncount, const_cast<long long*>(counters_copy), guard);
    MVF_LAUNCH_CHECK();
    return MVF_OK;
}

}  // extern "C"
