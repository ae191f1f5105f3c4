// Multi-label evaluation on the device: mvf_multilabel_record, mvf_multilabel_ap (the rules and the state layout are in include/mvfnet_hip.h).
//
// Mean average precision needs every video's score against every other video's, so unlike top-k accuracy (csrc/metrics.hip) it cannot be folded into a few
// counters per step: the scores are kept.  mvf_multilabel_record appends a pass's (rows, classes) score blocks and their multi-hot labels to a record in
// device memory, transposed to class-major so that a class's column is contiguous; the write offset is a word of device memory, so nothing synchronises.
// mvf_multilabel_ap turns the record into one average precision per class without a sort:
//
//   AP_c = (1 / |P_c|) * sum over the positives i of TP_i / N_i,   N_i = #{j : s_jc >= s_ic},   TP_i = #{j positive : s_jc >= s_ic}
//
// the step-wise AP of scikit-learn's average_precision_score.  Summed over a tie group the terms are dTP * TP / N at that threshold: ties need no special
// case, and the counts do not depend on the order of the rows.
//
// Launches of mvf_multilabel_ap, no atomics at all:
//   1. ap_pairs_kernel: a workgroup owns 256 consecutive rows of one class.  It walks the class's column in tiles of 256 scores and labels staged in LDS
//      (every thread reads the same LDS word: a broadcast); a thread whose row is a positive counts N_i and TP_i, integers.  A workgroup without a positive
//      returns at once, so the work is sum_c |P_c| * n comparisons rounded up to whole workgroups.
//   2. ap_sum_kernel: one wavefront per class adds TP_i / N_i in fp64 -- a lane takes rows l, l + 64, .. in ascending order, a shuffle tree adds the 64 lane
//      sums -- and counts the positives.
// Integers in launch 1, a fixed order in launch 2, grids that depend on capacity and classes alone: bit-identical from run to run.
//
// A row that holds a NaN score is stored as a row of NaN scores with no label set: a comparison with a NaN is false and the row is never a positive, so it
// is left out of every class while the slots stay in step with the rows; the state counts it.  The same property makes a NaN-filled, label-free slot the
// padding of a merged record (metrics.DeviceMultiLabelMetrics.all_gather).
#include <limits.h>

#include "common.h"

namespace {

constexpr int kWave = 64;
constexpr int kRowsPerBlock = 4;
constexpr int kRecThreads = kWave * kRowsPerBlock;
constexpr int kTile = 256;                           // rows per workgroup and scores per LDS tile of ap_pairs_kernel

__device__ __forceinline__ double wave_sum(double v) {
    for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
    return v;
}

__device__ __forceinline__ long long wave_sum(long long v) {
    for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
    return v;
}

// one wavefront per incoming row: is there a NaN, then the transposed store of the row's scores and labels at slot state[OFFSET] + row
__global__ __launch_bounds__(kRecThreads) void record_kernel(const float* __restrict__ scores, const unsigned char* __restrict__ labels, int rows, int classes,
                                                             float* __restrict__ rec_scores, unsigned char* __restrict__ rec_labels, long capacity,
                                                             unsigned long long* __restrict__ state) {
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    const long row = (long)blockIdx.x * kRowsPerBlock + wave;
    if (row >= rows) return;                             // wave-uniform
    const long long base = (long long)state[MVF_MULTILABEL_SLOTS];          // (advance_kernel, the next launch on the stream, is the only writer)
    const long long slot = base + row;
    if (base < 0 || slot >= (long long)capacity) return; // overflow: counted by advance_kernel, nothing stored
    const float* s = scores + row * (long)classes;
    const unsigned char* y = labels + row * (long)classes;
    bool nan = false;
    for (int k = lane; k < classes; k += kWave) {
        const float v = s[k];
        nan |= v != v;
    }
    nan = __ballot(nan) != 0;
    for (int k = lane; k < classes; k += kWave) {
        rec_scores[(long)k * capacity + slot] = nan ? __builtin_nanf("") : s[k];
        rec_labels[(long)k * capacity + slot] = nan ? (unsigned char)0 : (unsigned char)(y[k] != 0);
    }
    if (nan && lane == 0) atomicAdd(&state[MVF_MULTILABEL_NAN_ROWS], 1ull);       // an integer counter: the order of the additions does not show
}

__global__ void advance_kernel(int rows, long capacity, unsigned long long* __restrict__ state) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    long long base = (long long)state[MVF_MULTILABEL_SLOTS];
    if (base < 0) base = 0;
    if (base > (long long)capacity) base = (long long)capacity;
    const long long room = (long long)capacity - base;
    const long long stored = rows < room ? (long long)rows : room;
    state[MVF_MULTILABEL_SLOTS] = (unsigned long long)(base + stored);
    state[MVF_MULTILABEL_OVERFLOW] += (unsigned long long)((long long)rows - stored);
    state[MVF_MULTILABEL_SEEN] += (unsigned long long)rows;
}

__device__ __forceinline__ long slots_used(const long long* state, long capacity) {
    const long long n = state[MVF_MULTILABEL_SLOTS];
    return n < 0 ? 0 : n > (long long)capacity ? capacity : (long)n;
}

__global__ __launch_bounds__(kTile) void ap_pairs_kernel(const float* __restrict__ rec_scores, const unsigned char* __restrict__ rec_labels, long capacity,
                                                         const long long* __restrict__ state, int* __restrict__ tp, int* __restrict__ nn) {
    __shared__ float ts[kTile];
    __shared__ unsigned char tl[kTile];
    const long n = slots_used(state, capacity);
    const long first = (long)blockIdx.x * kTile;
    if (first >= n) return;                              // workgroup-uniform
    const long col = (long)blockIdx.y * capacity;
    const float* s = rec_scores + col;
    const unsigned char* y = rec_labels + col;
    const long i = first + threadIdx.x;
    const bool live = i < n;
    const bool pos = live && y[i] != 0;
    const float si = live ? s[i] : 0.f;
    if (!__syncthreads_or(pos ? 1 : 0)) {                // no positive among the workgroup's rows: their counts are zero
        if (live) tp[col + i] = nn[col + i] = 0;
        return;
    }
    int cn = 0, ct = 0;
    for (long t0 = 0; t0 < n; t0 += kTile) {
        const long j = t0 + threadIdx.x;
        __syncthreads();                                 // the previous tile's readers are done
        if (j < n) {
            ts[threadIdx.x] = s[j];
            tl[threadIdx.x] = y[j];
        }
        __syncthreads();
        if (pos) {
            const int m = (int)(n - t0 < (long)kTile ? n - t0 : (long)kTile);
            for (int u = 0; u < m; ++u) {
                const int ge = ts[u] >= si ? 1 : 0;
                cn += ge;
                ct += ge & (tl[u] != 0 ? 1 : 0);
            }
        }
    }
    if (live) {
        tp[col + i] = pos ? ct : 0;
        nn[col + i] = pos ? cn : 0;
    }
}

__global__ __launch_bounds__(kWave) void ap_sum_kernel(const int* __restrict__ tp, const int* __restrict__ nn, long capacity, const long long* __restrict__ state,
                                                       double* __restrict__ ap, long long* __restrict__ positives) {
    const long n = slots_used(state, capacity);
    const long col = (long)blockIdx.x * capacity;
    double acc = 0.0;
    long long cnt = 0;
    for (long i = threadIdx.x; i < n; i += kWave) {
        const int d = nn[col + i];
        if (d > 0) {                                     // a positive: N_i >= TP_i >= 1 (the row itself)
            acc += (double)tp[col + i] / (double)d;
            ++cnt;
        }
    }
    acc = wave_sum(acc);
    cnt = wave_sum(cnt);
    if (threadIdx.x == 0) {
        ap[blockIdx.x] = cnt > 0 ? acc / (double)cnt : (double)__builtin_nan("");
        positives[blockIdx.x] = cnt;
    }
}

bool record_fits(int classes, long capacity) { return capacity >= 1 && capacity <= (long)INT_MAX && (long)classes <= LONG_MAX / 8 / capacity; }

}  // namespace

extern "C" {

int mvf_multilabel_record(const float* scores, const unsigned char* labels, int rows, int classes, float* rec_scores, unsigned char* rec_labels, long capacity,
                          long long* state, void* stream) {
    MVF_REQUIRE(scores && labels && rec_scores && rec_labels && state, MVF_EINVAL, "multilabel_record: NULL %s",
                !scores ? "scores" : !labels ? "labels" : !rec_scores ? "rec_scores" : !rec_labels ? "rec_labels" : "state");
    MVF_REQUIRE(classes >= 1, MVF_ESHAPE, "multilabel_record: classes=%d must be >= 1", classes);
    MVF_REQUIRE(rows >= 0, MVF_ESHAPE, "multilabel_record: rows=%d is negative", rows);
    MVF_REQUIRE(record_fits(classes, capacity), MVF_ESHAPE, "multilabel_record: capacity=%ld x classes=%d is outside the record's range", capacity, classes);
    MVF_REQUIRE((uintptr_t)scores % 4 == 0 && (uintptr_t)rec_scores % 4 == 0 && (uintptr_t)state % 8 == 0, MVF_EINVAL,
                "multilabel_record: misaligned operand (state 8 bytes, scores and rec_scores 4)");
    if (rows == 0) return MVF_OK;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(record_kernel, dim3((rows + kRowsPerBlock - 1) / kRowsPerBlock), dim3(kRecThreads), 0, st, scores, labels, rows, classes, rec_scores,
                       rec_labels, capacity, (unsigned long long*)state);
    MVF_LAUNCH_CHECK();
    hipLaunchKernelGGL(advance_kernel, dim3(1), dim3(1), 0, st, rows, capacity, (unsigned long long*)state);
    MVF_LAUNCH_CHECK();
    return MVF_OK;
}

int mvf_multilabel_ap(const float* rec_scores, const unsigned char* rec_labels, long capacity, int classes, const long long* state, int* tp, int* nn, double* ap,
                      long long* positives, void* stream) {
    MVF_REQUIRE(rec_scores && rec_labels && state && tp && nn && ap && positives, MVF_EINVAL, "multilabel_ap: NULL %s",
                !rec_scores ? "rec_scores" : !rec_labels ? "rec_labels" : !state ? "state" : !tp ? "tp" : !nn ? "nn" : !ap ? "ap" : "positives");
    MVF_REQUIRE(classes >= 1 && classes <= 65535, MVF_ESHAPE, "multilabel_ap: classes=%d is outside [1, 65535]", classes);
    MVF_REQUIRE(record_fits(classes, capacity), MVF_ESHAPE, "multilabel_ap: capacity=%ld x classes=%d is outside the record's range", capacity, classes);
    MVF_REQUIRE((uintptr_t)rec_scores % 4 == 0 && (uintptr_t)tp % 4 == 0 && (uintptr_t)nn % 4 == 0 && (uintptr_t)state % 8 == 0 && (uintptr_t)ap % 8 == 0 &&
                    (uintptr_t)positives % 8 == 0,
                MVF_EINVAL, "multilabel_ap: misaligned operand (state, ap and positives 8 bytes, rec_scores, tp and nn 4)");
    MVF_REQUIRE((capacity + kTile - 1) / kTile * (long)classes <= (long)INT_MAX, MVF_ESHAPE, "multilabel_ap: capacity=%ld x classes=%d exceeds the grid", capacity,
                classes);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(ap_pairs_kernel, dim3((unsigned)((capacity + kTile - 1) / kTile), (unsigned)classes), dim3(kTile), 0, st, rec_scores, rec_labels, capacity,
                       state, tp, nn);
    MVF_LAUNCH_CHECK();
    hipLaunchKernelGGL(ap_sum_kernel, dim3(classes), dim3(kWave), 0, st, (const int*)tp, (const int*)nn, capacity, state, ap, positives);
    MVF_LAUNCH_CHECK();
    return MVF_OK;
}

}  // extern "C"
