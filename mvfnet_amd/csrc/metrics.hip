// Device-side accuracy: mvf_metrics_update, mvf_metrics_state_words (the rules and the state layout are in include/mvfnet_hip.h).
//
// Evaluation used to leave the device once per video (a 1.6 KB score row, a full drain of the stream) and the training log had no accuracy at all although the
// step's (B, classes) score matrix sits in the engine's buffer after every forward.  This kernel turns a score matrix and its labels into integer counters that
// stay on the device: rows seen, bad rows, hits per k, and optionally the confusion matrix.  The host reads the few words where it synchronises anyway.
//
// One wavefront per row, kRowsPerBlock rows per workgroup.  A lane walks the row with stride 64 and keeps three things: how many scores beat the label's
// (rank), whether it met a NaN, and its own first maximum.  Three wave reductions (shuffles) finish the row; lane 0 files the row's counts in LDS, and after
// the workgroup's barrier each non-zero word costs ONE global integer atomic.  The confusion cell is one global atomic per valid row.  Integer sums: the state
// is the same whatever the order, from run to run and under any split of the rows into calls.
//
// Latency-bound by design: the training step's matrix is 32 x 400 floats, a video's is 1 x 400.  Nothing here is worth tuning beyond one launch.
#include <limits.h>

#include "common.h"

namespace {

constexpr int kWave = 64;
constexpr int kRowsPerBlock = 4;
constexpr int kThreads = kWave * kRowsPerBlock;
constexpr int kHeader = MVF_METRICS_CONFUSION;      // words in front of the confusion matrix

struct KList {
    int k[MVF_METRICS_MAX_K];
};

__device__ __forceinline__ int wave_sum(int v) {
#pragma unroll
    for (int m = kWave / 2; m > 0; m >>= 1) v += __shfl_xor(v, m, kWave);
    return v;
}

// (value, index) of the maximum with the LOWEST index among equals; idx == INT_MAX marks "no element yet" (a lane past the row's end)
__device__ __forceinline__ void wave_argmax(float& best, int& idx) {
#pragma unroll
    for (int m = kWave / 2; m > 0; m >>= 1) {
        const float ob = __shfl_xor(best, m, kWave);
        const int oi = __shfl_xor(idx, m, kWave);
        if (oi != INT_MAX && (idx == INT_MAX || ob > best || (ob == best && oi < idx))) {
            best = ob;
            idx = oi;
        }
    }
}

__global__ __launch_bounds__(kThreads) void metrics_kernel(const float* __restrict__ scores, int rows, int classes, const long long* __restrict__ labels, KList ks,
                                                           int nk, unsigned long long* __restrict__ state, int with_confusion, int* __restrict__ rank_out,
                                                           int* __restrict__ pred_out) {
    __shared__ unsigned int cnt[kHeader];
    const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
    if (threadIdx.x < kHeader) cnt[threadIdx.x] = 0;
    __syncthreads();
    const long row = (long)blockIdx.x * kRowsPerBlock + wave;
    if (row < rows) {                                    // wave-uniform: a whole wavefront owns the row
        const long long y = labels[row];
        int rank = -1, pred = -1;
        int word = MVF_METRICS_BAD_LABEL;                // which bad-row counter, or -1 for a valid row
        if (y >= 0 && y < classes) {                     // (else: not one score of the row is read)
            const float* s = scores + row * (long)classes;
            const int yi = (int)y;
            const float sy = s[yi];
            int above = 0, bidx = INT_MAX;
            bool nan = false;
            float best = 0.f;
            for (int j = lane; j < classes; j += kWave) {
                const float v = s[j];
                nan |= v != v;
                above += (v > sy || (v == sy && j < yi)) ? 1 : 0;
                if (bidx == INT_MAX || v > best) {       // strictly greater: a lane keeps its first maximum
                    best = v;
                    bidx = j;
                }
            }
            above = wave_sum(above);
            wave_argmax(best, bidx);
            if (__ballot(nan) != 0) {
                word = MVF_METRICS_NAN_ROWS;
            } else {
                word = -1;
                rank = above;
                pred = bidx;
            }
        }
        if (lane == 0) {
            atomicAdd(&cnt[MVF_METRICS_ROWS], 1u);
            if (word >= 0) {
                atomicAdd(&cnt[word], 1u);
            } else {
#pragma unroll
                for (int i = 0; i < MVF_METRICS_MAX_K; ++i)
                    if (i < nk && rank < ks.k[i]) atomicAdd(&cnt[MVF_METRICS_HITS + i], 1u);
                if (with_confusion) atomicAdd(&state[kHeader + (long)y * classes + pred], 1ull);
            }
            if (rank_out) rank_out[row] = rank;
            if (pred_out) pred_out[row] = pred;
        }
    }
    __syncthreads();
    if (threadIdx.x < kHeader && cnt[threadIdx.x] != 0) atomicAdd(&state[threadIdx.x], (unsigned long long)cnt[threadIdx.x]);
}

bool confusion_fits(int classes) { return (long)classes * (long)classes <= (long)INT_MAX; }

}  // namespace

extern "C" {

size_t mvf_metrics_state_words(int classes, int with_confusion) {
    if (classes < 1) return 0;
    if (!with_confusion) return (size_t)kHeader;
    if (!confusion_fits(classes)) return 0;
    return (size_t)kHeader + (size_t)classes * (size_t)classes;
}

int mvf_metrics_update(const float* scores, int rows, int classes, const long long* labels, const int* ks, int nk, long long* state, int with_confusion,
                       int* rank_out, int* pred_out, void* stream) {
    MVF_REQUIRE(scores && labels && state && ks, MVF_EINVAL, "metrics_update: NULL %s", !scores ? "scores" : !labels ? "labels" : !state ? "state" : "ks");
    MVF_REQUIRE(classes >= 1, MVF_ESHAPE, "metrics_update: classes=%d must be >= 1", classes);
    MVF_REQUIRE(rows >= 0, MVF_ESHAPE, "metrics_update: rows=%d is negative", rows);
    MVF_REQUIRE(nk >= 1 && nk <= MVF_METRICS_MAX_K, MVF_ESHAPE, "metrics_update: nk=%d is outside [1, %d]", nk, (int)MVF_METRICS_MAX_K);
    KList kl;
    for (int i = 0; i < MVF_METRICS_MAX_K; ++i) kl.k[i] = 0;
    for (int i = 0; i < nk; ++i) {
        MVF_REQUIRE(ks[i] >= 1, MVF_ESHAPE, "metrics_update: ks[%d]=%d must be >= 1", i, ks[i]);
        kl.k[i] = ks[i];
    }
    MVF_REQUIRE(!with_confusion || confusion_fits(classes), MVF_ESHAPE, "metrics_update: classes=%d: the confusion matrix has more than 2^31 - 1 cells", classes);
    MVF_REQUIRE((uintptr_t)scores % 4 == 0 && (uintptr_t)labels % 8 == 0 && (uintptr_t)state % 8 == 0 && (uintptr_t)rank_out % 4 == 0 &&
                    (uintptr_t)pred_out % 4 == 0,
                MVF_EINVAL, "metrics_update: misaligned operand (labels and state 8 bytes, scores / rank_out / pred_out 4)");
    if (rows == 0) return MVF_OK;
    const int grid = (rows + kRowsPerBlock - 1) / kRowsPerBlock;
    hipLaunchKernelGGL(metrics_kernel, dim3(grid), dim3(kThreads), 0, (hipStream_t)stream, scores, rows, classes, labels, kl, nk, (unsigned long long*)state,
                       with_confusion ? 1 : 0, rank_out, pred_out);
    MVF_LAUNCH_CHECK();
    return MVF_OK;
}

}  // extern "C"
