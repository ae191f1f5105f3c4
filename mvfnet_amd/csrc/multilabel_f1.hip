// Multi-label evaluation beyond the per-class AP: mvf_multilabel_sample_ap, mvf_multilabel_prf, mvf_multilabel_best_f1 (the rules are in
// include/mvfnet_hip.h).  All three read the record that mvf_multilabel_record keeps (csrc/multilabel_metrics.hip) over slots [0, state[0]) on the device.
//
// A slot that holds a NaN score -- a NaN row is stored as a row of NaNs without a label, and so is the padding of a merged record -- takes part in nothing:
// a comparison with a NaN is false, the slot is no positive, and the counting kernels skip it explicitly.
//
//   sample_ap_kernel   the sample-wise AP (Multi-Moments in Time): the step-wise AP of ap_pairs_kernel taken along a row,
//                          AP_i = (1 / |P_i|) sum_{c in P_i} TP_ic / N_ic,   N_ic = #{k : s_ik >= s_ic},   TP_ic = #{k in P_i : s_ik >= s_ic}.
//                      The record is class-major, so a row is a stride-`capacity` walk.  A workgroup of four wavefronts owns 64 adjacent rows and stages
//                      tiles of 64 classes x 64 rows through LDS: every global read is a run of 64 consecutive rows of one class.  A wavefront takes 16
//                      of the rows; for a row, lane l holds the candidate class c0 + l of the current 64-class chunk and walks every class tile (all
//                      lanes read the same LDS word: a broadcast), counting N and TP as integers.  A lane adds TP / N of its classes l, l + 64, .. in
//                      ascending order in fp64, a shuffle tree adds the 64 lane sums.
//   prf_kernel         one wavefront per class: TP, FP, FN, TN of "value >= theta_c" as integers.
//   best_f1_kernel     one wavefront per class, behind mvf_multilabel_ap: the positive that maximises F_i = 2 TP_i / (N_i + |P_c|), compared exactly by
//                      cross-multiplication in 64 bits (TP <= 2^30, N + |P| <= 2^31); equal F: the larger score.  Candidates that compare equal in both
//                      hold the same counts, so the winner does not depend on the order of the comparisons.
// No atomics anywhere; the grids depend on capacity and classes alone: bit-identical from run to run.
#include <limits.h>

#include "common.h"

namespace {

constexpr int kWave = 64;
constexpr int kRows = 64;                            // rows per workgroup of sample_ap_kernel
constexpr int kCls = 64;                             // classes per LDS tile
constexpr int kSaThreads = 256;
constexpr int kSaWaves = kSaThreads / kWave;
constexpr int kRowsPerWave = kRows / kSaWaves;       // 16
constexpr int kPad = kRows + 1;                      // candidate tile pitch: lane l reads class l of one row, 65 words apart -> the 32 lanes of a read group on 32 different banks

__device__ __forceinline__ double wave_sum(double v) {
    for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
    return v;
}

__device__ __forceinline__ long long wave_sum(long long v) {
    for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
    return v;
}

__device__ __forceinline__ int wave_sum(int v) {
    for (int off = kWave / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
    return v;
}

__device__ __forceinline__ long slots_used(const long long* state, long capacity) {
    const long long n = state[MVF_MULTILABEL_SLOTS];
    return n < 0 ? 0 : n > (long long)capacity ? capacity : (long)n;
}

__global__ __launch_bounds__(kSaThreads) void sample_ap_kernel(const float* __restrict__ rec_scores, const unsigned char* __restrict__ rec_labels,
                                                               long capacity, int classes, const long long* __restrict__ state,
                                                               double* __restrict__ sample_ap, int* __restrict__ sample_positives) {
    __shared__ float cs[kCls * kPad];                // candidate chunk [class][row], padded
    __shared__ unsigned char cl[kCls * kPad];
    __shared__ float ts[kCls * kRows];               // class tile [class][row]
    __shared__ unsigned char tl[kCls * kRows];
    const long n = slots_used(state, capacity);
    const long r0 = (long)blockIdx.x * kRows;
    const int tid = threadIdx.x, lane = tid % kWave, wave = tid / kWave;
    if (r0 >= n) {                                   // workgroup-uniform: slots beyond the record
        if (tid < kRows && r0 + tid < capacity) {
            sample_ap[r0 + tid] = (double)__builtin_nan("");
            sample_positives[r0 + tid] = 0;
        }
        return;
    }
    const int rr = tid % kRows, kq = tid / kRows;    // staging: a thread copies row rr of classes kq, kq + 4, ..
    const bool row_live = r0 + rr < n;
    double acc[kRowsPerWave];
    int cnt[kRowsPerWave];
#pragma unroll
    for (int j = 0; j < kRowsPerWave; ++j) {
        acc[j] = 0.0;
        cnt[j] = 0;
    }
    for (int c0 = 0; c0 < classes; c0 += kCls) {
        __syncthreads();                             // the previous chunk's readers are done
        for (int kk = kq; kk < kCls; kk += kSaThreads / kRows) {
            const bool in = row_live && c0 + kk < classes;
            const long g = (long)(c0 + kk) * capacity + r0 + rr;
            cs[kk * kPad + rr] = in ? rec_scores[g] : __builtin_nanf("");
            cl[kk * kPad + rr] = in ? rec_labels[g] : (unsigned char)0;
        }
        __syncthreads();
        float si[kRowsPerWave];
        int cn[kRowsPerWave], ct[kRowsPerWave];
        unsigned any = 0;                            // bit j: some lane holds a positive of the wavefront's row j (wave-uniform)
#pragma unroll
        for (int j = 0; j < kRowsPerWave; ++j) {
            const int row = wave * kRowsPerWave + j;
            const bool pos = cl[lane * kPad + row] != 0;
            si[j] = pos ? cs[lane * kPad + row] : __builtin_nanf("");         // a NaN candidate counts nothing
            cn[j] = ct[j] = 0;
            any |= (__ballot(pos) != 0 ? 1u : 0u) << j;
        }
        if (__syncthreads_or(any != 0 ? 1 : 0)) {    // else: no positive in this chunk of the 64 rows, nothing to count
            for (int k0 = 0; k0 < classes; k0 += kCls) {
                __syncthreads();                     // the previous tile's readers are done
                for (int kk = kq; kk < kCls; kk += kSaThreads / kRows) {
                    const bool in = row_live && k0 + kk < classes;
                    const long g = (long)(k0 + kk) * capacity + r0 + rr;
                    ts[kk * kRows + rr] = in ? rec_scores[g] : __builtin_nanf("");
                    tl[kk * kRows + rr] = in ? rec_labels[g] : (unsigned char)0;
                }
                __syncthreads();
                const int m = classes - k0 < kCls ? classes - k0 : kCls;
#pragma unroll
                for (int j = 0; j < kRowsPerWave; ++j) {
                    if (!(any >> j & 1u)) continue;  // wave-uniform
                    const int row = wave * kRowsPerWave + j;
                    for (int u = 0; u < m; ++u) {
                        const int ge = ts[u * kRows + row] >= si[j] ? 1 : 0;
                        cn[j] += ge;
                        ct[j] += ge & (tl[u * kRows + row] != 0 ? 1 : 0);
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < kRowsPerWave; ++j) {
                if (cn[j] > 0) {                     // a positive: N >= TP >= 1 (the class itself)
                    acc[j] += (double)ct[j] / (double)cn[j];
                    ++cnt[j];
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < kRowsPerWave; ++j) {
        const double a = wave_sum(acc[j]);
        const int c = wave_sum(cnt[j]);
        const long i = r0 + wave * kRowsPerWave + j;
        if (lane == 0 && i < capacity) {
            sample_ap[i] = c > 0 ? a / (double)c : (double)__builtin_nan("");
            sample_positives[i] = c;
        }
    }
}

__global__ __launch_bounds__(kWave) void prf_kernel(const float* __restrict__ rec_scores, const unsigned char* __restrict__ rec_labels, long capacity,
                                                    const long long* __restrict__ state, float threshold, const float* __restrict__ thresholds,
                                                    long long* __restrict__ counts) {
    const long n = slots_used(state, capacity);
    const long col = (long)blockIdx.x * capacity;
    const float th = thresholds ? thresholds[blockIdx.x] : threshold;
    long long tp = 0, fp = 0, fn = 0, tn = 0;
    for (long i = threadIdx.x; i < n; i += kWave) {
        const float s = rec_scores[col + i];
        if (s != s) continue;                        // a NaN row or padding
        const bool pred = s >= th, pos = rec_labels[col + i] != 0;
        tp += pred && pos;
        fp += pred && !pos;
        fn += !pred && pos;
        tn += !pred && !pos;
    }
    tp = wave_sum(tp);
    fp = wave_sum(fp);
    fn = wave_sum(fn);
    tn = wave_sum(tn);
    if (threadIdx.x == 0) {
        long long* o = counts + (long)blockIdx.x * 4;
        o[0] = tp;
        o[1] = fp;
        o[2] = fn;
        o[3] = tn;
    }
}

// is candidate (tb, nb, sb) better than (ta, na, sa)?  n == 0: no candidate.  F = 2 tp / (n + P)
__device__ __forceinline__ bool f1_better(int tb, int nb, float sb, int ta, int na, float sa, long long P) {
    if (nb == 0) return false;
    if (na == 0) return true;
    const long long lhs = (long long)tb * ((long long)na + P), rhs = (long long)ta * ((long long)nb + P);
    return lhs > rhs || (lhs == rhs && sb > sa);
}

__global__ __launch_bounds__(kWave) void best_f1_kernel(const float* __restrict__ rec_scores, const int* __restrict__ tp, const int* __restrict__ nn,
                                                        const long long* __restrict__ positives, long capacity, const long long* __restrict__ state,
                                                        int* __restrict__ best_tp, int* __restrict__ best_n, float* __restrict__ best_threshold) {
    const long n = slots_used(state, capacity);
    const long col = (long)blockIdx.x * capacity;
    const long long P = positives[blockIdx.x];
    int bt = 0, bn = 0;
    float bs = 0.f;
    if (P > 0) {
        for (long i = threadIdx.x; i < n; i += kWave) {
            const int d = nn[col + i];
            if (d <= 0) continue;                    // not a positive
            const int t = tp[col + i];
            const float s = rec_scores[col + i];
            if (f1_better(t, d, s, bt, bn, bs, P)) {
                bt = t;
                bn = d;
                bs = s;
            }
        }
    }
    for (int off = kWave / 2; off > 0; off >>= 1) {
        const int ot = __shfl_xor(bt, off, kWave), on = __shfl_xor(bn, off, kWave);
        const float os = __shfl_xor(bs, off, kWave);
        if (f1_better(ot, on, os, bt, bn, bs, P)) {
            bt = ot;
            bn = on;
            bs = os;
        }
    }
    if (threadIdx.x == 0) {
        best_tp[blockIdx.x] = bt;
        best_n[blockIdx.x] = bn;
        best_threshold[blockIdx.x] = bn > 0 ? bs : __builtin_nanf("");
    }
}

bool record_fits(int classes, long capacity) { return capacity >= 1 && capacity <= (long)INT_MAX && (long)classes <= LONG_MAX / 8 / capacity; }

}  // namespace

extern "C" {

int mvf_multilabel_sample_ap(const float* rec_scores, const unsigned char* rec_labels, long capacity, int classes, const long long* state, double* sample_ap,
                             int* sample_positives, void* stream) {
    MVF_REQUIRE(rec_scores && rec_labels && state && sample_ap && sample_positives, MVF_EINVAL, "multilabel_sample_ap: NULL %s",
                !rec_scores ? "rec_scores" : !rec_labels ? "rec_labels" : !state ? "state" : !sample_ap ? "sample_ap" : "sample_positives");
    MVF_REQUIRE(classes >= 1 && classes <= 65535, MVF_ESHAPE, "multilabel_sample_ap: classes=%d is outside [1, 65535]", classes);
    MVF_REQUIRE(record_fits(classes, capacity), MVF_ESHAPE, "multilabel_sample_ap: capacity=%ld x classes=%d is outside the record's range", capacity, classes);
    MVF_REQUIRE((uintptr_t)rec_scores % 4 == 0 && (uintptr_t)sample_positives % 4 == 0 && (uintptr_t)state % 8 == 0 && (uintptr_t)sample_ap % 8 == 0, MVF_EINVAL,
                "multilabel_sample_ap: misaligned operand (state and sample_ap 8 bytes, rec_scores and sample_positives 4)");
    hipLaunchKernelGGL(sample_ap_kernel, dim3((unsigned)((capacity + kRows - 1) / kRows)), dim3(kSaThreads), 0, (hipStream_t)stream, rec_scores, rec_labels,
                       capacity, classes, state, sample_ap, sample_positives);
    MVF_LAUNCH_CHECK();
    return MVF_OK;
}

int mvf_multilabel_prf(const float* rec_scores, const unsigned char* rec_labels, long capacity, int classes, const long long* state, float threshold,
                       const float* thresholds, long long* counts, void* stream) {
    MVF_REQUIRE(rec_scores && rec_labels && state && counts, MVF_EINVAL, "multilabel_prf: NULL %s",
                !rec_scores ? "rec_scores" : !rec_labels ? "rec_labels" : !state ? "state" : "counts");
    MVF_REQUIRE(thresholds || threshold == threshold, MVF_EINVAL, "multilabel_prf: threshold is NaN and no per-class thresholds are given");
    MVF_REQUIRE(classes >= 1 && classes <= 65535, MVF_ESHAPE, "multilabel_prf: classes=%d is outside [1, 65535]", classes);
    MVF_REQUIRE(record_fits(classes, capacity), MVF_ESHAPE, "multilabel_prf: capacity=%ld x classes=%d is outside the record's range", capacity, classes);
    MVF_REQUIRE((uintptr_t)rec_scores % 4 == 0 && (uintptr_t)thresholds % 4 == 0 && (uintptr_t)state % 8 == 0 && (uintptr_t)counts % 8 == 0, MVF_EINVAL,
                "multilabel_prf: misaligned operand (state and counts 8 bytes, rec_scores and thresholds 4)");
    hipLaunchKernelGGL(prf_kernel, dim3(classes), dim3(kWave), 0, (hipStream_t)stream, rec_scores, rec_labels, capacity, state, threshold, thresholds, counts);
    MVF_LAUNCH_CHECK();
    return MVF_OK;
}

int mvf_multilabel_best_f1(const float* rec_scores, const int* tp, const int* nn, const long long* positives, long capacity, int classes,
                           const long long* state, int* best_tp, int* best_n, float* best_threshold, void* stream) {
    MVF_REQUIRE(rec_scores && tp && nn && positives && state && best_tp && best_n && best_threshold, MVF_EINVAL, "multilabel_best_f1: NULL %s",
                !rec_scores ? "rec_scores" : !tp ? "tp" : !nn ? "nn" : !positives ? "positives" : !state ? "state" : !best_tp ? "best_tp" : !best_n ? "best_n"
                                                                                                                                  : "best_threshold");
    MVF_REQUIRE(classes >= 1 && classes <= 65535, MVF_ESHAPE, "multilabel_best_f1: classes=%d is outside [1, 65535]", classes);
    MVF_REQUIRE(record_fits(classes, capacity), MVF_ESHAPE, "multilabel_best_f1: capacity=%ld x classes=%d is outside the record's range", capacity, classes);
    MVF_REQUIRE(capacity <= (1L << 30), MVF_ESHAPE, "multilabel_best_f1: capacity=%ld exceeds 2^30 (the 64-bit cross-multiplication of the F1 comparison)",
                capacity);
    MVF_REQUIRE((uintptr_t)rec_scores % 4 == 0 && (uintptr_t)tp % 4 == 0 && (uintptr_t)nn % 4 == 0 && (uintptr_t)best_tp % 4 == 0 && (uintptr_t)best_n % 4 == 0 &&
                    (uintptr_t)best_threshold % 4 == 0 && (uintptr_t)state % 8 == 0 && (uintptr_t)positives % 8 == 0,
                MVF_EINVAL, "multilabel_best_f1: misaligned operand (state and positives 8 bytes, fp32 / int32 arrays 4)");
    hipLaunchKernelGGL(best_f1_kernel, dim3(classes), dim3(kWave), 0, (hipStream_t)stream, rec_scores, tp, nn, positives, capacity, state, best_tp, best_n,
                       best_threshold);
    MVF_LAUNCH_CHECK();
    return MVF_OK;
}

}  // extern "C"
