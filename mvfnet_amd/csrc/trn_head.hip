// Temporal-relation head (TRN / TRNmultiscale consensus of TSNClsHead): mvf_trn_head_fwd, mvf_trn_head_bwd (the rules are in include/mvfnet_hip.h).
//
// The head is bandwidth-trivial (2.3 M parameters at T = 8) and launch-bound: 19 relation evaluations of two small Linears each.  Here every relation row of
// the step's table is one slice of ONE launch per stage -- 5 launches forward, 7 backward, whatever the number of rows:
//   forward    pool -> new_fc -> hidden partials (all rows, K split) -> hidden reduce -> scores (rows summed in table order)
//   backward   dW2/db2 -> dh -> dW1/db1 -> df (a gather over the rows that hold the frame) -> dW_fc/db_fc -> dpool -> dfeat
// Every sum has a fixed order: a k-loop per output element (or a fixed number of partial accumulators / K splits / wave quarters combined in a fixed tree),
// rows in table order, clips ascending.  No atomics, no counters: bit-identical from run to run.
// The per-scale operands travel BY VALUE in the kernel arguments (15 sets of 8 pointers), read from the caller's host array at each call: nothing on the
// device holds a parameter address.  The table is DEVICE memory; its indices are clamped, so a bad table cannot read outside a tensor.
#include <algorithm>

#include "common.h"

namespace {

constexpr int kMaxScales = MVF_TRN_MAX_FRAMES - 1;
struct TrnScales {
    mvf_trn_scale_t s[kMaxScales];
};

thread_local mvf_trn_launch_info_t t_last_trn = {};

__device__ __forceinline__ int trn_scale(const int* table, int r, int T, int ns) { return min(max(table[(long)r * (T + 1)], 0), ns - 1); }
__device__ __forceinline__ int trn_frame(const int* table, int r, int p, int T) { return min(max(table[(long)r * (T + 1) + 1 + p], 0), T - 1); }

// A workgroup of 256 threads as 64 output lanes x 4 quarters of a reduction: the four quarter sums of a lane, combined as (q0 + q1) + (q2 + q3).  Every thread calls it.
__device__ __forceinline__ float quarter_sum(float v, float (*red)[64]) {
    const int q = threadIdx.x >> 6, l = threadIdx.x & 63;
    red[q][l] = v;
    __syncthreads();
    const float s = (red[0][l] + red[1][l]) + (red[2][l] + red[3][l]);
    __syncthreads();
    return s;
}
__device__ __forceinline__ float tree8(const float* a) { return ((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7])); }

// pooled[frame][ch] = mean over hw (x the pre-scaled dropout mask): the average head's frame_pool_kernel (head.hip) with the row loop unrolled by 7 -- the same bits,
// 10 us faster per call at 7 x 7 x 2048, which this launch-bound head shows (profiles/head_refactor.txt)
template <typename ET>
__global__ void trn_pool_kernel(const ET* feat, int hw, int c, const float* drop_mask, float* pooled) {
    const int f = blockIdx.y, ch = blockIdx.x * blockDim.x + threadIdx.x;
    if (ch >= c) return;
    const ET* p = feat + (long)f * hw * c + ch;
    float s = 0.f;
#pragma unroll 7
    for (int r = 0; r < hw; ++r) s += ldf(p + (long)r * c);
    s = s / (float)hw;
    if (drop_mask) s *= drop_mask[(long)f * c + ch];
    pooled[(long)f * c + ch] = s;
}

// out(m, n) = sum over k in [kbeg, kend) of a_at(m, k0, kk) * B[n][k], k = k0 + kk: an 8 x 32 tile per workgroup of 256 threads (one output each), k in ascending
// chunks of 128 through LDS.  One accumulator per output: the order of the sum depends on [kbeg, kend) alone.
constexpr int kBK = 128, kTM = 8, kTN = 32;
template <class ALoad, class Store>
__device__ __forceinline__ void gemm_nt_tile(int M, int N, int K, int kbeg, int kend, int m0, int n0, const float* __restrict__ B, ALoad a_at, Store store) {
    __shared__ float As[kTM][kBK + 1];
    __shared__ float Bs[kTN][kBK + 1];
    const int tid = threadIdx.x, tx = tid & (kTN - 1), ty = tid / kTN;
    float acc = 0.f;
    for (int k0 = kbeg; k0 < kend; k0 += kBK) {
#pragma unroll
        for (int i = 0; i < kTM * kBK / 256; ++i) {
            const int e = tid + i * 256;
            const int r = e / kBK, kk = e % kBK, m = m0 + r;
            As[r][kk] = (m < M && k0 + kk < kend) ? a_at(m, k0, kk) : 0.f;
        }
#pragma unroll
        for (int i = 0; i < kTN * kBK / 256; ++i) {
            const int e = tid + i * 256;
            const int r = e / kBK, kk = e % kBK, n = n0 + r, k = k0 + kk;
            Bs[r][kk] = (n < N && k < kend) ? B[(long)n * K + k] : 0.f;
        }
        __syncthreads();
#pragma unroll 32
        for (int kk = 0; kk < kBK; ++kk) acc += As[ty][kk] * Bs[tx][kk];
        __syncthreads();
    }
    const int m = m0 + ty, n = n0 + tx;
    if (m < M && n < N) store(m, n, acc);
}

// f[frame][j] = pooled[frame] . fc_w[j] + fc_b[j]
__global__ __launch_bounds__(256) void trn_fc_kernel(const float* pooled, const float* w, const float* b, int frames, int c, int fdim, float* f) {
    gemm_nt_tile(frames, fdim, c, 0, c, blockIdx.x * kTM, blockIdx.y * kTN, w,
                 [=](int m, int k0, int kk) { return pooled[(long)m * c + k0 + kk]; },
                 [=](int m, int n, float v) { f[(long)m * fdim + n] = v + (b ? b[n] : 0.f); });
}

// hpart[sp][r][clip][j] = W1_s[j] . relu(concat_{p < s} f[clip][frame_r(p)]) over the sp-th K split of table row r (blockIdx.z = r * nsplit + sp); split
// boundaries are multiples of the 128-element chunk.  With fdim a multiple of 128 a chunk lies in one frame: its table lookup is hoisted out of the element loop.
__global__ __launch_bounds__(256) void trn_hidden_part_kernel(const float* f, TrnScales sc, int ns, const int* table, int rows, int nsplit, int clips, int T, int fdim,
                                                              int hidden, float* hpart) {
    const int r = blockIdx.z / nsplit, sp = blockIdx.z % nsplit, si = trn_scale(table, r, T, ns), K = (T - si) * fdim;
    const int chunk = ((K + nsplit - 1) / nsplit + kBK - 1) / kBK * kBK;
    const int kbeg = min(K, sp * chunk), kend = min(K, kbeg + chunk);
    float* out = hpart + ((long)sp * rows + r) * clips * hidden;
    const bool aligned = fdim % kBK == 0;
    gemm_nt_tile(clips, hidden, K, kbeg, kend, blockIdx.x * kTM, blockIdx.y * kTN, sc.s[si].w1,
                 [=](int m, int k0, int kk) {
                     int p, d;
                     if (aligned) { p = k0 / fdim; d = k0 % fdim + kk; }            // (k0 is uniform over the chunk: one division per chunk)
                     else { p = (k0 + kk) / fdim; d = (k0 + kk) % fdim; }
                     return fmaxf(f[((long)m * T + trn_frame(table, r, p, T)) * fdim + d], 0.f);
                 },
                 [=](int m, int n, float v) { out[(long)m * hidden + n] = v; });
}

// h[r][clip][j] = relu((sum over the K splits, ascending) + b1_s[j])
__global__ __launch_bounds__(256) void trn_hidden_reduce_kernel(const float* hpart, TrnScales sc, int ns, const int* table, int rows, int nsplit, int clips, int T,
                                                                int hidden, float* h) {
    const int r = blockIdx.z, cl = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    if (j >= hidden) return;
    const long o = ((long)r * clips + cl) * hidden + j, stride = (long)rows * clips * hidden;
    float v = 0.f;
    for (int sp = 0; sp < nsplit; ++sp) v += hpart[sp * stride + o];
    h[o] = fmaxf(v + sc.s[trn_scale(table, r, T, ns)].b1[j], 0.f);
}

// scores[clip][k] = sum over the table rows, in table order, of (W2_s[k] . h[r][clip] + b2_s[k]): one wavefront per (clip, class)
__global__ __launch_bounds__(256) void trn_scores_kernel(const float* h, TrnScales sc, int ns, const int* table, int rows, int clips, int T, int hidden, int classes,
                                                         float* scores) {
    const long o = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (o >= (long)clips * classes) return;
    const int clip = (int)(o / classes), k = (int)(o % classes);
    float acc = 0.f;
    for (int r = 0; r < rows; ++r) {
        const int si = trn_scale(table, r, T, ns);
        const float* w = sc.s[si].w2 + (long)k * hidden;
        const float* hr = h + ((long)r * clips + clip) * hidden;
        float v = 0.f;
        for (int j = lane; j < hidden; j += 64) v += hr[j] * w[j];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
        acc += v + sc.s[si].b2[k];
    }
    if (lane == 0) scores[o] = acc;
}

// dW2_s[k][j] = sum over the rows of scale s, in table order, over the clips ascending, of dscores[clip][k] * h[r][clip][j]; db2_s[k] likewise of dscores[clip][k]
__global__ __launch_bounds__(256) void trn_dw2_kernel(const float* dscores, const float* h, TrnScales sc, int ns, const int* table, int rows, int clips, int T,
                                                      int hidden, int classes) {
    const int si = blockIdx.z, k = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    float acc = 0.f, accb = 0.f;
    for (int r = 0; r < rows; ++r) {
        if (trn_scale(table, r, T, ns) != si) continue;
#pragma unroll 4
        for (int cl = 0; cl < clips; ++cl) {
            const float d = dscores[(long)cl * classes + k];
            if (j < hidden) acc += d * h[((long)r * clips + cl) * hidden + j];
            accb += d;
        }
    }
    if (j < hidden) sc.s[si].dw2[(long)k * hidden + j] = acc;
    if (j == 0) sc.s[si].db2[k] = accb;
}

// dh[r][clip][j] = [h[r][clip][j] > 0] * sum_k dscores[clip][k] * W2_s[k][j]: 64 j per workgroup, the classes in four quarters (one per wavefront)
__global__ __launch_bounds__(256) void trn_dh_kernel(const float* dscores, const float* h, TrnScales sc, int ns, const int* table, int clips, int T, int hidden,
                                                     int classes, float* dh) {
    __shared__ float red[4][64];
    const int r = blockIdx.z, cl = blockIdx.y, q = threadIdx.x >> 6, j = blockIdx.x * 64 + (threadIdx.x & 63), jj = min(j, hidden - 1);
    const float* w2 = sc.s[trn_scale(table, r, T, ns)].w2;
    const float* ds = dscores + (long)cl * classes;
    const int per = (classes + 3) / 4, k1 = min(classes, (q + 1) * per);
    float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int k = q * per;
    for (; k + 8 <= k1; k += 8) {
#pragma unroll
        for (int u = 0; u < 8; ++u) a[u] += ds[k + u] * w2[(long)(k + u) * hidden + jj];
    }
    for (; k < k1; ++k) a[0] += ds[k] * w2[(long)k * hidden + jj];
    const float acc = quarter_sum(tree8(a), red);
    if (q == 0 && j < hidden) {
        const long o = ((long)r * clips + cl) * hidden + j;
        dh[o] = h[o] > 0.f ? acc : 0.f;
    }
}

// dW1_s[j][k] = sum over the rows of scale s, in table order, over the clips ascending, of dh[r][clip][j] * relu(f[clip][frame_r(k / fdim)][k % fdim]);
// db1_s[j] likewise of dh[r][clip][j]
__global__ __launch_bounds__(256) void trn_dw1_kernel(const float* dh, const float* f, TrnScales sc, int ns, const int* table, int rows, int clips, int T, int fdim,
                                                      int hidden) {
    const int si = blockIdx.z, j = blockIdx.y, k = blockIdx.x * 256 + threadIdx.x, K = (T - si) * fdim;
    if (blockIdx.x * 256 >= K) return;
    const int p = min(k, K - 1) / fdim, d = min(k, K - 1) % fdim;
    float acc = 0.f, accb = 0.f;
    for (int r = 0; r < rows; ++r) {
        if (trn_scale(table, r, T, ns) != si) continue;
        const int fr = trn_frame(table, r, p, T);
#pragma unroll 4
        for (int cl = 0; cl < clips; ++cl) {
            const float g = dh[((long)r * clips + cl) * hidden + j];
            acc += g * fmaxf(f[((long)cl * T + fr) * fdim + d], 0.f);
            accb += g;
        }
    }
    if (k < K) sc.s[si].dw1[(long)j * K + k] = acc;
    if (k == 0) sc.s[si].db1[j] = accb;
}

// df[clip][t][d] = [f[clip][t][d] > 0] * sum over the table rows r that hold frame t at a position p, in table order (positions ascending), of
// sum_j dh[r][clip][j] * W1_s[j][p * fdim + d]: a gather per frame, no scatter.  64 d per workgroup, the hidden units in four quarters (one per wavefront).
__global__ __launch_bounds__(256) void trn_df_kernel(const float* dh, const float* f, TrnScales sc, int ns, const int* table, int rows, int clips, int T, int fdim,
                                                     int hidden, float* df) {
    __shared__ float red[4][64];
    const int cl = blockIdx.z, t = blockIdx.y, q = threadIdx.x >> 6, d = blockIdx.x * 64 + (threadIdx.x & 63), dd = min(d, fdim - 1);
    const int per = (hidden + 3) / 4, j0 = q * per, j1 = min(hidden, j0 + per);
    float acc = 0.f;
    for (int r = 0; r < rows; ++r) {
        const int si = trn_scale(table, r, T, ns), s = T - si;
        const long K = (long)s * fdim;
        const float* g = dh + ((long)r * clips + cl) * hidden;
        for (int p = 0; p < s; ++p) {
            if (trn_frame(table, r, p, T) != t) continue;
            const float* w = sc.s[si].w1 + (long)p * fdim + dd;
            float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
            int j = j0;
            for (; j + 8 <= j1; j += 8) {
#pragma unroll
                for (int u = 0; u < 8; ++u) a[u] += g[j + u] * w[(long)(j + u) * K];
            }
            for (; j < j1; ++j) a[0] += g[j] * w[(long)j * K];
            acc += tree8(a);
        }
    }
    acc = quarter_sum(acc, red);
    if (q == 0 && d < fdim) {
        const long o = ((long)cl * T + t) * fdim + d;
        df[o] = f[o] > 0.f ? acc : 0.f;
    }
}

// dfc_w[j][ch] = sum over the frames of df[frame][j] * pooled[frame][ch]; dfc_b[j] likewise of df[frame][j]: 64 ch per workgroup, the frames in four quarters
__global__ __launch_bounds__(256) void trn_dfc_kernel(const float* df, const float* pooled, int frames, int c, int fdim, float* dw, float* db) {
    __shared__ float red[4][64];
    const int j = blockIdx.y, q = threadIdx.x >> 6, ch = blockIdx.x * 64 + (threadIdx.x & 63), cc = min(ch, c - 1);
    const int per = (frames + 3) / 4, f1 = min(frames, (q + 1) * per);
    float acc = 0.f, accb = 0.f;
#pragma unroll 8
    for (int fr = q * per; fr < f1; ++fr) {
        const float g = df[(long)fr * fdim + j];
        acc += g * pooled[(long)fr * c + cc];
        accb += g;
    }
    acc = quarter_sum(acc, red);
    accb = quarter_sum(accb, red);
    if (q == 0 && ch < c) dw[(long)j * c + ch] = acc;
    if (threadIdx.x == 0 && blockIdx.x == 0) db[j] = accb;
}

// dpool[frame][ch] = (sum_j df[frame][j] * fc_w[j][ch]) / hw (x the dropout mask): the gradient of every pixel of the frame.  64 ch per workgroup, j in quarters.
__global__ __launch_bounds__(256) void trn_dpool_kernel(const float* df, const float* w, const float* drop_mask, int c, int fdim, int hw, float* dpool) {
    __shared__ float red[4][64];
    const int fr = blockIdx.y, q = threadIdx.x >> 6, ch = blockIdx.x * 64 + (threadIdx.x & 63), cc = min(ch, c - 1);
    const float* g = df + (long)fr * fdim;
    const int per = (fdim + 3) / 4, j1 = min(fdim, (q + 1) * per);
    float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    int j = q * per;
    for (; j + 8 <= j1; j += 8) {
#pragma unroll
        for (int u = 0; u < 8; ++u) a[u] += g[j + u] * w[(long)(j + u) * c + cc];
    }
    for (; j < j1; ++j) a[0] += g[j] * w[(long)j * c + cc];
    float acc = quarter_sum(tree8(a), red);
    if (q == 0 && ch < c) {
        acc = acc / (float)hw;             // one rounding, as the forward's mean
        if (drop_mask) acc *= drop_mask[(long)fr * c + ch];
        dpool[(long)fr * c + ch] = acc;
    }
}

template <typename ET>
__global__ void trn_dfeat_kernel(const float* dpool, int hw, int c, ET* dfeat) {
    const int frame = blockIdx.y, c4 = c >> 2, per = hw * c4;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < per; i += gridDim.x * blockDim.x) {
        const float4 v = *reinterpret_cast<const float4*>(dpool + (long)frame * c + (i % c4) * 4);
        st4(dfeat + ((long)frame * hw * c + (long)i * 4), v);
    }
}

inline void trn_rec_begin(int entry, int dtype) {
    t_last_trn = mvf_trn_launch_info_t{};
    t_last_trn.entry = entry;
    t_last_trn.dtype = dtype;
}

// the checks both entry points share, before any launch
int trn_check(const char* who, int clips, int t, int hw, int c, int fdim, const mvf_trn_scale_t* scales, int n_scales, int hidden, int classes, const int* table,
              int rows, int dtype, bool bwd) {
    MVF_REQUIRE(clips > 0 && t > 0 && hw > 0 && c > 0 && fdim > 0 && hidden > 0 && classes > 0 && rows > 0, MVF_EINVAL,
                "%s: bad argument (clips=%d t=%d hw=%d c=%d fdim=%d hidden=%d classes=%d rows=%d)", who, clips, t, hw, c, fdim, hidden, classes, rows);
    MVF_REQUIRE(dtype == MVF_F32 || dtype == MVF_BF16, MVF_EINVAL, "%s: dtype %d", who, dtype);
    MVF_REQUIRE(t >= 2 && t <= MVF_TRN_MAX_FRAMES, MVF_EUNSUPPORTED, "%s: t=%d outside [2, %d]", who, t, MVF_TRN_MAX_FRAMES);
    MVF_REQUIRE(n_scales >= 1 && n_scales <= t - 1, MVF_EINVAL, "%s: n_scales=%d outside [1, t - 1 = %d]", who, n_scales, t - 1);
    MVF_REQUIRE(scales && table, MVF_EINVAL, "%s: NULL scales / table", who);
    for (int i = 0; i < n_scales; ++i) {
        MVF_REQUIRE(scales[i].w1 && scales[i].b1 && scales[i].w2 && scales[i].b2, MVF_EINVAL, "%s: scale %d: NULL parameter", who, i);
        MVF_REQUIRE(!bwd || (scales[i].dw1 && scales[i].db1 && scales[i].dw2 && scales[i].db2), MVF_EINVAL, "%s: scale %d: NULL gradient destination", who, i);
    }
    MVF_REQUIRE(c % 4 == 0, MVF_ESHAPE, "%s: c=%d must be a multiple of 4", who, c);
    MVF_REQUIRE((long)clips * t <= 65535 && clips <= 65535 && classes <= 65535 && hidden <= 65535 && fdim <= 65535 && rows <= 1024, MVF_ESHAPE,
                "%s: %d clips x %d frames, %d classes, %d hidden, %d rows exceed the grid", who, clips, t, classes, hidden, rows);
    MVF_REQUIRE((long)clips * classes < (1L << 31) && (long)rows * clips * hidden < (1L << 40), MVF_ESHAPE, "%s: too large", who);
    return MVF_OK;
}

TrnScales pack_scales(const mvf_trn_scale_t* scales, int n) {
    TrnScales s = {};
    for (int i = 0; i < n; ++i) s.s[i] = scales[i];
    return s;
}

// K splits of the hidden GEMM: enough for about 256 workgroups, at most MVF_TRN_KSPLIT_MAX and never more than the shortest K has 128-element chunks
int hidden_splits(int clips, int hidden, int rows, int t, int n_scales, int fdim) {
    const long blocks = (long)((clips + kTM - 1) / kTM) * ((hidden + kTN - 1) / kTN) * rows;
    const int kmin = (t - (n_scales - 1)) * fdim;
    long s = (256 + blocks - 1) / blocks;
    s = std::min<long>(s, std::max(1, kmin / kBK));
    return (int)std::max<long>(1, std::min<long>(s, MVF_TRN_KSPLIT_MAX));
}

}  // namespace

extern "C" {

int mvf_trn_head_fwd(const void* feat, int clips, int t, int hw, int c, const float* fc_w, const float* fc_b, int fdim, const mvf_trn_scale_t* scales, int n_scales,
                     int hidden, int classes, const int* table, int rows, const float* drop_mask, float* pooled, float* f, float* h, float* hpart, float* scores,
                     int dtype, void* stream) {
    trn_rec_begin(MVF_TRN_ENTRY_FWD, dtype);
    const int rc = trn_check("trn_head_fwd", clips, t, hw, c, fdim, scales, n_scales, hidden, classes, table, rows, dtype, false);
    if (rc != MVF_OK) return rc;
    MVF_REQUIRE(feat && fc_w && pooled && f && h && hpart && scores, MVF_EINVAL, "trn_head_fwd: NULL argument");
    const int nsplit = hidden_splits(clips, hidden, rows, t, n_scales, fdim);
    MVF_REQUIRE((long)rows * nsplit <= 65535, MVF_ESHAPE, "trn_head_fwd: %d rows x %d splits exceed the grid", rows, nsplit);
    t_last_trn.rows = rows;
    t_last_trn.n_scales = n_scales;
    hipStream_t st = (hipStream_t)stream;
    const TrnScales sc = pack_scales(scales, n_scales);
    const int frames = clips * t;
    const dim3 gp((c + 255) / 256, frames);
    if (dtype == MVF_F32) hipLaunchKernelGGL(trn_pool_kernel<float>, gp, dim3(256), 0, st, (const float*)feat, hw, c, drop_mask, pooled);
    else hipLaunchKernelGGL(trn_pool_kernel<bf16_t>, gp, dim3(256), 0, st, (const bf16_t*)feat, hw, c, drop_mask, pooled);
    MVF_LAUNCH_CHECK();
    ++t_last_trn.launches;
    hipLaunchKernelGGL(trn_fc_kernel, dim3((frames + kTM - 1) / kTM, (fdim + kTN - 1) / kTN), dim3(256), 0, st, pooled, fc_w, fc_b, frames, c, fdim, f);
    MVF_LAUNCH_CHECK();
    ++t_last_trn.launches;
    hipLaunchKernelGGL(trn_hidden_part_kernel, dim3((clips + kTM - 1) / kTM, (hidden + kTN - 1) / kTN, rows * nsplit), dim3(256), 0, st, f, sc, n_scales, table, rows, nsplit,
                       clips, t, fdim, hidden, hpart);
    MVF_LAUNCH_CHECK();
    ++t_last_trn.launches;
    hipLaunchKernelGGL(trn_hidden_reduce_kernel, dim3((hidden + 255) / 256, clips, rows), dim3(256), 0, st, hpart, sc, n_scales, table, rows, nsplit, clips, t, hidden, h);
    MVF_LAUNCH_CHECK();
    ++t_last_trn.launches;
    hipLaunchKernelGGL(trn_scores_kernel, dim3((unsigned)(((long)clips * classes + 3) / 4)), dim3(256), 0, st, h, sc, n_scales, table, rows, clips, t, hidden, classes,
                       scores);
    MVF_LAUNCH_CHECK();
    ++t_last_trn.launches;
    return MVF_OK;
}

int mvf_trn_head_bwd(const float* dscores, const float* pooled, const float* f, const float* h, const float* fc_w, const mvf_trn_scale_t* scales, int n_scales,
                     int hidden, int classes, const int* table, int rows, const float* drop_mask, int clips, int t, int hw, int c, int fdim, float* dfc_w,
                     float* dfc_b, float* dh, float* df, float* dpool, void* dfeat, int dtype, void* stream) {
    trn_rec_begin(MVF_TRN_ENTRY_BWD, dtype);
    const int rc = trn_check("trn_head_bwd", clips, t, hw, c, fdim, scales, n_scales, hidden, classes, table, rows, dtype, true);
    if (rc != MVF_OK) return rc;
    MVF_REQUIRE(dscores && pooled && f && h && fc_w && dfc_w && dfc_b && dh && df && dpool && dfeat, MVF_EINVAL, "trn_head_bwd: NULL argument");
    MVF_REQUIRE(((uintptr_t)dpool & 15) == 0 && ((uintptr_t)dfeat & (dtype == MVF_F32 ? 15 : 7)) == 0, MVF_ESHAPE,
                "trn_head_bwd: dpool must be 16-byte aligned, dfeat 16-byte (fp32) / 8-byte (bf16)");
    t_last_trn.rows = rows;
    t_last_trn.n_scales = n_scales;
    hipStream_t st = (hipStream_t)stream;
    const TrnScales sc = pack_scales(scales, n_scales);
    const int frames = clips * t;
    hipLaunchKernelGGL(trn_dw2_kernel, dim3((hidden + 255) / 256, classes, n_scales), dim3(256), 0, st, dscores, h, sc, n_scales, table, rows, clips, t, hidden, classes);
    MVF_LAUNCH_CHECK();
    ++t_last_trn.launches;
    hipLaunchKernelGGL(trn_dh_kernel, dim3((hidden + 63) / 64, clips, rows), dim3(256), 0, st, dscores, h, sc, n_scales, table, clips, t, hidden, classes, dh);
    MVF_LAUNCH_CHECK();
    ++t_last_trn.launches;
    hipLaunchKernelGGL(trn_dw1_kernel, dim3((t * fdim + 255) / 256, hidden, n_scales), dim3(256), 0, st, dh, f, sc, n_scales, table, rows, clips, t, fdim, hidden);
    MVF_LAUNCH_CHECK();
    ++t_last_trn.launches;
    hipLaunchKernelGGL(trn_df_kernel, dim3((fdim + 63) / 64, t, clips), dim3(256), 0, st, dh, f, sc, n_scales, table, rows, clips, t, fdim, hidden, df);
    MVF_LAUNCH_CHECK();
    ++t_last_trn.launches;
    hipLaunchKernelGGL(trn_dfc_kernel, dim3((c + 63) / 64, fdim), dim3(256), 0, st, df, pooled, frames, c, fdim, dfc_w, dfc_b);
    MVF_LAUNCH_CHECK();
    ++t_last_trn.launches;
    hipLaunchKernelGGL(trn_dpool_kernel, dim3((c + 63) / 64, frames), dim3(256), 0, st, df, fc_w, drop_mask, c, fdim, hw, dpool);
    MVF_LAUNCH_CHECK();
    ++t_last_trn.launches;
    const dim3 gdf((unsigned)std::min<long>(((long)hw * (c / 4) + 255) / 256, 64), (unsigned)frames);
    if (dtype == MVF_F32) hipLaunchKernelGGL(trn_dfeat_kernel<float>, gdf, dim3(256), 0, st, dpool, hw, c, (float*)dfeat);
    else hipLaunchKernelGGL(trn_dfeat_kernel<bf16_t>, gdf, dim3(256), 0, st, dpool, hw, c, (bf16_t*)dfeat);
    MVF_LAUNCH_CHECK();
    ++t_last_trn.launches;
    return MVF_OK;
}

int mvf_trn_head_last_launch(mvf_trn_launch_info_t* out) {
    MVF_REQUIRE(out, MVF_EINVAL, "trn_head_last_launch: NULL argument");
    *out = t_last_trn;
    return MVF_OK;
}

}  // extern "C"
