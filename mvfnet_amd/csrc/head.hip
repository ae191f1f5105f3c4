// The TSN classification head: per-frame average pool -> fc -> mean over segments, for training (with the cross-entropy losses and the backward) and for
// inference (with clip averaging).  Reference semantics: TSNClsHead.forward + BaseHead.loss (heads/tsn_clshead.py:71-98, heads/base.py:40-45).
//
// Training: the four fused forward forms (mvf_head_train_fwd, _soft, _bce, _focal) are ONE argument check (head_fwd_check), ONE pair of score launches
// (head_scores_launch: frame_pool_kernel, head_fc_seg_kernel) and the form's own loss launches -- ce_launch here, bce_launch / focal_launch in bce.hip /
// focal.hip, which stay translation units of their own because they switch floating-point contraction off.  This file is compiled with contraction on.
// Every sum has a fixed order: no atomics, bit-identical from run to run.
#include <algorithm>
#include <math.h>

#include "common.h"

namespace {

// ---- training: per-frame avg-pool -> fc -> mean over segments -> cross-entropy (mean over clips) ----
// pooled[frame][ch] = mean over hw ; lanes along channels
template <typename ET>
__global__ void frame_pool_kernel(const ET* feat, int hw, int c, const float* drop_mask, float* pooled) {
    const int f = blockIdx.y, ch = blockIdx.x * blockDim.x + threadIdx.x;
    if (ch >= c) return;
    const ET* p = feat + (long)f * hw * c + ch;
    float s = 0.f;
    for (int r = 0; r < hw; ++r) s += ldf(p + (long)r * c);
    s = s / (float)hw;
    if (drop_mask) s *= drop_mask[(long)f * c + ch];      // nn.Dropout: mask already scaled by 1/(1-p) (tsn_clshead.py:86-87)
    pooled[(long)f * c + ch] = s;
}

// frame-level fc + segment mean (training keeps per-frame pooled features for the weight gradient)
// fc per frame, then consensus mean over the clip's T frames (tsn_clshead.py:92-96) -- both linear, so the clip's mean feature is
// formed once in LDS (fixed t order) and every class is one dot product with it: T x fewer multiply-adds and, with a workgroup per
// (clip, class range) instead of a wave per (clip, class), 8 x less L2 traffic than re-reading the T frame rows for every class
// (137 -> ~20 us at 32 clips x 400 classes x 2048 channels).
constexpr int kHeadSplit = 25;      // class ranges per clip (16 classes per workgroup at 400 classes: 4 per wave, all in flight)
__global__ __launch_bounds__(256) void head_fc_seg_kernel(const float* pooled, const float* w, const float* b, int clips, int T, int c, int classes, float* scores) {
    extern __shared__ float pc[];                   // [c] the clip's mean pooled feature
    const int clip = blockIdx.x, part = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float inv = 1.f / (float)T;
    for (int i = tid; i < c; i += 256) {
        float s = 0.f;
        for (int t = 0; t < T; ++t) s += pooled[((long)clip * T + t) * c + i];
        pc[i] = s * inv;
    }
    __syncthreads();
    const int per = (classes + kHeadSplit - 1) / kHeadSplit;
    const int k_end = min(classes, (part + 1) * per);
    // a wave takes classes k, k+4, k+8, k+12 of the range together: four independent dot products keep four weight rows in flight
    const int kb = part * per + wave;
    float s[4] = {0.f, 0.f, 0.f, 0.f};
    for (int i = lane; i < c; i += 64) {
        const float f = pc[i];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int k = kb + 4 * u;
            s[u] += f * w[(long)(k < k_end ? k : kb < k_end ? kb : 0) * c + i];       // clamped row: unconditional load
        }
    }
    for (int u0 = 0; u0 * 16 < per; ++u0) {            // ranges longer than 16 classes: further rounds of four
        if (u0 > 0) {
#pragma unroll
            for (int u = 0; u < 4; ++u) s[u] = 0.f;
            for (int i = lane; i < c; i += 64) {
                const float f = pc[i];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const int k = kb + 16 * u0 + 4 * u;
                    s[u] += f * w[(long)(k < k_end ? k : 0) * c + i];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            float v = s[u];
            for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
            const int k = kb + 16 * u0 + 4 * u;
            if (lane == 0 && k < k_end) scores[(long)clip * classes + k] = v + (b ? b[k] : 0.f);
        }
    }
}

// one block per clip: softmax CE of scores[clip] against label; writes loss contribution and dscores = (p - onehot)/clips
__global__ void ce_loss_kernel(const float* scores, const long long* labels, int clips, int classes, float* loss_part, float* dscores) {
    __shared__ float red[256];
    const int cl = blockIdx.x, tid = threadIdx.x;
    const float* s = scores + (long)cl * classes;
    float mx = -INFINITY;
    for (int k = tid; k < classes; k += blockDim.x) mx = fmaxf(mx, s[k]);
    red[tid] = mx;
    __syncthreads();
    for (int o = blockDim.x >> 1; o > 0; o >>= 1) { if (tid < o) red[tid] = fmaxf(red[tid], red[tid + o]); __syncthreads(); }
    mx = red[0];
    __syncthreads();
    float e = 0.f;
    for (int k = tid; k < classes; k += blockDim.x) e += expf(s[k] - mx);
    red[tid] = e;
    __syncthreads();
    for (int o = blockDim.x >> 1; o > 0; o >>= 1) { if (tid < o) red[tid] += red[tid + o]; __syncthreads(); }
    const float den = red[0];
    const int lab = (int)labels[cl];
    if (tid == 0) loss_part[cl] = (logf(den) + mx) - s[lab];
    if (!dscores) return;
    for (int k = tid; k < classes; k += blockDim.x) {
        const float p = expf(s[k] - mx) / den;
        dscores[(long)cl * classes + k] = (p - (k == lab ? 1.f : 0.f)) / (float)clips;
    }
}

// the same against a row of soft targets t (any non-negative fp32 row, not assumed to sum to 1: blended and / or smoothed labels, mvf_soft_targets):
// loss = sum_k t_k * (lse - s_k) -- exactly 0 for one class --, dscores = (softmax * sum_k t_k - t) / clips.  Fixed-order block reductions: deterministic.
__global__ void ce_loss_soft_kernel(const float* scores, const float* targets, int clips, int classes, float* loss_part, float* dscores) {
    __shared__ float red[256];
    const int cl = blockIdx.x, tid = threadIdx.x;
    const float* s = scores + (long)cl * classes;
    const float* tg = targets + (long)cl * classes;
    float mx = -INFINITY;
    for (int k = tid; k < classes; k += blockDim.x) mx = fmaxf(mx, s[k]);
    red[tid] = mx;
    __syncthreads();
    for (int o = blockDim.x >> 1; o > 0; o >>= 1) { if (tid < o) red[tid] = fmaxf(red[tid], red[tid + o]); __syncthreads(); }
    mx = red[0];
    __syncthreads();
    float e = 0.f;
    for (int k = tid; k < classes; k += blockDim.x) e += expf(s[k] - mx);
    red[tid] = e;
    __syncthreads();
    for (int o = blockDim.x >> 1; o > 0; o >>= 1) { if (tid < o) red[tid] += red[tid + o]; __syncthreads(); }
    const float den = red[0];
    __syncthreads();
    const float lse = logf(den) + mx;
    float acc = 0.f, tsum = 0.f;
    for (int k = tid; k < classes; k += blockDim.x) {
        const float tk = tg[k];
        acc += tk * (lse - s[k]);
        tsum += tk;
    }
    red[tid] = acc;
    __syncthreads();
    for (int o = blockDim.x >> 1; o > 0; o >>= 1) { if (tid < o) red[tid] += red[tid + o]; __syncthreads(); }
    if (tid == 0) loss_part[cl] = red[0];
    if (!dscores) return;
    __syncthreads();
    red[tid] = tsum;
    __syncthreads();
    for (int o = blockDim.x >> 1; o > 0; o >>= 1) { if (tid < o) red[tid] += red[tid + o]; __syncthreads(); }
    tsum = red[0];
    for (int k = tid; k < classes; k += blockDim.x) {
        const float p = expf(s[k] - mx) / den;
        dscores[(long)cl * classes + k] = (p * tsum - tg[k]) / (float)clips;
    }
}

// one thread, clips in ascending order (the fp64 losses' wave mean of loss_common.h orders its sum differently: the two are not interchangeable bit for bit)
__global__ void mean_reduce_kernel(const float* v, int n, float* out) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        double s = 0.0;
        for (int i = 0; i < n; ++i) s += v[i];
        out[0] = (float)(s / n);
    }
}

// dW[k][c] = sum_clip dscores[clip][k] * pooledclip[clip][c] ; db[k] = sum_clip dscores[clip][k]   (pooledclip = mean over T)
// thread = one channel, workgroup = (256 channels, kHeadKc classes): the channel's clip-mean features are formed once per thread
// (clips are walked in chunks of 16 registers) and reused for every class of the range, instead of re-reading the T frame rows for
// each of the 400 classes (69 -> ~15 us).  Fixed clip order: deterministic.
constexpr int kHeadKc = 4;
__global__ void head_clipmean_kernel(const float* pooled, int T, int c, float* pcm) {
    const int cl = blockIdx.y, ch = blockIdx.x * blockDim.x + threadIdx.x;
    if (ch >= c) return;
    float s = 0.f;
    for (int t = 0; t < T; ++t) s += pooled[((long)cl * T + t) * c + ch];
    pcm[(long)cl * c + ch] = s / (float)T;
}
__global__ __launch_bounds__(256) void head_fc_bwd_w_kernel(const float* dscores, const float* pcm, int clips, int T, int c, int classes, float* dw, float* db) {
    const int k0 = blockIdx.y * kHeadKc, ch = blockIdx.x * blockDim.x + threadIdx.x;
    const int nk = min(kHeadKc, classes - k0);
    if (ch < c) {
        float acc[kHeadKc];
#pragma unroll
        for (int j = 0; j < kHeadKc; ++j) acc[j] = 0.f;
        for (int cl0 = 0; cl0 < clips; cl0 += 16) {
            float pcv[16];
#pragma unroll
            for (int q = 0; q < 16; ++q) pcv[q] = pcm[(long)min(cl0 + q, clips - 1) * c + ch];      // clamped: unconditional loads
#pragma unroll
            for (int j = 0; j < kHeadKc; ++j) {
                if (j < nk) {
#pragma unroll
                    for (int q = 0; q < 16; ++q)
                        if (cl0 + q < clips) acc[j] += dscores[(long)(cl0 + q) * classes + k0 + j] * pcv[q];
                }
            }
        }
#pragma unroll
        for (int j = 0; j < kHeadKc; ++j)
            if (j < nk) dw[(long)(k0 + j) * c + ch] = acc[j];
    }
    if (blockIdx.x == 0 && threadIdx.x < nk) {
        float s = 0.f;
        for (int cl = 0; cl < clips; ++cl) s += dscores[(long)cl * classes + k0 + threadIdx.x];
        db[k0 + threadIdx.x] = s;
    }
}

// dfeat[frame][hw][ch] = (1/(T*hw)) * sum_k dscores[clip][k] * W[k][ch]
__global__ void head_dpool_kernel(const float* dscores, const float* w, int classes, int c, float scale, float* dpool) {
    const int cl = blockIdx.y, ch = blockIdx.x * blockDim.x + threadIdx.x;
    if (ch >= c) return;
    // eight independent accumulators: the class loop is a chain of L2 round trips otherwise (81 -> ~15 us)
    float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const float* ds = dscores + (long)cl * classes;
    int k = 0;
    for (; k + 8 <= classes; k += 8) {
#pragma unroll
        for (int u = 0; u < 8; ++u) a[u] += ds[k + u] * w[(long)(k + u) * c + ch];
    }
    for (; k < classes; ++k) a[0] += ds[k] * w[(long)k * c + ch];
    dpool[(long)cl * c + ch] = (((a[0] + a[1]) + (a[2] + a[3])) + ((a[4] + a[5]) + (a[6] + a[7]))) * scale;
}
template <typename ET>
__global__ void head_dfeat_kernel(const float* dpool, const float* drop_mask, int T, int hw, int c, long total, ET* dfeat) {
    // blockIdx.y = frame, threads over (row, 4 channels): the frame's gradient row (dpool x mask) is the same for its hw pixels
    const int frame = blockIdx.y, c4 = c >> 2;
    const int per = hw * c4;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < per; i += gridDim.x * blockDim.x) {
        const int q = i % c4;
        float4 v = *reinterpret_cast<const float4*>(dpool + (long)(frame / T) * c + q * 4);
        if (drop_mask) {
            const float4 mk = *reinterpret_cast<const float4*>(drop_mask + (long)frame * c + q * 4);
            v.x *= mk.x; v.y *= mk.y; v.z *= mk.z; v.w *= mk.w;
        }
        st4(dfeat + ((long)frame * hw * c + (long)i * 4), v);
    }
}

// ---- inference: clip-level avg-pool -> fc, clip averaging ----
// pooled[clip][ch] = mean over the clip's T*HW feature rows; lanes along channels (coalesced rows)
// workgroup = 64 channels (16 lanes x 4) x 16 row lanes: 8/16-byte loads, four rows in flight per thread, the 16 row-lane sums
// combined in lane order through LDS (fixed order).  The one-thread-per-channel form walked the clip's 392 rows serially with
// 2-byte loads from 128 workgroups: 134 us for 51 MB.
template <typename ET>
__global__ __launch_bounds__(256) void head_pool_kernel(const ET* feat, int rows_per_clip, int c, float* pooled) {
    __shared__ float4 red[256];
    const int clip = blockIdx.y, q = threadIdx.x & 15, rl = threadIdx.x >> 4;
    const int ch = (blockIdx.x * 16 + q) * 4;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    if (ch < c) {
        const ET* p = feat + (long)clip * rows_per_clip * c + ch;
        int r = rl;
        for (; r + 48 < rows_per_clip; r += 64) {
            const float4 a = ld4(p + (long)r * c), b = ld4(p + (long)(r + 16) * c), d = ld4(p + (long)(r + 32) * c), e = ld4(p + (long)(r + 48) * c);
            s.x += (a.x + b.x) + (d.x + e.x); s.y += (a.y + b.y) + (d.y + e.y);
            s.z += (a.z + b.z) + (d.z + e.z); s.w += (a.w + b.w) + (d.w + e.w);
        }
        for (; r < rows_per_clip; r += 16) {
            const float4 a = ld4(p + (long)r * c);
            s.x += a.x; s.y += a.y; s.z += a.z; s.w += a.w;
        }
    }
    red[threadIdx.x] = s;
    __syncthreads();
    if (rl == 0 && ch < c) {
        float4 t = red[q];
        for (int l = 1; l < 16; ++l) {
            const float4 v = red[l * 16 + q];
            t.x += v.x; t.y += v.y; t.z += v.z; t.w += v.w;
        }
        const float inv = 1.f / (float)rows_per_clip;
        *reinterpret_cast<float4*>(pooled + (long)clip * c + ch) = make_float4(t.x * inv, t.y * inv, t.z * inv, t.w * inv);
    }
}

// scores[clip][k] = b[k] + pooled[clip] . W[k]; one wave per (clip, class)
__global__ void head_fc_kernel(const float* pooled, const float* w, const float* b, int clips, int c, int classes,
                               float* scores) {
    const int gw = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
    if (gw >= clips * classes) return;
    const int clip = gw / classes, k = gw - clip * classes;
    const float* p = pooled + (long)clip * c;
    const float* wr = w + (long)k * c;
    float s = 0.f;
    for (int i = lane; i < c; i += 64) s += p[i] * wr[i];
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (lane == 0) scores[gw] = s + (b ? b[k] : 0.f);
}

// average_clip: kind 1 = mean of scores over clips, kind 2 = mean of softmax(scores) over clips; one block
__global__ void average_clip_kernel(const float* scores, int clips, int classes, int kind, float* out) {
    __shared__ float red[256];
    const int tid = threadIdx.x;
    for (int k = tid; k < classes; k += blockDim.x) out[k] = 0.f;
    __syncthreads();
    for (int cl = 0; cl < clips; ++cl) {
        const float* s = scores + (long)cl * classes;
        float mx = -INFINITY, den = 1.f;
        if (kind == 2) {
            for (int k = tid; k < classes; k += blockDim.x) mx = fmaxf(mx, s[k]);
            red[tid] = mx;
            __syncthreads();
            for (int o = blockDim.x >> 1; o > 0; o >>= 1) {
                if (tid < o) red[tid] = fmaxf(red[tid], red[tid + o]);
                __syncthreads();
            }
            mx = red[0];
            __syncthreads();
            float e = 0.f;
            for (int k = tid; k < classes; k += blockDim.x) e += expf(s[k] - mx);
            red[tid] = e;
            __syncthreads();
            for (int o = blockDim.x >> 1; o > 0; o >>= 1) {
                if (tid < o) red[tid] += red[tid + o];
                __syncthreads();
            }
            den = red[0];
            __syncthreads();
        }
        for (int k = tid; k < classes; k += blockDim.x) {
            const float v = kind == 2 ? expf(s[k] - mx) / den : s[k];
            out[k] += v;
        }
    }
    for (int k = tid; k < classes; k += blockDim.x) out[k] = out[k] / (float)clips;
}

// average_clips = 'sigmoid': out[k] = mean over the clips of sigmoid(s[cl][k]).  One thread per class, clips in ascending order, fp64 (exp(-|s|) <= 1 for
// either sign, so nothing overflows), rounded to fp32 once.
__global__ void average_clip_sigmoid_kernel(const float* __restrict__ scores, int clips, int classes, float* __restrict__ out) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= classes) return;
    double acc = 0.0;
    for (int cl = 0; cl < clips; ++cl) {
        const double s = (double)scores[(long)cl * classes + k];
        const double e = exp(-fabs(s));
        acc += s != s ? s : (s >= 0.0 ? 1.0 / (1.0 + e) : e / (1.0 + e));
    }
    out[k] = (float)(acc / (double)clips);
}

constexpr int kMaxGridY = 65535;

// What every fused forward form (mvf_head_train_fwd, _soft, _bce, _focal) requires of the arguments of its score launches, before any launch.
int head_fwd_check(const char* who, const void* feat, int clips, int t, int hw, int c, const float* fc_w, int classes, const float* pooled, const float* dscores,
                   int dtype) {
    MVF_REQUIRE(clips > 0 && t > 0 && hw > 0 && c > 0 && classes > 0, MVF_EINVAL, "%s: bad argument (clips=%d t=%d hw=%d c=%d classes=%d)", who, clips, t, hw, c,
                classes);
    MVF_REQUIRE(dtype == MVF_F32 || dtype == MVF_BF16, MVF_EINVAL, "%s: dtype %d", who, dtype);
    MVF_REQUIRE((size_t)c * sizeof(float) <= 160 * 1024, MVF_EUNSUPPORTED, "%s: c=%d does not fit the LDS feature buffer", who, c);
    MVF_REQUIRE((long)clips * t <= kMaxGridY, MVF_ESHAPE, "%s: %d x %d frames exceed the grid", who, clips, t);
    MVF_REQUIRE(feat && fc_w && pooled && dscores, MVF_EINVAL, "%s: NULL argument", who);
    return MVF_OK;
}

// the NULL and c % 4 tests mvf_head_train_bwd has always made, in their order, then the dtype and the three grids
int head_bwd_check(const float* dscores, const float* pooled, const float* fc_w, int clips, int t, int c, int classes, const float* dfc_w, const float* dfc_b,
                   const float* dpool_ws, const void* dfeat, int dtype) {
    MVF_REQUIRE(dscores && pooled && fc_w && dfc_w && dfc_b && dpool_ws && dfeat, MVF_EINVAL, "head_train_bwd: NULL argument");
    MVF_REQUIRE(c % 4 == 0, MVF_ESHAPE, "head_train_bwd: c=%d must be a multiple of 4", c);
    MVF_REQUIRE(dtype == MVF_F32 || dtype == MVF_BF16, MVF_EINVAL, "head_train_bwd: dtype %d", dtype);
    MVF_REQUIRE((long)clips * t <= kMaxGridY, MVF_ESHAPE, "head_train_bwd: %d x %d frames exceed the grid", clips, t);
    MVF_REQUIRE(clips <= kMaxGridY && (classes + 3) / 4 <= kMaxGridY, MVF_ESHAPE, "head_train_bwd: clips=%d / classes=%d exceed the grid", clips, classes);
    return MVF_OK;
}

// pooled (clips * t, c) and scores (clips, classes): the two launches every fused forward form starts with
int head_scores_launch(const void* feat, int clips, int t, int hw, int c, const float* fc_w, const float* fc_b, int classes, const float* drop_mask, float* pooled,
                       float* scores, int dtype, hipStream_t st) {
    const dim3 g((c + 255) / 256, clips * t);
    if (dtype == MVF_F32) hipLaunchKernelGGL(frame_pool_kernel<float>, g, dim3(256), 0, st, (const float*)feat, hw, c, drop_mask, pooled);
    else hipLaunchKernelGGL(frame_pool_kernel<bf16_t>, g, dim3(256), 0, st, (const bf16_t*)feat, hw, c, drop_mask, pooled);
    MVF_LAUNCH_CHECK();
    hipLaunchKernelGGL(head_fc_seg_kernel, dim3(clips, kHeadSplit), dim3(256), (size_t)c * sizeof(float), st, pooled, fc_w, fc_b, clips, t, c, classes, scores);
    MVF_LAUNCH_CHECK();
    return MVF_OK;
}

// cross-entropy against integer labels (targets NULL) or against soft targets (labels NULL), then the mean over the clips
int ce_launch(const float* scores, const long long* labels, const float* targets, int clips, int classes, float* dscores, float* loss_part, float* loss,
              hipStream_t st) {
    if (labels) hipLaunchKernelGGL(ce_loss_kernel, dim3(clips), dim3(256), 0, st, scores, labels, clips, classes, loss_part, dscores);
    else hipLaunchKernelGGL(ce_loss_soft_kernel, dim3(clips), dim3(256), 0, st, scores, targets, clips, classes, loss_part, dscores);
    MVF_LAUNCH_CHECK();
    hipLaunchKernelGGL(mean_reduce_kernel, dim3(1), dim3(64), 0, st, loss_part, clips, loss);
    MVF_LAUNCH_CHECK();
    return MVF_OK;
}

}  // namespace

extern "C" {

// head, training: feat (clips*T, hw, c) -> pooled (clips*T, c) fp32 [kept for backward] -> scores (clips, classes) -> loss
int mvf_head_train_fwd(const void* feat, int clips, int t, int hw, int c, const float* fc_w, const float* fc_b, int classes,
                       const long long* labels, const float* drop_mask, float* pooled, float* scores, float* dscores, float* loss_part, float* loss,
                       int dtype, void* stream) {
    int rc = head_fwd_check("head_train_fwd", feat, clips, t, hw, c, fc_w, classes, pooled, dscores, dtype);
    if (rc != MVF_OK) return rc;
    MVF_REQUIRE(labels && scores && loss_part && loss, MVF_EINVAL, "head_train_fwd: NULL argument");
    rc = head_scores_launch(feat, clips, t, hw, c, fc_w, fc_b, classes, drop_mask, pooled, scores, dtype, (hipStream_t)stream);
    return rc != MVF_OK ? rc : ce_launch(scores, labels, nullptr, clips, classes, dscores, loss_part, loss, (hipStream_t)stream);
}

// ... against soft targets (clips, classes) instead of integer labels
int mvf_head_train_fwd_soft(const void* feat, int clips, int t, int hw, int c, const float* fc_w, const float* fc_b, int classes,
                            const float* targets, const float* drop_mask, float* pooled, float* scores, float* dscores, float* loss_part, float* loss,
                            int dtype, void* stream) {
    int rc = head_fwd_check("head_train_fwd_soft", feat, clips, t, hw, c, fc_w, classes, pooled, dscores, dtype);
    if (rc != MVF_OK) return rc;
    MVF_REQUIRE(targets && scores && loss_part && loss, MVF_EINVAL, "head_train_fwd_soft: NULL argument");
    rc = head_scores_launch(feat, clips, t, hw, c, fc_w, fc_b, classes, drop_mask, pooled, scores, dtype, (hipStream_t)stream);
    return rc != MVF_OK ? rc : ce_launch(scores, nullptr, targets, clips, classes, dscores, loss_part, loss, (hipStream_t)stream);
}

// ... with the binary cross-entropy of mvf_bce_loss (bce.hip)
int mvf_head_train_fwd_bce(const void* feat, int clips, int t, int hw, int c, const float* fc_w, const float* fc_b, int classes,
                           const float* targets, const float* drop_mask, const float* pos_weight, float target_threshold, int sum_classes,
                           float* pooled, float* scores, float* dscores, float* loss_part, float* loss, int dtype, void* stream) {
    int rc = head_fwd_check("head_train_fwd_bce", feat, clips, t, hw, c, fc_w, classes, pooled, dscores, dtype);
    if (rc == MVF_OK) rc = mvf_internal::bce_check("head_train_fwd_bce", scores, targets, clips, classes, target_threshold, sum_classes, loss_part, loss);
    if (rc == MVF_OK) rc = head_scores_launch(feat, clips, t, hw, c, fc_w, fc_b, classes, drop_mask, pooled, scores, dtype, (hipStream_t)stream);
    if (rc != MVF_OK) return rc;
    return mvf_internal::bce_launch(scores, targets, clips, classes, pos_weight, target_threshold, sum_classes, dscores, loss_part, loss, (hipStream_t)stream);
}

// ... with the focal / asymmetric loss of mvf_focal_loss (focal.hip); prm is read here, on the host
int mvf_head_train_fwd_focal(const void* feat, int clips, int t, int hw, int c, const float* fc_w, const float* fc_b, int classes,
                             const float* targets, const float* drop_mask, const float* class_weight, const mvf_focal_params_t* prm,
                             float* pooled, float* scores, float* dscores, float* loss_part, float* loss, int dtype, void* stream) {
    int rc = head_fwd_check("head_train_fwd_focal", feat, clips, t, hw, c, fc_w, classes, pooled, dscores, dtype);
    if (rc == MVF_OK) rc = mvf_internal::focal_check("head_train_fwd_focal", scores, targets, clips, classes, prm, loss_part, loss);
    if (rc == MVF_OK) rc = head_scores_launch(feat, clips, t, hw, c, fc_w, fc_b, classes, drop_mask, pooled, scores, dtype, (hipStream_t)stream);
    if (rc != MVF_OK) return rc;
    return mvf_internal::focal_launch(scores, targets, clips, classes, class_weight, *prm, dscores, loss_part, loss, (hipStream_t)stream);
}

int mvf_ce_loss(const float* scores, const long long* labels, int clips, int classes, float* dscores, float* loss_part, float* loss, void* stream) {
    MVF_REQUIRE(scores && labels && loss_part && loss && clips > 0 && classes > 0, MVF_EINVAL, "ce_loss: bad argument");
    return ce_launch(scores, labels, nullptr, clips, classes, dscores, loss_part, loss, (hipStream_t)stream);
}

int mvf_ce_loss_soft(const float* scores, const float* targets, int clips, int classes, float* dscores, float* loss_part, float* loss, void* stream) {
    MVF_REQUIRE(clips > 0 && classes > 0, MVF_EINVAL, "ce_loss_soft: bad argument (clips=%d classes=%d)", clips, classes);
    MVF_REQUIRE(scores && targets && loss_part && loss, MVF_EINVAL, "ce_loss_soft: NULL argument");
    return ce_launch(scores, nullptr, targets, clips, classes, dscores, loss_part, loss, (hipStream_t)stream);
}

int mvf_head_train_bwd(const float* dscores, const float* pooled, const float* fc_w, const float* drop_mask, int clips, int t, int hw, int c, int classes,
                       float* dfc_w, float* dfc_b, float* dpool_ws, void* dfeat, int dtype, void* stream) {
    const int rc = head_bwd_check(dscores, pooled, fc_w, clips, t, c, classes, dfc_w, dfc_b, dpool_ws, dfeat, dtype);
    if (rc != MVF_OK) return rc;
    hipStream_t st = (hipStream_t)stream;
    // the clips' mean features borrow dpool_ws ([clips][c] floats), which the NEXT kernel of this call overwrites with its real content
    float* pcm = dpool_ws;
    hipLaunchKernelGGL(head_clipmean_kernel, dim3((c + 255) / 256, clips), dim3(256), 0, st, pooled, t, c, pcm);
    MVF_LAUNCH_CHECK();
    hipLaunchKernelGGL(head_fc_bwd_w_kernel, dim3((c + 255) / 256, (classes + kHeadKc - 1) / kHeadKc), dim3(256), 0, st, dscores, pcm, clips, t, c, classes, dfc_w, dfc_b);
    MVF_LAUNCH_CHECK();
    hipLaunchKernelGGL(head_dpool_kernel, dim3((c + 255) / 256, clips), dim3(256), 0, st, dscores, fc_w, classes, c, 1.0f / ((float)t * hw), dpool_ws);
    MVF_LAUNCH_CHECK();
    const long total = (long)clips * t * hw * c;
    const dim3 gdf((unsigned)std::min<long>(((long)hw * (c / 4) + 255) / 256, 64), (unsigned)(clips * t));
    if (dtype == MVF_F32) hipLaunchKernelGGL(head_dfeat_kernel<float>, gdf, dim3(256), 0, st, dpool_ws, drop_mask, t, hw, c, total, (float*)dfeat);
    else hipLaunchKernelGGL(head_dfeat_kernel<bf16_t>, gdf, dim3(256), 0, st, dpool_ws, drop_mask, t, hw, c, total, (bf16_t*)dfeat);
    MVF_LAUNCH_CHECK();
    return MVF_OK;
}

// head, inference: feat (clips*T, hw, c) -> pooled_ws (clips, c) fp32 -> scores (clips, classes)
int mvf_head_pool_fc(const void* feat, int clips, int t, int hw, int c, const float* fc_w, const float* fc_b, int classes,
                     float* pooled_ws, float* scores, int dtype, void* stream) {
    MVF_REQUIRE(feat && fc_w && pooled_ws && scores && clips > 0 && t > 0 && hw > 0 && c > 0 && classes > 0, MVF_EINVAL, "head_pool_fc: bad argument");
    hipStream_t st = (hipStream_t)stream;
    MVF_REQUIRE(c % 4 == 0, MVF_ESHAPE, "head_pool_fc: c=%d must be a multiple of 4", c);
    dim3 g((c + 63) / 64, clips);
    if (dtype == MVF_F32)
        hipLaunchKernelGGL(head_pool_kernel<float>, g, dim3(256), 0, st, (const float*)feat, t * hw, c, pooled_ws);
    else
        hipLaunchKernelGGL(head_pool_kernel<bf16_t>, g, dim3(256), 0, st, (const bf16_t*)feat, t * hw, c, pooled_ws);
    MVF_LAUNCH_CHECK();
    const long waves = (long)clips * classes;
    hipLaunchKernelGGL(head_fc_kernel, dim3((int)((waves * 64 + 255) / 256)), dim3(256), 0, st, pooled_ws, fc_w, fc_b, clips, c, classes, scores);
    MVF_LAUNCH_CHECK();
    return MVF_OK;
}

int mvf_average_clip(const float* scores, int clips, int classes, int kind, float* out, void* stream) {
    MVF_REQUIRE(scores && out && clips > 0 && classes > 0 && kind >= 0 && kind <= 2, MVF_EINVAL, "average_clip: bad argument");
    if (kind == 0) {
        MVF_HIP_OK(hipMemcpyAsync(out, scores, sizeof(float) * clips * classes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
        return MVF_OK;
    }
    hipLaunchKernelGGL(average_clip_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, scores, clips, classes, kind, out);
    MVF_LAUNCH_CHECK();
    return MVF_OK;
}

int mvf_average_clip_sigmoid(const float* scores, int clips, int classes, float* out, void* stream) {
    MVF_REQUIRE(scores && out && clips > 0 && classes > 0, MVF_EINVAL, "average_clip_sigmoid: bad argument (clips=%d classes=%d)", clips, classes);
    hipLaunchKernelGGL(average_clip_sigmoid_kernel, dim3((classes + 255) / 256), dim3(256), 0, (hipStream_t)stream, scores, clips, classes, out);
    MVF_LAUNCH_CHECK();
    return MVF_OK;
}

}  // extern "C"
