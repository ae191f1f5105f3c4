// Bandwidth-bound companions of the conv stack: stem input re-layout, max-pool, TSN head, clip averaging.
#include <algorithm>
#include <math.h>

#include "common.h"

namespace {

// (n,c<=4,h,w) fp32 NCHW -> zero-padded NHWC4: out[n][ih+pad][iw+pad][0..3]; lanes run along w (coalesced reads
// of each colour plane, 16-B/8-B stores).
// grid.x = (image, padded row), threads along the padded row: no per-element 64-bit division, and the colour-plane loads are
// unconditional on a clamped address (zeroed by a select) so the three of a pixel share one round trip
template <typename ET>
__global__ void stem_prep_kernel(const float* x, int n, int c, int h, int w, int pad, int hp, int wp, ET* out) {
    const int row = blockIdx.x, img = row / hp, yo = row - img * hp;
    const int ih = yo - pad;
    const bool rok = ih >= 0 && ih < h;
    const float* xi = x + ((long)img * c * h + (rok ? ih : 0)) * w;
    for (int xo = threadIdx.x; xo < wp; xo += blockDim.x) {
        const int iw = xo - pad;
        const bool ok = rok && iw >= 0 && iw < w;
        const int iwc = ok ? iw : 0;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float t = x ? xi[(long)(k < c ? k : 0) * h * w + iwc] : 0.f;
            v[k] = (ok && k < c) ? t : 0.f;
        }
        st4(out + ((long)row * wp + xo) * 4, make_float4(v[0], v[1], v[2], v[3]));
    }
}

// Decoded uint8 HWC frames -> normalised stem operand (and / or the reference's fp32 NCHW tensor): window (crop), mirror (flip),
// channel order (to_rgb), (float(px) [/ 255] - mean) * stdinv in two rounded fp32 steps (the reference subtracts, then multiplies
// by 1/std: no FMA), channels-first stacking.  Thread = one pixel of the padded stem image; 3 byte loads, one 8/16-byte store.
struct FramePrep {
    float mean[3], stdinv[3];
    int to_rgb, div_255;
};
template <typename ET>
__global__ void frames_prep_kernel(const unsigned char* frames, int n, int hs, int ws, const int* win, int h, int w, FramePrep fp,
                                   int pad, int hp, int wp, ET* out_stem, float* out_nchw) {
    const long total = (long)n * hp * wp;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int xo = (int)(i % wp);
        const long t = i / wp;
        const int yo = (int)(t % hp);
        const int img = (int)(t / hp);
        const int ih = yo - pad, iw = xo - pad;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        const bool inside = ih >= 0 && ih < h && iw >= 0 && iw < w;
        if (inside) {
            const int y0 = win ? win[img * 3 + 0] : 0, x0 = win ? win[img * 3 + 1] : 0, flip = win ? win[img * 3 + 2] : 0;
            const int sy = y0 + ih, sx = x0 + (flip ? w - 1 - iw : iw);
            const unsigned char* px = frames + (((long)img * hs + sy) * ws + sx) * 3;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                float f = (float)px[fp.to_rgb ? 2 - k : k];
                if (fp.div_255) f = __fdiv_rn(f, 255.f);
                v[k] = __fmul_rn(__fsub_rn(f, fp.mean[k]), fp.stdinv[k]);
            }
            if (out_nchw) {
#pragma unroll
                for (int k = 0; k < 3; ++k) out_nchw[(((long)img * 3 + k) * h + ih) * w + iw] = v[k];
            }
        }
        if (out_stem) st4(out_stem + i * 4, make_float4(v[0], v[1], v[2], v[3]));
    }
}

// The same, with a bilinear resample in front of the window: per frame one int32 row of RS_COLS
// (hs_i, ws_i, by, bx, bh, bw, rh, rw, oy, ox, flip): the patch [by, by+bh) x [bx, bx+bw) of frame i is resized to rh x rw with cv2
// INTER_LINEAR CV_8U arithmetic (resize.cpp: fp64 source coordinate rounded to fp32, 11-bit weights each rounded on its own, x taps
// zeroed at the border, y rows clamped, the vectorised row blend ((H0>>4)*b0>>16) + ((H1>>4)*b1>>16) + 2 >> 2; exactly 2x down in
// both axes is cv2's INTER_AREA switch, the rounded 2x2 mean), then resized[oy:oy+h, ox:ox+w] goes through frames_prep_kernel's crop
// arithmetic from the uint8 value on.  Rows are validated on the host (preprocess.ResamplingFramePipeline).
// Block = one (frame, padded output row): the row's descriptor, source rows and y weights are block-uniform; lanes run along x
// (two source rows, byte loads of neighbouring pixels), one 8/16-byte store per pixel as stem_prep_kernel.
// COLOR: the frame's ColorJitter (augmentations.py:238-339; every branch is affine in the pixel and nothing clips) sits between the
// resample and Normalize as q = M p + b on the resampled uint8 triple in STORED channel order: color = (n, 12) fp32 rows
// M[0][0..2], M[1][0..2], M[2][0..2], b[0..2], block-uniform like the int row, read once per block.  Every product and sum is rounded
// to fp32 on its own, summed left to right, so M = I gives p + b rounded once (the reference's float32 `img + bgr`).
// src_index (mvf_frames_gather_resample_u8): output image `img` is cut from frame src_index[img] instead of frame img, so the crops and
// clips of a video share its decoded frames; block-uniform like the row (blockIdx only: a scalar load), read once per block, and it
// enters nothing but the two source-row base addresses.  NULL = img.
constexpr int RS_COLS = 11, CJ_COLS = 12;
template <typename ET, bool COLOR>
__global__ void frames_resample_kernel(const unsigned char* frames, int hs, int ws, const int* src_index, const int* rows, const float* color,
                                       int h, int w, FramePrep fp, int pad, int hp, int wp, ET* out_stem, float* out_nchw) {
#pragma clang fp contract(off)
    const int orow = blockIdx.x, img = orow / hp, yo = orow - img * hp;
    float cm[CJ_COLS];
    if constexpr (COLOR) {
#pragma unroll
        for (int k = 0; k < CJ_COLS; ++k) cm[k] = color[(long)img * CJ_COLS + k];
    }
    const int ih = yo - pad;
    const bool rok = ih >= 0 && ih < h;
    const int* r = rows + (long)img * RS_COLS;
    const int by = r[2], bx = r[3], bh = r[4], bw = r[5], rh = r[6], rw = r[7], oy = r[8], ox = r[9], flip = r[10];
    const bool area2 = bh == 2 * rh && bw == 2 * rw;
    const int dy = oy + (rok ? ih : 0);
    int y0, y1, b0 = 0, b1 = 0;
    if (area2) {
        y0 = 2 * dy;
        y1 = y0 + 1;
    } else {
        const double scy = 1.0 / ((double)rh / bh);
        float fy = (float)((dy + 0.5) * scy - 0.5);
        const int sy = (int)floorf(fy);
        fy -= (float)sy;
        b0 = __float2int_rn((1.f - fy) * 2048.f);
        b1 = __float2int_rn(fy * 2048.f);
        y0 = min(max(sy, 0), bh - 1);
        y1 = min(max(sy + 1, 0), bh - 1);
    }
    const int src = src_index ? src_index[img] : img;
    const unsigned char* s0 = frames + (((long)src * hs + by + y0) * ws + bx) * 3;
    const unsigned char* s1 = frames + (((long)src * hs + by + y1) * ws + bx) * 3;
    const double scx = 1.0 / ((double)rw / bw);
    for (int xo = threadIdx.x; xo < wp; xo += blockDim.x) {
        const int iw = xo - pad;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (rok && iw >= 0 && iw < w) {
            const int dx = ox + (flip ? w - 1 - iw : iw);
            int px[3];
            if (area2) {
                const unsigned char *p0 = s0 + dx * 6, *p1 = s1 + dx * 6;
#pragma unroll
                for (int k = 0; k < 3; ++k) px[k] = (p0[k] + p0[k + 3] + p1[k] + p1[k + 3] + 2) >> 2;
            } else {
                float fx = (float)((dx + 0.5) * scx - 0.5);
                int sx = (int)floorf(fx);
                fx -= (float)sx;
                if (sx < 0) sx = 0, fx = 0.f;
                if (sx >= bw - 1) sx = bw - 1, fx = 0.f;
                const int a0 = __float2int_rn((1.f - fx) * 2048.f), a1 = __float2int_rn(fx * 2048.f);
                const int x0 = sx * 3, x1 = min(sx + 1, bw - 1) * 3;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const int h0 = s0[x0 + k] * a0 + s0[x1 + k] * a1, h1 = s1[x0 + k] * a0 + s1[x1 + k] * a1;
                    px[k] = min((((h0 >> 4) * b0 >> 16) + ((h1 >> 4) * b1 >> 16) + 2) >> 2, 255);
                }
            }
            float q[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) q[k] = (float)px[k];
            if constexpr (COLOR) {
                const float p0 = q[0], p1 = q[1], p2 = q[2];
#pragma unroll
                for (int k = 0; k < 3; ++k)            // plain operators: the contract(off) above covers them, not the bodies of inlined intrinsics
                    q[k] = ((cm[3 * k] * p0 + cm[3 * k + 1] * p1) + cm[3 * k + 2] * p2) + cm[9 + k];
            }
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                float f = q[fp.to_rgb ? 2 - k : k];
                if (fp.div_255) f = __fdiv_rn(f, 255.f);
                v[k] = __fmul_rn(__fsub_rn(f, fp.mean[k]), fp.stdinv[k]);
            }
            if (out_nchw) {
#pragma unroll
                for (int k = 0; k < 3; ++k) out_nchw[(((long)img * 3 + k) * h + ih) * w + iw] = v[k];
            }
        }
        if (out_stem) st4(out_stem + ((long)orow * wp + xo) * 4, make_float4(v[0], v[1], v[2], v[3]));
    }
}

// frames_resample_kernel for decoder-native YUV 4:2:0 frames (mvf_frames_yuv420_gather_resample_u8): a frame is a (3 * hs / 2, pitch) byte
// image -- hs luma rows, then I420's U and V planes (hs / 2 rows of pitch / 2 bytes each) or NV12's hs / 2 rows of interleaved U, V pairs --
// and stands for the packed frame the kernel above would have been given: each of the four taps (the bilinear neighbours, or the four pixels
// of the exact-2x area mean) is converted to the stored triple with the header's 20-bit integer formula, chroma REPLICATED from sample
// (y >> 1, x >> 1) of the absolute frame coordinate, and the blend, ColorJitter, Normalize and both outputs continue unchanged.
// Block = one (image, padded output row) as above: the row descriptor, src, the y taps and the luma / chroma row base addresses are
// block-uniform (the two layouts differ only in the uniform chroma row stride, sample step and V offset); lanes run along x.  The twelve
// byte loads of a lane are UNCONDITIONAL on clamped coordinates (maxpool_kernel's comment: a load inside an `if` is waited for on the
// spot) -- a padding lane or row computes a pixel of the crop's border and stores zeros.
struct YuvSrc {
    int y_off, cy, cvr, cvg, cug, cub;      // rint(c * 2^20) of the standard's decimal coefficients
    int pitch, cstride, cstep;              // bytes: luma row, chroma row, chroma sample
    long u_off, v_delta, frame_bytes;       // U plane in the frame, V sample - U sample, frame stride
    int swap_rb;                            // stored order BGR: R and B change places after the conversion
};
__device__ __forceinline__ void yuv_to_rgb(int y, int u, int v, const YuvSrc& ys, int* rgb) {
    const int yp = max(0, y - ys.y_off) * ys.cy + (1 << 19);
    u -= 128;
    v -= 128;
    rgb[0] = min(max((yp + ys.cvr * v) >> 20, 0), 255);
    rgb[1] = min(max((yp - ys.cvg * v - ys.cug * u) >> 20, 0), 255);
    rgb[2] = min(max((yp + ys.cub * u) >> 20, 0), 255);
}
template <typename ET, bool COLOR>
__global__ void frames_yuv420_resample_kernel(const unsigned char* frames, YuvSrc ys, const int* src_index, const int* rows, const float* color,
                                              int h, int w, FramePrep fp, int pad, int hp, int wp, ET* out_stem, float* out_nchw) {
#pragma clang fp contract(off)
    const int orow = blockIdx.x, img = orow / hp, yo = orow - img * hp;
    float cm[CJ_COLS];
    if constexpr (COLOR) {
#pragma unroll
        for (int k = 0; k < CJ_COLS; ++k) cm[k] = color[(long)img * CJ_COLS + k];
    }
    const int ih = yo - pad;
    const bool rok = ih >= 0 && ih < h;
    const int* r = rows + (long)img * RS_COLS;
    const int by = r[2], bx = r[3], bh = r[4], bw = r[5], rh = r[6], rw = r[7], oy = r[8], ox = r[9], flip = r[10];
    const bool area2 = bh == 2 * rh && bw == 2 * rw;
    const int dy = oy + (rok ? ih : 0);
    int y0, y1, b0 = 0, b1 = 0;
    if (area2) {
        y0 = 2 * dy;
        y1 = y0 + 1;
    } else {
        const double scy = 1.0 / ((double)rh / bh);
        float fy = (float)((dy + 0.5) * scy - 0.5);
        const int sy = (int)floorf(fy);
        fy -= (float)sy;
        b0 = __float2int_rn((1.f - fy) * 2048.f);
        b1 = __float2int_rn(fy * 2048.f);
        y0 = min(max(sy, 0), bh - 1);
        y1 = min(max(sy + 1, 0), bh - 1);
    }
    const int src = src_index ? src_index[img] : img;
    const unsigned char* fr = frames + (long)src * ys.frame_bytes;
    const unsigned char *l0 = fr + (long)(by + y0) * ys.pitch, *l1 = fr + (long)(by + y1) * ys.pitch;
    const unsigned char *u0 = fr + ys.u_off + (long)((by + y0) >> 1) * ys.cstride, *u1 = fr + ys.u_off + (long)((by + y1) >> 1) * ys.cstride;
    const unsigned char *v0 = u0 + ys.v_delta, *v1 = u1 + ys.v_delta;
    const double scx = 1.0 / ((double)rw / bw);
    for (int xo = threadIdx.x; xo < wp; xo += blockDim.x) {
        const int iw = xo - pad;
        const bool ok = rok && iw >= 0 && iw < w;
        const int iwc = min(max(iw, 0), w - 1);
        const int dx = ox + (flip ? w - 1 - iwc : iwc);
        int xa, xb, a0 = 0, a1 = 0;
        if (area2) {
            xa = 2 * dx;
            xb = xa + 1;
        } else {
            float fx = (float)((dx + 0.5) * scx - 0.5);
            int sx = (int)floorf(fx);
            fx -= (float)sx;
            if (sx < 0) sx = 0, fx = 0.f;
            if (sx >= bw - 1) sx = bw - 1, fx = 0.f;
            a0 = __float2int_rn((1.f - fx) * 2048.f);
            a1 = __float2int_rn(fx * 2048.f);
            xa = sx;
            xb = min(sx + 1, bw - 1);
        }
        xa += bx;
        xb += bx;
        const int ca = (xa >> 1) * ys.cstep, cb = (xb >> 1) * ys.cstep;
        const int ya0 = l0[xa], yb0 = l0[xb], ya1 = l1[xa], yb1 = l1[xb];
        const int ua0 = u0[ca], ub0 = u0[cb], ua1 = u1[ca], ub1 = u1[cb];
        const int va0 = v0[ca], vb0 = v0[cb], va1 = v1[ca], vb1 = v1[cb];
        int ta0[3], tb0[3], ta1[3], tb1[3], px[3];
        yuv_to_rgb(ya0, ua0, va0, ys, ta0);
        yuv_to_rgb(yb0, ub0, vb0, ys, tb0);
        yuv_to_rgb(ya1, ua1, va1, ys, ta1);
        yuv_to_rgb(yb1, ub1, vb1, ys, tb1);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (area2) {
                px[k] = (ta0[k] + tb0[k] + ta1[k] + tb1[k] + 2) >> 2;
            } else {
                const int h0 = ta0[k] * a0 + tb0[k] * a1, h1 = ta1[k] * a0 + tb1[k] * a1;
                px[k] = min((((h0 >> 4) * b0 >> 16) + ((h1 >> 4) * b1 >> 16) + 2) >> 2, 255);
            }
        }
        float q[3];
        q[0] = (float)(ys.swap_rb ? px[2] : px[0]);
        q[1] = (float)px[1];
        q[2] = (float)(ys.swap_rb ? px[0] : px[2]);
        if constexpr (COLOR) {
            const float p0 = q[0], p1 = q[1], p2 = q[2];
#pragma unroll
            for (int k = 0; k < 3; ++k)            // plain operators: the contract(off) above covers them, not the bodies of inlined intrinsics
                q[k] = ((cm[3 * k] * p0 + cm[3 * k + 1] * p1) + cm[3 * k + 2] * p2) + cm[9 + k];
        }
        float v[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            float f = q[fp.to_rgb ? 2 - k : k];
            if (fp.div_255) f = __fdiv_rn(f, 255.f);
            v[k] = ok ? __fmul_rn(__fsub_rn(f, fp.mean[k]), fp.stdinv[k]) : 0.f;
        }
        if (out_nchw && ok) {
#pragma unroll
            for (int k = 0; k < 3; ++k) out_nchw[(((long)img * 3 + k) * h + ih) * w + iw] = v[k];
        }
        if (out_stem) st4(out_stem + ((long)orow * wp + xo) * 4, make_float4(v[0], v[1], v[2], 0.f));
    }
}

// MaxPool2d(3, 2, 1) NHWC; thread = (output pixel, 4 channels).  The nine window loads are UNCONDITIONAL on clamped coordinates (a
// clamped tap re-reads a pixel that is inside the window anyway, so the maximum is unchanged): a load inside an `if` is waited
// for on the spot, nine serial round trips per output instead of one.
template <typename ET>
__global__ void maxpool_kernel(const ET* x, int n, int h, int w, int c, int ho, int wo, ET* y) {
    const int c4 = c >> 2;
    const long total = (long)n * ho * wo * c4;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
        const int cq = (int)(i % c4);
        long t = i / c4;
        const int ow = (int)(t % wo); t /= wo;
        const int oh = (int)(t % ho);
        const int img = (int)(t / ho);
        const ET* base = x + (long)img * h * w * c + cq * 4;
        float4 v[9];
#pragma unroll
        for (int dy = 0; dy < 3; ++dy) {
            const int ih = min(max(oh * 2 - 1 + dy, 0), h - 1);
#pragma unroll
            for (int dx = 0; dx < 3; ++dx) {
                const int iw = min(max(ow * 2 - 1 + dx, 0), w - 1);
                v[dy * 3 + dx] = ld4(base + ((long)ih * w + iw) * c);
            }
        }
        float4 m = v[0];
#pragma unroll
        for (int k = 1; k < 9; ++k) {
            m.x = fmaxf(m.x, v[k].x); m.y = fmaxf(m.y, v[k].y); m.z = fmaxf(m.z, v[k].z); m.w = fmaxf(m.w, v[k].w);
        }
        st4(y + (((long)img * ho + oh) * wo + ow) * c + cq * 4, m);
    }
}

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

inline int grid_for(long total, int per_block = 256, int cap = 256 * 32) {
    return (int)std::min<long>((total + per_block - 1) / per_block, cap);
}

// mvf_frames_resample_u8 (color == nullptr), mvf_frames_resample_color_u8, mvf_frames_gather_resample_u8 (n = output images, of
// n_src source frames) and mvf_frames_yuv420_gather_resample_u8 (yuv != nullptr: the frames are YUV 4:2:0): one validation, one launch
int frames_resample(const char* who, const unsigned char* frames_hwc, int n_src, int n, int hs, int ws, const int* src_index, const int* rows,
                    const float* color, int h, int w, const float* mean3, const float* std3, int to_rgb, int div_255, int pad, int wp,
                    void* out_stem, float* out_nchw, int dtype, void* stream, const YuvSrc* yuv = nullptr) {
    MVF_REQUIRE(frames_hwc && rows && mean3 && std3 && (out_stem || out_nchw) && n_src > 0 && n > 0 && hs > 0 && ws > 0 && h > 0 && w > 0 && pad >= 0,
                MVF_EINVAL, "%s: bad argument", who);
    MVF_REQUIRE(src_index || n_src == n, MVF_EINVAL, "%s: n_src=%d != n_out=%d without src_index", who, n_src, n);
    MVF_REQUIRE(!out_stem || wp >= w + 2 * pad, MVF_EINVAL, "%s: wp=%d < w + 2*pad", who, wp);
    MVF_REQUIRE(dtype == MVF_F32 || dtype == MVF_BF16, MVF_EINVAL, "%s: bad dtype", who);
    FramePrep fp;
    for (int k = 0; k < 3; ++k) {
        MVF_REQUIRE(std3[k] != 0.f, MVF_EINVAL, "%s: std[%d] is zero", who, k);
        fp.mean[k] = mean3[k];
        fp.stdinv[k] = (float)(1.0 / (double)std3[k]);      // the reference multiplies by 1 / float64(std)
    }
    fp.to_rgb = to_rgb;
    fp.div_255 = div_255;
    const int p = out_stem ? pad : 0, wpp = out_stem ? wp : w;
    const int hp = h + 2 * p;
    MVF_REQUIRE((long)n * hp < (1L << 31), MVF_ESHAPE, "%s: too many rows", who);
    const dim3 grid(n * hp);
    const hipStream_t st = (hipStream_t)stream;
    if (yuv) {
        if (dtype == MVF_F32 && !color)
            hipLaunchKernelGGL((frames_yuv420_resample_kernel<float, false>), grid, dim3(256), 0, st, frames_hwc, *yuv, src_index, rows, color, h, w, fp, p,
                               hp, wpp, (float*)out_stem, out_nchw);
        else if (dtype == MVF_F32)
            hipLaunchKernelGGL((frames_yuv420_resample_kernel<float, true>), grid, dim3(256), 0, st, frames_hwc, *yuv, src_index, rows, color, h, w, fp, p,
                               hp, wpp, (float*)out_stem, out_nchw);
        else if (!color)
            hipLaunchKernelGGL((frames_yuv420_resample_kernel<bf16_t, false>), grid, dim3(256), 0, st, frames_hwc, *yuv, src_index, rows, color, h, w, fp,
                               p, hp, wpp, (bf16_t*)out_stem, out_nchw);
        else
            hipLaunchKernelGGL((frames_yuv420_resample_kernel<bf16_t, true>), grid, dim3(256), 0, st, frames_hwc, *yuv, src_index, rows, color, h, w, fp,
                               p, hp, wpp, (bf16_t*)out_stem, out_nchw);
        MVF_LAUNCH_CHECK();
        return MVF_OK;
    }
    if (dtype == MVF_F32 && !color)
        hipLaunchKernelGGL((frames_resample_kernel<float, false>), grid, dim3(256), 0, st, frames_hwc, hs, ws, src_index, rows, color, h, w, fp, p,
                           hp, wpp, (float*)out_stem, out_nchw);
    else if (dtype == MVF_F32)
        hipLaunchKernelGGL((frames_resample_kernel<float, true>), grid, dim3(256), 0, st, frames_hwc, hs, ws, src_index, rows, color, h, w, fp, p,
                           hp, wpp, (float*)out_stem, out_nchw);
    else if (!color)
        hipLaunchKernelGGL((frames_resample_kernel<bf16_t, false>), grid, dim3(256), 0, st, frames_hwc, hs, ws, src_index, rows, color, h, w, fp, p,
                           hp, wpp, (bf16_t*)out_stem, out_nchw);
    else
        hipLaunchKernelGGL((frames_resample_kernel<bf16_t, true>), grid, dim3(256), 0, st, frames_hwc, hs, ws, src_index, rows, color, h, w, fp, p,
                           hp, wpp, (bf16_t*)out_stem, out_nchw);
    MVF_LAUNCH_CHECK();
    return MVF_OK;
}

}  // namespace

extern "C" {

int mvf_stem_prep(const float* x_nchw, int n, int c, int h, int w, int pad, int wp, void* out, int dtype, void* stream) {
    MVF_REQUIRE(x_nchw && out && n > 0 && c > 0 && c <= 4 && h > 0 && w > 0 && pad >= 0 && wp >= w + 2 * pad, MVF_EINVAL, "stem_prep: bad argument");
    const int hp = h + 2 * pad;
    MVF_REQUIRE((long)n * hp < (1L << 31), MVF_ESHAPE, "stem_prep: too many rows");
    const dim3 grid(n * hp);
    if (dtype == MVF_F32)
        hipLaunchKernelGGL(stem_prep_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, x_nchw, n, c, h, w, pad, hp, wp, (float*)out);
    else
        hipLaunchKernelGGL(stem_prep_kernel<bf16_t>, grid, dim3(256), 0, (hipStream_t)stream, x_nchw, n, c, h, w, pad, hp, wp, (bf16_t*)out);
    MVF_LAUNCH_CHECK();
    return MVF_OK;
}

int mvf_frames_prep_u8(const unsigned char* frames_hwc, int n, int hs, int ws, const int* window, int h, int w,
                       const float* mean3, const float* std3, int to_rgb, int div_255, int pad, int wp, void* out_stem,
                       float* out_nchw, int dtype, void* stream) {
    MVF_REQUIRE(frames_hwc && mean3 && std3 && (out_stem || out_nchw) && n > 0 && hs > 0 && ws > 0 && h > 0 && w > 0 && h <= hs && w <= ws && pad >= 0,
                MVF_EINVAL, "frames_prep_u8: bad argument");
    MVF_REQUIRE(!out_stem || wp >= w + 2 * pad, MVF_EINVAL, "frames_prep_u8: wp=%d < w + 2*pad", wp);
    MVF_REQUIRE(dtype == MVF_F32 || dtype == MVF_BF16, MVF_EINVAL, "frames_prep_u8: bad dtype");
    FramePrep fp;
    for (int k = 0; k < 3; ++k) {
        MVF_REQUIRE(std3[k] != 0.f, MVF_EINVAL, "frames_prep_u8: std[%d] is zero", k);
        fp.mean[k] = mean3[k];
        fp.stdinv[k] = (float)(1.0 / (double)std3[k]);      // the reference multiplies by 1 / float64(std)
    }
    fp.to_rgb = to_rgb;
    fp.div_255 = div_255;
    const int p = out_stem ? pad : 0, wpp = out_stem ? wp : w;
    const int hp = h + 2 * p;
    const long total = (long)n * hp * wpp;
    if (dtype == MVF_F32)
        hipLaunchKernelGGL(frames_prep_kernel<float>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, frames_hwc, n, hs, ws, window, h, w, fp,
                           p, hp, wpp, (float*)out_stem, out_nchw);
    else
        hipLaunchKernelGGL(frames_prep_kernel<bf16_t>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, frames_hwc, n, hs, ws, window, h, w, fp,
                           p, hp, wpp, (bf16_t*)out_stem, out_nchw);
    MVF_LAUNCH_CHECK();
    return MVF_OK;
}

int mvf_frames_resample_u8(const unsigned char* frames_hwc, int n, int hs, int ws, const int* rows, int h, int w,
                           const float* mean3, const float* std3, int to_rgb, int div_255, int pad, int wp, void* out_stem,
                           float* out_nchw, int dtype, void* stream) {
    return frames_resample("frames_resample_u8", frames_hwc, n, n, hs, ws, nullptr, rows, nullptr, h, w, mean3, std3, to_rgb, div_255, pad, wp, out_stem,
                           out_nchw, dtype, stream);
}

int mvf_frames_resample_color_u8(const unsigned char* frames_hwc, int n, int hs, int ws, const int* rows, const float* color, int h, int w,
                                 const float* mean3, const float* std3, int to_rgb, int div_255, int pad, int wp, void* out_stem,
                                 float* out_nchw, int dtype, void* stream) {
    return frames_resample("frames_resample_color_u8", frames_hwc, n, n, hs, ws, nullptr, rows, color, h, w, mean3, std3, to_rgb, div_255, pad,
                           wp, out_stem, out_nchw, dtype, stream);
}

int mvf_frames_gather_resample_u8(const unsigned char* frames_hwc, int n_src, int hs, int ws, const int* src_index, int n_out, const int* rows,
                                  const float* color, int h, int w, const float* mean3, const float* std3, int to_rgb, int div_255, int pad,
                                  int wp, void* out_stem, float* out_nchw, int dtype, void* stream) {
    return frames_resample("frames_gather_resample_u8", frames_hwc, n_src, n_out, hs, ws, src_index, rows, color, h, w, mean3, std3, to_rgb,
                           div_255, pad, wp, out_stem, out_nchw, dtype, stream);
}

int mvf_frames_yuv420_gather_resample_u8(const unsigned char* frames, int n_src, int hs, int ws, int pitch, int layout, int standard, int order,
                                         const int* src_index, int n_out, const int* rows, const float* color, int h, int w, const float* mean3,
                                         const float* std3, int to_rgb, int div_255, int pad, int wp, void* out_stem, float* out_nchw, int dtype,
                                         void* stream) {
    const char* who = "frames_yuv420_gather_resample_u8";
    MVF_REQUIRE(hs > 0 && ws > 0 && hs % 2 == 0, MVF_EINVAL, "%s: hs=%d must be positive and even (ws=%d)", who, hs, ws);
    MVF_REQUIRE(pitch % 2 == 0 && pitch >= ws, MVF_EINVAL, "%s: pitch=%d must be even and >= ws=%d", who, pitch, ws);
    MVF_REQUIRE(layout == 0 || layout == 1, MVF_EINVAL, "%s: unknown layout %d (0 = I420, 1 = NV12)", who, layout);
    MVF_REQUIRE(standard >= 0 && standard <= 2, MVF_EINVAL, "%s: unknown standard %d (0 = BT.601 limited, 1 = BT.601 full, 2 = BT.709 limited)", who,
                standard);
    MVF_REQUIRE(order == 0 || order == 1, MVF_EINVAL, "%s: unknown order %d (0 = BGR, 1 = RGB)", who, order);
    // y_off, cY, cVR, cVG, cUG, cUB: the header's table
    static const double coef[3][6] = {{16, 1.164, 1.596, 0.813, 0.391, 2.018},
                                      {0, 1.0, 1.402, 0.714136, 0.344136, 1.772},
                                      {16, 1.164384, 1.792741, 0.532909, 0.213249, 2.112402}};
    const double* c = coef[standard];
    const double one = (double)(1 << 20);
    YuvSrc ys;
    ys.y_off = (int)c[0];
    ys.cy = (int)rint(c[1] * one), ys.cvr = (int)rint(c[2] * one), ys.cvg = (int)rint(c[3] * one);
    ys.cug = (int)rint(c[4] * one), ys.cub = (int)rint(c[5] * one);
    ys.pitch = pitch;
    ys.cstride = layout == 0 ? pitch / 2 : pitch;
    ys.cstep = layout == 0 ? 1 : 2;
    ys.u_off = (long)hs * pitch;
    ys.v_delta = layout == 0 ? (long)(hs / 2) * (pitch / 2) : 1;
    ys.frame_bytes = (long)hs * pitch / 2 * 3;
    ys.swap_rb = order == 0;
    return frames_resample(who, frames, n_src, n_out, hs, ws, src_index, rows, color, h, w, mean3, std3, to_rgb, div_255, pad, wp, out_stem, out_nchw,
                           dtype, stream, &ys);
}

int mvf_maxpool3x3s2_nhwc(const void* x, int n, int h, int w, int c, void* y, int dtype, void* stream) {
    MVF_REQUIRE(x && y && n > 0 && h > 0 && w > 0 && c > 0 && c % 4 == 0, MVF_EINVAL, "maxpool: bad argument (c %% 4 != 0?)");
    const int ho = (h + 2 - 3) / 2 + 1, wo = (w + 2 - 3) / 2 + 1;
    const long total = (long)n * ho * wo * (c / 4);
    if (dtype == MVF_F32)
        hipLaunchKernelGGL(maxpool_kernel<float>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, (const float*)x, n, h, w, c, ho, wo, (float*)y);
    else
        hipLaunchKernelGGL(maxpool_kernel<bf16_t>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, n, h, w, c, ho, wo, (bf16_t*)y);
    MVF_LAUNCH_CHECK();
    return MVF_OK;
}

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

}  // extern "C"
