// Bandwidth-bound companions of the conv stack at inference: stem input re-layout, max-pool (the TSN head and clip averaging are csrc/head.hip).
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

inline int grid_for(long total, int per_block = 256, int cap = 256 * 32) {
    return (int)std::min<long>((total + per_block - 1) / per_block, cap);
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

}  // extern "C"
