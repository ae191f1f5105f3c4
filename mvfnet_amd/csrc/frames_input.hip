// The uint8 frame input: decoded frames (packed HWC, or decoder-native YUV 4:2:0) -> the normalised stem operand and / or the reference's
// fp32 NCHW tensor.  frames_prep_kernel crops; the two resample kernels put cv2's resize, the frame gather and ColorJitter in front of the
// crop, and share every step but the fetch of their four taps (the __device__ helpers below).  Where an image's source rows start is the
// kernels' SRC parameter: DenseSrc (frame index times a constant) or AddressedSrc (offsets and pitches the image's table row carries).
#include <algorithm>
#include <math.h>
#include <type_traits>

#include "common.h"

namespace {

// Normalize: (float(px) [/ 255] - mean) * stdinv in two rounded fp32 steps (the reference subtracts, then multiplies by 1/std: no FMA)
struct FramePrep {
    float mean[3], stdinv[3];
    int to_rgb, div_255;
};

constexpr int RS_COLS = 11, CJ_COLS = 12, AD_COLS = 5;

// ---- the steps of a resampled pixel, in order ----------------------------------------------------------------------------------------
// Row setup (block-uniform).  r = the frame's int32 row (hs_i, ws_i, by, bx, bh, bw, rh, rw, oy, ox, flip): the patch [by, by+bh) x
// [bx, bx+bw) of the frame is resized to rh x rw with cv2 INTER_LINEAR CV_8U arithmetic (resize.cpp: fp64 source coordinate rounded to
// fp32, 11-bit weights each rounded on its own, x taps zeroed at the border, y rows clamped; exactly 2x down in both axes is cv2's
// INTER_AREA switch, the rounded 2x2 mean), and resized[oy:oy+h, ox:ox+w] is the crop.  Output row ih of the crop (row 0 for a padding
// row) reads patch rows y0, y1 with weights b0, b1.  Rows are validated on the host (preprocess.FramePipeline._parse).
struct RowSetup {
    int by, bx, bh, bw, ox, flip, y0, y1, b0, b1;
    bool area2;
    double scx;
};
__device__ __forceinline__ RowSetup row_setup(const int* r, bool rok, int ih) {
#pragma clang fp contract(off)
    RowSetup s;
    s.by = r[2], s.bx = r[3], s.bh = r[4], s.bw = r[5], s.ox = r[9], s.flip = r[10];
    const int rh = r[6], rw = r[7], oy = r[8];
    s.area2 = s.bh == 2 * rh && s.bw == 2 * rw;
    s.b0 = s.b1 = 0;
    const int dy = oy + (rok ? ih : 0);
    if (s.area2) {
        s.y0 = 2 * dy;
        s.y1 = s.y0 + 1;
    } else {
        const double scy = 1.0 / ((double)rh / s.bh);
        float fy = (float)((dy + 0.5) * scy - 0.5);
        const int sy = (int)floorf(fy);
        fy -= (float)sy;
        s.b0 = __float2int_rn((1.f - fy) * 2048.f);
        s.b1 = __float2int_rn(fy * 2048.f);
        s.y0 = min(max(sy, 0), s.bh - 1);
        s.y1 = min(max(sy + 1, 0), s.bh - 1);
    }
    s.scx = 1.0 / ((double)rw / s.bw);
    return s;
}

// X taps: column dx of the resized patch reads patch pixels xa, xb with weights a0, a1 (the area mean: pixels 2 dx and 2 dx + 1)
struct XTaps {
    int xa, xb, a0, a1;
};
__device__ __forceinline__ XTaps x_taps(const RowSetup& s, int dx) {
#pragma clang fp contract(off)
    XTaps t;
    t.a0 = t.a1 = 0;
    if (s.area2) {
        t.xa = 2 * dx;
        t.xb = t.xa + 1;
    } else {
        float fx = (float)((dx + 0.5) * s.scx - 0.5);
        int sx = (int)floorf(fx);
        fx -= (float)sx;
        if (sx < 0) sx = 0, fx = 0.f;
        if (sx >= s.bw - 1) sx = s.bw - 1, fx = 0.f;
        t.a0 = __float2int_rn((1.f - fx) * 2048.f);
        t.a1 = __float2int_rn(fx * 2048.f);
        t.xa = sx;
        t.xb = min(sx + 1, s.bw - 1);
    }
    return t;
}

// Blend: per channel the four taps (row 0 / 1 at xa / xb) -> the uint8 value: cv2's vectorised row blend, or the rounded 2x2 mean
__device__ __forceinline__ void blend(const RowSetup& s, const XTaps& t, const int* a0, const int* b0, const int* a1, const int* b1, int* px) {
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int h0 = a0[k] * t.a0 + b0[k] * t.a1, h1 = a1[k] * t.a0 + b1[k] * t.a1;
        px[k] = s.area2 ? (a0[k] + b0[k] + a1[k] + b1[k] + 2) >> 2 : min((((h0 >> 4) * s.b0 >> 16) + ((h1 >> 4) * s.b1 >> 16) + 2) >> 2, 255);
    }
}

// Epilogue: the uint8 triple px in STORED channel order -> ColorJitter -> to_rgb -> Normalize -> v[3].
// COLOR: the frame's ColorJitter (augmentations.py:238-339; every branch is affine in the pixel and nothing clips) is q = M p + b with
// cm = the frame's fp32 row M[0][0..2], M[1][0..2], M[2][0..2], b[0..2], block-uniform like the int row, read once per block.  Every
// product and sum is rounded to fp32 on its own, summed left to right, so M = I gives p + b rounded once (the reference's float32
// `img + bgr`).
template <bool COLOR>
__device__ __forceinline__ void load_color(const float* color, int img, float* cm) {
    if constexpr (COLOR) {
#pragma unroll
        for (int k = 0; k < CJ_COLS; ++k) cm[k] = color[(long)img * CJ_COLS + k];
    }
}
template <bool COLOR>
__device__ __forceinline__ void epilogue(const int* px, const float* cm, const FramePrep& fp, float* v) {
#pragma clang fp contract(off)
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
}

// Stores: channels-first fp32 (the reference's tensor), and one 8/16-byte pixel of the zero-padded NHWC4 stem operand
__device__ __forceinline__ void store_nchw(float* out_nchw, int img, int h, int w, int ih, int iw, const float* v) {
#pragma unroll
    for (int k = 0; k < 3; ++k) out_nchw[(((long)img * 3 + k) * h + ih) * w + iw] = v[k];
}
template <typename ET>
__device__ __forceinline__ void store_stem(ET* pixel, const float* v) {
    st4(pixel, make_float4(v[0], v[1], v[2], 0.f));
}

// ---- kernels --------------------------------------------------------------------------------------------------------------------------
// Crop only: window (y0, x0, flip) per frame (NULL = the top-left corner), mirror, epilogue, channels-first stacking.  Thread = one pixel
// of the padded stem image; 3 byte loads, one 8/16-byte store.
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
        float v[3] = {0.f, 0.f, 0.f};
        if (ih >= 0 && ih < h && iw >= 0 && iw < w) {
            const int y0 = win ? win[img * 3 + 0] : 0, x0 = win ? win[img * 3 + 1] : 0, flip = win ? win[img * 3 + 2] : 0;
            const int sy = y0 + ih, sx = x0 + (flip ? w - 1 - iw : iw);
            const unsigned char* p = frames + (((long)img * hs + sy) * ws + sx) * 3;
            const int px[3] = {p[0], p[1], p[2]};
            epilogue<false>(px, nullptr, fp, v);
            if (out_nchw) store_nchw(out_nchw, img, h, w, ih, iw, v);
        }
        if (out_stem) store_stem(out_stem + i * 4, v);
    }
}

// ---- the address step: where the source rows of output image `img` start -------------------------------------------------------------
// Block-uniform like the geometry row (blockIdx only: scalar loads), read once per block, formed in 64-bit arithmetic; it enters nothing
// but the row base pointers.  YuvSrc (below) carries the colour standard and, for DenseSrc, the one layout every frame shares.
struct YuvSrc {
    int y_off, cy, cvr, cvg, cug, cub;      // rint(c * 2^20) of the standard's decimal coefficients
    int pitch, cstride, cstep;              // bytes: luma row, chroma row, chroma sample (DenseSrc; AddressedSrc reads cstep alone)
    long u_off, v_delta, frame_bytes;       // U plane in the frame, V sample - U sample, frame stride (DenseSrc)
    int swap_rb;                            // stored order BGR: R and B change places after the conversion
};
// Frame src_index[img] (NULL = img) of one dense batch in which every frame has the same padded extent and pitch: index times a constant.
struct DenseSrc {
    const int* src_index;
    int hs, ws;
    __device__ __forceinline__ void packed(const unsigned char* frames, int img, int y0, int y1, const unsigned char*& s0, const unsigned char*& s1) const {
        const int src = src_index ? src_index[img] : img;
        s0 = frames + ((long)src * hs + y0) * ws * 3;
        s1 = frames + ((long)src * hs + y1) * ws * 3;
    }
    __device__ __forceinline__ void yuv(const unsigned char* frames, const YuvSrc& ys, int img, int y0, int y1, const unsigned char*& l0,
                                        const unsigned char*& l1, const unsigned char*& u0, const unsigned char*& u1, const unsigned char*& v0,
                                        const unsigned char*& v1) const {
        const int src = src_index ? src_index[img] : img;
        const unsigned char* fr = frames + (long)src * ys.frame_bytes;
        l0 = fr + (long)y0 * ys.pitch, l1 = fr + (long)y1 * ys.pitch;
        u0 = fr + ys.u_off + (long)(y0 >> 1) * ys.cstride, u1 = fr + ys.u_off + (long)(y1 >> 1) * ys.cstride;
        v0 = u0 + ys.v_delta, v1 = u1 + ys.v_delta;
    }
};
// mvf_frames_addressed_resample_u8: the image's int32 address row (o0, p0, o1, o2, p1) = byte offsets from `frames` and row pitches of the
// planes it is cut from -- packed: pixels at o0 + y p0 + 3 x; YUV: luma at o0 + y p0 + x, U at o1 + (y >> 1) p1 + cstep (x >> 1), V
// likewise from o2 (I420) or one byte after U (NV12).  Rows are validated on the host (preprocess.check_addresses).
struct AddressedSrc {
    const int* addr;
    __device__ __forceinline__ void packed(const unsigned char* frames, int img, int y0, int y1, const unsigned char*& s0, const unsigned char*& s1) const {
        const int* a = addr + (long)img * AD_COLS;
        const unsigned char* fr = frames + (long)a[0];
        const long p0 = a[1];
        s0 = fr + y0 * p0;
        s1 = fr + y1 * p0;
    }
    __device__ __forceinline__ void yuv(const unsigned char* frames, const YuvSrc& ys, int img, int y0, int y1, const unsigned char*& l0,
                                        const unsigned char*& l1, const unsigned char*& u0, const unsigned char*& u1, const unsigned char*& v0,
                                        const unsigned char*& v1) const {
        const int* a = addr + (long)img * AD_COLS;
        const long o0 = a[0], p0 = a[1], o1 = a[2], o2 = a[3], p1 = a[4];
        const long c0 = (y0 >> 1) * p1, c1 = (y1 >> 1) * p1;
        l0 = frames + o0 + y0 * p0, l1 = frames + o0 + y1 * p0;
        u0 = frames + o1 + c0, u1 = frames + o1 + c1;
        const bool nv12 = ys.cstep == 2;
        v0 = nv12 ? u0 + 1 : frames + o2 + c0;
        v1 = nv12 ? u1 + 1 : frames + o2 + c1;
    }
};

// The resample in front of the crop, packed 3-byte pixels.  Block = one (image, padded output row): the row's descriptor,
// source rows and y weights are block-uniform; lanes run along x (two source rows, byte loads of neighbouring pixels), one 8/16-byte
// store per pixel as stem_prep_kernel.
// DenseSrc::src_index (mvf_frames_gather_resample_u8): output image `img` is cut from frame src_index[img] instead of frame img, so the
// crops and clips of a video share its decoded frames.
template <typename ET, bool COLOR, typename SRC>
__global__ void frames_resample_kernel(const unsigned char* frames, SRC src, const int* rows, const float* color,
                                       int h, int w, FramePrep fp, int pad, int hp, int wp, ET* out_stem, float* out_nchw) {
    const int orow = blockIdx.x, img = orow / hp, yo = orow - img * hp;
    float cm[CJ_COLS];
    load_color<COLOR>(color, img, cm);
    const int ih = yo - pad;
    const bool rok = ih >= 0 && ih < h;
    const RowSetup rs = row_setup(rows + (long)img * RS_COLS, rok, ih);
    const unsigned char *s0, *s1;
    src.packed(frames, img, rs.by + rs.y0, rs.by + rs.y1, s0, s1);
    s0 += rs.bx * 3;
    s1 += rs.bx * 3;
    for (int xo = threadIdx.x; xo < wp; xo += blockDim.x) {
        const int iw = xo - pad;
        float v[3] = {0.f, 0.f, 0.f};
        if (rok && iw >= 0 && iw < w) {
            const XTaps t = x_taps(rs, rs.ox + (rs.flip ? w - 1 - iw : iw));
            const int xa = t.xa * 3, xb = t.xb * 3;
            int ta0[3], tb0[3], ta1[3], tb1[3], px[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) ta0[k] = s0[xa + k], tb0[k] = s0[xb + k], ta1[k] = s1[xa + k], tb1[k] = s1[xb + k];      // all twelve in flight
            blend(rs, t, ta0, tb0, ta1, tb1, px);
            epilogue<COLOR>(px, cm, fp, v);
            if (out_nchw) store_nchw(out_nchw, img, h, w, ih, iw, v);
        }
        if (out_stem) store_stem(out_stem + ((long)orow * wp + xo) * 4, v);
    }
}

// The same for decoder-native YUV 4:2:0 frames (mvf_frames_yuv420_gather_resample_u8): a DenseSrc frame is a (3 * hs / 2, pitch) byte image
// -- hs luma rows, then I420's U and V planes (hs / 2 rows of pitch / 2 bytes each) or NV12's hs / 2 rows of interleaved U, V pairs --, an
// AddressedSrc frame is its three (NV12: two) planes wherever its address row puts them; either stands for the packed frame the kernel
// above would have been given: each of the four taps is converted to the stored triple with the header's 20-bit integer formula, chroma
// REPLICATED from sample (y >> 1, x >> 1) of the absolute frame coordinate.  The luma / chroma row base addresses are block-uniform (the
// two layouts differ only in the uniform chroma row stride, sample step and V offset).  The twelve byte loads of a lane are UNCONDITIONAL
// on clamped coordinates (maxpool_kernel's comment: a load inside an `if` is waited for on the spot) -- a padding lane or row computes a
// pixel of the crop's border, inside the image's own planes under either SRC, and stores zeros.
__device__ __forceinline__ void yuv_to_rgb(int y, int u, int v, const YuvSrc& ys, int* rgb) {
    const int yp = max(0, y - ys.y_off) * ys.cy + (1 << 19);
    u -= 128;
    v -= 128;
    rgb[0] = min(max((yp + ys.cvr * v) >> 20, 0), 255);
    rgb[1] = min(max((yp - ys.cvg * v - ys.cug * u) >> 20, 0), 255);
    rgb[2] = min(max((yp + ys.cub * u) >> 20, 0), 255);
}
template <typename ET, bool COLOR, typename SRC>
__global__ void frames_yuv420_resample_kernel(const unsigned char* frames, YuvSrc ys, SRC src, const int* rows, const float* color,
                                              int h, int w, FramePrep fp, int pad, int hp, int wp, ET* out_stem, float* out_nchw) {
    const int orow = blockIdx.x, img = orow / hp, yo = orow - img * hp;
    float cm[CJ_COLS];
    load_color<COLOR>(color, img, cm);
    const int ih = yo - pad;
    const bool rok = ih >= 0 && ih < h;
    const RowSetup rs = row_setup(rows + (long)img * RS_COLS, rok, ih);
    const unsigned char *l0, *l1, *u0, *u1, *v0, *v1;
    src.yuv(frames, ys, img, rs.by + rs.y0, rs.by + rs.y1, l0, l1, u0, u1, v0, v1);
    for (int xo = threadIdx.x; xo < wp; xo += blockDim.x) {
        const int iw = xo - pad;
        const bool ok = rok && iw >= 0 && iw < w;
        const int iwc = min(max(iw, 0), w - 1);
        const XTaps t = x_taps(rs, rs.ox + (rs.flip ? w - 1 - iwc : iwc));
        const int xa = t.xa + rs.bx, xb = t.xb + rs.bx;
        const int ca = (xa >> 1) * ys.cstep, cb = (xb >> 1) * ys.cstep;
        const int ya0 = l0[xa], yb0 = l0[xb], ya1 = l1[xa], yb1 = l1[xb];
        const int ua0 = u0[ca], ub0 = u0[cb], ua1 = u1[ca], ub1 = u1[cb];
        const int va0 = v0[ca], vb0 = v0[cb], va1 = v1[ca], vb1 = v1[cb];
        int ta0[3], tb0[3], ta1[3], tb1[3], rgb[3];
        yuv_to_rgb(ya0, ua0, va0, ys, ta0);
        yuv_to_rgb(yb0, ub0, vb0, ys, tb0);
        yuv_to_rgb(ya1, ua1, va1, ys, ta1);
        yuv_to_rgb(yb1, ub1, vb1, ys, tb1);
        blend(rs, t, ta0, tb0, ta1, tb1, rgb);
        const int px[3] = {ys.swap_rb ? rgb[2] : rgb[0], rgb[1], ys.swap_rb ? rgb[0] : rgb[2]};
        float v[3];
        epilogue<COLOR>(px, cm, fp, v);
#pragma unroll
        for (int k = 0; k < 3; ++k) v[k] = ok ? v[k] : 0.f;
        if (out_nchw && ok) store_nchw(out_nchw, img, h, w, ih, iw, v);
        if (out_stem) store_stem(out_stem + ((long)orow * wp + xo) * 4, v);
    }
}

// ---- host side ------------------------------------------------------------------------------------------------------------------------
inline int grid_for(long total, int per_block = 256, int cap = 256 * 32) {
    return (int)std::min<long>((total + per_block - 1) / per_block, cap);
}

int fill_frame_prep(const char* who, const float* mean3, const float* std3, int to_rgb, int div_255, FramePrep* fp) {
    for (int k = 0; k < 3; ++k) {
        MVF_REQUIRE(std3[k] != 0.f, MVF_EINVAL, "%s: std[%d] is zero", who, k);
        fp->mean[k] = mean3[k];
        fp->stdinv[k] = (float)(1.0 / (double)std3[k]);      // the reference multiplies by 1 / float64(std)
    }
    fp->to_rgb = to_rgb;
    fp->div_255 = div_255;
    return MVF_OK;
}

// launch(out, color): `out` is out_stem as the element type's pointer, decltype(color)::value the kernel's COLOR
template <typename F>
void with_dtype_color(int dtype, bool color, void* out_stem, F launch) {
    if (dtype == MVF_F32 && !color) launch((float*)out_stem, std::false_type());
    else if (dtype == MVF_F32) launch((float*)out_stem, std::true_type());
    else if (!color) launch((bf16_t*)out_stem, std::false_type());
    else launch((bf16_t*)out_stem, std::true_type());
}

// Every resample export: one validation, one launch.  `src` is the kernels' address step; yuv != nullptr: the frames are YUV 4:2:0.
template <typename SRC>
int frames_resample(const char* who, const unsigned char* frames, const SRC& src, int n, const int* rows, const float* color, int h, int w,
                    const float* mean3, const float* std3, int to_rgb, int div_255, int pad, int wp, void* out_stem, float* out_nchw, int dtype,
                    void* stream, const YuvSrc* yuv = nullptr) {
    MVF_REQUIRE(frames && rows && mean3 && std3 && (out_stem || out_nchw) && n > 0 && h > 0 && w > 0 && pad >= 0, MVF_EINVAL, "%s: bad argument", who);
    MVF_REQUIRE(!out_stem || wp >= w + 2 * pad, MVF_EINVAL, "%s: wp=%d < w + 2*pad", who, wp);
    MVF_REQUIRE(dtype == MVF_F32 || dtype == MVF_BF16, MVF_EINVAL, "%s: bad dtype", who);
    FramePrep fp;
    if (const int rc = fill_frame_prep(who, mean3, std3, to_rgb, div_255, &fp)) return rc;
    const int p = out_stem ? pad : 0, wpp = out_stem ? wp : w;
    const int hp = h + 2 * p;
    MVF_REQUIRE((long)n * hp < (1L << 31), MVF_ESHAPE, "%s: too many rows", who);
    const dim3 grid(n * hp);
    const hipStream_t st = (hipStream_t)stream;
    with_dtype_color(dtype, color != nullptr, out_stem, [&](auto* out, auto col) {
        using ET = std::remove_pointer_t<decltype(out)>;
        constexpr bool COLOR = decltype(col)::value;
        if (yuv)
            hipLaunchKernelGGL((frames_yuv420_resample_kernel<ET, COLOR, SRC>), grid, dim3(256), 0, st, frames, *yuv, src, rows, color, h, w, fp, p, hp, wpp,
                               out, out_nchw);
        else
            hipLaunchKernelGGL((frames_resample_kernel<ET, COLOR, SRC>), grid, dim3(256), 0, st, frames, src, rows, color, h, w, fp, p, hp, wpp, out,
                               out_nchw);
    });
    MVF_LAUNCH_CHECK();
    return MVF_OK;
}

// mvf_frames_resample_u8 (color == nullptr), mvf_frames_resample_color_u8, mvf_frames_gather_resample_u8 (n = output images, of n_src source
// frames) and mvf_frames_yuv420_gather_resample_u8: the dense batch's own checks in front of frames_resample
int frames_resample_dense(const char* who, const unsigned char* frames_hwc, int n_src, int n, int hs, int ws, const int* src_index, const int* rows,
                          const float* color, int h, int w, const float* mean3, const float* std3, int to_rgb, int div_255, int pad, int wp,
                          void* out_stem, float* out_nchw, int dtype, void* stream, const YuvSrc* yuv = nullptr) {
    MVF_REQUIRE(n_src > 0 && hs > 0 && ws > 0, MVF_EINVAL, "%s: bad argument", who);
    MVF_REQUIRE(src_index || n_src == n || n <= 0, MVF_EINVAL, "%s: n_src=%d != n_out=%d without src_index", who, n_src, n);
    return frames_resample(who, frames_hwc, DenseSrc{src_index, hs, ws}, n, rows, color, h, w, mean3, std3, to_rgb, div_255, pad, wp, out_stem, out_nchw,
                           dtype, stream, yuv);
}

// The header's table of 20-bit conversion constants -> ys; the layout fields are the caller's
int fill_yuv_standard(const char* who, int standard, int order, YuvSrc* ys) {
    MVF_REQUIRE(standard >= 0 && standard <= 2, MVF_EINVAL, "%s: unknown standard %d (0 = BT.601 limited, 1 = BT.601 full, 2 = BT.709 limited)", who,
                standard);
    MVF_REQUIRE(order == 0 || order == 1, MVF_EINVAL, "%s: unknown order %d (0 = BGR, 1 = RGB)", who, order);
    // y_off, cY, cVR, cVG, cUG, cUB: the header's table
    static const double coef[3][6] = {{16, 1.164, 1.596, 0.813, 0.391, 2.018},
                                      {0, 1.0, 1.402, 0.714136, 0.344136, 1.772},
                                      {16, 1.164384, 1.792741, 0.532909, 0.213249, 2.112402}};
    const double* c = coef[standard];
    const double one = (double)(1 << 20);
    ys->y_off = (int)c[0];
    ys->cy = (int)rint(c[1] * one), ys->cvr = (int)rint(c[2] * one), ys->cvg = (int)rint(c[3] * one);
    ys->cug = (int)rint(c[4] * one), ys->cub = (int)rint(c[5] * one);
    ys->swap_rb = order == 0;
    return MVF_OK;
}

}  // namespace

extern "C" {

int mvf_frames_prep_u8(const unsigned char* frames_hwc, int n, int hs, int ws, const int* window, int h, int w,
                       const float* mean3, const float* std3, int to_rgb, int div_255, int pad, int wp, void* out_stem,
                       float* out_nchw, int dtype, void* stream) {
    MVF_REQUIRE(frames_hwc && mean3 && std3 && (out_stem || out_nchw) && n > 0 && hs > 0 && ws > 0 && h > 0 && w > 0 && h <= hs && w <= ws && pad >= 0,
                MVF_EINVAL, "frames_prep_u8: bad argument");
    MVF_REQUIRE(!out_stem || wp >= w + 2 * pad, MVF_EINVAL, "frames_prep_u8: wp=%d < w + 2*pad", wp);
    MVF_REQUIRE(dtype == MVF_F32 || dtype == MVF_BF16, MVF_EINVAL, "frames_prep_u8: bad dtype");
    FramePrep fp;
    if (const int rc = fill_frame_prep("frames_prep_u8", mean3, std3, to_rgb, div_255, &fp)) return rc;
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
    return frames_resample_dense("frames_resample_u8", frames_hwc, n, n, hs, ws, nullptr, rows, nullptr, h, w, mean3, std3, to_rgb, div_255, pad, wp,
                                 out_stem, out_nchw, dtype, stream);
}

int mvf_frames_resample_color_u8(const unsigned char* frames_hwc, int n, int hs, int ws, const int* rows, const float* color, int h, int w,
                                 const float* mean3, const float* std3, int to_rgb, int div_255, int pad, int wp, void* out_stem,
                                 float* out_nchw, int dtype, void* stream) {
    return frames_resample_dense("frames_resample_color_u8", frames_hwc, n, n, hs, ws, nullptr, rows, color, h, w, mean3, std3, to_rgb, div_255, pad,
                                 wp, out_stem, out_nchw, dtype, stream);
}

int mvf_frames_gather_resample_u8(const unsigned char* frames_hwc, int n_src, int hs, int ws, const int* src_index, int n_out, const int* rows,
                                  const float* color, int h, int w, const float* mean3, const float* std3, int to_rgb, int div_255, int pad,
                                  int wp, void* out_stem, float* out_nchw, int dtype, void* stream) {
    return frames_resample_dense("frames_gather_resample_u8", frames_hwc, n_src, n_out, hs, ws, src_index, rows, color, h, w, mean3, std3, to_rgb,
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
    YuvSrc ys;
    if (const int rc = fill_yuv_standard(who, standard, order, &ys)) return rc;
    ys.pitch = pitch;
    ys.cstride = layout == 0 ? pitch / 2 : pitch;
    ys.cstep = layout == 0 ? 1 : 2;
    ys.u_off = (long)hs * pitch;
    ys.v_delta = layout == 0 ? (long)(hs / 2) * (pitch / 2) : 1;
    ys.frame_bytes = (long)hs * pitch / 2 * 3;
    return frames_resample_dense(who, frames, n_src, n_out, hs, ws, src_index, rows, color, h, w, mean3, std3, to_rgb, div_255, pad, wp, out_stem,
                                 out_nchw, dtype, stream, &ys);
}

int mvf_frames_addressed_resample_u8(const unsigned char* frames, long long frames_bytes, int format, int standard, int order, int n_out,
                                     const int* rows, const int* addr, const float* color, int h, int w, const float* mean3, const float* std3,
                                     int to_rgb, int div_255, int pad, int wp, void* out_stem, float* out_nchw, int dtype, void* stream) {
    const char* who = "frames_addressed_resample_u8";
    MVF_REQUIRE(format >= 0 && format <= 2, MVF_EINVAL, "%s: unknown format %d (0 = packed, 1 = I420, 2 = NV12)", who, format);
    MVF_REQUIRE(frames_bytes >= 1 && frames_bytes < (1LL << 31), MVF_EINVAL, "%s: frames_bytes=%lld must lie in [1, 2^31): offsets are int32", who,
                frames_bytes);
    MVF_REQUIRE(addr, MVF_EINVAL, "%s: bad argument (addr is NULL)", who);
    YuvSrc ys = {};
    if (format != 0) {
        if (const int rc = fill_yuv_standard(who, standard, order, &ys)) return rc;
        ys.cstep = format == 1 ? 1 : 2;
    }
    return frames_resample(who, frames, AddressedSrc{addr}, n_out, rows, color, h, w, mean3, std3, to_rgb, div_255, pad, wp, out_stem, out_nchw, dtype,
                           stream, format != 0 ? &ys : nullptr);
}

}  // extern "C"
