// RandAugment on the uploaded uint8 frames, in front of the frame kernels: mvf_frames_randaug_u8.
//
// timm's RandAugment (`rand-m7-n4-mstd0.5-inc1` in the PySlowFast / VideoMAE / mmaction2 fine-tuning recipes) applies `layers` ops to every frame of a clip,
// one draw per clip, BEFORE the random-resized crop.  Its ops are defined on 8-bit images -- bit masks, histograms, truncating blends --, so they run here on
// the bytes of the dense (n, hs, ws, 3) batch the frame kernels read, not on the normalised stem operand where erasing and blending live.  The host draws the
// table (mvfnet_amd/randaug.py); include/mvfnet_hip.h states the arithmetic of every kind, and that text is the specification.
//
// Per layer at most two launches:
//   statistics (only when the layer's bit of stats_layers is set): ONE workgroup per frame.  Kinds 5 / 6 build the three channel histograms in LDS with
//       integer atomics, kind 8 the 64-bit sum of the grey image; the same workgroup then turns them into what the apply pass needs -- the 3 x 256-byte lookup
//       table, or the grey mean -- and stores that into the frame's slot of the workspace.  Integer adds only: the result does not depend on their order, and
//       nothing has to be zeroed between layers.  A frame of any other kind returns before its first load.
//   apply: a workgroup works on one frame, so the kind is a uniform branch.  A thread owns an ALIGNED dword of the batch buffer: source, destination and
//       scratch are 4-byte aligned and have the same layout, so the four bytes of a pointwise op come from one dword load and go out in one dword store
//       although neither ws_i * 3 nor a frame's base (i * hs * ws * 3) is a multiple of 4.  The dword a frame shares with its neighbour is the only one loaded
//       and stored by bytes (the neighbour's workgroup writes its other bytes).  The neighbourhood kinds (9 colour, 10 sharpness, 11 affine) read their taps by
//       bytes -- they hit the lines the dword loads of the neighbouring threads bring in -- and still store dwords.
// Everything a thread addresses lies inside its own frame's hs x ws x 3 bytes: hs_i / ws_i are clamped to the extent, taps are clamped to the image.
// No float atomics, no cross-workgroup communication: bit-identical from run to run.
#include <algorithm>

#include "common.h"

// blends round every fp32 operation on its own, the affine map and the autocontrast table every fp64 one: no fused multiply-add anywhere in this file
#pragma clang fp contract(off)

namespace {

constexpr int kApplyThreads = 256;
constexpr int kApplyDwords = 4;                     // dwords per thread and workgroup pass
constexpr int kChunk = kApplyThreads * kApplyDwords;
constexpr int kStatsThreads = 1024;
constexpr int kLutBytes = 3 * 256;
constexpr int kFrameWs = MVF_RANDAUG_WS_PER_FRAME;  // lookup tables, then the grey mean
constexpr int kTableWords = 16;

enum { kIdentity = 0, kInvert, kPosterize, kSolarize, kSolarizeAdd, kAutoContrast, kEqualize, kBrightness, kContrast, kColor, kSharpness, kAffine };

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

__device__ __forceinline__ int grey_of(int c0, int c1, int c2, int order) {
    const int r = order ? c0 : c2, b = order ? c2 : c0;
    return (r * 19595 + c1 * 38470 + b * 7471 + 0x8000) >> 16;
}

__device__ __forceinline__ int blend_u8(float d, float f, float p) {
    float v = d + f * (p - d);
    if (!(f >= 0.0f && f <= 1.0f)) v = fminf(fmaxf(v, 0.0f), 255.0f);
    return (int)v;
}

// the frame's own image size, clamped to the padded extent
__device__ __forceinline__ void frame_size(const int* sizes, int f, int hs, int ws, int& hi, int& wi) {
    hi = sizes ? clampi(sizes[2 * f], 0, hs) : hs;
    wi = sizes ? clampi(sizes[2 * f + 1], 0, ws) : ws;
}

// ---- statistics: one workgroup per frame ------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kStatsThreads) void randaug_stats_kernel(const uint8_t* __restrict__ src, int hs, int ws, int t, int order,
                                                                      const int* __restrict__ sizes, const int* __restrict__ table, int layers, int layer,
                                                                      uint8_t* __restrict__ workspace) {
    const int f = blockIdx.x, tid = threadIdx.x;
    const int kind = table[((long)(f / t) * layers + layer) * kTableWords];
    if (kind != kAutoContrast && kind != kEqualize && kind != kContrast) return;          // uniform: this frame loads nothing
    __shared__ unsigned hist[kLutBytes];
    __shared__ unsigned long long gsum;
    __shared__ int lohi[6];
    __shared__ uint32_t lut_w[kLutBytes / 4];
    uint8_t* lut = reinterpret_cast<uint8_t*>(lut_w);
    if (tid < kLutBytes) hist[tid] = 0u;
    if (tid == 0) gsum = 0ull;
    __syncthreads();
    int hi, wi;
    frame_size(sizes, f, hs, ws, hi, wi);
    const int pitch = ws * 3, rowb = wi * 3;
    const long fb = (long)f * hs * pitch, fe = fb + (long)hi * pitch;                      // the rows that hold the image
    const uint8_t* fsrc = src + fb;
    unsigned long long gs = 0ull;
    for (long d = (fb >> 2) + tid; d * 4 < fe; d += kStatsThreads) {
        const long a0 = d * 4;
        const bool full = a0 >= fb && a0 + 4 <= fe;
        uint32_t word = 0u;
        if (full) word = reinterpret_cast<const uint32_t*>(src)[d];
        const int k0 = (int)(max(a0, fb) - fb);
        int xb = k0 % pitch;
        for (long a = max(a0, fb); a < min(a0 + 4, fe); ++a) {
            if (xb < rowb) {
                const int p = full ? (int)((word >> (8 * (int)(a - a0))) & 255u) : (int)src[a];
                const int c = xb % 3;
                if (kind != kContrast) {
                    atomicAdd(&hist[c * 256 + p], 1u);
                } else if (c == 0) {                                                       // the thread that owns a pixel's first byte adds its grey
                    const int k = (int)(a - fb);
                    gs += (unsigned)grey_of(p, fsrc[k + 1], fsrc[k + 2], order);
                }
            }
            if (++xb == pitch) xb = 0;
        }
    }
    if (kind == kContrast) {
        for (int o = 32; o > 0; o >>= 1) gs += __shfl_down(gs, o);
        if ((tid & 63) == 0) atomicAdd(&gsum, gs);
    }
    __syncthreads();
    uint8_t* slot = workspace + (long)f * kFrameWs;
    if (kind == kContrast) {
        if (tid == 0) {
            const unsigned long long n = (unsigned long long)hi * wi;
            *reinterpret_cast<int*>(slot + kLutBytes) = n ? (int)((2ull * gsum + n) / (2ull * n)) : 0;
        }
        return;
    }
    if (kind == kAutoContrast) {
        if (tid < 3) {
            int lo = 256, top = -1;
            for (int i = 0; i < 256; ++i)
                if (hist[tid * 256 + i]) {
                    lo = min(lo, i);
                    top = i;
                }
            lohi[2 * tid] = lo, lohi[2 * tid + 1] = top;
        }
        __syncthreads();
        if (tid < kLutBytes) {
            const int c = tid >> 8, i = tid & 255, lo = lohi[2 * c], top = lohi[2 * c + 1];
            int v = i;
            if (top > lo) {
                const double scale = 255.0 / (double)(top - lo), off = (double)(-lo) * scale;
                v = clampi((int)((double)i * scale + off), 0, 255);
            }
            lut[tid] = (uint8_t)v;
        }
    } else {
        if (tid < 3) {
            const unsigned* h = hist + tid * 256;
            unsigned total = 0u, last = 0u;
            int bins = 0;
            for (int i = 0; i < 256; ++i)
                if (h[i]) total += h[i], last = h[i], ++bins;
            const unsigned step = bins > 1 ? (total - last) / 255u : 0u;
            unsigned acc = step / 2u;
            for (int i = 0; i < 256; ++i) {
                lut[tid * 256 + i] = (uint8_t)(step ? min(255u, acc / step) : (unsigned)i);
                acc += h[i];
            }
        }
    }
    __syncthreads();
    if (tid < kLutBytes / 4) reinterpret_cast<uint32_t*>(slot)[tid] = lut_w[tid];
}

// ---- apply ------------------------------------------------------------------------------------------------------------------------------------------------
struct OpArgs {
    int kind, order, w1, w2, mean;
    float fac;
    double co[6];
    uint32_t fill;
};

// output byte (y, xb) of the frame's image (xb = 3 x + c), p = the input byte there; fsrc = the frame's first byte
__device__ __forceinline__ int apply_byte(const OpArgs& op, const uint8_t* __restrict__ fsrc, const uint8_t* __restrict__ lut, int pitch, int hi, int wi,
                                          int y, int xb, int p) {
    switch (op.kind) {
        case kInvert: return 255 - p;
        case kPosterize: return p & op.w1;
        case kSolarize: return p < op.w1 ? p : 255 - p;
        case kSolarizeAdd: return p < op.w1 ? min(255, p + op.w2) : p;
        case kAutoContrast:
        case kEqualize: return lut[(xb % 3) * 256 + p];
        case kBrightness: return blend_u8(0.0f, op.fac, (float)p);
        case kContrast: return blend_u8((float)op.mean, op.fac, (float)p);
        case kColor: {
            const uint8_t* px = fsrc + (long)y * pitch + (xb - xb % 3);
            return blend_u8((float)grey_of(px[0], px[1], px[2], op.order), op.fac, (float)p);
        }
        case kSharpness: {
            const int x = xb / 3;
            if (hi < 3 || wi < 3 || y == 0 || y == hi - 1 || x == 0 || x == wi - 1) return p;
            const uint8_t* r0 = fsrc + (long)(y - 1) * pitch + xb;
            const uint8_t *r1 = r0 + pitch, *r2 = r1 + pitch;
            const int acc = r0[-3] + r0[0] + r0[3] + r1[-3] + 5 * p + r1[3] + r2[-3] + r2[0] + r2[3];
            return blend_u8((float)((2 * acc + 13) / 26), op.fac, (float)p);
        }
        case kAffine: {
            const int x = xb / 3, c = xb - 3 * x;
            const double xc = (double)x + 0.5, yc = (double)y + 0.5;
            double xin = (op.co[0] * xc + op.co[1] * yc) + op.co[2];
            double yin = (op.co[3] * xc + op.co[4] * yc) + op.co[5];
            if (!(xin >= 0.0 && xin < (double)wi && yin >= 0.0 && yin < (double)hi)) return (int)((op.fill >> (8 * c)) & 255u);
            xin -= 0.5, yin -= 0.5;
            const double fx = floor(xin), fy = floor(yin);
            const double dx = xin - fx, dy = yin - fy;
            const int x0 = (int)fx, y0 = (int)fy;
            const int xa = clampi(x0, 0, wi - 1) * 3 + c, xq = clampi(x0 + 1, 0, wi - 1) * 3 + c;
            const uint8_t* ra = fsrc + (long)clampi(y0, 0, hi - 1) * pitch;
            const double pa = (double)ra[xa], qa = (double)ra[xq];
            const double v1 = pa + (qa - pa) * dx;
            double v2 = v1;
            if (y0 + 1 >= 0 && y0 + 1 < hi) {
                const uint8_t* rb = fsrc + (long)(y0 + 1) * pitch;
                const double pb = (double)rb[xa], qb = (double)rb[xq];
                v2 = pb + (qb - pb) * dx;
            }
            return (int)(v1 + (v2 - v1) * dy);
        }
        default: return p;                                                                   // identity, and any kind the table should not hold
    }
}

// grid.x = n * chunks; workgroup w works on frame w / chunks, dwords [chunk * kChunk, ...) of the aligned dwords that cover the frame
__global__ __launch_bounds__(kApplyThreads) void randaug_apply_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int hs, int ws, int t, int order,
                                                                      const int* __restrict__ sizes, const int* __restrict__ table, int layers, int layer,
                                                                      const uint8_t* __restrict__ workspace, int chunks) {
    const int f = blockIdx.x / chunks, chunk = blockIdx.x - f * chunks, tid = threadIdx.x;
    const int* row = table + ((long)(f / t) * layers + layer) * kTableWords;
    OpArgs op;
    op.kind = row[0], op.order = order, op.w1 = row[1], op.w2 = row[2], op.fac = __int_as_float(row[1]), op.fill = (uint32_t)row[13], op.mean = 0;
#pragma unroll
    for (int j = 0; j < 6; ++j) op.co[j] = __hiloint2double(row[2 + 2 * j], row[1 + 2 * j]);
    __shared__ uint32_t lut_w[kLutBytes / 4];
    const uint8_t* slot = workspace + (long)f * kFrameWs;
    if (op.kind == kAutoContrast || op.kind == kEqualize) {                                  // uniform
        if (tid < kLutBytes / 4) lut_w[tid] = reinterpret_cast<const uint32_t*>(slot)[tid];
        __syncthreads();
    } else if (op.kind == kContrast) {
        op.mean = *reinterpret_cast<const int*>(slot + kLutBytes);
    }
    const uint8_t* lut = reinterpret_cast<const uint8_t*>(lut_w);
    int hi, wi;
    frame_size(sizes, f, hs, ws, hi, wi);
    const int pitch = ws * 3, rowb = wi * 3;
    const long fb = (long)f * hs * pitch, fe = fb + (long)hs * pitch;
    const uint8_t* fsrc = src + fb;
#pragma unroll
    for (int it = 0; it < kApplyDwords; ++it) {
        const long d = (fb >> 2) + (long)chunk * kChunk + it * kApplyThreads + tid;
        const long a0 = d * 4;
        if (a0 >= fe) break;
        const bool full = a0 >= fb && a0 + 4 <= fe;
        const long lo = max(a0, fb), hi_a = min(a0 + 4, fe);
        uint32_t word = 0u;
        if (full) word = reinterpret_cast<const uint32_t*>(src)[d];
        const int k0 = (int)(lo - fb);
        int y = k0 / pitch, xb = k0 - y * pitch;
        uint32_t outw = 0u;
        for (long a = lo; a < hi_a; ++a) {
            const int sh = 8 * (int)(a - a0);
            const int p = full ? (int)((word >> sh) & 255u) : (int)src[a];
            const int v = (y < hi && xb < rowb) ? apply_byte(op, fsrc, lut, pitch, hi, wi, y, xb, p) : p;
            if (full)
                outw |= (uint32_t)(v & 255) << sh;
            else
                dst[a] = (uint8_t)v;
            if (++xb == pitch) xb = 0, ++y;
        }
        if (full) reinterpret_cast<uint32_t*>(dst)[d] = outw;
    }
}

}  // namespace

extern "C" {

int mvf_frames_randaug_u8(const unsigned char* frames_hwc, int n, int hs, int ws, int t, int order, const int* sizes, const int* table, int layers,
                          unsigned stats_layers, unsigned char* out, unsigned char* tmp, void* workspace, long long workspace_bytes, void* stream) {
    MVF_REQUIRE(n > 0 && hs > 0 && ws > 0 && t > 0, MVF_EINVAL, "frames_randaug: bad argument (n=%d hs=%d ws=%d t=%d)", n, hs, ws, t);
    MVF_REQUIRE(n % t == 0, MVF_EINVAL, "frames_randaug: n=%d is not a multiple of t=%d", n, t);
    MVF_REQUIRE(order == 0 || order == 1, MVF_EINVAL, "frames_randaug: order %d (0 = BGR, 1 = RGB)", order);
    MVF_REQUIRE(layers >= 1 && layers <= 8, MVF_EINVAL, "frames_randaug: layers=%d is outside [1, 8]", layers);
    MVF_REQUIRE((stats_layers >> layers) == 0u, MVF_EINVAL, "frames_randaug: stats_layers=0x%x names a layer at or above layers=%d", stats_layers, layers);
    MVF_REQUIRE(frames_hwc && table && out && tmp && workspace, MVF_EINVAL, "frames_randaug: NULL argument");
    MVF_REQUIRE(out != tmp && out != frames_hwc && tmp != frames_hwc, MVF_EINVAL, "frames_randaug: frames_hwc, out and tmp must be three buffers");
    MVF_REQUIRE((uintptr_t)frames_hwc % 4 == 0 && (uintptr_t)out % 4 == 0 && (uintptr_t)tmp % 4 == 0 && (uintptr_t)table % 4 == 0 &&
                    (uintptr_t)sizes % 4 == 0 && (uintptr_t)workspace % 4 == 0,
                MVF_EINVAL, "frames_randaug: frames_hwc / out / tmp / sizes / table / workspace must be 4-byte aligned");
    MVF_REQUIRE(workspace_bytes >= (long long)n * kFrameWs, MVF_EINVAL, "frames_randaug: workspace of %lld bytes, %lld needed (n * (3 * 256 + 16))",
                workspace_bytes, (long long)n * kFrameWs);
    const long long frame_bytes = (long long)hs * ws * 3;
    MVF_REQUIRE(frame_bytes < (1LL << 31) - 8, MVF_ESHAPE, "frames_randaug: a frame of %d x %d pixels is too large", hs, ws);
    // the aligned dwords that cover a frame: frame_bytes / 4, plus one where its base or its end is not aligned
    const int chunks = (int)((frame_bytes / 4 + 2 + kChunk - 1) / kChunk);
    MVF_REQUIRE((long long)n * chunks < (1LL << 31), MVF_ESHAPE, "frames_randaug: %d frames of %d x %d pixels are more than 2^31 workgroups", n, hs, ws);
    hipStream_t st = (hipStream_t)stream;
    const unsigned char* src = frames_hwc;
    for (int k = 0; k < layers; ++k) {
        unsigned char* dst = (layers - 1 - k) % 2 == 0 ? out : tmp;                          // the last layer writes out
        if (stats_layers >> k & 1u) {
            hipLaunchKernelGGL(randaug_stats_kernel, dim3(n), dim3(kStatsThreads), 0, st, src, hs, ws, t, order, sizes, table, layers, k, (uint8_t*)workspace);
            MVF_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL(randaug_apply_kernel, dim3((unsigned)(n * chunks)), dim3(kApplyThreads), 0, st, src, dst, hs, ws, t, order, sizes, table, layers, k,
                           (const uint8_t*)workspace, chunks);
        MVF_LAUNCH_CHECK();
        src = dst;
    }
    return MVF_OK;
}

}  // extern "C"
