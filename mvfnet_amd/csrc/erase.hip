// RandomErasing on the stem operand, with the noise made in the kernel: mvf_stem_erase.
//
// The fine-tuning recipes for small sets erase up to a third of every clip (timm's RandomErasing, unchanged in PySlowFast and mmaction2) and fill the boxes with
// a constant colour or with per-element N(0, 1) noise.  Like the blend (blend.hip) it runs on the zero-padded channels-last stem operand (planes, hp, wp, 4) that
// mvf_stem_prep and every uint8 frame kernel produce, so it works behind every input path; unlike the blend IN PLACE: no plane reads another plane, and a
// thread reads at most the one 16-byte unit it writes.
//
// One table per step, three device arrays (nothing that changes from step to step travels by value: a recorded launch plan replays them from the same buffers):
//   boxes int32 (planes, max_boxes, 5): y0, x0, y1, x1, mode -- a half-open box in image pixels (before the pad); mode 0 = unused slot, 1 = constant colour,
//                                       2 = per-element noise, anything else = unused.  Where boxes of a plane overlap the higher index wins.
//   fill  fp32  (planes, max_boxes, 4): mode 1: the colour of channels 0..2 (word 3 is ignored)
//   key   uint32 (2): the step's generator key
// Noise: w = Philox4x32-10(counter = (x, y, plane, 0), key) in IMAGE coordinates, two Box-Muller pairs from the four words (include/mvfnet_hip.h states the
// arithmetic; it is the specification), fp32 with the accurate math functions, rounded once to the storage type.  The counter does not know the storage
// layout, the box index or the grid, so fp32 and bf16 operands see the same noise and every cut of the grid gives the same bits.
//
// Memory-bound, and it writes at most the erased share of the operand: a thread owns one 16-byte unit (one fp32 pixel, two bf16 pixels); a unit no box touches
// costs neither a load nor a store, a unit wholly inside boxes is stored without being loaded, and a bf16 unit that straddles a box edge is read, modified per
// pixel and written by the one thread that owns it.  The plane's boxes are the same for the whole workgroup: scalar loads, once per plane.  No atomics, no
// LDS, no cross-thread communication: bit-identical from run to run.
#include <algorithm>

#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxBoxes = 8;

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

struct Philox4 {
    uint32_t w0, w1, w2, w3;
};

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): ten rounds, the key bumped by the Weyl constants between rounds
__device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
    constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(M0, c0), lo0 = M0 * c0, hi1 = __umulhi(M1, c2), lo1 = M1 * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += W0;
        k1 += W1;
    }
    return Philox4{c0, c1, c2, c3};
}

// the three N(0, 1) values of image pixel (x, y) of `plane`: channel 0 / 1 = the cosine / sine branch of the first Box-Muller pair, channel 2 = the cosine
// branch of the second.  u1, u3 in (0, 1] (the logarithm's argument is never 0), u2, u4 in [0, 1); all four are exact in fp32.
__device__ __forceinline__ void noise3(int x, int y, int plane, uint32_t k0, uint32_t k1, float v[3]) {
    const Philox4 w = philox4x32_10((uint32_t)x, (uint32_t)y, (uint32_t)plane, 0u, k0, k1);
    constexpr float kInv24 = 1.0f / 16777216.0f, kTwoPi = 6.283185307179586f;
    const float u1 = (float)((w.w0 >> 8) + 1u) * kInv24, u2 = (float)(w.w1 >> 8) * kInv24;
    const float u3 = (float)((w.w2 >> 8) + 1u) * kInv24, u4 = (float)(w.w3 >> 8) * kInv24;
    const float r1 = sqrtf(-2.0f * logf(u1)), t1 = kTwoPi * u2;
    const float r2 = sqrtf(-2.0f * logf(u3)), t2 = kTwoPi * u4;
    v[0] = r1 * cosf(t1);
    v[1] = r1 * sinf(t1);
    v[2] = r2 * cosf(t2);
}

// PX = pixels per 16-byte unit: 1 (fp32) or 2 (bf16).  units = hp * wp / PX per plane.  grid = (unit blocks, planes).
template <int PX>
__global__ __launch_bounds__(kThreads) void stem_erase_kernel(uint4* __restrict__ xp, int planes, int hp, int wp, int pad, const int* __restrict__ boxes,
                                                              int max_boxes, const float* __restrict__ fill, const uint32_t* __restrict__ key, int units) {
    const int u = blockIdx.x * kThreads + threadIdx.x;
    if (u >= units) return;
    // the unit's pixels: the same for every plane this thread visits
    int py[PX], px[PX];
#pragma unroll
    for (int j = 0; j < PX; ++j) {
        const int p = u * PX + j;
        py[j] = p / wp;
        px[j] = p - py[j] * wp;
    }
    const int h = hp - 2 * pad, w = wp - 2 * pad;
    const uint32_t k0 = key[0], k1 = key[1];
    for (int plane = blockIdx.y; plane < planes; plane += gridDim.y) {
        // the winning box of each pixel: the last slot that holds it.  A box is clamped to the image (as load_row of blend.hip clamps), so a bad table
        // cannot address outside the tensor and no box ever holds a pixel of the border or of the padding columns.
        const int* pb = boxes + (long)plane * max_boxes * 5;
        int win[PX], mode[PX];
#pragma unroll
        for (int j = 0; j < PX; ++j) win[j] = -1, mode[j] = 0;
        for (int k = 0; k < max_boxes; ++k) {
            const int m = pb[5 * k + 4];
            if (m != 1 && m != 2) continue;
            const int y0 = clampi(pb[5 * k], 0, h) + pad, x0 = clampi(pb[5 * k + 1], 0, w) + pad;
            const int y1 = clampi(pb[5 * k + 2], 0, h) + pad, x1 = clampi(pb[5 * k + 3], 0, w) + pad;
#pragma unroll
            for (int j = 0; j < PX; ++j)
                if (py[j] >= y0 && py[j] < y1 && px[j] >= x0 && px[j] < x1) win[j] = k, mode[j] = m;
        }
        bool any = false, all = true;
#pragma unroll
        for (int j = 0; j < PX; ++j) {
            any |= win[j] >= 0;
            all &= win[j] >= 0;
        }
        if (!any) continue;                                  // neither a load nor a store
        const long iu = (long)plane * units + u;
        uint4 o = make_uint4(0, 0, 0, 0);
        if (!all) o = xp[iu];                                // (bf16 only) the unit straddles a box edge: the other pixel keeps its bits
        uint32_t ow[4] = {o.x, o.y, o.z, o.w};
#pragma unroll
        for (int j = 0; j < PX; ++j) {
            if (win[j] < 0) continue;
            float v[3];
            if (mode[j] == 2) {
                noise3(px[j] - pad, py[j] - pad, plane, k0, k1, v);
            } else {
                const float* pf = fill + ((long)plane * max_boxes + win[j]) * 4;
                v[0] = pf[0], v[1] = pf[1], v[2] = pf[2];
            }
            // the fourth channel is zero in the operand and is stored as zero
            if (PX == 1) {
                ow[0] = __float_as_uint(v[0]), ow[1] = __float_as_uint(v[1]), ow[2] = __float_as_uint(v[2]), ow[3] = 0u;
            } else {
                ow[2 * j] = pack_bf16x2(v[0], v[1]);
                ow[2 * j + 1] = pack_bf16x2(v[2], 0.f);
            }
        }
        xp[iu] = make_uint4(ow[0], ow[1], ow[2], ow[3]);
    }
}

}  // namespace

extern "C" {

int mvf_stem_erase(void* xp, int planes, int hp, int wp, int pad, const int* boxes, int max_boxes, const float* fill, const unsigned int* key, int dtype,
                   void* stream) {
    MVF_REQUIRE(planes > 0 && hp > 0 && wp > 0 && pad >= 0 && 2 * pad <= hp && 2 * pad <= wp, MVF_EINVAL,
                "stem_erase: bad argument (planes=%d hp=%d wp=%d pad=%d)", planes, hp, wp, pad);
    MVF_REQUIRE(dtype == MVF_F32 || dtype == MVF_BF16, MVF_EINVAL, "stem_erase: dtype %d", dtype);
    MVF_REQUIRE(max_boxes >= 1 && max_boxes <= kMaxBoxes, MVF_EINVAL, "stem_erase: max_boxes=%d is outside [1, %d]", max_boxes, kMaxBoxes);
    MVF_REQUIRE(xp && boxes && fill && key, MVF_EINVAL, "stem_erase: NULL argument");
    const int px = dtype == MVF_F32 ? 1 : 2;
    const long plane_px = (long)hp * wp;
    MVF_REQUIRE(plane_px % px == 0, MVF_ESHAPE, "stem_erase: a bf16 plane of %d x %d pixels is not a whole number of 16-byte units", hp, wp);
    MVF_REQUIRE(plane_px / px < (1L << 31) - kThreads, MVF_ESHAPE, "stem_erase: plane too large");
    MVF_REQUIRE((uintptr_t)xp % 16 == 0, MVF_EINVAL, "stem_erase: xp must be 16-byte aligned");
    MVF_REQUIRE((uintptr_t)boxes % 4 == 0 && (uintptr_t)fill % 4 == 0 && (uintptr_t)key % 4 == 0, MVF_EINVAL, "stem_erase: boxes / fill / key must be 4-byte aligned");
    const int units = (int)(plane_px / px);
    const dim3 grid((units + kThreads - 1) / kThreads, (unsigned)std::min(planes, 65535));
    hipStream_t st = (hipStream_t)stream;
    if (px == 1)
        hipLaunchKernelGGL(stem_erase_kernel<1>, grid, dim3(kThreads), 0, st, (uint4*)xp, planes, hp, wp, pad, boxes, max_boxes, fill, key, units);
    else
        hipLaunchKernelGGL(stem_erase_kernel<2>, grid, dim3(kThreads), 0, st, (uint4*)xp, planes, hp, wp, pad, boxes, max_boxes, fill, key, units);
    MVF_LAUNCH_CHECK();
    return MVF_OK;
}

}  // extern "C"
