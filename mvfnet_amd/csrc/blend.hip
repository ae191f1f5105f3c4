// Batch blending (Mixup / CutMix) on the stem operand, and the soft targets that go with it: mvf_stem_blend, mvf_soft_targets.
//
// mmaction-style fine-tuning recipes blend every clip of a batch with a partner clip (train_cfg=dict(blending=dict(type='MixupBlending', alpha=.2)) or
// 'CutmixBlending') and train against the blended labels.  The blend runs on the zero-padded channels-last stem operand (n*t, hp, wp, 4) that mvf_stem_prep
// and every uint8 frame kernel produce, so it works behind every input path, and out of place: clip i reads clip `partner`, which another workgroup may be
// writing at the same time if the result went back into xp.
//
// One table per step, two device arrays (the values never travel by value: a recorded launch plan replays them from the same buffers):
//   rows int32 (clips, 5): partner, y0, x0, y1, x1 -- a half-open box in image pixels (before the pad)
//   wts  fp32  (clips, 2): lam_px (weight of the clip's own pixel outside the box), lam_lab (weight of the clip's own label)
// Inside the box out = partner's element (a copy); elsewhere out = own element (a copy) when lam_px == 1 or partner == clip, else
// lam_px * a + (1 - lam_px) * b in fp32, rounded once to the storage type.  Border and fourth channel are zero in both operands and stay zero.
//
// Memory-bound: two planes read, one written.  A thread moves one 16-byte unit (one fp32 pixel, two bf16 pixels); the box test is per pixel, since a bf16 unit
// can straddle a box edge.  Operands that are not needed are not loaded (a unit wholly inside the box needs only b, one wholly outside with lam_px == 1 only a).
#include <algorithm>

#include "common.h"

namespace {

constexpr int kThreads = 256;

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return min(max(v, lo), hi); }

struct BlendRow {
    int partner, y0, x0, y1, x1;      // the box already shifted by the pad
    float lam;
};

__device__ __forceinline__ BlendRow load_row(const int* rows, const float* wts, int clip, int clips, int hp, int wp, int pad) {
    const int* r = rows + 5L * clip;
    BlendRow o;
    // a bad table cannot send a load outside the tensor: only `partner` enters an address, and it is clamped like the rest
    o.partner = clampi(r[0], 0, clips - 1);
    const int h = hp - 2 * pad, w = wp - 2 * pad;
    o.y0 = clampi(r[1], 0, h) + pad;
    o.x0 = clampi(r[2], 0, w) + pad;
    o.y1 = clampi(r[3], 0, h) + pad;
    o.x1 = clampi(r[4], 0, w) + pad;
    o.lam = fminf(fmaxf(wts[2L * clip], 0.f), 1.f);      // (fmaxf(NaN, 0) = 0)
    return o;
}

__device__ __forceinline__ float mix(float a, float b, float lam, float oml) { return lam * a + oml * b; }

// PX = pixels per 16-byte unit: 1 (fp32) or 2 (bf16).  units = hp * wp / PX per plane.  grid = (unit blocks, planes): plane = clip * t + frame.
template <int PX>
__global__ __launch_bounds__(kThreads) void stem_blend_kernel(const uint4* __restrict__ xp, int clips, int t, int hp, int wp, int pad, const int* __restrict__ rows,
                                                              const float* __restrict__ wts, uint4* __restrict__ out, int units) {
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
    const int planes = clips * t;
    for (int plane = blockIdx.y; plane < planes; plane += gridDim.y) {
        const int clip = plane / t, f = plane - clip * t;
        const BlendRow r = load_row(rows, wts, clip, clips, hp, wp, pad);
        bool in[PX], any_in = false, any_out = false;
#pragma unroll
        for (int j = 0; j < PX; ++j) {
            in[j] = py[j] >= r.y0 && py[j] < r.y1 && px[j] >= r.x0 && px[j] < r.x1;
            any_in |= in[j];
            any_out |= !in[j];
        }
        const bool copy_a = r.lam == 1.f || r.partner == clip;
        const long ia = (long)plane * units + u, ib = ((long)r.partner * t + f) * units + u;
        uint4 a = make_uint4(0, 0, 0, 0), b = a, o;
        if (any_out) a = xp[ia];
        if (any_in || !copy_a) b = xp[ib];
        if (PX == 1) {
            if (in[0]) o = b;
            else if (copy_a) o = a;
            else {
                const float lam = r.lam, oml = 1.f - r.lam;
                o.x = __float_as_uint(mix(__uint_as_float(a.x), __uint_as_float(b.x), lam, oml));
                o.y = __float_as_uint(mix(__uint_as_float(a.y), __uint_as_float(b.y), lam, oml));
                o.z = __float_as_uint(mix(__uint_as_float(a.z), __uint_as_float(b.z), lam, oml));
                o.w = __float_as_uint(mix(__uint_as_float(a.w), __uint_as_float(b.w), lam, oml));
            }
        } else {
            const float lam = r.lam, oml = 1.f - r.lam;
            const uint32_t aw[4] = {a.x, a.y, a.z, a.w}, bw[4] = {b.x, b.y, b.z, b.w};
            uint32_t ow[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {             // word q = two bf16 channels of pixel q / 2
                const int j = (q >> 1) & (PX - 1);
                if (in[j]) ow[q] = bw[q];
                else if (copy_a) ow[q] = aw[q];
                else
                    ow[q] = pack_bf16x2(mix(__uint_as_float(aw[q] << 16), __uint_as_float(bw[q] << 16), lam, oml),
                                        mix(__uint_as_float(aw[q] & 0xffff0000u), __uint_as_float(bw[q] & 0xffff0000u), lam, oml));
            }
            o = make_uint4(ow[0], ow[1], ow[2], ow[3]);
        }
        out[ia] = o;
    }
}

// targets[clip][k] = (1 - eps) * (lam * [k == y] + (1 - lam) * [k == y_partner]) + eps / classes; one workgroup per clip.  eps == 0: exactly lam, 1.0f - lam
// (or their fp32 sum where both labels coincide).
__global__ __launch_bounds__(kThreads) void soft_targets_kernel(const long long* __restrict__ labels, const int* __restrict__ rows, const float* __restrict__ wts,
                                                                int clips, int classes, float eps, float* __restrict__ targets) {
    const int clip = blockIdx.x;
    long long y = labels[clip], yp = y;
    float lam = 1.f;
    if (rows) {
        yp = labels[clampi(rows[5L * clip], 0, clips - 1)];
        lam = fminf(fmaxf(wts[2L * clip + 1], 0.f), 1.f);
    }
    const float oml = 1.0f - lam, keep = 1.0f - eps, uni = eps / (float)classes;
    float* trow = targets + (long)clip * classes;
    for (int k = threadIdx.x; k < classes; k += kThreads) {
        const float v = (k == y ? lam : 0.f) + (k == yp ? oml : 0.f);
        trow[k] = eps == 0.f ? v : keep * v + uni;
    }
}

}  // namespace

extern "C" {

int mvf_stem_blend(const void* xp, int clips, int t, int hp, int wp, int pad, const int* rows, const float* wts, void* out, int dtype, void* stream) {
    MVF_REQUIRE(clips > 0 && t > 0 && hp > 0 && wp > 0 && pad >= 0 && 2 * pad <= hp && 2 * pad <= wp, MVF_EINVAL,
                "stem_blend: bad argument (clips=%d t=%d hp=%d wp=%d pad=%d)", clips, t, hp, wp, pad);
    MVF_REQUIRE(dtype == MVF_F32 || dtype == MVF_BF16, MVF_EINVAL, "stem_blend: dtype %d", dtype);
    MVF_REQUIRE(xp && out && rows && wts, MVF_EINVAL, "stem_blend: NULL argument");
    const int px = dtype == MVF_F32 ? 1 : 2;
    const long plane_px = (long)hp * wp;
    MVF_REQUIRE(plane_px % px == 0, MVF_ESHAPE, "stem_blend: a bf16 plane of %d x %d pixels is not a whole number of 16-byte units", hp, wp);
    MVF_REQUIRE(plane_px / px < (1L << 31) - kThreads && (long)clips * t < (1L << 31), MVF_ESHAPE, "stem_blend: plane or batch too large");
    const uintptr_t pa = (uintptr_t)xp, po = (uintptr_t)out;
    const uintptr_t bytes = (uintptr_t)clips * t * (uintptr_t)(plane_px / px) * 16;
    // clip i reads clip `partner`: in place, a workgroup would read planes another one is overwriting
    MVF_REQUIRE(pa + bytes <= po || po + bytes <= pa, MVF_EINVAL, "stem_blend: out overlaps xp (the blend is out of place)");
    MVF_REQUIRE(pa % 16 == 0 && po % 16 == 0, MVF_EINVAL, "stem_blend: xp / out must be 16-byte aligned");
    const int units = (int)(plane_px / px);
    const dim3 grid((units + kThreads - 1) / kThreads, (unsigned)std::min<long>((long)clips * t, 65535));
    hipStream_t st = (hipStream_t)stream;
    if (px == 1)
        hipLaunchKernelGGL(stem_blend_kernel<1>, grid, dim3(kThreads), 0, st, (const uint4*)xp, clips, t, hp, wp, pad, rows, wts, (uint4*)out, units);
    else
        hipLaunchKernelGGL(stem_blend_kernel<2>, grid, dim3(kThreads), 0, st, (const uint4*)xp, clips, t, hp, wp, pad, rows, wts, (uint4*)out, units);
    MVF_LAUNCH_CHECK();
    return MVF_OK;
}

int mvf_soft_targets(const long long* labels, const int* rows, const float* wts, int clips, int classes, float eps, float* targets, void* stream) {
    MVF_REQUIRE(clips > 0 && classes > 0, MVF_EINVAL, "soft_targets: bad argument (clips=%d classes=%d)", clips, classes);
    MVF_REQUIRE(eps >= 0.f && eps < 1.f, MVF_EINVAL, "soft_targets: eps=%g is outside [0, 1)", (double)eps);
    MVF_REQUIRE(labels && targets, MVF_EINVAL, "soft_targets: NULL argument");
    MVF_REQUIRE(!rows || wts, MVF_EINVAL, "soft_targets: rows without wts");
    hipLaunchKernelGGL(soft_targets_kernel, dim3(clips), dim3(kThreads), 0, (hipStream_t)stream, labels, rows, wts, clips, classes, eps, targets);
    MVF_LAUNCH_CHECK();
    return MVF_OK;
}

}  // extern "C"
