// Stochastic depth (drop path) on the residual branch of a bottleneck: out = relu(s * bn3(conv3(a2)) + identity) with one fp32 scale s per IMAGE
// (timm drop_path(x, p, training, scale_by_keep): s = Bernoulli(1 - p) / (1 - p), drawn on the host per clip or per frame -- droppath.py -- and uploaded as
// a table of one value per image, so the kernels do not know the unit).  Two byte-bound streams over channels-last [M][C] matrices:
//   mvf_bn_apply_bits_rowscale   mvf_bn_apply_bits with the BatchNorm output scaled per row before the residual is added (forward)
//   mvf_gate_rowscale            gm = [out > 0] * s * g from the sign bits (backward: the gradient into bn3's output; the identity path keeps g and the bits)
// Column-tiled as the BatchNorm kernels of train_ops.hip: a lane owns VN channels (16 bytes: 4 fp32 / 8 bf16; 8 bytes for bf16 with c % 8 == 4) and walks
// rows; a row's image index is carried along the walk (one division per lane at its first row), its scale is one load per row.  No atomics, no reductions:
// every element is a function of its own operands, so results are bit-identical from run to run.
#include <algorithm>

#include "common.h"

namespace {

constexpr int kThreads = 256;

struct ColPlan {
    int cqb;     // channel groups (VN elements each) handled by one block (threads along channels)
    int rl;      // row lanes = 256 / cqb
    int gx;      // blocks along channels
    int gy;      // blocks along rows
    int rows;    // rows per block
};

// train_ops.hip's col_plan (mvf_bn_apply_bits sizes its grid with blocks = 4096)
ColPlan col_plan(long M, int C, int vn, int blocks) {
    ColPlan p;
    const int cq = C / vn;
    int cqb = 1;
    while (cqb < cq && cqb < 64) cqb <<= 1;
    p.cqb = cqb;
    p.rl = kThreads / cqb;
    p.gx = (cq + cqb - 1) / cqb;
    long want = std::max<long>(1, blocks / p.gx);
    long rows = std::max<long>((M + want - 1) / want, (long)p.rl * 8);
    rows = (rows + p.rl - 1) / p.rl * p.rl;
    p.rows = (int)rows;
    p.gy = (int)((M + rows - 1) / rows);
    return p;
}

// lane vectors: VN elements of ET <-> VN floats.  (float,4) and (bf16,8) are 16-byte accesses, (bf16,4) is 8 bytes.
template <typename ET, int VN>
__device__ __forceinline__ void ldv(const ET* p, float (&f)[VN]) {
    if constexpr (sizeof(ET) == 4) {
        static_assert(VN == 4, "fp32 lane vector is 4 wide");
        const float4 v = *reinterpret_cast<const float4*>(p);
        f[0] = v.x; f[1] = v.y; f[2] = v.z; f[3] = v.w;
    } else if constexpr (VN == 4) {
        const uint2 r = *reinterpret_cast<const uint2*>(p);
        f[0] = __uint_as_float(r.x << 16); f[1] = __uint_as_float(r.x & 0xffff0000u);
        f[2] = __uint_as_float(r.y << 16); f[3] = __uint_as_float(r.y & 0xffff0000u);
    } else {
        static_assert(VN == 8, "bf16 lane vector is 4 or 8 wide");
        const uint4 r = *reinterpret_cast<const uint4*>(p);
        f[0] = __uint_as_float(r.x << 16); f[1] = __uint_as_float(r.x & 0xffff0000u);
        f[2] = __uint_as_float(r.y << 16); f[3] = __uint_as_float(r.y & 0xffff0000u);
        f[4] = __uint_as_float(r.z << 16); f[5] = __uint_as_float(r.z & 0xffff0000u);
        f[6] = __uint_as_float(r.w << 16); f[7] = __uint_as_float(r.w & 0xffff0000u);
    }
}
template <typename ET, int VN>
__device__ __forceinline__ void stv(ET* p, const float (&f)[VN]) {
    if constexpr (sizeof(ET) == 4) {
        *reinterpret_cast<float4*>(p) = make_float4(f[0], f[1], f[2], f[3]);
    } else if constexpr (VN == 4) {
        uint2 r;
        r.x = pack_bf16x2(f[0], f[1]);
        r.y = pack_bf16x2(f[2], f[3]);
        *reinterpret_cast<uint2*>(p) = r;
    } else {
        uint4 r;
        r.x = pack_bf16x2(f[0], f[1]);
        r.y = pack_bf16x2(f[2], f[3]);
        r.z = pack_bf16x2(f[4], f[5]);
        r.w = pack_bf16x2(f[6], f[7]);
        *reinterpret_cast<uint4*>(p) = r;
    }
}
// per-channel fp32 parameters of the lane's VN channels (null -> fill)
template <int VN>
__device__ __forceinline__ void ldp(const float* p, int c, float (&f)[VN], float fill = 0.f) {
#pragma unroll
    for (int j = 0; j < VN; j += 4) {
        const float4 v = p ? *reinterpret_cast<const float4*>(p + c + j) : make_float4(fill, fill, fill, fill);
        f[j] = v.x; f[j + 1] = v.y; f[j + 2] = v.z; f[j + 3] = v.w;
    }
}

// A lane's walk over its rows (stride rl) with the image index of the current row: img = row / rpi and rem = row % rpi are taken once, every step adds the
// quotient and remainder of rl / rpi (at most one carry).  Exact for any rows_per_image >= 1.
struct RowWalk {
    long row, img;
    int rem, rpi, dq, dr;
    __device__ __forceinline__ RowWalk(long row0, int rl, int rows_per_image) : row(row0), rpi(rows_per_image) {
        img = row0 / rows_per_image;
        rem = (int)(row0 - img * rows_per_image);
        dq = rl / rows_per_image;
        dr = rl - dq * rows_per_image;
    }
    __device__ __forceinline__ void step(int rl) {
        row += rl;
        img += dq;
        rem += dr;
        if (rem >= rpi) { rem -= rpi; img += 1; }
    }
};

// v = s * u, then v + res: two roundings, never one fused multiply-add (s = 1 must reproduce mvf_bn_apply_bits' u + res in ITS order, and the product is the
// value torch's drop_path materialises)
__device__ __forceinline__ float scale_then_add(float s, float u, float res) {
#pragma clang fp contract(off)
    const float v = s * u;
    return v + res;
}
__device__ __forceinline__ float scale_only(float s, float g) {
#pragma clang fp contract(off)
    return s * g;
}

// ---- out = act(s_row * (z * scale + shift) + (r | r * rscale + rshift)), + the sign bits of what is stored ----
template <typename ET, int VN>
__global__ __launch_bounds__(kThreads) void bn_apply_rowscale_kernel(const ET* z, long M, int C, const float* scale, const float* shift, const ET* r,
                                                                     const float* rscale, const float* rshift, const float* row_scale, int rpi, int act, ET* out,
                                                                     unsigned char* bits, int cqb, int rows) {
    const int rl = kThreads / cqb;
    const int cq = blockIdx.x * cqb + threadIdx.x % cqb, lane_r = threadIdx.x / cqb;
    if (cq * VN >= C) return;
    const int c = cq * VN;
    float s[VN], b[VN], rs[VN], rb[VN];
    ldp<VN>(scale, c, s);
    ldp<VN>(shift, c, b);
    ldp<VN>(rscale, c, rs, 1.f);
    ldp<VN>(rshift, c, rb, 0.f);
    const long r0 = (long)blockIdx.y * rows, r1 = min(M, r0 + rows);
    auto one = [&](long row, float sr, float (&v)[VN], const float (&q)[VN]) {
#pragma unroll
        for (int j = 0; j < VN; ++j) {
            const float u = v[j] * s[j] + b[j];                 // as bn_apply_body forms it
            const float res = q[j] * rs[j] + rb[j];             // likewise (rs = 1, rb = 0 without rscale / rshift: exact)
            float t = scale_then_add(sr, u, res);
            if (act == 1) t = fmaxf(t, 0.f);
            v[j] = t;
        }
        stv<ET, VN>(out + row * C + c, v);
        if (bits) {                                             // sign bits of the result, one byte per 4 channels: [M][C/4]
            unsigned mb = 0;
#pragma unroll
            for (int j = 0; j < VN; ++j) mb |= (v[j] > 0.f ? 1u : 0u) << (j + (j >= 4 ? 4 : 0));
            if constexpr (VN == 8) *reinterpret_cast<unsigned short*>(bits + row * (C / 4) + c / 4) = (unsigned short)mb;
            else bits[row * (C / 4) + c / 4] = (unsigned char)mb;
        }
    };
    if (r0 + lane_r >= r1) return;
    RowWalk w(r0 + lane_r, rl, rpi);
    while (w.row + rl < r1) {                                   // two rows per trip: 4 independent vector loads in flight per lane
        const long ra = w.row;
        const float sa = row_scale[w.img];
        w.step(rl);
        const long rb_ = w.row;
        const float sb = row_scale[w.img];
        w.step(rl);
        float z0[VN], z1[VN], q0[VN], q1[VN];
        ldv<ET, VN>(z + ra * C + c, z0);
        ldv<ET, VN>(z + rb_ * C + c, z1);
        ldv<ET, VN>(r + ra * C + c, q0);
        ldv<ET, VN>(r + rb_ * C + c, q1);
        one(ra, sa, z0, q0);
        one(rb_, sb, z1, q1);
    }
    if (w.row < r1) {
        float z0[VN], q0[VN];
        const float sa = row_scale[w.img];
        ldv<ET, VN>(z + w.row * C + c, z0);
        ldv<ET, VN>(r + w.row * C + c, q0);
        one(w.row, sa, z0, q0);
    }
}

// ---- gm = bit ? s_row * g : 0 ----
template <typename ET, int VN>
__global__ __launch_bounds__(kThreads) void gate_rowscale_kernel(const ET* g, int g_pitch, const unsigned char* bits, const float* row_scale, int rpi, long M, int C,
                                                                 ET* gm, int cqb, int rows) {
    const int rl = kThreads / cqb;
    const int cq = blockIdx.x * cqb + threadIdx.x % cqb, lane_r = threadIdx.x / cqb;
    if (cq * VN >= C) return;
    const int c = cq * VN;
    const long r0 = (long)blockIdx.y * rows, r1 = min(M, r0 + rows);
    auto ldbits = [&](long row) -> unsigned {
        const unsigned char* p = bits + row * (C / 4) + c / 4;
        if constexpr (VN == 8) return *reinterpret_cast<const unsigned short*>(p);
        else return *p;
    };
    auto one = [&](long row, float sr, unsigned mb, float (&v)[VN]) {
#pragma unroll
        for (int j = 0; j < VN; ++j) v[j] = ((mb >> (j + (j >= 4 ? 4 : 0))) & 1u) ? scale_only(sr, v[j]) : 0.f;
        stv<ET, VN>(gm + row * C + c, v);
    };
    if (r0 + lane_r >= r1) return;
    RowWalk w(r0 + lane_r, rl, rpi);
    while (w.row + rl < r1) {
        const long ra = w.row;
        const float sa = row_scale[w.img];
        w.step(rl);
        const long rb_ = w.row;
        const float sb = row_scale[w.img];
        w.step(rl);
        float g0[VN], g1[VN];
        ldv<ET, VN>(g + ra * g_pitch + c, g0);
        ldv<ET, VN>(g + rb_ * g_pitch + c, g1);
        const unsigned m0 = ldbits(ra), m1 = ldbits(rb_);
        one(ra, sa, m0, g0);
        one(rb_, sb, m1, g1);
    }
    if (w.row < r1) {
        float g0[VN];
        const float sa = row_scale[w.img];
        ldv<ET, VN>(g + w.row * g_pitch + c, g0);
        one(w.row, sa, ldbits(w.row), g0);
    }
}

inline bool al(const void* p, unsigned a) { return ((uintptr_t)p & (a - 1)) == 0; }

}  // namespace

extern "C" {

int mvf_bn_apply_bits_rowscale(const void* z, long m, int c, const float* scale, const float* shift, const void* residual, const float* rscale, const float* rshift,
                               const float* row_scale, int rows_per_image, int act, void* out, unsigned char* sign_bits, int dtype, void* stream) {
    MVF_REQUIRE(z && scale && shift && residual && row_scale && out && sign_bits, MVF_EINVAL, "bn_apply_bits_rowscale: NULL operand");
    MVF_REQUIRE(m > 0 && c > 0 && c % 4 == 0, MVF_EINVAL, "bn_apply_bits_rowscale: bad shape (m %ld, c %d; c %% 4?)", m, c);
    MVF_REQUIRE(rows_per_image >= 1 && m % rows_per_image == 0, MVF_EINVAL, "bn_apply_bits_rowscale: m = %ld is no multiple of rows_per_image = %d", m, rows_per_image);
    MVF_REQUIRE((rscale == nullptr) == (rshift == nullptr), MVF_EINVAL, "bn_apply_bits_rowscale: rscale / rshift must come together");
    MVF_REQUIRE(dtype == MVF_F32 || dtype == MVF_BF16, MVF_EINVAL, "bn_apply_bits_rowscale: unknown dtype %d", dtype);
    MVF_REQUIRE(act == 0 || act == 1, MVF_EINVAL, "bn_apply_bits_rowscale: act %d (0 none, 1 ReLU)", act);
    MVF_REQUIRE(al(z, 16) && al(residual, 16) && al(out, 16) && al(scale, 16) && al(shift, 16) && al(rscale, 16) && al(rshift, 16) && al(row_scale, 4),
                MVF_EINVAL, "bn_apply_bits_rowscale: z / residual / out / scale / shift / rscale / rshift must be 16-byte aligned, row_scale 4-byte");
    hipStream_t st = (hipStream_t)stream;
#define MVF_DP_APPLY(ET_, VN_)                                                                                                                              \
    do {                                                                                                                                                    \
        const ColPlan p = col_plan(m, c, VN_, 4096);                                                                                                        \
        hipLaunchKernelGGL((bn_apply_rowscale_kernel<ET_, VN_>), dim3(p.gx, p.gy), dim3(kThreads), 0, st, (const ET_*)z, m, c, scale, shift,                \
                           (const ET_*)residual, rscale, rshift, row_scale, rows_per_image, act, (ET_*)out, sign_bits, p.cqb, p.rows);                      \
    } while (0)
    if (dtype == MVF_F32) MVF_DP_APPLY(float, 4);
    else if (c % 8 == 0 && al(sign_bits, 2)) MVF_DP_APPLY(bf16_t, 8);
    else MVF_DP_APPLY(bf16_t, 4);
#undef MVF_DP_APPLY
    MVF_LAUNCH_CHECK();
    return MVF_OK;
}

int mvf_gate_rowscale(const void* g, int g_pitch, const unsigned char* sign_bits, const float* row_scale, int rows_per_image, long m, int c, void* gm_out, int dtype,
                      void* stream) {
    MVF_REQUIRE(g && sign_bits && row_scale && gm_out, MVF_EINVAL, "gate_rowscale: NULL operand");
    MVF_REQUIRE(m > 0 && c > 0 && c % 4 == 0, MVF_EINVAL, "gate_rowscale: bad shape (m %ld, c %d; c %% 4?)", m, c);
    MVF_REQUIRE(rows_per_image >= 1 && m % rows_per_image == 0, MVF_EINVAL, "gate_rowscale: m = %ld is no multiple of rows_per_image = %d", m, rows_per_image);
    MVF_REQUIRE(g_pitch >= c && g_pitch % 4 == 0, MVF_EINVAL, "gate_rowscale: g_pitch %d (>= c = %d, a multiple of 4)", g_pitch, c);
    MVF_REQUIRE(dtype == MVF_F32 || dtype == MVF_BF16, MVF_EINVAL, "gate_rowscale: unknown dtype %d", dtype);
    MVF_REQUIRE(al(g, 16) && al(gm_out, 16) && al(row_scale, 4), MVF_EINVAL, "gate_rowscale: g / gm_out must be 16-byte aligned, row_scale 4-byte");
    hipStream_t st = (hipStream_t)stream;
#define MVF_DP_GATE(ET_, VN_)                                                                                                                               \
    do {                                                                                                                                                    \
        const ColPlan p = col_plan(m, c, VN_, 4096);                                                                                                        \
        hipLaunchKernelGGL((gate_rowscale_kernel<ET_, VN_>), dim3(p.gx, p.gy), dim3(kThreads), 0, st, (const ET_*)g, g_pitch, sign_bits, row_scale,         \
                           rows_per_image, m, c, (ET_*)gm_out, p.cqb, p.rows);                                                                              \
    } while (0)
    if (dtype == MVF_F32) MVF_DP_GATE(float, 4);
    else if (c % 8 == 0 && g_pitch % 8 == 0 && al(sign_bits, 2)) MVF_DP_GATE(bf16_t, 8);
    else MVF_DP_GATE(bf16_t, 4);
#undef MVF_DP_GATE
    MVF_LAUNCH_CHECK();
    return MVF_OK;
}

}  // extern "C"
