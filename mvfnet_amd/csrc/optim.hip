// The fused optimizer steps on flat fp32 buffers: global gradient norm (two-stage, atomic-free) + clip, then ONE update rule per entry-point family --
// SGD with momentum (mvf_sgd_*), Adam / AdamW (mvf_adamw_step), LAMB (mvf_lamb_step) -- each optionally with a segment table (per-segment multipliers,
// excluded segments), the averaged weights (EMA, ema.hip) and the non-finite guard.  Reference semantics: DistOptimizerHook.after_train_iter
// (core/dist_utils.py:61-67) with SGD(nesterov) (configs/.../mvf_kinetics400_2d_rgb_r50_dense.py:152-154), build_optimizer's paramwise_options
// (codes/core/train.py:117-156); torch.optim.Adam / AdamW; timm's optim/lamb.py.
//
// Every step is: sqsum_* (per-block partial sums of g^2) -> norm_finalize_kernel (one lane: norm, clip coefficient, guard counters, and for the Adam forms
// the applied-step counter and bias corrections) -> the update kernel(s).  Every partial is formed by a fixed lane in a fixed order: bit-identical run to run.
#include <algorithm>
#include <climits>
#include <math.h>
#include <type_traits>

#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr size_t kPartBytes = 1024 * sizeof(float);      // the norm's partial sums: the SGD workspace; the Adam forms' two bias-correction doubles follow them

inline int grid_for(long total, int cap = 256 * 16) { return (int)std::min<long>((total + 255) / 256, cap); }
inline int norm_blocks(long n) { return (int)std::min<long>((n + 255) / 256, 1024); }

// ---- the norm: partial sums of squares, then one finalize lane ----
// the tail of every sqsum_* kernel: this lane's sum -> LDS tree over the 256 lanes -> part[block]
__device__ __forceinline__ void block_sum_store(float s, float* part) {
    __shared__ float red[256];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = blockDim.x >> 1; o > 0; o >>= 1) { if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
    if (threadIdx.x == 0) part[blockIdx.x] = red[0];
}
__global__ void sqsum_partial_kernel(const float* g, long n, float* part) {
    float s = 0.f;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) s += g[i] * g[i];
    block_sum_store(s, part);
}
// sum of squares over the elements of the segments that take part in training (lr_mult >= 0): the clip norm of
// torch.nn.utils.clip_grad_norm_(filter(requires_grad, params)) when parameters are excluded in scattered places
__device__ __forceinline__ int seg_of(const mvf_sgd_segment_t* seg, int nseg, long i) {
    int lo = 0, hi = nseg - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (seg[mid].first <= i) lo = mid; else hi = mid - 1;
    }
    return lo;
}
// Every segment form's norm pass, from the merged tables of the SGD / Adam forms to mvf_lamb_step's one segment per parameter tensor (~200 on ResNet-50).  A
// binary search per element would cost seven times the load it guards there (330 us against the flat kernel's 46 us on ResNet-50's 24.3 M elements).  A
// workgroup's 256-element runs climb through the flat range, so the segment of a run's first element is found by stepping on from the previous run's
// (workgroup-uniform), and only the lanes behind a boundary inside the run step further.  Lane t still sums elements t, t + stride, ... in ascending order.
__global__ void sqsum_segment_runs_kernel(const float* g, long n, const mvf_sgd_segment_t* seg, int nseg, float* part) {
    float s = 0.f;
    long i0 = (long)blockIdx.x * blockDim.x;
    int lo = i0 < n ? seg_of(seg, nseg, i0) : 0;
    for (; i0 < n; i0 += (long)gridDim.x * blockDim.x) {
        while (lo + 1 < nseg && (long)seg[lo + 1].first <= i0) ++lo;
        const long i = i0 + threadIdx.x;
        if (i < n) {
            const float gv = g[i];                                // issued ahead of the table reads: it does not wait for them
            int k = lo;
            while (k + 1 < nseg && (long)seg[k + 1].first <= i) ++k;
            if (seg[k].lr_mult >= 0.f) s += gv * gv;
        }
    }
    block_sum_store(s, part);
}
// GUARD: the lane that finishes the norm also decides whether the step is skipped -- the scaled norm is not finite: a NaN / inf in a gradient that entered
// the sum, or a sum of squares beyond fp32 -- and keeps the counters guard[0..4) = {this step's flag, skipped in total, consecutive skips, steps seen}.
// Exponent bits, not isfinite(): the test must survive any floating-point flag the library is ever built with.
// ADAM (mvf_adamw_step, mvf_lamb_step): the lane ALSO keeps the step count: *steps is the number of APPLIED steps, so a step the guard skips does not move it
// and the next good step is bias-corrected with the t it would have had without the skipped one (torch: GradScaler does not call optimizer.step(), and
// state['step'] stays).  For the update kernel the lane leaves bc[0] = 1 / (1 - b1^t) and bc[1] = sqrt(1 - b2^t), formed in double from the new t.
template <bool GUARD, bool ADAM>
__global__ void norm_finalize_kernel(const float* part, int nblk, float max_norm, float gscale, float* out /*[0]=norm,[1]=coef*/, int* guard, long long* steps,
                                     double b1, double b2, double* bc) {
    // 64 lanes sum strided slices of the partials (fixed order), lane 0 combines them in lane order: one wave, a handful of
    // memory round trips instead of nblk serial ones (47 -> ~6 us on the optimizer's critical path)
    __shared__ double red[64];
    double acc = 0.0;
    for (int i = threadIdx.x; i < nblk; i += 64) acc += part[i];
    red[threadIdx.x] = acc;
    __syncthreads();
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        double s = 0.0;
        for (int i = 0; i < 64; ++i) s += red[i];
        const float nrm = fabsf(gscale) * (float)sqrt(s);      // of the scaled gradient (all-reduce sum / world happens before clipping, dist_utils.py:63-66)
        out[0] = nrm;
        float coef = max_norm > 0.f ? max_norm / (nrm + 1e-6f) : 1.f;     // torch clip_grad_norm_
        out[1] = coef < 1.f ? coef : 1.f;
        int bad = 0;
        if (GUARD) {
            bad = (__float_as_uint(nrm) & 0x7f800000u) == 0x7f800000u;
            guard[0] = bad;
            guard[1] += bad;
            guard[2] = bad ? guard[2] + 1 : 0;
            guard[3] += 1;
        }
        if (ADAM && !bad) {
            const long long t = *steps + 1;
            *steps = t;
            bc[0] = 1.0 / (1.0 - pow(b1, (double)t));
            bc[1] = sqrt(1.0 - pow(b2, (double)t));
        }
    }
}
// launches 1 and 2 of the SGD and Adam steps; ws = the partial sums, then (ADAM) bc[0..1]
template <bool SEG, bool GUARD, bool ADAM>
int norm_launch(const float* grads, long n, const mvf_sgd_segment_t* segments, int nseg, float max_norm, float grad_scale, float* norm_out, int* guard,
                long long* steps, double b1, double b2, void* ws, hipStream_t st) {
    float* part = (float*)ws;
    const int nb = norm_blocks(n);
    if (SEG) hipLaunchKernelGGL(sqsum_segment_runs_kernel, dim3(nb), dim3(256), 0, st, grads, n, segments, nseg, part);
    else hipLaunchKernelGGL(sqsum_partial_kernel, dim3(nb), dim3(256), 0, st, grads, n, part);
    MVF_LAUNCH_CHECK();
    hipLaunchKernelGGL((norm_finalize_kernel<GUARD, ADAM>), dim3(1), dim3(64), 0, st, (const float*)part, nb, max_norm, grad_scale, norm_out, guard, steps, b1, b2,
                       ADAM ? (double*)((char*)ws + kPartBytes) : nullptr);
    MVF_LAUNCH_CHECK();
    return MVF_OK;
}

// (segments != NULL, ema != NULL, guard != NULL) -> f(std::bool_constant<SEG>, <EMA>, <GUARD>): the update kernels are templates on the three
template <class F>
int dispatch_forms(bool seg, bool ema, bool guard, F f) {
    auto with_ema = [&](auto s, auto e) { return guard ? f(s, e, std::true_type{}) : f(s, e, std::false_type{}); };
    auto with_seg = [&](auto s) { return ema ? with_ema(s, std::true_type{}) : with_ema(s, std::false_type{}); };
    return seg ? with_seg(std::true_type{}) : with_seg(std::false_type{});
}

// ---- operand checks: `s` has its alignment and overlaps none of the (non-NULL) others ----
struct Operand {
    const char* name;
    uintptr_t at, bytes, align;
};
int check_operand(const char* who, const Operand& s, const Operand* others, int nothers) {
    MVF_REQUIRE(s.at % s.align == 0, MVF_EINVAL, "%s: %s must be %d-byte aligned", who, s.name, (int)s.align);
    for (int k = 0; k < nothers; ++k) {
        const Operand& o = others[k];
        MVF_REQUIRE(!o.at || s.at + s.bytes <= o.at || o.at + o.bytes <= s.at, MVF_EINVAL, "%s: %s and %s overlap", who, s.name, o.name);
    }
    return MVF_OK;
}

// ---- SGD: clip + weight decay + momentum (Nesterov or plain) ----
// One element: d = g * coef + wd_i * p, buf' = momentum * buf + d (first_step: d), p' = p - lr_i * (nesterov ? d + momentum * buf' : buf').
// SEG: per-SEGMENT learning-rate / weight-decay multipliers (build_optimizer's paramwise_options) and the optional plain-momentum form: seg[k] = {first
// element, lr multiplier, decay multiplier}, sorted by first element, seg[0].first == 0, found by binary search per element; lr_mult < 0 = excluded.
// SEG = false is the one-segment table {0, 1, 1} with Nesterov momentum: the same expressions with both multipliers 1 (lr * 1.f is lr).
// EMA: the averaged copy of the parameters (ema.hip) takes its update from the value this lane has just computed: ema[i] = ema_step(ema[i], p', ema_m), one
// more read and one more write of a flat buffer instead of a launch that re-reads the parameters.
// GUARD: every workgroup reads the step's flag (one scalar load) and leaves before any store when the step is skipped.
template <bool SEG, bool EMA, bool GUARD>
__global__ void sgd_kernel(float* p, const float* g, float* buf, long n, const float* coef_ptr, float gscale, float lr, float momentum, float wd, int first_step,
                           int nesterov, const mvf_sgd_segment_t* seg, int nseg, float* ema, float ema_m, const int* guard) {
    if (GUARD) { if (guard[0] != 0) return; }
    const float coef = coef_ptr[1] * gscale;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        float lr_mult = 1.f, decay_mult = 1.f;
        if (SEG) {
            const int lo = seg_of(seg, nseg, i);
            lr_mult = seg[lo].lr_mult;
            decay_mult = seg[lo].decay_mult;
            if (lr_mult < 0.f) continue;                     // excluded from training (requires_grad False): parameter, momentum and average untouched
        }
        const float lr_i = lr * lr_mult, wd_i = wd * decay_mult;
        const float pv = p[i];
        const float d = g[i] * coef + wd_i * pv;
        const float b = first_step ? d : momentum * buf[i] + d;
        buf[i] = b;
        const float pn = pv - lr_i * ((!SEG || nesterov) ? d + momentum * b : b);
        p[i] = pn;
        if (EMA) ema[i] = ema_step(ema[i], pn, ema_m);
    }
}

template <bool SEG, bool EMA, bool GUARD>
int sgd_launch(float* params, const float* grads, float* momentum_buf, long n, float grad_scale, float max_norm, float lr, float momentum, float weight_decay,
               int first_step, int nesterov, const mvf_sgd_segment_t* segments, int nseg, float* ema, float ema_m, int* guard, float* norm_out, void* ws,
               hipStream_t st) {
    const int rc = norm_launch<SEG, GUARD, false>(grads, n, segments, nseg, max_norm, grad_scale, norm_out, guard, nullptr, 0.0, 0.0, ws, st);
    if (rc != MVF_OK) return rc;
    hipLaunchKernelGGL((sgd_kernel<SEG, EMA, GUARD>), dim3(grid_for(n)), dim3(256), 0, st, params, grads, momentum_buf, n, (const float*)norm_out, grad_scale, lr,
                       momentum, weight_decay, first_step, nesterov, segments, nseg, ema, ema_m, (const int*)guard);
    MVF_LAUNCH_CHECK();
    return MVF_OK;
}

// What the five mvf_sgd_* entry points share; the *_form flags say which operands the entry point takes.  ema: n floats, disjoint from the three buffers the
// step reads and writes; guard: four ints, disjoint from everything the step reads or writes.  Every check comes before the first launch.
int sgd_step(const char* who, bool seg_form, bool ema_form, bool guard_form, float* params, const float* grads, float* momentum_buf, long n, float grad_scale,
             float max_norm, float lr, float momentum, float weight_decay, int first_step, int nesterov, const mvf_sgd_segment_t* segments, int nseg, float* ema,
             float ema_m, int* guard, float* norm_out, void* ws, size_t ws_bytes, void* stream) {
    MVF_REQUIRE(params && grads && momentum_buf && norm_out && n > 0 && (!seg_form || (segments && nseg > 0)), MVF_EINVAL, "%s: bad argument", who);
    const uintptr_t len = (uintptr_t)n * 4;
    const Operand others[7] = {{"params", (uintptr_t)params, len, 4},
                               {"grads", (uintptr_t)grads, len, 4},
                               {"momentum_buf", (uintptr_t)momentum_buf, len, 4},
                               {"ema", ema_form ? (uintptr_t)ema : 0, len, 4},
                               {"norm_out", (uintptr_t)norm_out, 2 * sizeof(float), 4},
                               {"the workspace", (uintptr_t)ws, (uintptr_t)ws_bytes, 4},
                               {"the segment table", seg_form ? (uintptr_t)segments : 0, (uintptr_t)nseg * sizeof(mvf_sgd_segment_t), 8}};
    if (ema_form) {
        MVF_REQUIRE(ema, MVF_EINVAL, "%s: NULL ema", who);
        MVF_REQUIRE(ema_m >= 0.f && ema_m <= 1.f, MVF_EINVAL, "%s: ema_momentum=%g is outside [0, 1]", who, (double)ema_m);      // (NaN fails both)
        const int rc = check_operand(who, others[3], others, 3);
        if (rc != MVF_OK) return rc;
    }
    if (guard_form) {
        MVF_REQUIRE(guard, MVF_EINVAL, "%s: NULL guard", who);
        const int rc = check_operand(who, Operand{"guard", (uintptr_t)guard, 4 * sizeof(int), 4}, others, 7);
        if (rc != MVF_OK) return rc;
    }
    MVF_REQUIRE(ws && ws_bytes >= mvf_sgd_workspace_bytes(n), MVF_EWS, "%s: workspace too small", who);
    return dispatch_forms(seg_form, ema_form, guard_form, [&](auto S, auto E, auto G) {
        return sgd_launch<decltype(S)::value, decltype(E)::value, decltype(G)::value>(params, grads, momentum_buf, n, grad_scale, max_norm, lr, momentum,
                                                                                     weight_decay, first_step, nesterov, segments, nseg, ema, ema_m, guard,
                                                                                     norm_out, ws, (hipStream_t)stream);
    });
}

// ---- Adam / AdamW and LAMB: what the two share on the host ----
// The hyper-parameters as the update kernels take them: lr and weight_decay stay double (a segment's lr * lr_mult, 1 - lr_i * wd_i and lr_i / (1 - b1^t) are
// formed in double and rounded to fp32 ONCE, as torch rounds its Python scalars); the betas, their complements and eps are rounded once on the host.
struct AdamConst {
    double lr, wd;
    float b1, omb1, b2, omb2, eps;
};
int adam_hyper(const char* who, double lr, double b1, double b2, double eps, double wd, AdamConst* k) {
    MVF_REQUIRE(lr == lr && b1 == b1 && b2 == b2 && eps == eps && wd == wd, MVF_EINVAL, "%s: NaN in the hyper-parameters", who);
    MVF_REQUIRE(b1 >= 0.0 && b1 < 1.0 && b2 >= 0.0 && b2 < 1.0, MVF_EINVAL, "%s: betas (%g, %g) are outside [0, 1)", who, b1, b2);
    MVF_REQUIRE(eps > 0.0, MVF_EINVAL, "%s: eps=%g must be positive", who, eps);
    MVF_REQUIRE(lr >= 0.0 && wd >= 0.0, MVF_EINVAL, "%s: lr=%g and weight_decay=%g must not be negative", who, lr, wd);
    k->lr = lr;
    k->wd = wd;
    k->b1 = (float)b1;
    k->omb1 = (float)(1.0 - b1);          // rounded once from the double: forming 1 - beta2 from a float 0.999 misses it by 1.3e-5 relative
    k->b2 = (float)b2;
    k->omb2 = (float)(1.0 - b2);
    k->eps = (float)eps;
    return MVF_OK;
}
// the step counter, the average's momentum, then every operand, its extent in bytes and the alignment it needs; no two of them may overlap
// (ratio_out: mvf_lamb_step's, NULL for mvf_adamw_step)
int adam_operands(const char* who, const float* params, const float* grads, const float* exp_avg, const float* exp_avg_sq, long n, const float* ema, float ema_m,
                  const int* guard, const long long* applied_steps, const float* norm_out, const float* ratio_out, const void* ws, size_t ws_bytes,
                  const mvf_sgd_segment_t* segments, int nseg) {
    MVF_REQUIRE(applied_steps && (uintptr_t)applied_steps % 8 == 0, MVF_EINVAL, "%s: applied_steps must be a non-NULL, 8-byte aligned device pointer", who);
    if (ema) MVF_REQUIRE(ema_m >= 0.f && ema_m <= 1.f, MVF_EINVAL, "%s: ema_momentum=%g is outside [0, 1]", who, (double)ema_m);      // (NaN fails both)
    const uintptr_t len = (uintptr_t)n * 4;
    constexpr int kOps = 11;
    const Operand ops[kOps] = {{"params", (uintptr_t)params, len, 4},
                               {"grads", (uintptr_t)grads, len, 4},
                               {"exp_avg", (uintptr_t)exp_avg, len, 4},
                               {"exp_avg_sq", (uintptr_t)exp_avg_sq, len, 4},
                               {"ema", (uintptr_t)ema, len, 4},
                               {"guard", (uintptr_t)guard, 4 * sizeof(int), 4},
                               {"applied_steps", (uintptr_t)applied_steps, sizeof(long long), 8},
                               {"norm_out", (uintptr_t)norm_out, 2 * sizeof(float), 4},
                               {"ratio_out", (uintptr_t)ratio_out, (uintptr_t)nseg * sizeof(float), 4},
                               {"the workspace", (uintptr_t)ws, (uintptr_t)ws_bytes, 8},
                               {"the segment table", (uintptr_t)segments, (uintptr_t)nseg * sizeof(mvf_sgd_segment_t), 8}};
    for (int a = 0; a < kOps; ++a) {
        if (!ops[a].at) continue;
        const int rc = check_operand(who, ops[a], ops + a + 1, kOps - a - 1);
        if (rc != MVF_OK) return rc;
    }
    return MVF_OK;
}

// ---- Adam / AdamW (mvf_adamw_step): the norm as above, then one update kernel ----
struct AdamwConst : AdamConst {
    int decoupled;
};

// One element: d = g * coef [+ wd_i * p], m' = b1 m + (1 - b1) d, v' = b2 v + (1 - b2) d^2, p' = p [* (1 - lr_i wd_i)] - step_i * m' / (sqrt(v') / bc2 + eps).
// SEG = false is the one-segment table {0, 1, 1}: the same expressions with both multipliers 1 (lr * 1.0 is lr), hoisted out of the loop by the compiler.
template <bool SEG, bool EMA, bool GUARD>
__global__ void adamw_kernel(float* p, const float* g, float* m, float* v, long n, const float* coef_ptr, float gscale, AdamwConst k, const double* bc,
                             const mvf_sgd_segment_t* seg, int nseg, float* ema, float ema_m, const int* guard) {
    if (GUARD) { if (guard[0] != 0) return; }
    const float coef = coef_ptr[1] * gscale;
    const double inv_bc1 = bc[0];
    const float bc2 = (float)bc[1];
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        float lr_mult = 1.f, decay_mult = 1.f;
        if (SEG) {
            const int lo = seg_of(seg, nseg, i);
            lr_mult = seg[lo].lr_mult;
            decay_mult = seg[lo].decay_mult;
            if (lr_mult < 0.f) continue;                     // excluded from training: parameter, both moments and the average untouched
        }
        const double lr_i = k.lr * (double)lr_mult, wd_i = k.wd * (double)decay_mult;
        const float step = (float)(lr_i * inv_bc1);
        float pv = p[i];
        float d = g[i] * coef;
        if (k.decoupled) pv = pv * (float)(1.0 - lr_i * wd_i);
        else d = d + (float)wd_i * pv;
        const float mn = k.b1 * m[i] + k.omb1 * d;
        const float vn = k.b2 * v[i] + k.omb2 * (d * d);
        m[i] = mn;
        v[i] = vn;
        const float pn = pv - step * (mn / (sqrtf(vn) / bc2 + k.eps));
        p[i] = pn;
        if (EMA) ema[i] = ema_step(ema[i], pn, ema_m);
    }
}

template <bool SEG, bool EMA, bool GUARD>
int adamw_launch(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, long n, float grad_scale, float max_norm, const AdamwConst& k,
                 double b1, double b2, const mvf_sgd_segment_t* segments, int nseg, float* ema, float ema_m, int* guard, long long* steps, float* norm_out,
                 void* ws, hipStream_t st) {
    const int rc = norm_launch<SEG, GUARD, true>(grads, n, segments, nseg, max_norm, grad_scale, norm_out, guard, steps, b1, b2, ws, st);
    if (rc != MVF_OK) return rc;
    hipLaunchKernelGGL((adamw_kernel<SEG, EMA, GUARD>), dim3(grid_for(n)), dim3(256), 0, st, params, grads, exp_avg, exp_avg_sq, n, (const float*)norm_out,
                       grad_scale, k, (const double*)((char*)ws + kPartBytes), segments, nseg, ema, ema_m, (const int*)guard);
    MVF_LAUNCH_CHECK();
    return MVF_OK;
}

// ---- LAMB (mvf_lamb_step, timm's optim/lamb.py) ----
// LAMB scales every parameter tensor's step by ||w|| / ||update||: two norms per SEGMENT of the table (one segment = one trust-ratio unit), ~200 tensors of
// 64 .. 2.36 M elements on ResNet-50, every step, without a host round trip or a float atomic.  The reduction is csrc/layer_stats.hip's: fixed 4096-element
// chunks, one fp64 partial pair per (chunk, segment) intersection at workspace slot chunk + segment, one wavefront per segment adds its slots.  Five launches:
//   1. sqsum_segment_runs_kernel, 2. norm_finalize_kernel<GUARD, true>: norm, clip coefficient, guard counters, applied-step counter, bc[0..1] -- as
//      mvf_adamw_step with a table.
//   3. lamb_moments_kernel: workgroup c owns chunk c and walks the segments that intersect it; it stores m' and v', forms the update u in registers and
//      reduces p^2 and u^2 in fp64 (shuffle tree per wave, the four waves meet in LDS) to slot c + s.
//   4. lamb_ratio_kernel: one wavefront per segment adds its slots in ascending order and stores ratio_out[k].
//   5. lamb_apply_kernel: re-reads m', v' and p, forms u AGAIN through lamb_update -- the same function with every rounding pinned, so both sites hold the same
//      bits -- and stores p' = p - (lr_k r_k) u (and the average).
// Forming u twice costs what a u buffer would (4 B written + 4 B read per element against 8 B of m', v' read again) and needs no n-sized scratch (97 MB on
// ResNet-50).  Traffic by count, without the norm pass: 24 B (moments: p g m v in, m' v' out) + 16 B (apply: m' v' p in, p' out) = 40 B per element against the
// Adam kernel's 28.  That is a count, not a measurement.
// Every partial is formed by a fixed lane in a fixed order and the grids depend on n and nseg alone: bit-identical from run to run (for given operand alignment).
constexpr long kLambChunk = 4096;                   // elements per workgroup of launches 3 and 5: 4 dwordx4 loads per lane and array
constexpr int kLambWave = 64, kLambWaves = kThreads / kLambWave;

struct LambConst : AdamConst {
    int trust_clip, always_adapt;
};

struct LambSlot {
    double p2, u2;
};

// u = (m' / (1 - b1^t)) / (sqrt(v') / sqrt(1 - b2^t) + eps) + wd_i p, with inv_bc1 = (float)(1 / (1 - b1^t)) and bc2 = (float)sqrt(1 - b2^t).  Called by the
// moments pass (for the norm) and by the apply pass (for the step): no contraction across the operations, one explicit fma, so the two calls round alike.
__device__ __forceinline__ float lamb_update(float mn, float vn, float pv, float inv_bc1, float bc2, float eps, float wd_i) {
#pragma clang fp contract(off)
    const float mhat = mn * inv_bc1;
    const float den = sqrtf(vn) / bc2 + eps;
    const float q = mhat / den;
    return fmaf(wd_i, pv, q);
}

// this lane's share of [b, e): stride kThreads; f4(i) takes the four elements from i on the 16-byte-aligned body (when `vec`: every operand equally aligned
// modulo 16, `anchor` being one of them), f1(i) one element of the ragged head and tail
template <class F4, class F1>
__device__ __forceinline__ void lamb_for_range(const float* anchor, long b, long e, bool vec, F4 f4, F1 f1) {
    const int t = threadIdx.x;
    if (vec && e - b >= 8) {
        const long head = (long)((4 - (int)(((uintptr_t)(anchor + b) >> 2) & 3)) & 3);      // elements in front of the first aligned one
        const long vb = b + head, nv = (e - vb) >> 2, ve = vb + (nv << 2);
        if (t < head) f1(b + t);
        for (long q = t; q < nv; q += kThreads) f4(vb + (q << 2));
        if (ve + t < e) f1(ve + t);                                                         // (at most 3 elements)
    } else {
        for (long i = b + t; i < e; i += kThreads) f1(i);
    }
}

__device__ __forceinline__ bool lamb_same_mod16(const void* a, const void* b) { return (((uintptr_t)a ^ (uintptr_t)b) & 15) == 0; }

// the element range of segment s inside chunk [c0, c1): empty when the table breaks its contract (never an access outside [c0, c1))
__device__ __forceinline__ void lamb_intersection(const mvf_sgd_segment_t* seg, int nseg, int s, long n, long c0, long c1, long& b, long& e, long& se) {
    const long sb = s == 0 ? 0 : (long)seg[s].first;             // (segment 0 starts at 0 whatever the table says: every element has an owner)
    se = s + 1 < nseg ? (long)seg[s + 1].first : n;
    b = sb > c0 ? sb : c0;
    e = se < c1 ? se : c1;
}

__global__ __launch_bounds__(kThreads) void lamb_moments_kernel(const float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                                float* __restrict__ v, long n, const float* __restrict__ coef_ptr, float gscale, LambConst k,
                                                                const double* __restrict__ bc, const mvf_sgd_segment_t* __restrict__ seg, int nseg,
                                                                const int* __restrict__ guard, LambSlot* __restrict__ slots) {
    if (guard && guard[0] != 0) return;
    __shared__ LambSlot part[2][kLambWaves];
    const int lane = threadIdx.x % kLambWave, wave = threadIdx.x / kLambWave;
    const long c = blockIdx.x, c0 = c * kLambChunk, c1 = c0 + kLambChunk < n ? c0 + kLambChunk : n;
    const float coef = coef_ptr[1] * gscale;
    const float inv_bc1 = (float)bc[0], bc2 = (float)bc[1];
    const bool vec = lamb_same_mod16(p, g) && lamb_same_mod16(p, m) && lamb_same_mod16(p, v);
    int s = seg_of(seg, nseg, c0);
    for (int turn = 0; s < nseg; ++s, turn ^= 1) {
        long b, e, se;
        lamb_intersection(seg, nseg, s, n, c0, c1, b, e, se);
        if (b >= e) break;                                       // (workgroup-uniform, and only under a table that breaks its contract)
        double p2 = 0.0, u2 = 0.0;
        if (seg[s].lr_mult >= 0.f) {                             // an excluded segment: nothing read, nothing stored, a zero partial
            const float wd_i = (float)(k.wd * (double)seg[s].decay_mult);
            auto one = [&](float pv, float gv, float& mv, float& vv) {
                const float d = gv * coef;
                mv = k.b1 * mv + k.omb1 * d;
                vv = k.b2 * vv + k.omb2 * (d * d);
                const float u = lamb_update(mv, vv, pv, inv_bc1, bc2, k.eps, wd_i);
                p2 += (double)pv * (double)pv;
                u2 += (double)u * (double)u;
            };
            lamb_for_range(
                p, b, e, vec,
                [&](long i) {
                    const float4 pv = *reinterpret_cast<const float4*>(p + i), gv = *reinterpret_cast<const float4*>(g + i);
                    float4 mv = *reinterpret_cast<const float4*>(m + i), vv = *reinterpret_cast<const float4*>(v + i);
                    one(pv.x, gv.x, mv.x, vv.x);
                    one(pv.y, gv.y, mv.y, vv.y);
                    one(pv.z, gv.z, mv.z, vv.z);
                    one(pv.w, gv.w, mv.w, vv.w);
                    *reinterpret_cast<float4*>(m + i) = mv;
                    *reinterpret_cast<float4*>(v + i) = vv;
                },
                [&](long i) {
                    float mv = m[i], vv = v[i];
                    one(p[i], g[i], mv, vv);
                    m[i] = mv;
                    v[i] = vv;
                });
        }
#pragma unroll
        for (int o = kLambWave / 2; o > 0; o >>= 1) {            // butterfly: a + b is commutative, so every lane ends with the same bits
            p2 += __shfl_xor(p2, o, kLambWave);
            u2 += __shfl_xor(u2, o, kLambWave);
        }
        if (lane == 0) part[turn][wave] = LambSlot{p2, u2};
        __syncthreads();        // one barrier per intersection: the next turn writes the OTHER half, and the turn after it starts behind the next barrier
        if (threadIdx.x == 0) {
            LambSlot r = part[turn][0];
#pragma unroll
            for (int w = 1; w < kLambWaves; ++w) {
                r.p2 += part[turn][w].p2;
                r.u2 += part[turn][w].u2;
            }
            slots[c + s] = r;                                    // along the intersections in flat order either c or s grows by one: c + s is unique
        }
        if (se >= c1) break;
    }
}

__global__ __launch_bounds__(kLambWave) void lamb_ratio_kernel(long n, LambConst k, const mvf_sgd_segment_t* __restrict__ seg, int nseg, long nchunks,
                                                               const int* __restrict__ guard, const LambSlot* __restrict__ slots, float* __restrict__ ratio_out) {
    if (guard && guard[0] != 0) return;
    const int s = blockIdx.x, lane = threadIdx.x;
    const long sb = s == 0 ? 0 : (long)seg[s].first;
    const long se = s + 1 < nseg ? (long)seg[s + 1].first : n;
    const bool trained = seg[s].lr_mult >= 0.f;
    double p2 = 0.0, u2 = 0.0;
    if (trained && sb < se && sb >= 0 && se <= n) {              // (a table that breaks its contract gives ratio 1, never an access outside the workspace)
        const long lo = sb / kLambChunk, last = (se - 1) / kLambChunk, hi = last < nchunks - 1 ? last : nchunks - 1;
        for (long c = lo + lane; c <= hi; c += kLambWave) {
            const LambSlot q = slots[c + s];
            p2 += q.p2;
            u2 += q.u2;
        }
    }
#pragma unroll
    for (int o = kLambWave / 2; o > 0; o >>= 1) {
        p2 += __shfl_xor(p2, o, kLambWave);
        u2 += __shfl_xor(u2, o, kLambWave);
    }
    if (lane == 0) {
        float r = 0.f;                                           // excluded: nothing is applied
        if (trained) {
            const double wn = sqrt(p2), un = sqrt(u2);
            const bool adapts = k.wd * (double)seg[s].decay_mult != 0.0 || k.always_adapt;
            r = adapts && wn > 0.0 && un > 0.0 ? (float)(wn / un) : 1.f;
            if (k.trust_clip) r = r < 1.f ? r : 1.f;
        }
        ratio_out[s] = r;
    }
}

__global__ __launch_bounds__(kThreads) void lamb_apply_kernel(float* __restrict__ p, const float* __restrict__ m, const float* __restrict__ v, long n, LambConst k,
                                                              const double* __restrict__ bc, const mvf_sgd_segment_t* __restrict__ seg, int nseg,
                                                              const float* __restrict__ ratio, float* __restrict__ ema, float ema_m,
                                                              const int* __restrict__ guard) {
    if (guard && guard[0] != 0) return;
    const long c = blockIdx.x, c0 = c * kLambChunk, c1 = c0 + kLambChunk < n ? c0 + kLambChunk : n;
    const float inv_bc1 = (float)bc[0], bc2 = (float)bc[1];
    const bool vec = lamb_same_mod16(p, m) && lamb_same_mod16(p, v) && (!ema || lamb_same_mod16(p, ema));
    for (int s = seg_of(seg, nseg, c0); s < nseg; ++s) {
        long b, e, se;
        lamb_intersection(seg, nseg, s, n, c0, c1, b, e, se);
        if (b >= e) break;
        if (seg[s].lr_mult >= 0.f) {                             // excluded: parameter, both moments and the average untouched
            const float wd_i = (float)(k.wd * (double)seg[s].decay_mult);
            const float step = (float)(k.lr * (double)seg[s].lr_mult * (double)ratio[s]);
            auto one = [&](float pv, float mv, float vv) { return fmaf(-step, lamb_update(mv, vv, pv, inv_bc1, bc2, k.eps, wd_i), pv); };
            lamb_for_range(
                p, b, e, vec,
                [&](long i) {
                    float4 pv = *reinterpret_cast<const float4*>(p + i);
                    const float4 mv = *reinterpret_cast<const float4*>(m + i), vv = *reinterpret_cast<const float4*>(v + i);
                    pv.x = one(pv.x, mv.x, vv.x);
                    pv.y = one(pv.y, mv.y, vv.y);
                    pv.z = one(pv.z, mv.z, vv.z);
                    pv.w = one(pv.w, mv.w, vv.w);
                    *reinterpret_cast<float4*>(p + i) = pv;
                    if (ema) {
                        float4 ev = *reinterpret_cast<const float4*>(ema + i);
                        ev.x = ema_step(ev.x, pv.x, ema_m);
                        ev.y = ema_step(ev.y, pv.y, ema_m);
                        ev.z = ema_step(ev.z, pv.z, ema_m);
                        ev.w = ema_step(ev.w, pv.w, ema_m);
                        *reinterpret_cast<float4*>(ema + i) = ev;
                    }
                },
                [&](long i) {
                    const float pn = one(p[i], m[i], v[i]);
                    p[i] = pn;
                    if (ema) ema[i] = ema_step(ema[i], pn, ema_m);
                });
        }
        if (se >= c1) break;
    }
}

inline long lamb_chunks(long n) { return (n + kLambChunk - 1) / kLambChunk; }
constexpr size_t kLambSlotOffset = kPartBytes + 2 * sizeof(double);      // the norm's partial sums, bc[0..1], then the (chunk, segment) slots

}  // namespace

extern "C" {

// clip_grad_norm_(max_norm, L2) over the flat gradient, then p -= lr * (d + mom*buf), d = g*coef*gscale + wd*p, buf = mom*buf + d
// (torch.optim.SGD nesterov; first_step: buf = d).  norm_out[0] = total norm (after gscale), norm_out[1] = clip coefficient.
size_t mvf_sgd_workspace_bytes(long n) { return kPartBytes; }

int mvf_sgd_nesterov_step(float* params, const float* grads, float* momentum_buf, long n, float grad_scale, float max_norm,
                          float lr, float momentum, float weight_decay, int first_step, float* norm_out, void* ws,
                          size_t ws_bytes, void* stream) {
    return sgd_step("sgd_nesterov_step", false, false, false, params, grads, momentum_buf, n, grad_scale, max_norm, lr, momentum, weight_decay, first_step, 1, nullptr,
                    0, nullptr, 0.f, nullptr, norm_out, ws, ws_bytes, stream);
}

int mvf_sgd_nesterov_step_ema(float* params, const float* grads, float* momentum_buf, long n, float grad_scale, float max_norm, float lr, float momentum,
                              float weight_decay, int first_step, float* ema, float ema_momentum, float* norm_out, void* ws, size_t ws_bytes, void* stream) {
    return sgd_step("sgd_nesterov_step_ema", false, true, false, params, grads, momentum_buf, n, grad_scale, max_norm, lr, momentum, weight_decay, first_step, 1,
                    nullptr, 0, ema, ema_momentum, nullptr, norm_out, ws, ws_bytes, stream);
}

int mvf_sgd_step_segments(float* params, const float* grads, float* momentum_buf, long n, float grad_scale, float max_norm, float lr,
                          float momentum, float weight_decay, int first_step, int nesterov, const mvf_sgd_segment_t* segments, int nseg,
                          float* norm_out, void* ws, size_t ws_bytes, void* stream) {
    return sgd_step("sgd_step_segments", true, false, false, params, grads, momentum_buf, n, grad_scale, max_norm, lr, momentum, weight_decay, first_step, nesterov,
                    segments, nseg, nullptr, 0.f, nullptr, norm_out, ws, ws_bytes, stream);
}

int mvf_sgd_step_segments_ema(float* params, const float* grads, float* momentum_buf, long n, float grad_scale, float max_norm, float lr, float momentum,
                              float weight_decay, int first_step, int nesterov, const mvf_sgd_segment_t* segments, int nseg, float* ema, float ema_momentum,
                              float* norm_out, void* ws, size_t ws_bytes, void* stream) {
    return sgd_step("sgd_step_segments_ema", true, true, false, params, grads, momentum_buf, n, grad_scale, max_norm, lr, momentum, weight_decay, first_step, nesterov,
                    segments, nseg, ema, ema_momentum, nullptr, norm_out, ws, ws_bytes, stream);
}

// The four forms above behind the non-finite guard (mvfnet_hip.h): segments == NULL selects the flat Nesterov form, ema == NULL keeps no average.
int mvf_sgd_step_guarded(float* params, const float* grads, float* momentum_buf, long n, float grad_scale, float max_norm, float lr, float momentum,
                         float weight_decay, int first_step, int nesterov, const mvf_sgd_segment_t* segments, int nseg, float* ema, float ema_momentum,
                         int* guard, float* norm_out, void* ws, size_t ws_bytes, void* stream) {
    return sgd_step("sgd_step_guarded", segments != nullptr, ema != nullptr, true, params, grads, momentum_buf, n, grad_scale, max_norm, lr, momentum, weight_decay,
                    first_step, nesterov, segments, nseg, ema, ema_momentum, guard, norm_out, ws, ws_bytes, stream);
}

// clip_grad_norm_ + torch.optim.Adam / AdamW on the flat buffers (mvfnet_hip.h).  Every check comes before the first launch.
size_t mvf_adamw_workspace_bytes(long n) { return kPartBytes + 2 * sizeof(double); }

int mvf_adamw_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, long n, float grad_scale, float max_norm,
                   const mvf_adamw_hyper_t* hyper, const mvf_sgd_segment_t* segments, int nseg, float* ema, float ema_momentum, int* guard,
                   long long* applied_steps, float* norm_out, void* ws, size_t ws_bytes, void* stream) {
    const char* who = "adamw_step";
    MVF_REQUIRE(params && grads && exp_avg && exp_avg_sq && norm_out && n > 0 && (!segments || nseg > 0), MVF_EINVAL, "%s: bad argument", who);
    MVF_REQUIRE(hyper, MVF_EINVAL, "%s: NULL hyper", who);
    AdamwConst k;
    int rc = adam_hyper(who, hyper->lr, hyper->beta1, hyper->beta2, hyper->eps, hyper->weight_decay, &k);
    if (rc != MVF_OK) return rc;
    MVF_REQUIRE(hyper->decoupled == 0 || hyper->decoupled == 1, MVF_EINVAL, "%s: decoupled=%d is neither 0 (Adam) nor 1 (AdamW)", who, hyper->decoupled);
    k.decoupled = hyper->decoupled;
    rc = adam_operands(who, params, grads, exp_avg, exp_avg_sq, n, ema, ema_momentum, guard, applied_steps, norm_out, nullptr, ws, ws_bytes, segments, nseg);
    if (rc != MVF_OK) return rc;
    MVF_REQUIRE(ws && ws_bytes >= mvf_adamw_workspace_bytes(n), MVF_EWS, "%s: workspace too small", who);
    return dispatch_forms(segments != nullptr, ema != nullptr, guard != nullptr, [&](auto S, auto E, auto G) {
        return adamw_launch<decltype(S)::value, decltype(E)::value, decltype(G)::value>(params, grads, exp_avg, exp_avg_sq, n, grad_scale, max_norm, k, hyper->beta1,
                                                                                       hyper->beta2, segments, nseg, ema, ema_momentum, guard, applied_steps,
                                                                                       norm_out, ws, (hipStream_t)stream);
    });
}

// clip_grad_norm_ + timm's Lamb on the flat buffers, one table segment per trust-ratio unit (mvfnet_hip.h).  Every check comes before the first launch.
size_t mvf_lamb_workspace_bytes(long n, int nseg) {
    if (n <= 0 || nseg <= 0 || (long)nseg > n) return 0;
    return kLambSlotOffset + ((size_t)lamb_chunks(n) + (size_t)nseg) * sizeof(LambSlot);
}

int mvf_lamb_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, long n, float grad_scale, float max_norm,
                  const mvf_lamb_hyper_t* hyper, const mvf_sgd_segment_t* segments, int nseg, float* ema, float ema_momentum, int* guard,
                  long long* applied_steps, float* norm_out, float* ratio_out, void* ws, size_t ws_bytes, void* stream) {
    const char* who = "lamb_step";
    MVF_REQUIRE(params && grads && exp_avg && exp_avg_sq && norm_out && ratio_out && n > 0, MVF_EINVAL, "%s: bad argument", who);
    MVF_REQUIRE(segments, MVF_EINVAL, "%s: NULL segment table (one segment per trust-ratio unit)", who);
    MVF_REQUIRE(nseg > 0 && (long)nseg <= n, MVF_EINVAL, "%s: nseg=%d must be in [1, n=%ld]", who, nseg, n);
    MVF_REQUIRE(lamb_chunks(n) <= (long)INT_MAX, MVF_EINVAL, "%s: n=%ld is beyond one launch", who, n);
    MVF_REQUIRE(hyper, MVF_EINVAL, "%s: NULL hyper", who);
    LambConst k;
    int rc = adam_hyper(who, hyper->lr, hyper->beta1, hyper->beta2, hyper->eps, hyper->weight_decay, &k);
    if (rc != MVF_OK) return rc;
    MVF_REQUIRE((hyper->trust_clip == 0 || hyper->trust_clip == 1) && (hyper->always_adapt == 0 || hyper->always_adapt == 1), MVF_EINVAL,
                "%s: trust_clip=%d and always_adapt=%d must be 0 or 1", who, hyper->trust_clip, hyper->always_adapt);
    k.trust_clip = hyper->trust_clip;
    k.always_adapt = hyper->always_adapt;
    rc = adam_operands(who, params, grads, exp_avg, exp_avg_sq, n, ema, ema_momentum, guard, applied_steps, norm_out, ratio_out, ws, ws_bytes, segments, nseg);
    if (rc != MVF_OK) return rc;
    MVF_REQUIRE(ws && ws_bytes >= mvf_lamb_workspace_bytes(n, nseg), MVF_EWS, "%s: workspace too small", who);
    hipStream_t st = (hipStream_t)stream;
    float* part = (float*)ws;
    double* bc = (double*)((char*)ws + kPartBytes);
    LambSlot* slots = (LambSlot*)((char*)ws + kLambSlotOffset);
    const int nb = norm_blocks(n);
    const long nchunks = lamb_chunks(n);
    hipLaunchKernelGGL(sqsum_segment_runs_kernel, dim3(nb), dim3(256), 0, st, grads, n, segments, nseg, part);
    MVF_LAUNCH_CHECK();
    if (guard) hipLaunchKernelGGL((norm_finalize_kernel<true, true>), dim3(1), dim3(64), 0, st, (const float*)part, nb, max_norm, grad_scale, norm_out, guard, applied_steps, hyper->beta1, hyper->beta2, bc);
    else hipLaunchKernelGGL((norm_finalize_kernel<false, true>), dim3(1), dim3(64), 0, st, (const float*)part, nb, max_norm, grad_scale, norm_out, guard, applied_steps, hyper->beta1, hyper->beta2, bc);
    MVF_LAUNCH_CHECK();
    hipLaunchKernelGGL(lamb_moments_kernel, dim3((unsigned)nchunks), dim3(kThreads), 0, st, (const float*)params, grads, exp_avg, exp_avg_sq, n,
                       (const float*)norm_out, grad_scale, k, (const double*)bc, segments, nseg, (const int*)guard, slots);
    MVF_LAUNCH_CHECK();
    hipLaunchKernelGGL(lamb_ratio_kernel, dim3((unsigned)nseg), dim3(kLambWave), 0, st, n, k, segments, nseg, nchunks, (const int*)guard, (const LambSlot*)slots,
                       ratio_out);
    MVF_LAUNCH_CHECK();
    hipLaunchKernelGGL(lamb_apply_kernel, dim3((unsigned)nchunks), dim3(kThreads), 0, st, params, (const float*)exp_avg, (const float*)exp_avg_sq, n, k,
                       (const double*)bc, segments, nseg, (const float*)ratio_out, ema, ema_momentum, (const int*)guard);
    MVF_LAUNCH_CHECK();
    return MVF_OK;
}

}  // extern "C"
