/* mvfnet_hip.h -- C ABI of libmvfnet_hip.so (MI355X / gfx950 only).
 *
 * The reference (whwu95/MVFNet) is 100 % Python and has NO FFI boundary of its own: its hot path calls
 * torch.nn modules.  This header is therefore this build's own boundary; each entry point
 * cites the reference code whose arithmetic it replaces.  INTEGRATION.md shows the ctypes binding a
 * maintainer of the reference would add.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (e.g. torch tensors' data_ptr()); the library
 *     never allocates or frees user-visible memory; scratch comes in through (ws, ws_bytes) with a
 *     *_workspace_bytes() query;
 *   - every entry takes the HIP stream as an opaque void* (hipStream_t; pass
 *     torch.cuda.current_stream().cuda_stream) and is asynchronous on it;
 *   - return value: 0 = OK, <0 = MVF_E*; never throws; mvf_last_error() = thread-local message;
 *   - no global mutable state besides the thread-local error string: safe from several host threads/streams;
 *   - dtype = storage type of activations (weights / BN parameters / statistics are always fp32,
 *     accumulation is always fp32).
 */
#ifndef MVFNET_HIP_H
#define MVFNET_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MVF_ABI_VERSION 2    /* 2: mvf_conv_desc_t.x_c0 */

enum { MVF_OK = 0, MVF_EINVAL = -1, MVF_ESHAPE = -2, MVF_EWS = -3, MVF_EHIP = -4, MVF_EUNSUPPORTED = -5 };
enum { MVF_F32 = 0, MVF_BF16 = 1 };
enum { MVF_NCHW = 0, MVF_NHWC = 1 };                       /* memory order of the (N*T, C, H, W) tensor */
enum { MVF_VIEW_T = 1, MVF_VIEW_H = 2, MVF_VIEW_W = 4 };   /* mode 'T' = 1, 'TH' = 3, 'THW' = 7 (MVF.py:112-129) */

int mvf_abi_version(void);
const char* mvf_last_error(void);

/* ------------------------------------------------------------------------------------------------
 * MVF-proper: everything in MVF.forward except self.net (codes/models/modules/MVF.py:104-137).
 * Tensor x is (nt, c, h, w) in `layout`; clips are runs of n_segment consecutive images (MVF.py:107-109).
 * Only channels [0, cs) are read/written by the stencil; channels >= cs pass through (MVF.py:110,135).
 * Tap weights are fp32 [cs][3]: tap j multiplies the element at offset (j-1) along the view axis
 * (= shift_conv.weight (cs,1,3,1,1) / h_conv.weight (cs,1,1,3,1) / w_conv.weight (cs,1,1,1,3) flattened).
 * share=True (MVF.py:114-116,125-126): pass w_h = w_w = w_t and add the three weight grads.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t nt, c, h, w;      /* tensor dims                                      */
    int32_t n_segment;        /* T: frames per clip, nt % n_segment == 0          */
    int32_t cs;               /* num_shift_channel = int(c * alpha), 0 < cs <= c  */
    int32_t mode;             /* MVF_VIEW_* bitmask, T bit mandatory              */
    int32_t layout;           /* MVF_NCHW | MVF_NHWC                              */
    int32_t dtype;            /* MVF_F32 | MVF_BF16                               */
} mvf_desc_t;

/* Inference / eval-BN forward (MVF.py:118-134 with BatchNorm3d in eval mode folded by the caller:
 * bn_scale = gamma/sqrt(running_var+eps), bn_shift = beta - running_mean*bn_scale).
 * bn_scale == NULL  <=>  use_hs=False: no BN, no activation (MVF.py:131-134).
 * out == x: in place on the slice (allowed; nothing else is touched).  out != x: channels >= cs are copied. */
int mvf_fwd_infer(const mvf_desc_t* d, const void* x, void* out,
                  const float* w_t, const float* w_h, const float* w_w,
                  const float* bn_scale, const float* bn_shift, void* stream);

/* Engine variant (MVF_NHWC only): writes ONLY the cs slice, compactly, to out_slice (nt, h, w, cs).  The wrapped
 * 1x1 conv then reads channels [0, cs) from it and the rest from x (mvf_conv_desc_t.split_c): the pass-through
 * channels are never copied and x stays intact for the residual branch (replaces cat + transpose + contiguous,
 * MVF.py:135-137). */
int mvf_fwd_infer_slice(const mvf_desc_t* d, const void* x, void* out_slice,
                        const float* w_t, const float* w_h, const float* w_w,
                        const float* bn_scale, const float* bn_shift, void* stream);

/* Training forward: BatchNorm3d with batch statistics over (n,t,h,w) (biased variance), running-stat
 * update (momentum, unbiased variance; torch defaults used at MVF.py:69), then hard-swish.
 * save_mean / save_invstd (fp32 [cs]) are outputs kept for mvf_bwd.  running_* may be NULL. */
size_t mvf_fwd_train_workspace_bytes(const mvf_desc_t* d);
int mvf_fwd_train(const mvf_desc_t* d, const void* x, void* out,
                  const float* w_t, const float* w_h, const float* w_w,
                  const float* gamma, const float* beta, float eps, float momentum,
                  float* running_mean, float* running_var, float* save_mean, float* save_invstd,
                  void* ws, size_t ws_bytes, void* stream);

/* Backward of MVF-proper (the reference relies on autograd; formulas in SURVEY.md Appendix B).
 * g = dL/d(out) (full tensor), x = the forward input.  training != 0: batch-stat BN backward using
 * save_mean/save_invstd; training == 0: eval BN (pass mean = running_mean, invstd = 1/sqrt(var+eps)).
 * gamma == NULL <=> use_hs=False.  dx == g allowed (in place on the slice); otherwise channels >= cs
 * are copied from g.  dw_* are fp32 [cs][3], dgamma/dbeta fp32 [cs]; all are overwritten. */
size_t mvf_bwd_workspace_bytes(const mvf_desc_t* d);
int mvf_bwd(const mvf_desc_t* d, const void* g, const void* x,
            const float* w_t, const float* w_h, const float* w_w,
            const float* gamma, const float* beta, const float* mean, const float* invstd, int training,
            void* dx, float* dw_t, float* dw_h, float* dw_w, float* dgamma, float* dbeta,
            void* ws, size_t ws_bytes, void* stream);


/* ------------------------------------------------------------------------------------------------
 * Conv / BN / ReLU stack of the backbone (codes/models/backbones/resnet.py:208-244 Bottleneck.forward,
 * :479-494 ResNet.forward) as implicit-GEMM on the matrix cores.  Activations are channels-last
 * (N, H, W, C); weights are pre-packed [cout][kh][kw][cin] in the activation dtype with the eval-mode
 * BatchNorm scale folded in (mvf_pack_conv_weight), the BN shift arrives as `bias`.
 *   y = act( conv(x, w) + bias [+ residual] )
 * replaces nn.Conv2d -> BatchNorm2d(eval) -> [+= identity] -> ReLU  (resnet.py:213-242).
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t n, h, w;          /* input: images, height, width                                        */
    int32_t cin, cout;        /* channels contracted per tap / output channels                       */
    int32_t kh, kw, stride, pad;
    int32_t ho, wo;           /* output height / width (validated against the formula)               */
    int32_t x_pix_stride;     /* elements between consecutive input pixels (>= cin; = C of x)        */
    int32_t dtype;            /* MVF_F32 | MVF_BF16 (storage of x, w, residual, y)                   */
    int32_t relu;             /* apply ReLU in the epilogue                                          */
    int32_t split_c;          /* 0, or: channels [0, split_c) are read from x2 instead of x (the    */
    int32_t x2_pix_stride;    /*   compact MVF slice, pitch x2_pix_stride); 1x1 convs only           */
    int32_t in_dil;           /* 0/1, or s > 1: x is read as if zero-upsampled by s (data-gradient of a       */
                              /*   stride-s conv: y = dgrad needs stride == 1 here; ho,wo up to (h-1)*s+1+... ) */
    int32_t res_c0;           /* the residual is added to output channels >= res_c0 only (multiple of 4; 0 = all).   */
                              /*   MVF block backward: channels [0, cs) of the conv1 data gradient go through the    */
                              /*   transposed stencil first, which adds their share (mvf_nhwc_stencil addend)        */
    int32_t x_c0;             /* [r5] 0, or with split_c > 0: x holds channels [split_c, cin) at column (channel - x_c0) of its rows  */
                              /*   (x_pix_stride >= cin - x_c0): the contraction runs over the CONCATENATION [x2 | x] of two compact   */
                              /*   tensors (x_c0 = split_c) instead of over x with its first split_c channels replaced               */
} mvf_conv_desc_t;

int mvf_conv2d_nhwc_fwd(const mvf_conv_desc_t* d, const void* x, const void* x2, const void* w_packed,
                        const float* bias, const void* residual, void* y, void* stream);
/* Same, with a scratch buffer (>= mvf_conv2d_workspace_bytes) that enables the stream-K decomposition of the last,
 * partial wave of output tiles (partial accumulators + publication flags live there).  One buffer per stream. */
size_t mvf_conv2d_workspace_bytes(const mvf_conv_desc_t* d);
int mvf_conv2d_nhwc_fwd_ws(const mvf_conv_desc_t* d, const void* x, const void* x2, const void* w_packed,
                           const float* bias, const void* residual, void* y, void* ws, size_t ws_bytes, void* stream);
/* The MVF module FUSED into its wrapped 1x1 conv (MVF.forward, codes/models/modules/MVF.py:104-138, followed by conv1 -> bn1 -> relu of
 * Bottleneck.forward, resnet.py:213-215, eval mode): y = relu(conv1x1(x') + bias) where x' = x with channels [0, cs) replaced by
 * act(scale * (T/H/W 3-tap views of x, zero padded inside the clip / image) + shift) -- computed in the conv's A-operand loader from
 * the seven neighbours of each pixel; no slice buffer, no separate stencil launch.  d: kh = kw = 1, stride 1, ho x wo = h x w,
 * x_pix_stride = cin, d->n = clips * n_segment frames, relu = 1.  mvf_coef: [cs][12] fp32 = {w_t[3], w_h[3], w_w[3], scale, shift, 0} per
 * channel (absent views: zeros); act = 1: affine + hard-swish (use_hs), 0: the bare tap sum.  cs % 64 == 0 (bf16) / 32 (fp32). */
int mvf_conv2d_nhwc_fwd_mvf(const mvf_conv_desc_t* d, const void* x, const void* w_packed, const float* bias, const float* mvf_coef,
                            int cs, int n_segment, int act, void* y, void* ws, size_t ws_bytes, void* stream);
/* [r3] Second pass of a bottleneck's last conv in TRAINING (Bottleneck.forward, codes/models/backbones/resnet.py:229-244: out = conv3(out);
 * out = norm3(out); out += identity; out = relu(out)): the conv is recomputed from its narrow input (a quarter of z3's bytes) and the epilogue
 * applies the BatchNorm whose batch statistics the first pass (mvf_conv2d_nhwc_fwd_stats) produced: the accumulators are rounded to the storage
 * type (= the z3 that first pass stored), out = relu(bn_scale * z3 + bn_shift + r), r = residual or -- a downsample block -- res_scale * residual
 * + res_shift (that branch's BatchNorm applied to its raw conv output); sign_bits [n*ho*wo][cout/4] bytes as mvf_bn_apply_bits writes them.
 * Same result as mvf_bn_apply_bits on the z3 THIS entry point's first pass (mvf_conv2d_nhwc_fwd_stats through the same kernel) stored, bit for bit,
 * without reading z3; a statistics pass through another kernel (csrc/pw_sums.hip) may have seen individual z3 elements one storage-type ulp away.
 * d->relu = 0, in_dil <= 1. */
int mvf_conv2d_nhwc_fwd_bnapply(const mvf_conv_desc_t* d, const void* x, const void* x2, const void* w_packed, const float* bn_scale,
                                const float* bn_shift, const void* residual, const float* res_scale, const float* res_shift, void* out,
                                unsigned char* sign_bits, void* ws, size_t ws_bytes, void* stream);
/* [r3] BatchNorm backward of that bn3 WITHOUT a stored z3 (autograd of resnet.py:229-244): the conv is recomputed from its input and its
 * accumulators, rounded to the storage type, are z3; g = gradient of the block output, sign_bits = the bits the forward wrote, gm = g * bit.
 *   _sums : sums_part CHANNEL-MAJOR [cout][mvf_conv2d_stats_rows(d)][2] = per-128-row column sums of gm and gm * (z3 - mean) * invstd;
 *           mvf_bn_bwd_finalize turns them into dbeta / dgamma.  Nothing else is written.
 *   _apply: dz = gamma * invstd * (gm - dbeta / M - (z3 - mean) * invstd * dgamma / M), M = n*ho*wo (bn_bwd_apply's formula, mask mode 4).
 * With these two and mvf_conv2d_nhwc_fwd_bnapply the first pass may run as a statistics-only pass: mvf_conv2d_nhwc_fwd_stats(..., y = NULL). */
int mvf_conv2d_nhwc_fwd_bnbwd_sums(const mvf_conv_desc_t* d, const void* x, const void* x2, const void* w_packed, const void* g,
                                   const unsigned char* sign_bits, const float* bn_mean, const float* bn_invstd, float* sums_part, void* ws,
                                   size_t ws_bytes, void* stream);
int mvf_conv2d_nhwc_fwd_bnbwd_apply(const mvf_conv_desc_t* d, const void* x, const void* x2, const void* w_packed, const void* g,
                                    const unsigned char* sign_bits, const float* bn_gamma, const float* bn_mean, const float* bn_invstd,
                                    const float* dgamma, const float* dbeta, void* dz, void* ws, size_t ws_bytes, void* stream);
/* ... with the residual gated per element by sign bits ([n*ho*wo][cout/4] bytes, see mvf_bn_apply_bits); stride-1 launches */
int mvf_conv2d_nhwc_fwd_resmask(const mvf_conv_desc_t* d, const void* x, const void* x2, const void* w_packed,
                                const float* bias, const void* residual, const unsigned char* res_sign_bits, void* y,
                                void* ws, size_t ws_bytes, void* stream);
/* [r5] ... and with the OUTPUT gated as well: y[.., c] = (conv + bias + gated residual) * [out_gate bit] for c >= d->res_c0 (channels below res_c0 --
 * the MVF slice of a block's conv1 data gradient -- are written ungated).  out_gate_bits: the sign bits of the block output whose gradient y is
 * ([n*ho*wo][cout/4] bytes).  The block below then receives gm = g * [out > 0] (torch autograd's relu backward, resnet.py:244) as a tensor: its
 * BatchNorm backward, data gradient and weight gradient read it without the bits.  res_sign_bits may be NULL (an ungated residual). */
int mvf_conv2d_nhwc_fwd_resmask_gate(const mvf_conv_desc_t* d, const void* x, const void* x2, const void* w_packed, const float* bias,
                                     const void* residual, const unsigned char* res_sign_bits, const unsigned char* out_gate_bits, void* y,
                                     void* ws, size_t ws_bytes, void* stream);
/* [r5] ... and the column sums of the gated output in the same epilogue: with gm = y (as stored), sums_part CHANNEL-MAJOR [cout][mvf_conv2d_stats_rows(d)][2] =
 * per-128-row column sums of gm and gm^2.  The dz3-free block below (resnet.py:236-244 under autograd) takes bn3's dbeta from them and dgamma from its
 * weight-gradient GEMM (mvf_bn_bwd_dzfree_sums): no pass over (gm, z3), no read of z3.  (Channels below res_c0 belong to the MVF stencil's launch.)
 * ([r6] the form that read z3 here for the complete sums measured neutral for two rounds and was removed.) */
int mvf_conv2d_nhwc_fwd_resmask_gate_colsums(const mvf_conv_desc_t* d, const void* x, const void* x2, const void* w_packed, const void* residual,
                                             const unsigned char* res_sign_bits, const unsigned char* out_gate_bits, void* y, float* sums_part, void* ws,
                                             size_t ws_bytes, void* stream);
/* Stride-1 data gradient whose output da feeds the backward of a = ReLU(BN(z)): besides y = dgrad(dz) it accumulates that
 * BatchNorm's backward sums in the epilogue -- sums_part, CHANNEL-MAJOR [cout][mvf_conv2d_stats_rows(d)][2] = per-128-row column sums of gm and
 * gm * xhat with gm = y * [bn_scale*z + bn_shift > 0], xhat = (z - bn_mean) * bn_invstd (z: the forward conv output the BN
 * normalised, same shape as y).  mvf_bn_bwd_finalize (nblk = that row count) turns them into dgamma / dbeta; no separate
 * mvf_bn_bwd_reduce pass.  (Channel-major: a channel's rows are contiguous, the finalize reads whole cache lines.) */
int mvf_conv2d_nhwc_dgrad_bnsums(const mvf_conv_desc_t* d, const void* dz, const void* w_packed_dgrad, void* y, const void* bn_z,
                                 const float* bn_mean, const float* bn_invstd, const float* bn_scale, const float* bn_shift,
                                 float* sums_part, void* ws, size_t ws_bytes, void* stream);
int mvf_bn_bwd_finalize(const float* sums_part, int nblk, int c, float* dgamma, float* dbeta, void* stream);
/* Training forward: plain conv (no bias / residual / ReLU) whose epilogue also accumulates the BatchNorm batch statistics of
 * the tensor it writes: stats_part, CHANNEL-MAJOR [cout][mvf_conv2d_stats_rows(d)][2] = per-128-row column sums of (y-K), (y-K)^2 with
 * K = stats_shift[cout] (pass the BN's running_mean; NULL = 0).  Feed stats_part to mvf_bn_train_finalize. */
int mvf_conv2d_stats_rows(const mvf_conv_desc_t* d);
int mvf_conv2d_nhwc_fwd_stats(const mvf_conv_desc_t* d, const void* x, const void* x2, const void* w_packed, void* y,
                              float* stats_part, const float* stats_shift, void* ws, size_t ws_bytes, void* stream);

/* Which kernel the calling thread's LAST mvf_conv2d_* call launched: a host-side record (thread-local, plain stores next to each launch; no device
 * work, no synchronisation) for tests and tools -- the launch policy (csrc/conv_nhwc.hip launch_conv, MVF_POLICY) decides it per shape, and nothing else
 * tells a caller which kernel family its shape reached.  A call that launches several kernels (a strided data gradient: one per parity class with
 * taps) leaves the record of its last launch and the count; a call refused before its first launch leaves launches = 0, family = MVF_CONV_FAM_NONE. */
enum {
    MVF_CONV_FAM_NONE = 0,
    MVF_CONV_FAM_REG = 1,          /* register-staged, single LDS buffer (conv_igemm_lowk_kernel)                                  */
    MVF_CONV_FAM_X3 = 2,           /* the same with fp32 storage on the bf16 matrix cores (conv_igemm_x3_kernel)                    */
    MVF_CONV_FAM_LDS_DMA = 3,      /* 4-wave LDS-DMA kernel, `buffers` = 1 | 2 (conv_igemm_glds_kernel)                             */
    MVF_CONV_FAM_T256_2B = 4,      /* 256 x 256 tile, two-barrier loop (conv_igemm_big2_kernel)                                     */
    MVF_CONV_FAM_T256_P4 = 5,      /* 256 x 256 tile, four-phase loop (conv_igemm_p4_kernel)                                        */
    MVF_CONV_FAM_DBUF = 6,         /* register-staged, double-buffered (conv_igemm_kernel)                                          */
    MVF_CONV_FAM_DBUF_PF2 = 7,     /* ... with the two-chunk register prefetch (conv_igemm_pf2_kernel)                              */
    MVF_CONV_FAM_STREAMK = 8,      /* double-buffered full waves + the stream-K tail (conv_streamk_kernel)                          */
    MVF_CONV_FAM_GENERIC = 9,      /* generic-shape fallback (conv_igemm_gen_kernel)                                                */
    MVF_CONV_FAM_MVF_LOADER = 10,  /* MVF fused into the A loader; `buffers` = 0 register-staged, 1 | 2 LDS-DMA                     */
    MVF_CONV_FAM_STEM_DIRECT = 11, /* csrc/stem_direct.hip                                                                          */
    MVF_CONV_FAM_PW_SUMS = 12,     /* csrc/pw_sums.hip                                                                              */
    MVF_CONV_FAM_C3X3_C64 = 13     /* csrc/conv3x3_c64.hip                                                                          */
};
typedef struct {
    int32_t family;                /* MVF_CONV_FAM_*                                                                                */
    int32_t epi_asked;             /* the epilogue the launch asked for (conv_epi_of; the direct kernels: their own epilogue code)  */
    int32_t epi_run;               /* the epilogue instantiated: 0 (generic, run-time arguments) when the family has not epi_asked  */
    int32_t pointwise;             /* 1: the pointwise loader specialisation                                                        */
    int32_t buffers;               /* LDS A/B buffers of the main loop (0: not applicable)                                          */
    int32_t tile_m, tile_n;        /* output tile of a workgroup                                                                    */
    int32_t dtype;                 /* MVF_F32 | MVF_BF16                                                                            */
    int32_t k_chunks;              /* 128-byte K chunks of the last launch                                                          */
    int32_t half_k;                /* 1: the half-chunk variant of the LDS-DMA kernel (the bf16 stem)                               */
    int32_t launches;              /* kernel launches the call made                                                                 */
} mvf_conv_launch_info_t;
int mvf_conv2d_last_launch(mvf_conv_launch_info_t* out);

/* w_oihw fp32 (cout, cin, kh, kw) [x scale[cout]] -> packed [cout][kh][kw_pad][cin_pad] in `dtype`
 * (zero padded; kw_pad >= kw, cin_pad >= cin).  bias_out[co] = shift[co] (copied) when given.
 * scale/shift = folded eval BatchNorm2d: scale = gamma/sqrt(var+eps), shift = beta - mean*scale. */
int mvf_pack_conv_weight(const float* w_oihw, int cout, int cin, int kh, int kw, int kw_pad, int cin_pad,
                         const float* scale, void* w_packed, int dtype, void* stream);
/* scale = gamma/sqrt(var+eps), shift = beta - mean*scale  (resnet eval BN, norm.py:59 eps) */
int mvf_bn_fold(const float* gamma, const float* beta, const float* mean, const float* var, float eps, int c,
                float* scale, float* shift, void* stream);

/* Stem input: (n,3,h,w) fp32 NCHW -> zero-padded channels-last (n, h+2*pad, wp, 4) in `dtype`
 * (wp >= w + 2*pad + 2) so that the 7x7/2 stem (resnet.py:424-425,481) becomes 7 K-chunks of 8 px x 4 ch. */
int mvf_stem_prep(const float* x_nchw, int n, int c, int h, int w, int pad, int wp, void* out, int dtype, void* stream);

/* The device side of the input pipeline, fused: decoded uint8 frames (n, hs, ws, 3) HWC -> the h x w window at
 * (y0, x0) of each frame [crop: augmentations.py CenterCrop / ThreeCrop :465-540 offsets], mirrored when flip != 0 [Flip :196-228],
 * channels reversed when to_rgb [Normalize.imnormalize :365-374], value = (float(px) [/ 255 when div_255] - mean[c]) * (1/std[c])
 * in two rounded fp32 steps as the reference's subtract-then-multiply, stacked channels-first [FormatShape formating.py:146-160].
 * window = device int32 (n,3) rows (y0, x0, flip) or NULL (= 0,0,0).  mean3 / std3 are HOST pointers (3 floats each).
 * Outputs (either may be NULL): out_stem = (n, h+2*pad, wp, 4) `dtype`, zero padded, the 7x7 stem's operand exactly as
 * mvf_stem_prep lays it out; out_nchw = (n,3,h,w) fp32, the tensor the reference's collate would hand to the model.
 * The host then ships uint8 frames (1/4 of the fp32 bytes, distributed.py:40-62 scatter) instead of normalised floats. */
int mvf_frames_prep_u8(const unsigned char* frames_hwc, int n, int hs, int ws, const int* window, int h, int w,
                       const float* mean3, const float* std3, int to_rgb, int div_255, int pad, int wp, void* out_stem,
                       float* out_nchw, int dtype, void* stream);
/* mvf_frames_prep_u8 with a bilinear resample in front of the crop [Resize / RandomResizedCrop augmentations.py:13-68, 600-661]:
 * rows = device int32 (n, 11), one row per frame: (hs_i, ws_i, by, bx, bh, bw, rh, rw, oy, ox, flip).  Frame i's image is
 * frames_hwc[i, :hs_i, :ws_i] of the (n, hs, ws, 3) batch (padded to the largest frame); its patch [by, by+bh) x [bx, bx+bw), already
 * clipped to the image, is resized to rh x rw with cv2 INTER_LINEAR CV_8U arithmetic (exactly 2x down in both axes: INTER_AREA's
 * rounded 2x2 mean, as cv2 switches), and resized[oy:oy+h, ox:ox+w], mirrored when flip != 0, continues exactly as in
 * mvf_frames_prep_u8.  A row with bh == rh and bw == rw gives mvf_frames_prep_u8's output for the window (by+oy, bx+ox, flip), bit
 * for bit.  rows must be non-NULL; their contents are NOT checked here (the caller validates them: out-of-range rows read out of
 * bounds).  Same outputs, dtypes and host-side mean3 / std3 as mvf_frames_prep_u8. */
int mvf_frames_resample_u8(const unsigned char* frames_hwc, int n, int hs, int ws, const int* rows, int h, int w,
                           const float* mean3, const float* std3, int to_rgb, int div_255, int pad, int wp, void* out_stem,
                           float* out_nchw, int dtype, void* stream);
/* mvf_frames_resample_u8 with a per-frame affine colour transform between the resample and Normalize [ColorJitter
 * augmentations.py:238-339: brightness, contrast, saturation, hue and the PCA lighting term are all affine in the pixel and nothing
 * clips, so one frame's whole jitter is q = M p + b].  color = device fp32 (n, 12), one row per frame: M[0][0..2], M[1][0..2],
 * M[2][0..2], b[0..2], indices in the STORED channel order of the frame (before to_rgb); preprocess.color_jitter_table composes it.
 * p[k] = float(resampled uint8 px[k]); q[c] = ((M[c][0]*p[0] + M[c][1]*p[1]) + M[c][2]*p[2]) + b[c], every product and sum rounded to
 * fp32 on its own (no FMA); then f = q[to_rgb ? 2 - k : k] continues as in mvf_frames_prep_u8.  M = I gives p + b rounded once, the
 * reference's float32 `img + bgr`.  color == NULL gives mvf_frames_resample_u8's output, bit for bit.  The coefficients are NOT
 * checked here (the caller refuses non-finite ones).  Everything else as mvf_frames_resample_u8. */
int mvf_frames_resample_color_u8(const unsigned char* frames_hwc, int n, int hs, int ws, const int* rows, const float* color, int h, int w,
                                 const float* mean3, const float* std3, int to_rgb, int div_255, int pad, int wp, void* out_stem,
                                 float* out_nchw, int dtype, void* stream);
/* mvf_frames_resample_color_u8 with a frame index in front, so that several output images share one decoded frame [whole-video testing:
 * SampleFrames(num_clips) clips that overlap or clamp, ThreeCrop / TenCrop augmentations.py:465-596]: frames_hwc = (n_src, hs, ws, 3),
 * src_index = device int32 (n_out,), rows = (n_out, 11), color = (n_out, 12) or NULL; output image i is cut from frame src_index[i],
 * whose real size is row i's (hs_i, ws_i); the outputs hold n_out images.  The arithmetic per pixel is mvf_frames_resample_color_u8's:
 * the result equals that export run on the gathered batch frames_hwc[src_index], bit for bit, and src_index == NULL means i -> i
 * (n_src must equal n_out then).  The index contents are NOT checked here (the caller validates 0 <= src_index[i] < n_src, as for the
 * rows: an out-of-range index reads out of bounds).  Everything else as mvf_frames_resample_color_u8. */
int mvf_frames_gather_resample_u8(const unsigned char* frames_hwc, int n_src, int hs, int ws, const int* src_index, int n_out, const int* rows,
                                  const float* color, int h, int w, const float* mean3, const float* std3, int to_rgb, int div_255, int pad,
                                  int wp, void* out_stem, float* out_nchw, int dtype, void* stream);
/* mvf_frames_gather_resample_u8 for decoder-native YUV 4:2:0 frames (what every video decoder produces; the packed frames the other
 * exports take are a CPU colour conversion on top of it, at twice the bytes).  frames = (n_src, 3 * hs / 2, pitch) bytes, hs and pitch even,
 * pitch >= ws:
 *   layout 0 = I420: hs luma rows of pitch bytes, then the U plane (hs / 2 rows of pitch / 2 bytes), then the V plane likewise;
 *   layout 1 = NV12: hs luma rows of pitch bytes, then hs / 2 rows of pitch bytes of interleaved U, V pairs.
 * A frame stands for the packed (hs, ws, 3) uint8 frame with, at luma pixel (y, x) and the chroma sample (y >> 1, x >> 1) (replicated, not
 * interpolated; absolute frame coordinates, so odd by / bx are fine), in int32 with an arithmetic shift:
 *   y' = max(0, Y - y_off) * CY
 *   R = sat8((y' + (1 << 19) + CVR * (V - 128)) >> 20)
 *   G = sat8((y' + (1 << 19) - CVG * (V - 128) - CUG * (U - 128)) >> 20)
 *   B = sat8((y' + (1 << 19) + CUB * (U - 128)) >> 20)
 * every constant rint(c * 2^20) of the decimal coefficient c:
 *   standard 0 = BT.601 limited: y_off 16, cY 1.164,    cVR 1.596,    cVG 0.813,    cUG 0.391,    cUB 2.018
 *   standard 1 = BT.601 full:    y_off 0,  cY 1.0,      cVR 1.402,    cVG 0.714136, cUG 0.344136, cUB 1.772     (yuvj420p)
 *   standard 2 = BT.709 limited: y_off 16, cY 1.164384, cVR 1.792741, cVG 0.532909, cUG 0.213249, cUB 2.112402
 * (this table's conversion, within 1 of the rounded float definition; NOT bit-equal to any particular decoder library's).  order = the
 * stored channel order of that packed frame: 0 = BGR (what the raw-frame path stores), 1 = RGB.  The four taps of the resample (or the four
 * pixels of the exact-2x area mean) are converted, and everything after them -- blend, colour map in stored order, to_rgb, div_255,
 * Normalize, both outputs -- is mvf_frames_gather_resample_u8's: the result equals that export run on the converted packed frames, bit for
 * bit.  rows' (hs_i, ws_i) may be odd (a frame of odd size lies in even-sized planes, chroma ceil(hs_i / 2) x ceil(ws_i / 2)).  Odd hs or
 * pitch, pitch < ws and an unknown layout / standard / order return MVF_EINVAL; rows and src_index are NOT checked here, as above. */
int mvf_frames_yuv420_gather_resample_u8(const unsigned char* frames, int n_src, int hs, int ws, int pitch, int layout, int standard, int order,
                                         const int* src_index, int n_out, const int* rows, const float* color, int h, int w, const float* mean3,
                                         const float* std3, int to_rgb, int div_255, int pad, int wp, void* out_stem, float* out_nchw, int dtype,
                                         void* stream);
/* mvf_frames_gather_resample_u8 / mvf_frames_yuv420_gather_resample_u8 over frames WHERE AND HOW THE DECODER LEFT THEM: instead of a dense
 * batch in which every frame shares one padded extent and one row pitch, every output image carries the byte offsets and row pitches of
 * the planes it is cut from.  frames = one byte buffer of frames_bytes bytes, 1 <= frames_bytes < 2^31 (so offsets fit int32);
 *   format 0 = packed 3-byte pixels in stored channel order (standard and order are ignored), 1 = I420, 2 = NV12; standard and order as in
 *   mvf_frames_yuv420_gather_resample_u8.
 * rows = device int32 (n_out, 11) and color = device fp32 (n_out, 12) or NULL as in mvf_frames_gather_resample_u8, one row per OUTPUT image;
 * addr = device int32 (n_out, 5), (o0, p0, o1, o2, p1): byte offsets from `frames` and row pitches in bytes of the image row i is cut from:
 *   format 0: pixel (y, x) at o0 + y * p0 + 3 * x;  o1 = o2 = p1 = 0;
 *   I420:     luma at o0 + y * p0 + x, U at o1 + (y >> 1) * p1 + (x >> 1), V at o2 + (y >> 1) * p1 + (x >> 1);
 *   NV12:     luma as I420, U at o1 + (y >> 1) * p1 + 2 * (x >> 1), V one byte after it;  o2 = 0.
 * Pitches may be odd and may exceed the row; a frame of odd size has chroma planes of ceil(hs_i / 2) x ceil(ws_i / 2) samples.  Rows may name
 * the same planes -- that is how clips and crops share a decoded frame, so there is no src_index -- and images of one launch may differ in
 * size, pitch and plane placement.  Addresses are formed in 64-bit arithmetic.  The arithmetic per pixel is the dense exports': for format 0
 * the result equals mvf_frames_gather_resample_u8 on the dense batch that holds the same frames, for formats 1 and 2
 * mvf_frames_yuv420_gather_resample_u8 likewise, bit for bit, both outputs and both dtypes; bytes outside the addressed planes never reach
 * the result.  An unknown format / standard / order / dtype, NULL rows or addr, frames_bytes outside [1, 2^31) and wp < w + 2 * pad return
 * MVF_EINVAL; the CONTENTS of rows and addr are NOT checked here (the caller validates them, preprocess.check_addresses: a bad offset or
 * pitch reads out of bounds).  Everything else as mvf_frames_gather_resample_u8. */
int mvf_frames_addressed_resample_u8(const unsigned char* frames, long long frames_bytes, int format, int standard, int order,
                                     int n_out, const int* rows, const int* addr, const float* color, int h, int w,
                                     const float* mean3, const float* std3, int to_rgb, int div_255, int pad, int wp,
                                     void* out_stem, float* out_nchw, int dtype, void* stream);

/* MaxPool2d(3, stride 2, pad 1) on NHWC (resnet.py:431,484). */
int mvf_maxpool3x3s2_nhwc(const void* x, int n, int h, int w, int c, void* y, int dtype, void* stream);

/* Head (codes/models/heads/tsn_clshead.py:71-117): per clip, mean over (T,H,W) of the NHWC features
 * (AdaptiveAvgPool2d + consensus mean are both linear, so they commute with the FC; the fcn_testing
 * branch :99-117 is the same expression), then new_fc.  feat (clips*T, H, W, c) -> scores (clips, classes). */
int mvf_head_pool_fc(const void* feat, int clips, int t, int hw, int c, const float* fc_w, const float* fc_b,
                     int classes, float* pooled_ws, float* scores, int dtype, void* stream);
/* average_clip (codes/models/recognizers/base.py:43-74): kind 0 = None (copy), 1 = 'score', 2 = 'prob'. */
int mvf_average_clip(const float* scores, int clips, int classes, int kind, float* out, void* stream);
/* average_clips = 'sigmoid' (multi-label heads): out[k] = the mean over the clips, in ascending order, of sigmoid(scores[cl][k]); fp64 arithmetic that
 * cannot overflow for either sign of the score, rounded to fp32 once; a NaN score gives a NaN.  scores (clips, classes) -> out (1, classes), any
 * classes >= 1.  MVF_EINVAL before any launch: NULL scores / out, clips < 1 or classes < 1. */
int mvf_average_clip_sigmoid(const float* scores, int clips, int classes, float* out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Training step (fp32 this round).  Mirrors, in order: Bottleneck.forward with batch-statistics BatchNorm2d
 * (codes/models/backbones/resnet.py:208-244; torch defaults momentum 0.1, eps from norm.py:59), its autograd
 * backward, TSNClsHead.forward + BaseHead.loss (heads/tsn_clshead.py:71-98, heads/base.py:40-45) and
 * DistOptimizerHook.after_train_iter (core/dist_utils.py:61-67: backward, all-reduce/world, clip_grad_norm_(40),
 * SGD-nesterov step; optimizer cfg mvf_kinetics400_2d_rgb_r50_dense.py:152-154).
 * All tensors are channels-last matrices [m][c] (m = n*h*w), c % 4 == 0.
 * ---------------------------------------------------------------------------------------------- */
/* [r5] mvf_conv2d_nhwc_dgrad_bnsums over a SPLIT operand and with a bias: y = [x2 | x] * w_packed^T + bias (d->split_c channels from x2, the rest
 * from x, see mvf_conv_desc_t.x_c0), pointwise, stride 1 -- the data gradient of a bottleneck's conv3 taken on (gm, a2) instead of on dz3
 * (mvf_bn_bwd_dzfree_prep makes w_packed and bias). */
int mvf_conv2d_nhwc_dgrad_bnsums_split(const mvf_conv_desc_t* d, const void* x, const void* x2, const void* w_packed, const float* bias, void* y,
                                       const void* bn_z, const float* bn_mean, const float* bn_invstd, const float* bn_scale, const float* bn_shift,
                                       float* sums_part, void* ws, size_t ws_bytes, void* stream);
/* [r5] BatchNorm backward of out = relu(bn3(conv3(a2)) + identity) (Bottleneck.forward, codes/models/backbones/resnet.py:229-244, under torch autograd)
 * WITHOUT the dz3 tensor (csrc/bn_dzfree.hip).  dz3 = a (gm - d0 - kx (z3 - mean)) with a = gamma invstd, d0 = dbeta / m, kx = invstd dgamma / m is
 * affine in (gm, z3) and z3 = a2 W^T, so
 *   da2 = dz3 W    = [gm | a2] [a.W ; -G] - v      G = W^T diag(a kx) W,  v_k = sum_c a_c (d0_c - kx_c mean_c) W[c][k]
 *   dW  = dz3^T a2 = a . (Q - d0 (x) sa - kx . (W A2 - mean (x) sa))     Q = gm^T a2, A2 = a2^T a2, sa = m * a_mean
 * _prep : w_out [k][c + k] (the data-gradient pack's layout: row = conv input channel) and bias_out [k] = -v for mvf_conv2d_nhwc_dgrad_bnsums_split,
 *         from w_packed_dgrad [k][c] (mvf_pack_conv_weight_dgrad of the c x k pointwise weights) and the BatchNorm's dgamma / dbeta
 *         (mvf_bn_bwd_reduce on gm and the stored z3; zeros for a BatchNorm with frozen statistics).
 * _wgrad: dw [c][k] holds Q on entry (mvf_conv2d_nhwc_wgrad with dz = gm) and dW on return; gram [k][k] = A2 (the same call with dz = x = a2),
 *         a_mean [k] = column means of a2, w_packed [c][k] = the forward pack.  bf16 storage. */
int mvf_bn_bwd_dzfree_prep(const void* w_packed_dgrad, int c, int k, const float* gamma, const float* mean, const float* invstd, const float* dgamma,
                           const float* dbeta, long m, void* w_out, float* bias_out, int dtype, void* stream);
int mvf_bn_bwd_dzfree_wgrad(float* dw, const void* w_packed, const float* gram, const float* a_mean, const float* gamma, const float* mean,
                            const float* invstd, const float* dgamma, const float* dbeta, long m, int c, int k, int dtype, void* stream);
/* _sums : dgamma / dbeta WITHOUT the pass over (gm, z3) either: sum_m gm z3 = sum_k W[c][k] Q[c][k] (Q = the weight-gradient GEMM of _wgrad, taken FIRST) and
 *         sum_m gm from the column sums the kernels that stored gm took in their epilogues -- part_lo [c_split][rows_lo][2] (the MVF stencil's slice,
 *         mvf_nhwc_stencil_gate_colsums) and part_hi [c][rows_hi][2] indexed by the absolute channel (mvf_conv2d_nhwc_fwd_resmask_gate_colsums); element
 *         [.][.][0] is read.  dgamma[c] = invstd (W[c].Q[c] - mean sum gm), dbeta[c] = sum gm. */
int mvf_bn_bwd_dzfree_sums(const float* q, const void* w_packed, int c, int k, const float* mean, const float* invstd, const float* part_lo, int rows_lo,
                           int c_split, const float* part_hi, int rows_hi, float* dgamma, float* dbeta, int dtype, void* stream);
size_t mvf_bn_workspace_bytes(long m, int c);
/* batch mean / biased var of z over m -> save_mean, save_invstd, scale = gamma*invstd, shift = beta - mean*scale;
 * running_mean/var updated in place (unbiased var).  Shifted single-pass sums (shift = old running_mean). */
int mvf_bn_train_stats(const void* z, long m, int c, const float* gamma, const float* beta, float eps, float momentum,
                       float* running_mean, float* running_var, float* save_mean, float* save_invstd, float* scale,
                       float* shift, void* ws, size_t ws_bytes, int dtype, void* stream);
/* second half of mvf_bn_train_stats for the channel-major partial sums [c][nblk][2] produced by mvf_conv2d_nhwc_fwd_stats
 * (nblk = mvf_conv2d_stats_rows(d); K must be the same running_mean) */
int mvf_bn_train_finalize(const float* part, int nblk, long m, int c, const float* gamma, const float* beta, float eps,
                          float momentum, float* running_mean, float* running_var, float* save_mean, float* save_invstd,
                          float* scale, float* shift, void* stream);
/* [r5] The same outputs for z = a W^T, the output of a POINTWISE conv (Bottleneck.conv3 -> norm3, resnet.py:236-237), WITHOUT computing z: mean_c = W[c].abar,
 * var_c = W[c] (A2 / m - abar abar^T) W[c]^T from the Gram matrix gram [k][k] = a^T a of the conv's input (mvf_conv2d_nhwc_wgrad with dz = x = a), its
 * column means a_mean [k] (mvf_bn_train_stats on a) and the forward pack w_packed [c][k].  Replaces the statistics pass of a block that applies this
 * BatchNorm in a second conv pass (mvf_conv2d_nhwc_fwd_bnapply); the dz3-free backward reuses gram / a_mean.  bf16 storage, c and k multiples of 32.
 * Up to 16 rows (m <= 16: a variance of at most 15 squares, which some channels take 1e6 times below its terms) the sums are taken in fp64. */
int mvf_bn_train_stats_gram(const float* gram, const float* a_mean, const void* w_packed, long m, int c, int k, const float* gamma, const float* beta,
                            float eps, float momentum, float* running_mean, float* running_var, float* save_mean, float* save_invstd, float* scale,
                            float* shift, int dtype, void* stream);
/* out = act(z * scale + shift) (mvf_bn_apply without a residual) + the column means of what it stores: a_mean for mvf_bn_train_stats_gram from the kernel that
 * WRITES conv3's input (norm2 + relu, resnet.py:233-234) instead of a pass over it.  ws >= max(mvf_bn_workspace_bytes(m, c), 4608 * c * 8) bytes
 * (one partial row per workgroup row band of the apply plan). */
int mvf_bn_apply_colmeans(const void* z, long m, int c, const float* scale, const float* shift, int act, void* out, float* mean_out, void* ws,
                          size_t ws_bytes, int dtype, void* stream);
/* out = act(z*scale + shift [+ residual | + residual*rscale + rshift]); act: 0 none, 1 ReLU, 2 hard-swish */
int mvf_bn_apply(const void* z, long m, int c, const float* scale, const float* shift, const void* residual,
                 const float* rscale, const float* rshift, int act, void* out, int dtype, void* stream);
/* gm = g * act'(.) ; dbeta = sum gm ; dgamma = sum gm * xhat.  mask_mode: 0 none, 1 ReLU via ymask > 0 (ymask = the
 * forward output), 2 ReLU via scale*z+shift > 0, 3 hard-swish'(scale*z+shift), 4 sign bits (see mvf_bn_apply_bits).
 * g rows are g_pitch apart (>= c).
 * gm_out (optional, pitch c) receives gm. */
int mvf_bn_bwd_reduce(const void* g, int g_pitch, const void* z, const void* ymask, long m, int c, const float* mean,
                      const float* invstd, const float* scale, const float* shift, int mask_mode, void* gm_out,
                      float* dgamma, float* dbeta, void* ws, size_t ws_bytes, int dtype, void* stream);
/* dz = gamma*invstd*(gm - dbeta/m - xhat*dgamma/m), gm recomputed from g with mask_mode 0 / 2 / 3 */
int mvf_bn_bwd_apply(const void* g, int g_pitch, const void* z, long m, int c, const float* gamma, const float* mean,
                     const float* invstd, const float* scale, const float* shift, const float* dgamma,
                     const float* dbeta, int mask_mode, void* dz, int dtype, void* stream);
/* The same with the ReLU mask of a block output kept as SIGN BITS instead of re-reading the tensor (1/8 of its bf16 bytes):
 * mvf_bn_apply_bits also writes sign_bits [m][c/4] bytes (bit j of byte k <=> out[.., 4k+j] > 0); mask_mode 4 of
 * mvf_bn_bwd_reduce / mvf_bn_bwd_apply_masked takes them as ymask (mask_mode 1 there = the tensor itself).  The skip-connection
 * gradient g*mask is then never materialised: mvf_conv2d_nhwc_fwd_resmask / mvf_nhwc_stencil gate their residual / addend
 * with the same bits (torch autograd's relu backward, Bottleneck.forward codes/models/backbones/resnet.py:238-244). */
int mvf_bn_apply_bits(const void* z, long m, int c, const float* scale, const float* shift, const void* residual,
                      const float* rscale, const float* rshift, int relu, void* out, unsigned char* sign_bits, int dtype,
                      void* stream);
/* Stochastic depth (drop path, timm drop_path(x, p, training, scale_by_keep)) on the residual branch of a bottleneck, csrc/drop_path.hip:
 * mvf_bn_apply_bits with the BatchNorm output scaled per ROW before the residual is added.  row_scale: m / rows_per_image fp32 values in device memory,
 * image r / rows_per_image owns row r (the host draws them: mvfnet_amd/droppath.py; the kernels do not know whether a draw is per clip or per frame).
 * In fp32, per element of row r and channel k, with s = row_scale[r / rows_per_image]:
 *     u   = scale[k] * z + shift[k]                              formed exactly as mvf_bn_apply_bits forms it
 *     v   = s * u                                                one product, rounded
 *     res = residual  |  rscale[k] * residual + rshift[k]        as mvf_bn_apply_bits forms it; the residual is REQUIRED and never scaled
 *     out = act(v + res)                                         one sum, rounded (never fused with the product); act: 0 none, 1 ReLU
 * stored once in the storage type; sign_bits [m][c/4] (required) hold the signs of the STORED output in mvf_bn_apply_bits' layout.  With every s = 1.0f, out
 * and sign_bits equal mvf_bn_apply_bits on the same operands bit for bit; with s = 0 and a finite z, out = act(res) exactly; IEEE arithmetic throughout (a
 * non-finite z in a dropped row gives NaN, as 0 * inf does in torch).  The grid is mvf_bn_apply_bits' (its column plan at 4096 workgroups); no atomics, so
 * results are bit-identical from run to run.  Nothing is added to the mvf_bn_last_launch record.
 * Checked before any launch (MVF_EINVAL): a NULL operand (rscale / rshift may both be NULL), rows_per_image < 1, m % rows_per_image != 0, c % 4 != 0,
 * an unknown dtype or act, and the alignment: z, residual, out, scale, shift, rscale, rshift 16 bytes, row_scale 4 bytes.  fp32 and bf16 storage; bf16 takes
 * 16-byte lanes when c % 8 == 0 and sign_bits is 2-byte aligned, 8-byte lanes otherwise. */
int mvf_bn_apply_bits_rowscale(const void* z, long m, int c, const float* scale, const float* shift, const void* residual, const float* rscale,
                               const float* rshift, const float* row_scale, int rows_per_image, int act, void* out, unsigned char* sign_bits, int dtype,
                               void* stream);
/* The backward companion: the gradient into the scaled BatchNorm output, gm[r][k] = bit(r, k) ? s * g[r][k] : 0 with the sign bits mvf_bn_apply_bits_rowscale
 * wrote and the same row_scale table -- one fp32 product per element, stored once ([m][c], pitch c); g rows are g_pitch >= c apart.  (The gradient of the
 * identity path stays g gated by the bits, unscaled.)  With every s = 1.0f, gm equals the gm_out mvf_bn_bwd_reduce writes in mask mode 4, bit for bit.
 * Checked before any launch (MVF_EINVAL): a NULL operand, rows_per_image < 1, m % rows_per_image != 0, c % 4 != 0, g_pitch < c or g_pitch % 4 != 0, an
 * unknown dtype, and the alignment: g and gm_out 16 bytes, row_scale 4 bytes.  bf16 takes 16-byte lanes when c % 8 == 0, g_pitch % 8 == 0 and sign_bits is
 * 2-byte aligned. */
int mvf_gate_rowscale(const void* g, int g_pitch, const unsigned char* sign_bits, const float* row_scale, int rows_per_image, long m, int c, void* gm_out,
                      int dtype, void* stream);
int mvf_bn_bwd_apply_masked(const void* g, int g_pitch, const void* z, const void* ymask, long m, int c, const float* gamma,
                            const float* mean, const float* invstd, const float* scale, const float* shift,
                            const float* dgamma, const float* dbeta, int mask_mode, void* dz, int dtype, void* stream);
/* PAIRED backward of the two BatchNorms of a downsample block, out = relu(bn3(z3) + bnd(zd)) (Bottleneck.forward, resnet.py:227-233): both
 * receive the same masked gradient g * [out > 0] (sign_bits as written by mvf_bn_apply_bits), so g and the bits are read once for
 * both: dgamma / dbeta of a and b, then dz_a, dz_b.  Results are bit-identical to two mvf_bn_bwd_reduce + mvf_bn_bwd_apply_masked
 * (mask_mode 4) calls.  ws: 2 x mvf_bn_workspace_bytes(m, c). */
int mvf_bn_bwd_pair(const void* g, int g_pitch, const void* z_a, const void* z_b, const unsigned char* sign_bits, long m, int c,
                    const float* gamma_a, const float* mean_a, const float* invstd_a, float* dgamma_a, float* dbeta_a,
                    const float* gamma_b, const float* mean_b, const float* invstd_b, float* dgamma_b, float* dbeta_b,
                    void* dz_a, void* dz_b, void* ws, size_t ws_bytes, int dtype, void* stream);
/* [r4] BatchNorm backward APPLY fused with the weight gradient of the pointwise (1x1, stride 1) conv that produced the BatchNorm's input
 * (autograd of Bottleneck.forward, resnet.py:213-244: z = conv(x); out = relu(bn(z) [+ identity])): the pass that forms
 * dz = gamma * invstd * (gm - dbeta / m - xhat * dgamma / m) also contracts it with the conv input, dW[co][ci] = sum_m dz[m][co] * x[m][ci],
 * so dz is read once afterwards (by the data gradient) instead of twice.  dz is BIT-identical to mvf_bn_bwd_apply_masked; the weight gradient
 * is left as `splits` fp32 partial slabs [splits][c][k] that mvf_wgrad_slab_reduce sums in fixed order into dw (c, k, 1, 1) -- on any stream
 * that is ordered behind this call.  dgamma / dbeta must be final (mvf_bn_bwd_reduce / mvf_bn_bwd_finalize ran).  bf16 storage only; built for
 * the byte-bound shapes whose c x k accumulator fits one workgroup: mask_mode 4 (sign bits) with c % 256 == 0 and k = 64 / 128, mask_mode 2
 * (gate = scale * z + shift > 0) with c = 64 / 128 / 256 and k % 256 == 0; mvf_bn_bwd_wgrad_splits returns 0 for every other shape (use the
 * separate calls).  nbn = 1 here, 2 for the paired form below. */
int mvf_bn_bwd_wgrad_splits(long m, int c, int k, int nbn, int mask_mode);
size_t mvf_bn_bwd_wgrad_slab_bytes(long m, int c, int k, int nbn, int mask_mode);
int mvf_bn_bwd_apply_wgrad(const void* g, int g_pitch, const void* z, const void* ymask, long m, int c, const float* gamma, const float* mean,
                           const float* invstd, const float* scale, const float* shift, const float* dgamma, const float* dbeta, int mask_mode,
                           void* dz, const void* x, int x_pitch, int k, float* slabs, size_t slab_bytes, int dtype, void* stream);
/* [r4] The same for the PAIRED backward of a downsample block (mvf_bn_bwd_pair: sums of both BatchNorms, then both dz): dz_a / dz_b are
 * contracted with x_a (conv3's input) / x_b (the downsample conv's input = the block input; stride 1 only).  x_b = NULL: only conv a's weight
 * gradient is fused (k = 128; a stride-2 downsample conv keeps its GEMM).  ws: 2 x mvf_bn_workspace_bytes(m, c); slabs_*: slab_bytes each. */
int mvf_bn_bwd_pair_wgrad(const void* g, int g_pitch, const void* z_a, const void* z_b, const unsigned char* sign_bits, long m, int c,
                          const float* gamma_a, const float* mean_a, const float* invstd_a, float* dgamma_a, float* dbeta_a,
                          const float* gamma_b, const float* mean_b, const float* invstd_b, float* dgamma_b, float* dbeta_b,
                          void* dz_a, void* dz_b, const void* x_a, int xa_pitch, const void* x_b, int xb_pitch, int k,
                          float* slabs_a, float* slabs_b, size_t slab_bytes, void* ws, size_t ws_bytes, int dtype, void* stream);
/* [r4] The WHOLE backward of the last conv of a bottleneck that never stored its conv output (autograd of Bottleneck.forward, resnet.py:229-244:
 * out = relu(bn3(conv3(a2)) + identity), a2 = relu(bn2(z2))) in ONE pass: the 64 -> 256 channel pointwise conv is recomputed per 64-pixel chunk,
 * dz3 = gamma invstd (gm - dbeta / m - xhat dgamma / m) (gm = g gated by the block output's sign bits; bn3's dgamma / dbeta must be final) stays in
 * LDS and is contracted three ways: the weight gradient (fp32 slabs [splits][256][64] for mvf_wgrad_slab_reduce), the data gradient
 * dx = round_bf16(dz3 W) (m, 64), and the backward sums of bn2 over dx gated by scale2 z2 + shift2 > 0 (partial rows [64][sums_rows][2] for
 * mvf_bn_bwd_finalize, sums_rows = 2 x splits).  Replaces mvf_conv2d_nhwc_fwd_bnbwd_apply + mvf_conv2d_nhwc_dgrad_bnsums + mvf_conv2d_nhwc_wgrad
 * (dz3 is neither written nor re-read).  z_in = NULL: the conv input is not a BatchNorm's activation (a downsample branch, resnet.py:227-228, reading the block
 * input): dx is the plain data gradient, no sums (in_* / sums_part unused).  bf16 storage, c = 256, k = 64 only: mvf_conv1x1_bwd_fused_splits returns 0 for
 * anything else.  sign_bits: 16-byte aligned. */
int mvf_conv1x1_bwd_fused_splits(long m, int c, int k);
int mvf_conv1x1_bwd_fused(const void* a_in, int a_pitch, const void* w_packed, const void* g, int g_pitch, const unsigned char* sign_bits, long m, int c,
                          int k, const float* gamma, const float* mean, const float* invstd, const float* dgamma, const float* dbeta, const void* z_in,
                          const float* in_mean, const float* in_invstd, const float* in_scale, const float* in_shift, void* dx, float* sums_part,
                          int sums_rows, float* slabs, size_t slab_bytes, int dtype, void* stream);
/* [r4] BatchNorm-backward sums of BOTH branches of a downsample bottleneck that stored no z3 (resnet.py:227-244: out = relu(bn3(conv3(a2)) + bn_d(conv_d(x)))) in one
 * pass over g: sum gm and sum gm xhat for bn3 (a: conv3 on a_in) and bn_d (b: the downsample conv on x_in), both convs recomputed, g and the sign bits read once
 * (mvf_conv2d_nhwc_fwd_bnbwd_sums twice reads them twice).  Partial rows [256][rows][2] each for mvf_bn_bwd_finalize, rows = 2 x mvf_conv1x1_bwd_fused_splits.
 * x_in = NULL: the sums of bn3 alone (a plain block: conv a only; w_b / mean_b / invstd_b / part_b unused).  bf16 storage, c = 256, k = 64 for both convs. */
int mvf_conv1x1_bnbwd_sums_pair(const void* a_in, int a_pitch, const void* w_a, const void* x_in, int x_pitch, const void* w_b, const void* g, int g_pitch,
                                const unsigned char* sign_bits, long m, int c, int k, const float* mean_a, const float* invstd_a, const float* mean_b,
                                const float* invstd_b, float* part_a, float* part_b, int rows, int dtype, void* stream);
int mvf_wgrad_slab_reduce(const float* slabs, int nsplit, int cout, int k, float* dw_oihw, void* stream);
/* stem: y = maxpool3x3/2(relu(z*scale+shift)) (resnet.py:482-484).  argmax (optional, one byte per element of y) receives
 * the window position dy*3+dx of the first maximum; the backward routes g to it: ga = dL/d relu(bn(z)). */
int mvf_maxpool_bn_relu_fwd(const void* z, int n, int h, int w, int c, const float* scale, const float* shift, void* y,
                            unsigned char* argmax, int dtype, void* stream);
int mvf_maxpool_bn_relu_bwd(const unsigned char* argmax, const void* g, int n, int h, int w, int c, void* ga, int dtype,
                            void* stream);
/* The same scatter that also accumulates the backward sums of the BatchNorm under the pool (stem: pool(relu(bn(z))), reference
 * resnet.py:461-466): gm = ga * [scale*z + shift > 0], sums of gm and gm * (z - mean) * invstd per channel into the channel-major
 * partials sums_part [c][mvf_maxpool_bwd_sums_rows(n, h)][2]; mvf_bn_bwd_finalize turns them into dgamma / dbeta, so the
 * BatchNorm backward only needs its apply pass (mask_mode 2 over ga).  Needs c/4 to divide 256.  ga may be NULL. */
int mvf_maxpool_bwd_sums_rows(int n, int h);
/* ... and the matching apply pass that re-gathers ga instead of reading it (pass ga = NULL to mvf_maxpool_bn_relu_bwd_sums then):
 * dz = gamma*invstd * (gm - dbeta/M - xhat*dgamma/M), M = n*h*w, gm as above.  dgamma / dbeta: the finalized sums, or zeros for
 * a BatchNorm in eval mode (no batch-statistics term). */
int mvf_maxpool_bn_relu_bwd_apply(const unsigned char* argmax, const void* g, int n, int h, int w, int c, const void* z, const float* gamma,
                                  const float* mean, const float* invstd, const float* scale, const float* shift, const float* dgamma,
                                  const float* dbeta, void* dz, int dtype, void* stream);
int mvf_maxpool_bn_relu_bwd_sums(const unsigned char* argmax, const void* g, int n, int h, int w, int c, void* ga, const void* z, const float* mean,
                                 const float* invstd, const float* scale, const float* shift, float* sums_part, int dtype, void* stream);
/* Which kernels the calling thread's LAST BatchNorm / max-pool call launched: the counterpart of mvf_conv2d_wgrad_last_launch for csrc/train_ops.hip
 * (host-side, thread-local, plain stores next to the launches; no device work).  The entry points that have an MVF_BN_ENTRY_* value below, and only those,
 * start a new record: mvf_bn_train_stats, mvf_bn_train_finalize, mvf_bn_apply[_bits], mvf_bn_apply_colmeans, mvf_bn_bwd_reduce, mvf_bn_bwd_finalize,
 * mvf_bn_bwd_apply[_masked], mvf_bn_bwd_pair, mvf_bn_bwd_pair_wgrad and the four mvf_maxpool_bn_relu_* calls.  A call refused before its first launch leaves
 * `entry` = that entry point, launches = 0, vn = 0 and both forms NONE; a launch the runtime refuses (MVF_EHIP) is not counted.  Every other call leaves the
 * record alone: the plan queries (mvf_bn_workspace_bytes, mvf_maxpool_bwd_sums_rows, mvf_bn_bwd_wgrad_*) and the entry points whose kernels live in other
 * files (mvf_bn_train_stats_gram, mvf_bn_bwd_apply_wgrad, mvf_conv1x1_bwd_fused, mvf_conv1x1_bnbwd_sums_pair).  mvf_bn_bwd_pair_wgrad records its sums
 * (reduce + finalize: launches = 2, the reduce kernel's plan); the fused apply + weight-gradient launch of csrc/bnbwd_wgrad.hip is not part of the record. */
enum {
    MVF_BN_ENTRY_NONE = 0,
    MVF_BN_ENTRY_TRAIN_STATS = 1, MVF_BN_ENTRY_TRAIN_FINALIZE = 2,
    MVF_BN_ENTRY_APPLY = 3,               /* mvf_bn_apply / mvf_bn_apply_bits                                                                */
    MVF_BN_ENTRY_APPLY_COLMEANS = 4,
    MVF_BN_ENTRY_BWD_REDUCE = 5, MVF_BN_ENTRY_BWD_FINALIZE = 6,
    MVF_BN_ENTRY_BWD_APPLY = 7,           /* mvf_bn_bwd_apply / mvf_bn_bwd_apply_masked                                                      */
    MVF_BN_ENTRY_BWD_PAIR = 8, MVF_BN_ENTRY_BWD_PAIR_WGRAD = 9,
    MVF_BN_ENTRY_POOL_FWD = 10, MVF_BN_ENTRY_POOL_BWD = 11, MVF_BN_ENTRY_POOL_BWD_SUMS = 12, MVF_BN_ENTRY_POOL_BWD_APPLY = 13
};
enum {
    MVF_BN_FIN_NONE = 0,
    MVF_BN_FIN_ROW_MAJOR = 1,             /* partials [rows][c][2]: a workgroup per 4 channels (the library's own column kernels)            */
    MVF_BN_FIN_CM_WORKGROUP = 2,          /* channel-major partials [c][rows][2], rows >= 1024: a workgroup per channel                      */
    MVF_BN_FIN_CM_WAVE = 3                /* channel-major, fewer rows: a wave per channel, 4 channels per workgroup                         */
};
enum {
    MVF_POOL_FORM_NONE = 0,
    MVF_POOL_FORM_ELEMENT = 1,            /* forward / backward: a thread per (pixel, 4 channels)                                            */
    MVF_POOL_FORM_ROWS = 2,               /* backward: a workgroup per input row (w * c / 4 >= 256)                                          */
    MVF_POOL_FORM_BLOCK = 3,              /* forward (h, w % 4 == 0), backward sums / apply (even h, w; policy pool_*_block): 2 x 2 blocks   */
    MVF_POOL_FORM_ROWS_SUMS = 4,          /* mvf_maxpool_bn_relu_bwd_sums: 8 input rows per workgroup + the BatchNorm sums                   */
    MVF_POOL_FORM_ROWS_APPLY = 5          /* mvf_maxpool_bn_relu_bwd_apply: the same walk, re-gathering ga                                   */
};
typedef struct {
    int32_t entry;                        /* MVF_BN_ENTRY_*                                                                                  */
    int32_t dtype;                        /* MVF_F32 | MVF_BF16 (the two finalize entry points: MVF_F32)                                     */
    int32_t vn;                           /* elements per lane of the LAST column-plan kernel of the call: 4 (fp32, or bf16 in 8-byte        */
                                          /* lanes) | 8 (bf16 in 16-byte lanes); 0: none ran (finalize and pool entry points, refusals)      */
    int32_t cqb, rows, gx, gy;            /* that kernel's column plan: channel groups and rows per workgroup, grid                          */
    int32_t mask_mode;                    /* the backward entry points: 0 - 4 (pair: 4; pool sums / apply: 2); else -1                       */
    int32_t specialised;                  /* 1: the kernel instantiated for that mask mode ran (policy bn_spec); 0: the run-time select      */
    int32_t finalize;                     /* MVF_BN_FIN_*                                                                                    */
    int32_t part_rows;                    /* partial rows per channel the finalize summed, or the pool sums kernel wrote; else 0             */
    int32_t pool;                         /* MVF_POOL_FORM_*                                                                                 */
    int32_t launches;                     /* kernel launches the call made                                                                   */
} mvf_bn_launch_info_t;
int mvf_bn_last_launch(mvf_bn_launch_info_t* out);
/* The train head (csrc/head.hip).  The four fused forward forms -- mvf_head_train_fwd, _soft, _bce, _focal -- make the same two score launches (pooled and
 * scores hold the same bits in every form) and share one argument check, made before any launch (a refused call enqueues nothing and touches no output), in
 * this order: clips, t, hw, c, classes >= 1 (MVF_EINVAL); dtype MVF_F32 or MVF_BF16 (MVF_EINVAL); c * 4 bytes <= 160 KiB, the LDS feature buffer
 * (MVF_EUNSUPPORTED); clips * t <= 65535, a grid dimension (MVF_ESHAPE); feat, fc_w, pooled, dscores non-NULL (MVF_EINVAL).  Then the form's own loss check:
 * labels / targets, scores, loss_part, loss non-NULL (MVF_EINVAL), for _bce and _focal the checks of mvf_bce_loss / mvf_focal_loss.  mvf_head_train_bwd checks,
 * before any launch: its pointers (MVF_EINVAL), c % 4 (MVF_ESHAPE), dtype (MVF_EINVAL), clips * t, clips and (classes + 3) / 4 <= 65535 (MVF_ESHAPE).
 * (mvf_head_train_fwd used to take any dtype != 0 as bf16, test the LDS limit after its first launch and leave the grid to the runtime, and mvf_head_train_bwd
 * tested neither dtype nor grids: those calls, which ended in MVF_EHIP or in undefined results, are now refused as the other three forms always refused them.)
 *
 * head: avg-pool per frame -> new_fc -> mean over the clip's t frames -> cross-entropy (mean over clips).
 * pooled (clips*t, c), scores (clips, classes), dscores = dloss/dscores, loss_part (clips), loss (1): all fp32. */
int mvf_head_train_fwd(const void* feat, int clips, int t, int hw, int c, const float* fc_w, const float* fc_b, int classes,
                       const long long* labels, const float* drop_mask /* (clips*t, c) pre-scaled keep mask or NULL */,
                       float* pooled, float* scores, float* dscores, float* loss_part, float* loss, int dtype, void* stream);
/* BaseHead.loss (codes/models/heads/base.py:40-45): loss[0] = mean over clips of softmax cross-entropy(scores[clip], labels[clip]);
 * loss_part (clips) = the per-clip terms; dscores (clips, classes) = dloss/dscores or NULL.  All fp32. */
int mvf_ce_loss(const float* scores, const long long* labels, int clips, int classes, float* dscores, float* loss_part, float* loss,
                void* stream);
int mvf_head_train_bwd(const float* dscores, const float* pooled, const float* fc_w, const float* drop_mask, int clips, int t,
                       int hw, int c, int classes, float* dfc_w, float* dfc_b, float* dpool_ws /* clips*c */, void* dfeat, int dtype,
                       void* stream);
/* Batch blending (mmaction's MixupBlending / CutmixBlending) and soft labels.  One table per step, two DEVICE arrays:
 *   rows int32 (clips, 5): partner, y0, x0, y1, x1 -- a half-open box in image pixels (before the pad); 0 <= y0 <= y1 <= H, 0 <= x0 <= x1 <= W,
 *                          0 <= partner < clips
 *   wts  fp32  (clips, 2): lam_px = weight of the clip's own pixel outside the box, lam_lab = weight of the clip's own label, both in [0, 1]
 * Mixup: empty box, lam_px = lam_lab = lambda.  CutMix: lam_px = 1, a box, lam_lab = 1 - box_area / (H * W).
 *
 * mvf_stem_blend: xp / out = the stem operand (clips * t, hp, wp, 4) in `dtype` as mvf_stem_prep lays it out.  For clip i, each frame f and each element, with
 * a = xp[i, f], b = xp[partner, f]: inside the box (shifted by pad) out = b, a copy; elsewhere out = a, a copy, when lam_px == 1 or partner == i, otherwise
 * lam_px * a + (1 - lam_px) * b in fp32 rounded once to `dtype`.  The zero border and fourth channel stay zero.  OUT OF PLACE: out == xp or overlapping
 * ranges are MVF_EINVAL (clip i reads clip partner).  xp / out 16-byte aligned.  The kernel clamps partner, the box and lam_px into range: a bad table
 * cannot read outside the tensor (rejecting bad tables is the caller's job: mvfnet_amd.blending.check_blend_rows). */
int mvf_stem_blend(const void* xp, int clips, int t, int hp, int wp, int pad, const int* rows, const float* wts, void* out, int dtype, void* stream);
/* targets[i][k] = (1 - eps) * (lam_lab_i * [k == labels[i]] + (1 - lam_lab_i) * [k == labels[partner_i]]) + eps / classes, fp32 (clips, classes); eps in
 * [0, 1) = label smoothing.  eps == 0: the two entries are exactly lam_lab and 1.0f - lam_lab (their fp32 sum where both labels coincide).
 * rows == NULL: smoothing only (lam_lab = 1). */
int mvf_soft_targets(const long long* labels, const int* rows, const float* wts, int clips, int classes, float eps, float* targets, void* stream);
/* mvf_ce_loss against soft targets (clips, classes), any non-negative fp32 matrix (not assumed to sum to 1): loss_part[i] = sum_k t_ik * (lse_i - s_ik) --
 * exactly 0 for one class --, loss = their mean, dscores = (softmax_ik * sum_k t_ik - t_ik) / clips or NULL. */
int mvf_ce_loss_soft(const float* scores, const float* targets, int clips, int classes, float* dscores, float* loss_part, float* loss, void* stream);
/* mvf_head_train_fwd with soft targets (clips, classes) in place of the integer labels: the same pool and fc launches, then the loss of mvf_ce_loss_soft. */
int mvf_head_train_fwd_soft(const void* feat, int clips, int t, int hw, int c, const float* fc_w, const float* fc_b, int classes,
                            const float* targets, const float* drop_mask /* (clips*t, c) pre-scaled keep mask or NULL */,
                            float* pooled, float* scores, float* dscores, float* loss_part, float* loss, int dtype, void* stream);
/* Binary cross-entropy with logits (csrc/bce.hip): the sigmoid head of multi-label recognition and of BCE training against Mixup / CutMix targets.
 * scores, targets (clips, classes) fp32; pos_weight (classes) fp32 or NULL (= all ones); target_threshold NaN = off.  Per element, with s the score,
 * t the target and w = pos_weight[k]:
 *   t   <- (t > target_threshold) ? 1 : 0                          -- only with the threshold on (timm's bce_target_thresh)
 *   lw   = 1 + (w - 1) * t
 *   l    = (1 - t) * s + lw * (max(-s, 0) + log1p(exp(-|s|)))
 *   dl/ds = (1 - t) - lw * sigmoid(-s),   sigmoid(-s) = e / (1 + e) for s >= 0 and 1 / (1 + e) for s < 0, e = exp(-|s|) <= 1
 * i.e. torch.nn.functional.binary_cross_entropy_with_logits(s, t, pos_weight=w) and its gradient.  With D = classes (sum_classes = 0, torch's 'mean',
 * mmaction2's BCELossWithLogits) or D = 1 (sum_classes = 1, timm's option):
 *   loss_part[i]  = sum_k l_ik / D
 *   loss[0]       = the mean of loss_part, clips in ascending order
 *   dscores[i][k] = (dl/ds)_ik / (clips * D), or dscores == NULL: the same loss_part and loss bits, no gradient
 * -- the contract of mvf_ce_loss_soft, which mvf_head_train_bwd and mvf_distill_loss build on.
 * Precision: all per-row arithmetic runs in fp64 from widened fp32 inputs (exp / log1p in double), sums have a fixed order (wavefront shuffle tree, wave
 * partials in wave order, clips ascending) and every output is rounded to fp32 once.  No atomics, no workspace: bit-identical from run to run.  Any
 * classes >= 1.  target_threshold travels as float (a launch plan's call record carries no double).
 * MVF_EINVAL, checked before any launch (nothing is enqueued, no output is touched): a NULL scores / targets / loss_part / loss; clips < 1 or classes < 1;
 * an infinite target_threshold; sum_classes outside {0, 1}.
 * A NaN score or a non-finite pos_weight entry makes that clip's loss_part and loss[0] NaN (a NaN score's dscores element too): the non-finite step guard
 * then skips the step. */
int mvf_bce_loss(const float* scores, const float* targets, int clips, int classes, const float* pos_weight /* (classes) or NULL */,
                 float target_threshold /* NaN = off */, int sum_classes, float* dscores /* or NULL */, float* loss_part, float* loss, void* stream);
/* mvf_head_train_fwd_soft with the loss of mvf_bce_loss in place of the soft-target cross-entropy: the same pool and fc launches (pooled and scores hold
 * the same bits), then the two loss launches.  dscores is required. */
int mvf_head_train_fwd_bce(const void* feat, int clips, int t, int hw, int c, const float* fc_w, const float* fc_b, int classes,
                           const float* targets, const float* drop_mask /* (clips*t, c) pre-scaled keep mask or NULL */,
                           const float* pos_weight /* (classes) or NULL */, float target_threshold /* NaN = off */, int sum_classes,
                           float* pooled, float* scores, float* dscores, float* loss_part, float* loss, int dtype, void* stream);
/* Focal / asymmetric sigmoid losses (csrc/focal.hip) for long-tailed multi-label data: one element function covers the sigmoid focal loss (Lin et al.;
 * torchvision's sigmoid_focal_loss), its class-balanced form (a per-class weight) and the asymmetric loss of Ridnik et al.  scores, targets (clips, classes)
 * fp32; class_weight (classes) fp32 or NULL (= all ones).  Settings, in a host struct read at the call (a launch plan's call record carries at most four
 * floats): gamma_pos, gamma_neg the focusing exponents g+ / g-, margin m the probability shift of the negatives, alpha the balance (alpha < 0 = off:
 * a+ = a- = 1; else a+ = alpha, a- = 1 - alpha), target_threshold (NaN = off), sum_classes.  Per element, with s the score, t the target, c = class_weight[k],
 * e = exp(-|s|), p = sigmoid(s) and pn = sigmoid(-s) both formed from e (e / (1 + e) or 1 / (1 + e) by the sign of s), never as 1 - p:
 *   t    <- (t > target_threshold) ? 1 : 0                                  -- only with the threshold on, as in mvf_bce_loss
 *   logp  = -(max(-s, 0) + log1p(e))                                        -- log sigmoid(s)
 *   L+    = -(pn^g+) * logp                                                 -- pn^0 := 1
 *   pm    = (p > m) ? p - m : 0                                             -- the shifted negative probability; m = 0: pm = p
 *   log1m = (p > m) ? log(pn + m) : 0                                       -- log(1 - pm); with m = 0 it is -(max(s, 0) + log1p(e))
 *   L-    = -(pm^g-) * log1m                                                -- pm^0 := 1
 *   l     = c * (a+ * t * L+ + a- * (1 - t) * L-)
 *   dL+/ds = pn^g+ * (g+ * p * logp - pn)
 *   dpm/ds = (p > m) ? p * pn : 0
 *   dL-/ds = -(g- * pm^(g- - 1) * dpm/ds) * log1m + pm^g- * (dpm/ds) / (pn + m)       -- the first term is absent for g- = 0
 *   dl/ds  = c * (a+ * t * dL+/ds + a- * (1 - t) * dL-/ds)
 * With m = 0 the closed forms stand in: log1m as above and (dpm/ds) / pn = p (pn is zero in fp64 beyond s = 745).
 * The loss is LINEAR IN THE TARGET, as binary cross-entropy is: for a soft (Mixup / CutMix, smoothed) target it is the expectation of the hard-label loss.
 * This differs from the formulas as published for soft targets only: the asymmetric paper's code mixes the exponents, (1 - p_t)^(g+ t + g- (1 - t)), and
 * torchvision mixes p_t = p t + (1 - p)(1 - t); the mixed exponent has an infinite derivative where it falls below 1, the linear form has none.  For hard
 * targets it is torchvision's sigmoid_focal_loss (g+ = g- = gamma, m = 0, alpha) and the paper's asymmetric loss (g+ = 1, g- = 4, m = 0.05) wherever that
 * implementation's clamp(min=1e-8) is inactive; with g+ = g- = 0, m = 0, alpha off it is mvf_bce_loss without pos_weight.  No epsilon clamp: logp and log1m
 * are finite for every finite s.  (Parity with timm's AsymmetricLossMultiLabel and mmaction2's CBFocalLoss is claimed from the papers' formulas, not from
 * those sources.)
 * Reduction, precision and determinism are those of mvf_bce_loss: with D = classes (sum_classes = 0) or D = 1 (sum_classes = 1)
 *   loss_part[i]  = sum_k l_ik / D
 *   loss[0]       = the mean of loss_part, clips in ascending order
 *   dscores[i][k] = (dl/ds)_ik / (clips * D), or dscores == NULL: the same loss_part and loss bits, no gradient
 * all per-row arithmetic in fp64 from widened fp32 inputs (pow, exp, log, log1p in double), sums in a fixed order (wavefront shuffle tree, wave partials in
 * wave order, clips ascending), every output rounded to fp32 once.  No atomics, no workspace: bit-identical from run to run.  Any classes >= 1.
 * MVF_EINVAL, checked before any launch (nothing is enqueued, no output is touched): a NULL scores / targets / prm / loss_part / loss; clips < 1 or
 * classes < 1; a gamma that is neither 0 nor in [1, 16]; margin outside [0, 1); alpha NaN or > 1; an infinite target_threshold; sum_classes outside {0, 1}.
 * A NaN score or a non-finite class_weight entry makes that clip's loss_part and loss[0] NaN (a NaN score's dscores element too): the non-finite step guard
 * then skips the step. */
typedef struct mvf_focal_params {
    float gamma_pos, gamma_neg, margin, alpha, target_threshold;
    int sum_classes, reserved[2];
} mvf_focal_params_t;
int mvf_focal_loss(const float* scores, const float* targets, int clips, int classes, const float* class_weight /* (classes) or NULL */,
                   const mvf_focal_params_t* prm, float* dscores /* or NULL */, float* loss_part, float* loss, void* stream);
/* mvf_head_train_fwd_bce with the loss of mvf_focal_loss in place of the binary cross-entropy: the same pool and fc launches (pooled and scores hold the
 * same bits), then the two loss launches.  dscores is required. */
int mvf_head_train_fwd_focal(const void* feat, int clips, int t, int hw, int c, const float* fc_w, const float* fc_b, int classes,
                             const float* targets, const float* drop_mask /* (clips*t, c) pre-scaled keep mask or NULL */,
                             const float* class_weight /* (classes) or NULL */, const mvf_focal_params_t* prm,
                             float* pooled, float* scores, float* dscores, float* loss_part, float* loss, int dtype, void* stream);
/* Knowledge distillation (Hinton's loss) behind mvf_head_train_fwd / mvf_head_train_fwd_soft, which left the cross-entropy's dscores (clips, classes),
 * loss_part (clips) and loss (1) in device memory; scores = the student's (clips, classes), teacher_scores = the teacher's, all fp32.  Per clip i, with
 * s = scores[i], z = teacher_scores[i], T = temperature, a = alpha, p = softmax(z / T), q = softmax(s / T):
 *   kd_i          = sum_k p_k * ((z_k / T - s_k / T) - (lse(z / T) - lse(s / T)))        -- KL(p || q); exactly 0 when z and s hold the same bits, and for
 *                                                                                           one class
 *   loss_part[i] <- (1 - a) * loss_part[i] + a * T * T * kd_i
 *   dscores[i][k] <- (1 - a) * dscores[i][k] + a * T * (q_k - p_k) / clips
 *   loss[0]      <- the mean of the new loss_part, clips in a fixed order
 *   terms[0]      = the mean of the INCOMING loss_part (the cross-entropy term), terms[1] = the mean of T * T * kd_i; terms may be NULL, the other outputs
 *                   are then the same bits
 * i.e. (1 - a) * CE + a * T^2 * kl_div(log_softmax(s / T), softmax(z / T), 'batchmean') and its gradient with respect to the scores.
 * Precision: all per-row arithmetic runs in fp64 -- inputs are widened, exp / log are taken in double, 1 - a is formed in double from the fp32 a, sums have
 * a fixed order (wavefront shuffle tree, wave partials in wave order, clips ascending) -- and every output is rounded to fp32 once.  No atomics, no
 * workspace: bit-identical from run to run.  temperature and alpha travel as float (a launch plan's call record carries no double).
 * MVF_EINVAL, checked before any launch (nothing is enqueued, no output is touched): a NULL scores / teacher_scores / dscores / loss_part / loss; clips < 1 or
 * classes < 1; temperature not finite or <= 0; alpha not finite or outside (0, 1].
 * A NaN or inf in a row of teacher_scores (or scores) makes that row's loss_part and dscores, loss[0] and terms[1] NaN: the non-finite step guard then
 * skips the step.  scores / teacher_scores must not overlap the outputs. */
int mvf_distill_loss(const float* scores, const float* teacher_scores, int clips, int classes, float temperature, float alpha,
                     float* dscores /* in/out */, float* loss_part /* in/out */, float* loss /* out */, float* terms /* out, 2 floats, or NULL */,
                     void* stream);
/* Temporal-relation head (csrc/trn_head.hip): TSNClsHead with consensus 'TRN' / 'TRNmultiscale' (Zhou et al., "Temporal Relational Reasoning in Videos";
 * the reference's segmental_consensuses/relation_consensus.py).  feat (clips * t, hw, c) in `dtype`; everything else fp32.  2 <= t <= MVF_TRN_MAX_FRAMES.
 * Scale index i (0 <= i < n_scales <= t - 1) is the s_i = t - i frame relation; its operands, one mvf_trn_scale_t of a HOST array read at the call:
 *   w1 (hidden, s_i * fdim), b1 (hidden), w2 (classes, hidden), b2 (classes) and, for the backward, the gradient destinations dw1, db1, dw2, db2.
 * 'TRN' is n_scales = 1 (hidden 512 in the reference), 'TRNmultiscale' n_scales = t - 1 (hidden 256); fdim is new_fc's output width (256).
 * table: int32 (rows, 1 + t) in DEVICE memory, one relation per row: scale_index, then the s_i frame indices of the relation, then -1 padding.  The kernels
 * clamp scale_index into [0, n_scales) and every frame index into [0, t): a bad table cannot read outside a tensor (refusing bad tables is the caller's job:
 * mvfnet_amd.heads.relation.check_relation_table).
 * mvf_trn_head_fwd, 5 launches whatever `rows` is (the hidden GEMM runs as up to MVF_TRN_KSPLIT_MAX K splits into hpart and a reduce over them in ascending order):
 *   pooled[n][ch]   = (mean over hw of feat[n][.][ch]) * drop_mask[n][ch]              (clips * t, c); drop_mask the pre-scaled keep mask or NULL
 *   f[n][d]         = fc_w[d] . pooled[n] + fc_b[d]                                    (clips * t, fdim); fc_b may be NULL
 *   h[r][i][j]      = relu(w1_s[j] . relu(concat_{p < s} f[i * t + frame_r(p)]) + b1_s[j])   (rows, clips, hidden), s the scale of row r
 *   scores[i][k]    = sum over r = 0 .. rows - 1, in that order, of (w2_s[k] . h[r][i] + b2_s[k])   (clips, classes): b2_s counts once per row
 * mvf_trn_head_bwd, 7 launches whatever `rows` is, from dscores (clips, classes) and the forward's pooled, f, h:
 *   dw2_s[k][j]     = sum over the rows of scale s in table order, clips ascending, of dscores[i][k] * h[r][i][j];   db2_s[k] the same sum of dscores[i][k]
 *   dh[r][i][j]     = [h[r][i][j] > 0] * sum_k dscores[i][k] * w2_s[k][j]
 *   dw1_s[j][q]     = the same row / clip sum of dh[r][i][j] * relu(f[i * t + frame_r(q / fdim)][q % fdim]);           db1_s[j] the same sum of dh[r][i][j]
 *   df[n][d]        = [f[n][d] > 0] * sum over the rows that hold frame n % t, in table order (a gather, no scatter), of sum_j dh[r][i][j] * w1_s[j][p * fdim + d]
 *   dfc_w[d][ch]    = sum over the frames ascending of df[n][d] * pooled[n][ch];   dfc_b[d] the same sum of df[n][d]
 *   dpool[n][ch]    = (sum_d df[n][d] * fc_w[d][ch]) / hw * drop_mask[n][ch]       (clips * t, c) workspace
 *   dfeat[n][.][ch] = dpool[n][ch], rounded once to `dtype`
 * A scale without a row in the table gets zero gradients.  Every sum is taken in fp32 in a fixed order: one accumulator per output element, or a fixed number of
 * partial sums (the K splits of the hidden GEMM; 8 interleaved accumulators and four quarters of the reduction in dh, df, dfc_w, dpool) combined in a fixed tree,
 * rows in table order.  No atomics, no counters: bit-identical from run to run.  Any clips >= 1, classes >= 1, hw >= 1; c a multiple of 4 (as mvf_head_train_bwd).
 * Checked before any launch: MVF_EINVAL (a NULL argument, a size < 1, a dtype, n_scales outside [1, t - 1], a NULL operand of a scale), MVF_EUNSUPPORTED (t outside
 * [2, MVF_TRN_MAX_FRAMES]), MVF_ESHAPE (c % 4, clips * t > 65535, classes / hidden / fdim > 65535, rows > 1024, dpool not 16-byte aligned, dfeat not 16-byte (fp32) / 8-byte (bf16) aligned).
 * hpart: a workspace of MVF_TRN_KSPLIT_MAX * rows * clips * hidden floats.
 * mvf_trn_head_last_launch: the calling thread's last call of the two (a host-side record): a refused call leaves launches = 0. */
#define MVF_TRN_MAX_FRAMES 16
#define MVF_TRN_KSPLIT_MAX 8
typedef struct mvf_trn_scale {
    const float *w1, *b1, *w2, *b2;
    float *dw1, *db1, *dw2, *db2;
} mvf_trn_scale_t;
enum { MVF_TRN_ENTRY_NONE = 0, MVF_TRN_ENTRY_FWD = 1, MVF_TRN_ENTRY_BWD = 2 };
typedef struct mvf_trn_launch_info {
    int32_t entry;                        /* MVF_TRN_ENTRY_*                                                                                  */
    int32_t dtype;
    int32_t rows, n_scales;               /* 0 after a refused call                                                                           */
    int32_t launches;                     /* kernel launches the call made: 5 (forward) / 7 (backward)                                        */
} mvf_trn_launch_info_t;
int mvf_trn_head_fwd(const void* feat, int clips, int t, int hw, int c, const float* fc_w, const float* fc_b, int fdim, const mvf_trn_scale_t* scales,
                     int n_scales, int hidden, int classes, const int* table, int rows, const float* drop_mask /* (clips*t, c) or NULL */, float* pooled,
                     float* f, float* h, float* hpart /* workspace */, float* scores, int dtype, void* stream);
int mvf_trn_head_bwd(const float* dscores, const float* pooled, const float* f, const float* h, const float* fc_w, const mvf_trn_scale_t* scales, int n_scales,
                     int hidden, int classes, const int* table, int rows, const float* drop_mask /* (clips*t, c) or NULL */, int clips, int t, int hw, int c,
                     int fdim, float* dfc_w, float* dfc_b, float* dh /* (rows, clips, hidden) */, float* df /* (clips*t, fdim) */, float* dpool /* (clips*t, c) */,
                     void* dfeat, int dtype, void* stream);
int mvf_trn_head_last_launch(mvf_trn_launch_info_t* out);
/* RandomErasing (timm's, as PySlowFast and mmaction2 use it) on the stem operand, IN PLACE.  xp = (planes, hp, wp, 4) in `dtype` as mvf_stem_prep lays it
 * out, 16-byte aligned; no plane reads another plane.  One table per step, three DEVICE arrays:
 *   boxes int32  (planes, max_boxes, 5): y0, x0, y1, x1, mode -- a half-open box in image pixels (before the pad), 0 <= y0 <= y1 <= H, 0 <= x0 <= x1 <= W;
 *                                        mode 0 = unused slot, 1 = constant colour, 2 = per-element noise, any other value = unused.  1 <= max_boxes <= 8;
 *                                        where boxes of one plane overlap, the box with the higher index wins.
 *   fill  fp32   (planes, max_boxes, 4): mode 1: the colour of channels 0..2 in normalised space, rounded once to `dtype`; word 3 is ignored
 *   key   uint32 (2):                    the step's generator key (in device memory: a replayed launch plan gets fresh noise from the same address)
 * Noise (mode 2), the specification: for image pixel (y, x) of plane p
 *   (w0, w1, w2, w3) = Philox4x32-10(counter = (x, y, p, 0), key = (key[0], key[1]))       (Salmon et al., SC'11; multiply-high in plain integer arithmetic)
 *   u1 = ((w0 >> 8) + 1) * 2^-24,  u2 = (w1 >> 8) * 2^-24,  u3 = ((w2 >> 8) + 1) * 2^-24,  u4 = (w3 >> 8) * 2^-24
 *   channel 0 = sqrt(-2 ln u1) * cos(2 pi u2),  channel 1 = sqrt(-2 ln u1) * sin(2 pi u2),  channel 2 = sqrt(-2 ln u3) * cos(2 pi u4)
 * N(0, 1) values with |n| <= sqrt(48 ln 2) < 5.77, each computed in fp32 with the accurate math functions (no fast intrinsics, no fast-math) and rounded once
 * to `dtype`.  The counter holds image coordinates, never the storage layout: fp32 and bf16 operands see the same noise before the final rounding, and it
 * depends neither on the box index nor on how the grid is cut.
 * The border of `pad` pixels and the padding columns up to wp are never written; the fourth channel of an erased pixel is stored as the zero it already is;
 * every element outside all boxes keeps its bits.  No atomics: bit-identical from run to run for the same table and key.  The kernel clamps every box to
 * the operand's interior, (hp - 2 pad) x (wp - 2 pad), as mvf_stem_blend does: a bad table cannot address outside the tensor (rejecting bad tables is the caller's job: mvfnet_amd.erasing.check_erase_table).
 * MVF_EINVAL: NULL pointer, dtype, max_boxes outside [1, 8], 2 * pad > hp or wp, misalignment; MVF_ESHAPE: a bf16 plane that is not a whole number of
 * 16-byte units, a plane beyond int -- all before any launch. */
int mvf_stem_erase(void* xp, int planes, int hp, int wp, int pad, const int* boxes, int max_boxes, const float* fill, const unsigned int* key, int dtype,
                   void* stream);
/* RandAugment (timm's `rand-m7-n4-mstd0.5-inc1` of the fine-tuning recipes) on the uploaded uint8 frames, IN FRONT of the frame kernels: RandAugment is
 * defined on 8-bit images (bit masks, histograms, truncating blends), so it runs on the bytes and not on the normalised stem operand.
 *   frames_hwc (n, hs, ws, 3) uint8, the dense packed batch of mvf_frames_prep_u8; n % t == 0, frames [c t, (c + 1) t) are clip c and share its ops.
 *   order      the stored channel order, 0 = BGR, 1 = RGB (as mvf_frames_yuv420_gather_resample_u8): only the grey weights depend on it.
 *   sizes      DEVICE int32 (n, 2) rows (hs_i, ws_i), or NULL = (hs, ws).  Every op works on the frame's own hs_i x ws_i image (its centre, its width, its
 *              histogram); bytes of the hs x ws extent outside that image are copied unchanged.  The kernel clamps hs_i / ws_i to [0, hs] / [0, ws].
 *   table      DEVICE int32 (n / t, layers, 16), 1 <= layers <= 8.  Word 0 = kind; words 1..12 = the op's arguments; word 13 = the fill colour of kind 11,
 *              three bytes in STORED order (byte c = bits 8 c .. 8 c + 7); words 14..15 = 0.  Contents are not checked here (mvfnet_amd.randaug.check_randaug_table).
 *   out, tmp   two buffers of n * hs * ws * 3 bytes; the layers ping-pong between them and the result is ALWAYS in out; frames_hwc is never written.
 *   stats_layers  bit k set = layer k gets its statistics pass (some clip's kind there is 5, 6 or 8).  With the bit clear such an op still touches only the
 *              workspace and its frame; its pixels are then unspecified.
 *   workspace  at least n * MVF_RANDAUG_WS_PER_FRAME bytes, MVF_RANDAUG_WS_PER_FRAME = 3 * 256 + 16: per frame the three 256-byte lookup tables of kinds 5 / 6
 *              and one int32 (the grey mean of kind 8) in the 16 bytes behind them.
 * At most two launches per layer: the statistics pass (only where the bit is set; one workgroup per frame, LDS histograms and integer sums only, so the
 * result does not depend on the order of the adds; a frame whose op needs no statistics loads nothing) and the apply pass (a workgroup works on ONE frame, the
 * op is a uniform branch; a thread owns an aligned dword of the batch, so loads of the pointwise ops and all stores are dword wide although neither
 * ws_i * 3 nor a frame's base is a multiple of 4; only a dword shared with the neighbouring frame is stored by bytes).  No float atomics; bit-identical
 * from run to run.
 * Kinds and their arithmetic (p = a byte of the image, per channel unless stated; this is the specification, and what was compared with Pillow):
 *    0 identity      p
 *    1 invert        255 - p
 *    2 posterize     p & w1                           (the host gives w1 = ~(2^(8 - bits) - 1) & 255; bits = 0 -> 0, a black frame)
 *    3 solarize      p < w1 ? p : 255 - p             (w1 = thresh in 0 .. 256)
 *    4 solarize-add  p < w1 ? min(255, p + w2) : p
 *    5 autocontrast  per channel lo / hi = min / max of the frame; hi <= lo: identity; else in fp64 without FMA scale = 255.0 / (hi - lo), off = -lo * scale,
 *                    lut[i] = clamp((int)(i * scale + off), 0, 255)
 *    6 equalize      per channel, h = the histogram: at most one non-empty bin: identity; step = (sum(h) - last non-empty bin) / 255 (integer); step == 0:
 *                    identity; else acc = step / 2 and for i = 0 .. 255: lut[i] = min(255, acc / step), acc += h[i]
 *    7 brightness    blend(0, f, p)                   (f = the fp32 whose bits are w1, kinds 7 .. 10)
 *    8 contrast      blend(m, f, p), m = (2 S + N) / (2 N) in integers, S = the sum of the frame's grey image, N = hs_i * ws_i
 *    9 color         blend(grey, f, p), grey = (R * 19595 + G * 38470 + B * 7471 + 0x8000) >> 16 of the pixel
 *   10 sharpness     blend(s, f, p); interior pixels: s = (2 acc + 13) / 26 in integers, acc = the 3 x 3 sum with centre weight 5; the one-pixel border has
 *                    s = p; frames with hs_i < 3 or ws_i < 3 are copied whole
 *   11 affine        the inverse map with six fp64 coefficients a .. f (words 1..12, low word first), see below
 * blend(d, f, p), fp32 with every operation rounded on its own: v = d + f * (p - d); 0 <= f <= 1: (uint8)v, truncated; else v clamped to [0, 255], then truncated.
 * Affine, output pixel (x, y), fp64 without FMA contraction: xin = (a * (x + .5) + b * (y + .5)) + c, yin likewise with d, e, f.  Unless 0 <= xin < ws_i and
 * 0 <= yin < hs_i the pixel takes the fill colour.  Otherwise .5 is subtracted from both, x0 = floor(xin), dx = xin - x0, the taps are x0 and x0 + 1 clamped to
 * the frame, the rows y0 (clamped) and y0 + 1 -- the first row again when y0 + 1 is outside the frame --, each lerp is p + (q - p) * d, and the result is
 * truncated to uint8.  Pillow steps the source coordinate incrementally along a row; this direct evaluation equals it bit for bit on the fixtures of
 * tests/golden/randaug_cases.npz -- measured there, not guaranteed for every matrix.
 * Not built: bicubic interpolation, YUV / addressed input, AutoAugment / AugMix policies.
 * MVF_EINVAL (before any launch, nothing enqueued): a NULL pointer (sizes may be NULL), n / hs / ws / t < 1, n % t != 0, order not 0 / 1, layers outside [1, 8],
 * bits of stats_layers at or above `layers`, out == tmp or either == frames_hwc, a buffer or table that is not 4-byte aligned, a workspace smaller than the
 * formula above; MVF_ESHAPE: a frame of 2^31 bytes or more, a batch of more than 2^31 workgroups. */
#define MVF_RANDAUG_WS_PER_FRAME (3 * 256 + 16)
int mvf_frames_randaug_u8(const unsigned char* frames_hwc, int n, int hs, int ws, int t, int order, const int* sizes, const int* table, int layers,
                          unsigned stats_layers, unsigned char* out, unsigned char* tmp, void* workspace, long long workspace_bytes, void* stream);
/* conv weight gradient dw_oihw (cout, cin_real, kh, kw_real) fp32; d describes the FORWARD conv (x dims, ho/wo = dz dims).
 * kw_packed*cin_packed == d->kw*d->cin; they differ from (kw_real, cin_real) only for the stem view (8x4 vs 7x3).
 * fp32 accumulation over the pixels in a fixed order (per-split partial tiles, then a split-lane reduce): deterministic, no atomics.  fp32
 * operands are multiplied on the bf16 matrix cores as exact three-term bf16 splits, six partial products per product -- as accurate against
 * an fp64 weight gradient as the exact-fp32 matrix instruction, which MVF_WGRAD_X3=0 (or MVF_F32_X3=0) selects. */
size_t mvf_conv2d_wgrad_workspace_bytes(const mvf_conv_desc_t* d);
int mvf_conv2d_nhwc_wgrad(const mvf_conv_desc_t* d, const void* dz, const void* x, const void* x2, int kw_real,
                          int cin_real, int kw_packed, int cin_packed, float* dw_oihw, void* ws, size_t ws_bytes,
                          void* stream);
/* [r5] the same GEMM with the workgroup count to aim at named by the caller (the library's own plans size weight gradients for a side stream: half the
 * chip); results differ from mvf_conv2d_nhwc_wgrad only by the fp32 summation order of the pixel split.  `wgs` (8 .. 4096) is a count to AIM at: where it
 * asks for more pixel splits than the workspace of mvf_conv2d_wgrad_workspace_bytes holds slabs, the rows per split are raised to the smallest multiple of
 * 64 that fits, so every wgs of the range runs in the published workspace. */
int mvf_conv2d_nhwc_wgrad_wgs(const mvf_conv_desc_t* d, const void* dz, const void* x, const void* x2, int kw_real,
                              int cin_real, int kw_packed, int cin_packed, float* dw_oihw, void* ws, size_t ws_bytes, int wgs, void* stream);
/* Which kernel the calling thread's LAST mvf_conv2d_nhwc_wgrad[_wgs] call launched: the weight gradient's counterpart of mvf_conv2d_last_launch (host-side,
 * thread-local, plain stores next to the launches; no device work).  A call refused before its first launch leaves launches = 0, family =
 * MVF_WGRAD_FAM_NONE.  The two direct kernels report nsplit = their partial-slab count (one per workgroup) and rows_per_split = 0. */
enum {
    MVF_WGRAD_FAM_NONE = 0,
    MVF_WGRAD_FAM_F32_REG = 1,     /* wgrad_kernel<float>, register-staged loaders (exact-fp32 MFMA)                                */
    MVF_WGRAD_FAM_F32_DMA = 2,     /* wgrad_kernel<float, .., DMA>: the same with LDS-DMA loaders                                   */
    MVF_WGRAD_FAM_X3 = 3,          /* wgrad_x3_kernel: fp32 storage on the bf16 matrix cores                                        */
    MVF_WGRAD_FAM_BF16_WIDEN = 4,  /* wgrad_kernel<bf16_t>: bf16 widened to fp32 on the way into LDS (channel counts % 8 != 0)      */
    MVF_WGRAD_FAM_BF16_REG = 5,    /* wgrad_bf16_kernel, register-staged loaders                                                    */
    MVF_WGRAD_FAM_BF16_DMA2 = 6,   /* wgrad_bf16_kernel, two-buffer LDS-DMA                                                         */
    MVF_WGRAD_FAM_BF16_PIPE = 7,   /* wgrad_bf16_pipe_kernel<stages>: `stages` = 3 | 4                                              */
    MVF_WGRAD_FAM_T256_2B = 8,     /* 256 x 256 tile, two-barrier loop (wgrad_bf16_kernel<2, 4, true, 4>)                           */
    MVF_WGRAD_FAM_T256_P4 = 9,     /* 256 x 256 tile, four-phase loop (wgrad_bf16_p4_kernel)                                        */
    MVF_WGRAD_FAM_C3X3_C64 = 10,   /* csrc/wgrad3x3_c64.hip                                                                         */
    MVF_WGRAD_FAM_STEM = 11        /* csrc/wgrad_stem.hip                                                                           */
};
typedef struct {
    int32_t family;                /* MVF_WGRAD_FAM_*                                                                               */
    int32_t stages;                /* LDS ring depth of the main loop (BF16_PIPE: 3 | 4; the other LDS-DMA loops: 2; else 0)        */
    int32_t tile_co, tile_k;       /* output tile of a workgroup (the direct kernels: the whole 64 x K slab)                        */
    int32_t dtype;                 /* MVF_F32 | MVF_BF16                                                                            */
    int32_t nsplit;                /* pixel splits = fp32 partial slabs the reduce sums                                             */
    int32_t rows_per_split;        /* pixels per split                                                                              */
    int32_t xcd_rr;                /* 1: splits round-robin over the XCDs; 0: contiguous balanced ranges of (split, tile) pairs     */
    int32_t split_operand;         /* 1: channels < split_c were read from x2                                                       */
    int32_t gram;                  /* 1: the Gram plan (dz == x, pointwise, cin == cout; policy gram_wgs workgroups)                */
    int32_t wgs_target;            /* the workgroup count the pixel split aimed at (the caller's for _wgs; 0: the direct kernels)    */
    int32_t launches;              /* kernel launches the call made (the GEMM and the slab reduce: 2)                               */
} mvf_wgrad_launch_info_t;
int mvf_conv2d_wgrad_last_launch(mvf_wgrad_launch_info_t* out);
/* Every weight pack of a training step in one launch.  jobs_dev = DEVICE array of njobs records sorted by first_block;
 * job k owns workgroups [first_block, first_block + ceil(elements / 2048)), total_blocks = their sum.  kind 0 = the forward
 * pack of mvf_pack_conv_weight (no scale), kind 1 = the data-gradient pack of mvf_pack_conv_weight_dgrad.  kind 2 / 3 = the
 * same two packs as an LDS-tiled transpose for cout % 32 == 0, cin % 32 == 0, kh * kw <= 9, kw_pad == kw, cin_pad == cin:
 * such a job owns (cout / 32) * (cin / 32) workgroups. */
typedef struct {
    const float* w;      /* fp32 OIHW parameter */
    void* out;           /* packed operand in `dtype` */
    int cout, cin, kh, kw, kw_pad, cin_pad;
    int kind, first_block;
} mvf_pack_job_t;
int mvf_pack_conv_weights_batched(const mvf_pack_job_t* jobs_dev, int njobs, int total_blocks, int dtype, void* stream);

/* data gradient = mvf_conv2d_nhwc_fwd on dz with these weights: packed[ci][kh'][kw'][co] = w[co][ci][KH-1-kh'][KW-1-kw'],
 * pad' = k-1-pad, stride 1, in_dil = forward stride */
int mvf_pack_conv_weight_dgrad(const float* w_oihw, int cout, int cin, int kh, int kw, void* w_packed, int dtype,
                               void* stream);
/* MVF training primitives, channels-last (the engine composes MVF fwd/bwd from these + the BN calls above) */
/* out[..., :cs] = f(stencil(x[..., :cs])) [+ addend[..., :cs] (pitch addend_c; NULL = none), gated per channel by
 * addend_sign_bits ([pixels][addend_c/4] bytes as written by mvf_bn_apply_bits; NULL = ungated)]; flip = transposed stencil.
 * Channels >= cs of a wider `out` are left as they are -- EXCEPT when x and out have the same pitch (x_c == out_c > cs): the call then also copies channels
 * [cs, x_c) of every pixel from x to out (the pass-through channels of the MVF module, a second launch), for every entry point of this family. */
int mvf_nhwc_stencil(const mvf_desc_t* d, const void* x, int x_c, void* out, int out_c, const float* w_t,
                     const float* w_h, const float* w_w, const float* scale, const float* shift, int flip,
                     const void* addend, int addend_c, const unsigned char* addend_sign_bits, void* stream);
/* [r5] ... with the OUTPUT gated per channel by out_gate_bits ([pixels][out_c/4] bytes): out = (f(stencil(x)) + gated addend) * [bit] */
int mvf_nhwc_stencil_gate(const mvf_desc_t* d, const void* x, int x_c, void* out, int out_c, const float* w_t,
                          const float* w_h, const float* w_w, const float* scale, const float* shift, int flip,
                          const void* addend, int addend_c, const unsigned char* addend_sign_bits,
                          const unsigned char* out_gate_bits, void* stream);
/* [r5] mvf_nhwc_stencil_gate + the column sums of the gated slice: sums_part CHANNEL-MAJOR [cs][mvf_nhwc_stencil_stats_rows(d, x_c, out_c)][2] = per-workgroup
 * sums of gm and gm^2 -- the slice's share of mvf_conv2d_nhwc_fwd_resmask_gate_colsums. */
int mvf_nhwc_stencil_gate_colsums(const mvf_desc_t* d, const void* x, int x_c, void* out, int out_c, const float* w_t, const float* w_h,
                                  const float* w_w, int flip, const void* addend, int addend_c, const unsigned char* addend_sign_bits,
                                  const unsigned char* out_gate_bits, float* sums_part, void* stream);
/* [r5] the plain stencil (no activation) that also accumulates the batch statistics of MVF's BatchNorm3d (MVF.py:131-134, training mode) over the
 * values it stores: stats_part CHANNEL-MAJOR [cs][mvf_nhwc_stencil_stats_rows(d, x_c, out_c)][2] = per-workgroup sums of (y - K), (y - K)^2, K =
 * stats_shift (the old running mean; NULL = 0) -> mvf_bn_train_finalize.  Replaces the statistics pass over y. */
int mvf_nhwc_stencil_stats_rows(const mvf_desc_t* d, int x_c, int out_c);
/* [r6] plan query (nothing is launched): 1 = a stencil launch of this shape (16-byte aligned operands) runs on the LDS-tiled bf16 kernel, with
 * rows_per_band x chan_per_wg (both optional) its tile; 0 = the register-chunked kernel (fp32, slices not in 16-channel chunks, one clip of the source
 * larger than a 32-bit buffer descriptor, fewer workgroups than the tile needs). */
int mvf_nhwc_stencil_tile_plan(const mvf_desc_t* d, int x_c, int out_c, int* rows_per_band, int* chan_per_wg);
int mvf_nhwc_stencil_stats(const mvf_desc_t* d, const void* x, int x_c, void* out, int out_c, const float* w_t, const float* w_h,
                           const float* w_w, float* stats_part, const float* stats_shift, void* stream);
size_t mvf_nhwc_tapgrad_workspace_bytes(const mvf_desc_t* d);
int mvf_nhwc_tapgrad(const mvf_desc_t* d, const void* x, int x_c, const void* dy, int dy_c, float* dw_t, float* dw_h,
                     float* dw_w, void* ws, size_t ws_bytes, void* stream);
/* Which kernel the calling thread's LAST mvf_nhwc_stencil* / mvf_nhwc_tapgrad call launched: the MVF primitives' counterpart of
 * mvf_conv2d_wgrad_last_launch (host-side, thread-local, plain stores next to the launches; no device work).  A call refused before its first launch
 * leaves launches = 0 and kernel = NONE; the plan queries (mvf_nhwc_stencil_stats_rows, mvf_nhwc_stencil_tile_plan) leave the record alone. */
enum {
    MVF_STENCIL_KERNEL_NONE = 0,
    MVF_STENCIL_KERNEL_WALK1 = 1,    /* mvf_nhwc_apply<T, 1>: one channel per thread, serial walk over t (cs or a pitch % 4 != 0, misaligned operands) */
    MVF_STENCIL_KERNEL_WALK4 = 2,    /* mvf_nhwc_apply<T, 4>: four channels per thread, serial walk (policy stencil_chunked=0, taps not 16-byte aligned) */
    MVF_STENCIL_KERNEL_CHUNKED = 3,  /* mvf_nhwc_apply_chunked<T, 4 | 8>: all loads of a chunk of frames in flight at once                             */
    MVF_STENCIL_KERNEL_LDS = 4       /* mvf_nhwc_apply_lds<T, CW>: bf16, a (band of rows, CW channels, all frames) tile in LDS                         */
};
enum {
    MVF_STENCIL_FLIP = 1, MVF_STENCIL_HSWISH = 2, MVF_STENCIL_ADDEND = 4, MVF_STENCIL_ADDEND_BITS = 8, MVF_STENCIL_OUT_GATE = 16,
    MVF_STENCIL_STATS = 32,          /* partial sums were written (the statistics of mvf_nhwc_stencil_stats or the column sums of _gate_colsums)       */
    MVF_STENCIL_TAIL_COPY = 64       /* x_c == out_c > cs: channels >= cs were copied from x to out by a second launch                                */
};
typedef struct {
    int32_t kernel;                  /* MVF_STENCIL_KERNEL_*                                                                          */
    int32_t dtype;                   /* MVF_F32 | MVF_BF16                                                                            */
    int32_t frames_per_chunk;        /* CHUNKED: 4 (fp32) | 8 (bf16); the walk and the LDS kernel: 0                                  */
    int32_t rows_per_band, chan_per_wg;   /* LDS: the tile (as mvf_nhwc_stencil_tile_plan); else 0                                    */
    int32_t bands;                   /* workgroups per clip along the pixels                                                          */
    int32_t pixels_per_wg;           /* pixels of one frame a workgroup owns (LDS: rows_per_band * w); it owns them in all T frames   */
    int32_t grid_x, grid_y;          /* clips * bands, channel slabs                                                                  */
    int32_t partial_rows;            /* rows of stats_part / sums_part per channel (= grid_x); 0 without MVF_STENCIL_STATS            */
    int32_t flags;                   /* MVF_STENCIL_* bits                                                                            */
    int32_t launches;                /* 1, or 2 with the tail copy                                                                    */
} mvf_stencil_launch_info_t;
int mvf_nhwc_stencil_last_launch(mvf_stencil_launch_info_t* out);
enum {
    MVF_TAPGRAD_KERNEL_NONE = 0,
    MVF_TAPGRAD_KERNEL_ROWS = 1,     /* mvf_nhwc_tapgrad_rows_kernel: contiguous ranges of the (n, t, h, w) rows                      */
    MVF_TAPGRAD_KERNEL_BANDS = 2     /* mvf_nhwc_tapgrad_kernel: (clip, band of pixels) workgroups walking t (policy tapgrad_rows=0)  */
};
typedef struct {
    int32_t kernel;                  /* MVF_TAPGRAD_KERNEL_*                                                                          */
    int32_t dtype;
    int32_t nblk;                    /* partial rows [nblk][cs][7] the finalize kernel sums (= grid x)                                */
    int32_t rows_per_blk;            /* ROWS: rows per block; BANDS: pixels of one frame per block (it owns them in all T frames)     */
    int32_t cgp;                     /* threads along the 4-channel groups per block                                                  */
    int32_t grid_y;                  /* channel slabs                                                                                 */
    int32_t launches;                /* the partial sums and their finalize: 2                                                        */
} mvf_tapgrad_launch_info_t;
int mvf_nhwc_tapgrad_last_launch(mvf_tapgrad_launch_info_t* out);
/* clip_grad_norm_(max_norm) on grad_scale*grads, then torch.optim.SGD(nesterov) on flat fp32 buffers.
 * norm_out[0] = total norm, norm_out[1] = clip coefficient. */
size_t mvf_sgd_workspace_bytes(long n);
int mvf_sgd_nesterov_step(float* params, const float* grads, float* momentum_buf, long n, float grad_scale, float max_norm,
                          float lr, float momentum, float weight_decay, int first_step, float* norm_out, void* ws,
                          size_t ws_bytes, void* stream);
/* The same step with per-segment multipliers = build_optimizer's paramwise_options (codes/core/train.py:117-156: bias_lr_mult,
 * bias_decay_mult, norm_decay_mult give every parameter its own lr / weight_decay) on the flat buffers: segment k covers elements
 * [first_k, first_{k+1}) (sorted, first_0 = 0) with lr * lr_mult, weight_decay * decay_mult.  nesterov = 0 gives the plain
 * momentum update (p -= lr * buf).  The gradient norm / clip coefficient are global, as clip_grad_norm_ over all parameters.
 * lr_mult < 0 marks a segment EXCLUDED from training (requires_grad False: norm_frozen / partial_norm, resnet.py:496-527): its
 * gradient does not enter the norm, its parameters and momentum are left untouched. */
typedef struct mvf_sgd_segment {
    long long first;
    float lr_mult, decay_mult;
} mvf_sgd_segment_t;
int mvf_sgd_step_segments(float* params, const float* grads, float* momentum_buf, long n, float grad_scale, float max_norm, float lr,
                          float momentum, float weight_decay, int first_step, int nesterov, const mvf_sgd_segment_t* segments, int nseg,
                          float* norm_out, void* ws, size_t ws_bytes, void* stream);
/* Gradient accumulation over the micro-batches of one optimizer step (the reference's 8 ranks x 12 clips run one after another on one GPU, each micro-batch
 * under its own BatchNorm statistics; codes/core/dist_utils.py:61-67 sums the same per-rank gradients with an all-reduce): first != 0: acc[i] = g[i] (the
 * accumulator is never cleared), first == 0: acc[i] = acc[i] + g[i], one fp32 add per element, i in [0, n).  No atomics and a grid that depends only on n and the
 * operands' alignment: the result is bit-identical from run to run.  acc and g are flat fp32 device arrays that need only 4-byte alignment (views
 * flat_*[off:] of the engine's buffers) and must not overlap; nothing outside [0, n) is read or written.  n == 0 succeeds without a launch; n < 0 or a NULL
 * pointer with n > 0 is MVF_EINVAL.  The optimizer then runs on acc with grad_scale = 1 / (micro-batches * world). */
int mvf_grad_accumulate(float* acc, const float* g, long n, int first, void* stream);
/* Exponential moving average of the parameters (the weights the fine-tuning recipes evaluate and ship), kept on a flat fp32 buffer laid out like params.
 * One update, every element, every entry point below:  ema' = fmaf(m, p' - ema, ema)  in fp32, with p' the parameter value this optimizer step stores -- and
 * ema' = p' itself at m = 1 (the mean of one iterate; the two roundings of the formula can miss p' by an ulp there).  ema == p' is an exact fixed point for
 * every m (a -0 comes back as +0), and the rounding of 1 - m never enters.  The update rounds to nothing once m |p' - ema| < ulp(ema) / 2.
 *
 * mvf_sgd_nesterov_step_ema / mvf_sgd_step_segments_ema: the arguments of their plain twins with `float* ema, float ema_momentum` inserted directly in front
 * of norm_out.  params, momentum_buf and norm_out come out bit-identical to the plain entry points (same kernels, same grids, the update compiled in), ema
 * bit-identical to the plain step followed by mvf_ema_update.  In the segment form an excluded segment (lr_mult < 0) leaves ema untouched as well.  ema is n
 * floats, 4-byte aligned, and overlaps none of params / grads / momentum_buf; a NULL, misaligned or overlapping ema, or an ema_momentum outside [0, 1] (or
 * NaN), is MVF_EINVAL and nothing is launched. */
int mvf_sgd_nesterov_step_ema(float* params, const float* grads, float* momentum_buf, long n, float grad_scale, float max_norm, float lr, float momentum,
                              float weight_decay, int first_step, float* ema, float ema_momentum, float* norm_out, void* ws, size_t ws_bytes, void* stream);
int mvf_sgd_step_segments_ema(float* params, const float* grads, float* momentum_buf, long n, float grad_scale, float max_norm, float lr, float momentum,
                              float weight_decay, int first_step, int nesterov, const mvf_sgd_segment_t* segments, int nseg, float* ema, float ema_momentum,
                              float* norm_out, void* ws, size_t ws_bytes, void* stream);
/* The same update as a launch of its own (after an optimizer that is not this library's, and the twin the fused kernels are tested against), and the in-place
 * exchange of two flat buffers (averaged <-> live parameters for evaluation: the model's parameters are views of the flat buffer, so pointers cannot be
 * swapped; no third buffer is allocated).  Operands are flat fp32 device arrays that need only 4-byte alignment (they may be misaligned relative to each
 * other) and must not overlap; nothing outside [0, n) is read or written; the grid depends on n and the alignment only, no atomics: bit-identical from run to
 * run.  n == 0 succeeds without a launch; n < 0, a NULL pointer with n > 0, overlap, or a momentum outside [0, 1] (or NaN) is MVF_EINVAL. */
int mvf_ema_update(float* ema, const float* params, long n, float momentum, void* stream);
int mvf_ema_swap(float* a, float* b, long n, void* stream);
/* Precise BatchNorm (mmaction2's PreciseBNHook, fvcore's update_bn_stats): before evaluation the running statistics of every BatchNorm in training mode are
 * replaced by the plain average of the per-batch statistics over a few hundred forward-only batches with the weights held fixed.  The statistics stay in the
 * modules' own buffers; a persistent DEVICE table of segments lays them out as one flat "shadow" range [0, n): segment k = {ptr, first} owns shadow elements
 * [first_k, first_{k+1}) (the last one up to n), element first_k + j being ptr[j].  Each entry point is ONE launch over the whole table, one thread per
 * element, no atomics: bit-identical from run to run.
 *   accumulate:  acc[i] += (double)value_i                                   (after a forward whose statistics kernels ran with momentum 1: value = the batch's)
 *   finalize:    (float)(acc[i] / (double)count) -> dst_flat_or_null[i], or with NULL through the table into the segments; equals numpy's
 *                np.float32(sum_in_call_order(np.float64(x)) / np.float64(count)) bit for bit
 *   exchange:    mode 0 flat[i] = value_i (gather), 1 value_i = flat[i] (scatter), 2 swap; 32-bit words moved unchanged (NaN payloads, -0.0)
 * Checked before any launch, MVF_EINVAL otherwise: non-NULL seg / acc / flat (acc 8-byte, flat and every segment pointer 4-byte aligned), nseg > 0, n > 0,
 * count > 0, mode in 0..2, first_0 == 0, first strictly ascending and below n, no segment overlapping the flat array of the call.  The table is read on the
 * host for that check: directly when `seg` is host memory (only the checks can succeed then), through a private non-blocking stream when it is device memory
 * -- that waits for a 16 * nseg byte copy, never for the caller's stream; the table's upload must be complete, and the calls cannot be captured into a HIP graph. */
typedef struct mvf_stat_segment {
    float* ptr;
    long first;
} mvf_stat_segment_t;
int mvf_bn_stats_accumulate(const mvf_stat_segment_t* seg, int nseg, long n, double* acc, void* stream);
int mvf_bn_stats_finalize(const mvf_stat_segment_t* seg, int nseg, long n, const double* acc, long count, float* dst_flat_or_null, void* stream);
int mvf_bn_stats_exchange(const mvf_stat_segment_t* seg, int nseg, long n, float* flat, int mode, void* stream);
/* Non-finite step guard: an optimizer step whose clip norm is not finite becomes a no-op ON THE DEVICE, with no host synchronisation, and the BatchNorm
 * statistics the step's forward passes have already updated are put back (torch's GradScaler.step skips on found_inf, clip_grad_norm_ has
 * error_if_nonfinite; here the decision never leaves the device).
 *
 * guard: four ints in device memory, 4-byte aligned, owned by the caller, zero at the start of a run:
 *   guard[0]  this step's flag, 1 = skipped        guard[1]  skipped steps in total
 *   guard[2]  the current run of consecutive skips  guard[3]  steps seen
 *
 * mvf_sgd_step_guarded: ONE entry point for the four forms of the step above -- segments == NULL (nseg ignored) is the flat Nesterov form
 * (mvf_sgd_nesterov_step; `nesterov` is ignored), ema == NULL (ema_momentum ignored) keeps no average.  The flag is decided where the norm is finished, by
 * the one lane that writes norm_out: flag = the scaled norm grad_scale * sqrt(sum g^2) is not finite.  That is a NaN or an infinity anywhere in a gradient
 * that enters the norm, AND a finite gradient whose sum of squares overflows fp32 (|g| ~ 1.8e19 and beyond): such a step is SKIPPED too, where the plain
 * entry points would clip it to nothing (coef = max_norm / inf = 0) or, with clipping off, apply it.  The same lane updates the counters (a good step
 * resets guard[2]); norm_out is written as always, so a logged nan / inf is the honest value.  Every workgroup of the update kernel reads guard[0] and returns
 * before any store when it is set: params, momentum_buf and ema keep their bits.  With the flag clear, params, momentum_buf, ema and norm_out are
 * bit-identical to the plain entry point of the same form (the same kernel bodies and grids, instantiated with the check).  Excluded segments
 * (lr_mult < 0) stay outside the norm and therefore outside the decision; so does whatever the caller cuts off in front of `params`.
 * Checked as the _ema entry points are, and: a NULL or misaligned guard, or a guard that overlaps params / grads / momentum_buf / ema / norm_out / ws /
 * the segment table, is MVF_EINVAL and nothing is launched.
 *
 * mvf_bn_stats_snapshot / mvf_bn_stats_restore: ONE launch each over a segment table of running statistics (as above) and an int64 array (the
 * num_batches_tracked counters).  snapshot: flat[i] = value_i for i in [0, n), counters_copy[j] = counters[j] for j in [0, ncount).  restore: the inverse
 * (value_i = flat[i], counters[j] = counters_copy[j]) when guard[0] != 0, and NOT ONE STORE otherwise.  Words travel as uint32 / int64 (NaN payloads, -0.0),
 * one thread per element, no atomics.  ncount == 0 (then the two counter pointers may be NULL) moves the statistics alone.
 * These two run every training step, so UNLIKE the three entry points above they do NOT read the table back to the host: they check their by-value arguments
 * (nseg > 0, n > 0, nseg <= n, ncount >= 0), non-NULL pointers and their alignment (seg 8, flat and guard 4, counters 8 bytes), and that guard overlaps
 * neither flat nor the counter arrays nor the table -- MVF_EINVAL otherwise, nothing launched.  The table's CONTENT (first_0 == 0, ascending offsets below n,
 * valid pointers, no overlap with flat) must have been validated once by the caller when it built the table: any mvf_bn_stats_exchange call on it does. */
int mvf_sgd_step_guarded(float* params, const float* grads, float* momentum_buf, long n, float grad_scale, float max_norm, float lr, float momentum,
                         float weight_decay, int first_step, int nesterov, const mvf_sgd_segment_t* segments, int nseg, float* ema, float ema_momentum,
                         int* guard, float* norm_out, void* ws, size_t ws_bytes, void* stream);
int mvf_bn_stats_snapshot(const mvf_stat_segment_t* seg, int nseg, long n, float* flat, const long long* counters, long ncount, long long* counters_copy,
                          void* stream);
int mvf_bn_stats_restore(const mvf_stat_segment_t* seg, int nseg, long n, const float* flat, long long* counters, long ncount,
                         const long long* counters_copy, const int* guard, void* stream);
/* clip_grad_norm_(max_norm) on grad_scale * grads, then torch.optim.AdamW (decoupled = 1) or torch.optim.Adam (decoupled = 0), non-amsgrad, non-maximize, on
 * flat fp32 device buffers that need only 4-byte alignment -- ONE entry point beside mvf_sgd_step_guarded, with its conventions: caller-owned workspace
 * (mvf_adamw_workspace_bytes, 8-byte aligned), every check before any launch, no atomics, a grid that depends only on n, bit-identical from run to run.
 * Per trained element, in fp32, with coef = norm_out[1] and t the step count AFTER this step:
 *     d  = g * grad_scale * coef
 *     decoupled = 0:  d = d + wd_i * p            decoupled = 1:  p = p * (1 - lr_i * wd_i)
 *     m' = b1 * m + (1 - b1) * d
 *     v' = b2 * v + (1 - b2) * d^2
 *     p' = p - (lr_i / (1 - b1^t)) * m' / (sqrt(v') / sqrt(1 - b2^t) + eps)
 * hyper is HOST memory, read during the call; its fields are doubles because 1 - beta1, 1 - beta2, 1 - lr_i * wd_i and lr_i / (1 - b1^t) are formed in double
 * and rounded to fp32 once, as torch does with its Python scalars (1 - 0.999f misses 1 - 0.999 by 1.3e-5 relative, which would land in exp_avg_sq).
 * applied_steps: one long long in DEVICE memory, 8-byte aligned, owned by the caller, zero at the start of a run: the number of steps applied so far.  The
 * lane that finishes the norm writes norm_out and the guard counters, increments *applied_steps and leaves the two bias-correction factors of the new t (formed
 * in double) in the workspace for the update kernel.  With guard != NULL and a non-finite scaled norm it does neither: the skipped step does not count, the
 * next good step is corrected with the t it would have had -- torch's GradScaler, under which optimizer.step() is not called and state['step'] does not move.
 * segments: the table of mvf_sgd_step_segments (lr * lr_mult, weight_decay * decay_mult per segment; lr_mult < 0 = excluded: the gradient stays outside the
 * norm, params, exp_avg, exp_avg_sq and ema keep their bits); NULL (nseg ignored) = flat, bit-identical to the one-segment table {0, 1, 1}.
 * ema: NULL (ema_momentum ignored) = none; else ema[i] = ema_step(ema[i], p', ema_momentum) where p' is in a register, bit-identical to the plain step
 * followed by mvf_ema_update.  guard: NULL = unguarded; else the four counters of mvf_sgd_step_guarded with the same rule, every workgroup of the update
 * kernel returns before any store when the flag is set, and with the flag clear the results are bit-identical to guard == NULL.
 * MVF_EINVAL, nothing launched: a NULL params / grads / exp_avg / exp_avg_sq / norm_out / hyper / applied_steps, n <= 0, segments with nseg <= 0, a misaligned
 * operand (applied_steps, ws and segments 8 bytes, the others 4), any two operands that overlap (the four arrays, ema, guard, applied_steps, norm_out, ws, the
 * segment table), a beta outside [0, 1), eps <= 0, a negative lr or weight_decay, a NaN anywhere in the struct, decoupled other than 0 / 1, an ema_momentum
 * outside [0, 1] (or NaN) when ema is given.  MVF_EWS: a NULL or short workspace. */
typedef struct mvf_adamw_hyper {
    double lr, beta1, beta2, eps, weight_decay;
    int decoupled;
} mvf_adamw_hyper_t;
size_t mvf_adamw_workspace_bytes(long n);
int mvf_adamw_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, long n, float grad_scale, float max_norm,
                   const mvf_adamw_hyper_t* hyper, const mvf_sgd_segment_t* segments, int nseg, float* ema, float ema_momentum, int* guard,
                   long long* applied_steps, float* norm_out, void* ws, size_t ws_bytes, void* stream);
/* clip_grad_norm_(max_norm) on grad_scale * grads, then LAMB with the arithmetic of timm's Lamb (optim/lamb.py: bias correction on, grad_averaging on), on
 * flat fp32 device buffers that need only 4-byte alignment -- beside mvf_adamw_step, with its conventions: caller-owned workspace
 * (mvf_lamb_workspace_bytes(n, nseg), 8-byte aligned), every check before any launch, no atomics, grids that depend on n and nseg alone, bit-identical from
 * run to run.  The clip in front is this library's, coef = min(1, max_norm / (norm + 1e-6)) (clip_grad_norm_; max_norm <= 0 = off); timm's own max_grad_norm
 * divides by max(1, norm / max_grad_norm) and so differs by that 1e-6 alone.
 * segments is REQUIRED, and ONE SEGMENT IS ONE TRUST-RATIO UNIT: the caller passes one entry per parameter tensor (segment k covers elements
 * [first_k, first_{k+1}), sorted, first_0 = 0; lr * lr_mult, weight_decay * decay_mult; lr_mult < 0 = excluded: the gradient stays outside the norm, params,
 * exp_avg, exp_avg_sq and ema keep their bits).
 * Per trained element, in fp32, with coef = norm_out[1], wd_i = weight_decay * decay_mult and t the applied-step count AFTER this step:
 *     d  = g * grad_scale * coef
 *     m' = b1 * m + (1 - b1) * d
 *     v' = b2 * v + (1 - b2) * d^2
 *     u  = (m' / (1 - b1^t)) / (sqrt(v') / sqrt(1 - b2^t) + eps) + wd_i * p
 * Per segment k, the two sums in fp64 (the square of an fp32 value is exact there), each rounded once:
 *     wn = sqrt(sum p^2)   (p before the update)          un = sqrt(sum u^2)
 *     adapts_k = (wd_k != 0) or always_adapt
 *     r_k = adapts_k and wn > 0 and un > 0 ? (float)(wn / un) : 1 ;     trust_clip: r_k = min(r_k, 1)
 *     p'  = p - (float)(lr_k * (double)r_k) * u
 * hyper is HOST memory, read during the call; 1 - beta1, 1 - beta2, 1 / (1 - b1^t), sqrt(1 - b2^t), wd_i and lr_k * r_k are formed in double and rounded to
 * fp32 once.  u is formed twice -- for un, and again when p' is stored -- by one function whose roundings are pinned, so no n-sized scratch is needed.
 * ratio_out: nseg floats in DEVICE memory, 4-byte aligned: the ratio applied to each segment, 1 where the segment does not adapt, 0 where it is excluded.
 * applied_steps, ema, guard, norm_out: as in mvf_adamw_step (ema[i] = ema_step(ema[i], p', ema_momentum), bit-identical to the plain step followed by
 * mvf_ema_update; the lane that finishes the norm keeps the guard counters and the applied-step count).  With guard != NULL and a non-finite scaled norm every
 * workgroup of the three LAMB launches returns before any store: params, exp_avg, exp_avg_sq, ema, ratio_out and *applied_steps keep their bits.  With the flag
 * clear the results are bit-identical to guard == NULL.
 * The table's CONTENT (ascending first, first_0 == 0) is the caller's contract, validated once where the table is built, as for mvf_flat_segment_stats: a table
 * that breaks it gives meaningless figures but no access outside the operands.
 * MVF_EINVAL, nothing launched: a NULL params / grads / exp_avg / exp_avg_sq / norm_out / ratio_out / hyper / applied_steps / segments, n <= 0, nseg outside
 * [1, n], a misaligned operand (applied_steps, ws and segments 8 bytes, the others 4), any two operands that overlap (the four arrays, ema, guard,
 * applied_steps, norm_out, ratio_out, ws, the segment table), a beta outside [0, 1), eps <= 0, a negative lr or weight_decay, a NaN anywhere in the struct,
 * trust_clip or always_adapt other than 0 / 1, an ema_momentum outside [0, 1] (or NaN) when ema is given.  MVF_EWS: a NULL or short workspace.
 * mvf_lamb_workspace_bytes is 0 for n <= 0 or nseg outside [1, n]. */
typedef struct mvf_lamb_hyper {
    double lr, beta1, beta2, eps, weight_decay;
    int trust_clip, always_adapt;
} mvf_lamb_hyper_t;
size_t mvf_lamb_workspace_bytes(long n, int nseg);
int mvf_lamb_step(float* params, const float* grads, float* exp_avg, float* exp_avg_sq, long n, float grad_scale, float max_norm,
                  const mvf_lamb_hyper_t* hyper, const mvf_sgd_segment_t* segments, int nseg, float* ema, float ema_momentum, int* guard,
                  long long* applied_steps, float* norm_out, float* ratio_out, void* ws, size_t ws_bytes, void* stream);
/* Device-side accuracy: top-k hits and confusion counts of a (rows, classes) fp32 score matrix against integer labels, summed into a state array that stays
 * on the device (evaluation without one readback per video, training accuracy in the log without a readback per step).
 *
 * state: a flat int64 array in device memory, 8-byte aligned, owned by the caller, zero at the start of a window; mvf_metrics_state_words(classes,
 * with_confusion) words (0 for classes < 1, or for classes * classes beyond int32 with the matrix on).  int64 so that a SUM all-reduce of the array merges ranks.
 *   word 0          rows seen
 *   word 1          rows whose label is outside [0, classes)
 *   word 2          rows holding a NaN score
 *   words 3..7      reserved (zero)
 *   words 8..15     hits for ks[0..nk)                               (MVF_METRICS_HITS; words 8 + nk .. 15 stay zero)
 *   words 16..      only with_confusion: the classes x classes confusion matrix, row = real label, column = prediction      (MVF_METRICS_CONFUSION)
 *
 * Per row, with label y and scores s:
 *   - a label outside [0, classes), or a NaN anywhere in the row, increments word 1 or word 2 (a bad label wins; word 0 as well) and touches nothing else;
 *     for a bad label no score of the row -- and no memory outside the row -- is read.  rank_out / pred_out get -1 for such a row.
 *   - rank = #{j : s_j > s_y, or s_j == s_y and j < y}; hit_k holds iff rank < k.  Ties go to the lower class index; +inf and -inf are ordinary values.
 *   - pred = the lowest index of the maximum (np.argmax of a NaN-free row).  Hence hits(k = 1) == trace(confusion).
 *   - k >= classes always hits on a valid row.
 * rank_out / pred_out: NULL, or `rows` ints each in device memory (the per-row record: a whole-dataset prediction dump in one read).
 * One wavefront per row with a strided loop over the classes (any classes >= 1); counters are integers added with integer atomics (per workgroup in LDS,
 * then one global atomic per non-zero word), so the state does not depend on the order of accumulation.  Asynchronous on `stream`.
 * ks is HOST memory, read during the call.  Checked before any launch: a NULL scores / labels / state / ks, or a misaligned operand (labels and state 8
 * bytes, the others 4) is MVF_EINVAL; classes < 1, rows < 0, nk outside [1, 8], any k < 1, or classes * classes beyond int32 with the matrix on is
 * MVF_ESHAPE.  rows == 0 is MVF_OK without a launch. */
enum { MVF_METRICS_ROWS = 0, MVF_METRICS_BAD_LABEL = 1, MVF_METRICS_NAN_ROWS = 2, MVF_METRICS_HITS = 8, MVF_METRICS_MAX_K = 8, MVF_METRICS_CONFUSION = 16 };
size_t mvf_metrics_state_words(int classes, int with_confusion);
int mvf_metrics_update(const float* scores, int rows, int classes, const long long* labels, const int* ks, int nk, long long* state, int with_confusion,
                       int* rank_out, int* pred_out, void* stream);
/* Multi-label evaluation (csrc/multilabel_metrics.hip): per-class average precision of everything recorded in a pass, without a sort and without a
 * readback.  Definition -- the step-wise AP of scikit-learn's average_precision_score, what mmaction2 reports as mean_average_precision -- for class c
 * with positives P_c:
 *   AP_c = (1 / |P_c|) * sum_{i in P_c} TP_i / N_i,     N_i = #{j : s_jc >= s_ic},     TP_i = #{j in P_c : s_jc >= s_ic}
 * Summed over a group of tied scores the terms are dTP * TP / N at that threshold, so ties need no special case and nothing depends on the order of the
 * rows.  +inf and -inf are ordinary values.  mAP = the mean of AP_c over the classes with at least one positive (the caller's division).
 *
 * The record, owned by the caller, in device memory:
 *   rec_scores fp32  (classes, capacity)   class-major: a class's column is contiguous
 *   rec_labels uint8 (classes, capacity)   0 / 1
 *   state      int64 (MVF_MULTILABEL_STATE_WORDS), 8-byte aligned, zero at the start of a pass:
 *     word 0  slots used: the write offset, in device memory, so that appending synchronises nothing        (MVF_MULTILABEL_SLOTS)
 *     word 1  rows that held a NaN score                                                                     (MVF_MULTILABEL_NAN_ROWS)
 *     word 2  rows that did not fit (overflow): counted, not stored                                          (MVF_MULTILABEL_OVERFLOW)
 *     word 3  rows seen                                                                                      (MVF_MULTILABEL_SEEN)
 *     words 4..7 reserved (zero)
 *   so the rows that take part are word 3 - word 2 - word 1, and SUM-merging words 1..3 merges ranks.
 * mvf_multilabel_record: appends scores (rows, classes) fp32 and labels (rows, classes) uint8 (non-zero = positive) at slot word 0 + row.  A row holding a
 * NaN score is stored as NaN scores without a label: a comparison with a NaN is false and the row is no positive, so it is left out of every class (and
 * counted in word 1) while slots and rows stay in step.  For the same reason a NaN-filled, label-free slot is padding: records whose unused slots are
 * filled that way merge by concatenation along `capacity` with word 0 = the total capacity.  Two launches (the store; one thread that advances the words);
 * rows == 0 is MVF_OK without a launch.
 * mvf_multilabel_ap: two launches over slots [0, word 0), read on the device.  (1) a workgroup per 256 rows of a class walks the class's column in 256-entry
 * LDS tiles and writes the integer pair tp[c][i] = TP_i, nn[c][i] = N_i for each positive i, 0 / 0 for the other rows (a workgroup without a positive
 * returns at once: sum_c |P_c| * n comparisons, to workgroup granularity); (2) one wavefront per class sums TP_i / N_i in fp64 -- lane l takes rows l, l + 64, ..
 * in ascending order, a shuffle tree adds the lane sums -- into ap[c] (NaN for a class without a positive) and positives[c] = |P_c|.  tp, nn int32 and
 * (classes, capacity); ap fp64 (classes); positives int64 (classes).  Integer counts in launch 1, no atomics in either: bit-identical from run to run.
 * Checked before any launch: a NULL or misaligned operand (state, ap, positives 8 bytes; fp32 / int32 arrays 4) is MVF_EINVAL; classes < 1 (ap: > 65535),
 * rows < 0, capacity outside [1, 2^31 - 1], or a record beyond the grid / 2^63 bytes is MVF_ESHAPE. */
enum { MVF_MULTILABEL_SLOTS = 0, MVF_MULTILABEL_NAN_ROWS = 1, MVF_MULTILABEL_OVERFLOW = 2, MVF_MULTILABEL_SEEN = 3, MVF_MULTILABEL_STATE_WORDS = 8 };
int mvf_multilabel_record(const float* scores, const unsigned char* labels, int rows, int classes, float* rec_scores, unsigned char* rec_labels, long capacity,
                          long long* state, void* stream);
int mvf_multilabel_ap(const float* rec_scores, const unsigned char* rec_labels, long capacity, int classes, const long long* state, int* tp, int* nn, double* ap,
                      long long* positives, void* stream);
/* Sample-wise AP, precision / recall / F1 counts and the best-F1 threshold per class (csrc/multilabel_f1.hip), all over slots [0, word 0) of the record
 * above, read on the device.  A slot that holds a NaN score (a NaN row, or padding) takes part in nothing.  No atomics; integer counts, or an fp64 sum in a
 * fixed order: bit-identical from run to run.
 * mvf_multilabel_sample_ap: the sample-wise AP that Multi-Moments in Time reports (mmaction2's mmit_mean_average_precision), the step-wise AP taken along
 * a row.  For row i with positives P_i:
 *   AP_i = (1 / |P_i|) * sum_{c in P_i} TP_ic / N_ic,     N_ic = #{k : s_ik >= s_ic},     TP_ic = #{k in P_i : s_ik >= s_ic}
 * so ties need no special case.  sample_ap fp64 (capacity), sample_positives int32 (capacity): NaN and 0 for a row without a positive and for the slots
 * beyond word 0.  sample mAP = the mean of AP_i over the rows with at least one positive (the caller's division).  One wavefront per row: a workgroup of
 * four wavefronts owns 64 adjacent rows and stages tiles of 64 rows x 64 classes through LDS, so that the class-major record is read along its contiguous
 * axis; lane l counts for classes l, l + 64, .. and adds their TP / N in ascending order, a shuffle tree adds the 64 lane sums.
 * mvf_multilabel_prf: counts (classes, 4) int64 = TP, FP, FN, TN of "row i is predicted for class c iff its recorded value >= theta_c", theta_c =
 * thresholds[c] (device, fp32, (classes)) when given and `threshold` otherwise.  The recorded values are compared as they are (probabilities under
 * average_clips='sigmoid').  One wavefront per class.  A NaN `threshold` with thresholds == NULL is MVF_EINVAL; a NaN entry of `thresholds` is the
 * caller's to refuse before the upload (the kernel then predicts nothing for that class).
 * mvf_multilabel_best_f1: behind mvf_multilabel_ap, from its tp / nn / positives.  Per class it takes the positive i that maximises
 *   F_i = 2 * TP_i / (N_i + |P_c|)        -- the F1 of the threshold s_ic: precision TP_i / N_i, recall TP_i / |P_c|
 * compared exactly by integer cross-multiplication in 64 bits (capacity > 2^30 is MVF_ESHAPE here); among equal F the larger score wins (equal scores
 * have equal counts).  The maximum of F1 over ALL thresholds is attained at a positive's score -- raising a threshold to the next predicted positive drops
 * only false positives -- so best_tp[c], best_n[c] give the class's best achievable F1 = 2 best_tp / (best_n + |P_c|) and best_threshold[c] the threshold
 * (>=) that attains it.  A class without a positive gets 0, 0, NaN.  best_tp, best_n int32 (classes), best_threshold fp32 (classes).  One wavefront per
 * class: lane l takes rows l, l + 64, .. in ascending order, then a shuffle tree with the same comparison.
 * Checked before any launch, as mvf_multilabel_ap: a NULL or misaligned operand (state, sample_ap, counts, positives 8 bytes; fp32 / int32 arrays 4) is
 * MVF_EINVAL; classes outside [1, 65535] or a capacity outside the record's range is MVF_ESHAPE. */
int mvf_multilabel_sample_ap(const float* rec_scores, const unsigned char* rec_labels, long capacity, int classes, const long long* state, double* sample_ap,
                             int* sample_positives, void* stream);
int mvf_multilabel_prf(const float* rec_scores, const unsigned char* rec_labels, long capacity, int classes, const long long* state, float threshold,
                       const float* thresholds /* (classes) or NULL */, long long* counts /* (classes, 4): TP, FP, FN, TN */, void* stream);
int mvf_multilabel_best_f1(const float* rec_scores, const int* tp, const int* nn, const long long* positives, long capacity, int classes,
                           const long long* state, int* best_tp, int* best_n, float* best_threshold, void* stream);
/* Per-parameter training statistics and the diagnosis of a skipped step (csrc/layer_stats.hip): where a NaN came from and whether every layer is learning,
 * from figures that stay on the device until the host asks.
 *
 * mvf_flat_segment_stats: per SEGMENT of a flat fp32 array x of n elements -- or of the element-wise difference x - y when y is given -- four figures.
 * Segment k covers [first[k], first[k + 1]), the last one runs up to n; `first` is a DEVICE array of nseg int64 with first[0] == 0, strictly ascending and
 * below n, validated ONCE by the caller when it builds it (as the table of mvf_bn_stats_snapshot): it is not read back per call.  With
 * d_i = (double)x[i], or (double)x[i] - (double)y[i]:
 *   sumsq   the sum of d_i * d_i over the finite d_i            absmax  the largest |d_i| over the finite d_i (0 if there are none)
 *   n_nan   the number of d_i that are NaN                      n_inf   the number that are +inf or -inf   (inf - inf is a NaN: d_i is classified, not x and y)
 * Arithmetic: fp64 throughout.  The square of an fp32 value is exact in fp64, and so is the difference of two fp32 values unless their exponents lie more
 * than 29 binades apart (then it is rounded once, and its square once more); what differs from a serial fp64 sum is the ORDER of at most n_k non-negative
 * additions, so sumsq agrees with any fp64 restatement within a relative (n_k + 4) * 2^-52; absmax and the counts are exact.  1e20 does not overflow and
 * 1e-30 does not vanish.  No floating-point atomics; two launches whose grids depend on n and nseg alone (fixed 4096-element chunks, one workgroup each,
 * write one partial per (chunk c, segment s) intersection to workspace slot c + s; one wavefront per segment adds its slots in a fixed order): bit-identical
 * from run to run.  x, y need 4-byte alignment only and segment boundaries may fall anywhere (16-byte loads are used where the addresses allow).
 * guard_or_null: NULL = always; else the four ints of mvf_sgd_step_guarded: every workgroup of both launches reads guard[0], and when it is 0 NOT ONE byte of
 * out, *step_out or the workspace is stored (the rule of mvf_bn_stats_restore); when it is non-zero the figures are written and, with step_out given,
 * *step_out = guard[3] (the index of the step they belong to).  step_out without a guard is MVF_EINVAL.
 * ws: mvf_flat_stats_workspace_bytes(n, nseg) bytes (0 for arguments the call would refuse), 8-byte aligned, owned by the caller; it needs no initialisation.
 * Checked before any launch, nothing launched otherwise.  MVF_EINVAL: NULL x / first / out; n <= 0; nseg <= 0 or nseg > n; a misaligned operand (first, out,
 * step_out and ws 8 bytes, x, y and guard 4 bytes); out or ws overlapping x / y or one another; guard overlapping out / step_out / ws.  MVF_EWS: a NULL or
 * short workspace.
 *
 * mvf_bn_stats_nonfinite: counts[k] = the number of non-finite 32-bit words (exponent all ones) in segment k of a running-statistics table, the table
 * mvf_bn_stats_snapshot takes.  ONE launch, one wavefront per segment with a strided loop, integer sums.  guard_or_null as above: guard[0] == 0 stores
 * nothing.  Like snapshot / restore it does not read the table back: checked are the by-value arguments (nseg > 0, n > 0, nseg <= n), non-NULL seg / counts
 * and alignment (seg and counts 8 bytes, guard 4), and that counts, the table and guard do not overlap -- MVF_EINVAL otherwise, nothing launched. */
typedef struct mvf_flat_stats {
    double sumsq;
    double absmax;
    long long n_nan;
    long long n_inf;
} mvf_flat_stats_t;
size_t mvf_flat_stats_workspace_bytes(long n, int nseg);
int mvf_flat_segment_stats(const float* x, const float* y_or_null, long n, const long long* first, int nseg, mvf_flat_stats_t* out, const int* guard_or_null,
                           long long* step_out_or_null, void* ws, size_t ws_bytes, void* stream);
int mvf_bn_stats_nonfinite(const mvf_stat_segment_t* seg, int nseg, long n, long long* counts, const int* guard_or_null, void* stream);

/* ------------------------------------------------------------------------------------------------
 * [r6] Launch-table replay.  One training step (the reference's batch_processor + DistOptimizerHook.after_train_iter, codes/core/train.py:45-60,
 * codes/core/dist_utils.py:61-67) is a fixed sequence of this library's entry points on two HIP streams; the host code records it once and replays it from C
 * instead of re-issuing ~650 calls from Python (mvfnet_amd/launch_plan.py).  An op is
 *   MVF_PLAN_CALL    fn(words[word0 .. word0 + n_int), floats[float0 .. float0 + n_flt)): fn = the address of ANY int-returning entry point of this header,
 *                    its integer-class arguments (pointers, int, long, size_t, the stream) in prototype order as 64-bit words, its float arguments in order
 *   MVF_PLAN_RECORD  hipEventRecord(event = words[word0], stream = words[word0 + 1])
 *   MVF_PLAN_WAIT    hipStreamWaitEvent(stream = words[word0], event = words[word0 + 1])
 * Events are the caller's.  The run stops at the first op that fails: its index goes to *failed_op (else -1), its status is returned and mvf_last_error()
 * describes it.  Arguments that change between runs are patched in `words` by the caller.  x86-64 System V hosts only. */
enum { MVF_PLAN_CALL = 0, MVF_PLAN_RECORD = 1, MVF_PLAN_WAIT = 2 };
typedef struct mvf_plan_op {
    int kind, n_int, n_flt, reserved;
    void* fn;
    long long word0, float0;
} mvf_plan_op_t;
int mvf_plan_run(const mvf_plan_op_t* ops, int n_ops, const unsigned long long* words, const float* floats, int* failed_op);

#ifdef __cplusplus
}
#endif
#endif /* MVFNET_HIP_H */
