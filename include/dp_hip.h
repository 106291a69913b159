/* dp_hip.h -- C-ABI of the MI355X-native Diff-Pruning hot path (libdp_hip.so).
 *
 * The reference (VainF/Diff-Pruning) is pure Python on top of ATen; it has no FFI of its own.  The
 * boundary a maintainer would bind is therefore the set of ATen calls its hot path makes; each entry
 * point below names the reference call site it replaces (paths relative to the reference root).
 * All pointers are DEVICE pointers owned by the caller (PyTorch owns every allocation); `stream` is a
 * hipStream_t passed as void*; every function only enqueues work on `stream` and returns a
 * hipError_t-style int (0 = success).  Nothing here throws, allocates or synchronises.
 *
 * Activation layout everywhere: channel-major planes, element (img, c, h, w) at
 *     base + img*img_stride + c*H*W + h*W + w          (NCHW with an explicit image stride)
 * Linear layers on [B, C] vectors use the same convention with H = W = 1.
 */
#ifndef DP_HIP_H
#define DP_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

/* Gather geometry shared by the implicit-GEMM kernels (see csrc/dp_common.h ConvGeom). */
typedef struct dp_conv_geom {
    int Ho, Wo, Hs, Ws, Hv, Wv, kw, stride, sden, pad_t, pad_l, ups, c_split, _pad;
    long long x1_img_stride, x2_img_stride;
} dp_conv_geom;

/* D[m][pix] = sum_{tap,c} A(tap,c,m) * X(pix,tap,c)  -- conv3x3 / conv1x1 / linear forward and dgrad,
 * attention QK^T and dP (batched).  Replaces F.conv2d / F.linear / torch.baddbmm forward and the
 * input-gradient half of ConvolutionBackward / AddmmBackward:
 *   diffusers/models/resnet.py:606,630,633 (conv1, conv2, conv_shortcut), :612 (time_emb_proj),
 *   diffusers/models/resnet.py:166,218 (Upsample2D/Downsample2D conv), unet_2d.py:273,304 (conv_in/out),
 *   diffusers/models/attention_processor.py:438-445 (to_q/k/v), :339-345 (baddbmm), :455 (to_out).
 * a_kc = 0: A is a packed weight  A[(tap*C + c)*lda + m]  (m contiguous, lda % 4 == 0, zero padded)
 * a_kc = 1: A[m*lda + c]  (c contiguous; taps must be 1)
 * Epilogue: v = alpha*acc (+bias[m]) (+tadd[img*tadd_stride + m]) (+res[img*r_img_stride + m*HoWo + r]);
 *           v *= post_scale; (act: v = max(v, 0)); out = accumulate ? out + v : v.
 * ksplit > 1 (small pixel counts): the K loop is split over workgroups, raw partial tiles go to ws and a second
 * kernel sums them in a fixed order and applies the same epilogue (deterministic). */
typedef struct dp_conv_gemm_params {
    const float* A; long long a_bs; int lda; int a_kc;
    const float* X1; const float* X2; long long x_bs;
    unsigned a_bytes, x1_bytes, x2_bytes, _pad0;   /* readable extent of A / X1 / X2 (per batch), each < 2 GiB */
    dp_conv_geom g;
    int M, C, NPIX, ntaps, batches, tile;      /* tile: 0 = 128x128, 1 = 64x128, 2 = 64x64, 3 = 96x128 (stride-1 fast kernel; else as 0) */
    float* out; long long o_img_stride; long long o_bs;
    float alpha; float post_scale;
    const float* bias; const float* tadd; long long tadd_stride;
    const float* res; long long r_img_stride;
    int accumulate; int ksplit;            /* ksplit > 1: split the K loop over blockIdx.z, partials in ws (non-batched only) */
    float* ws;                             /* >= ksplit*M*NPIX floats when ksplit > 1 */
    int x_guard; int act;                  /* act = 1: ReLU after post_scale (BasicConv2d of the FID Inception network).
                                              x_guard = 1: the 4 bytes in front of X1 (and X2) are readable memory.  The 16-byte B-tile
                                              loads of the stride-1 fast kernel read one element to the left of an image
                                              row for the shifted taps (overwritten with 0 in LDS); for the first row of the
                                              tensor that element lies in front of it.  0 = use the 4-byte loads. */
    unsigned* tile_counters;               /* ksplit > 1, optional: one zero-initialised counter per output tile (grid x * grid y).
                                              The LAST workgroup to deliver its partial tile sums the ksplit partials of that tile in
                                              ascending split order (the same fixed order as the separate reduction kernel: same bits,
                                              whoever arrives last), applies the epilogue and re-zeroes the counter; NULL = a second
                                              launch does that. */
} dp_conv_gemm_params;
int dp_conv_gemm(const dp_conv_gemm_params* p, void* stream);

/* The same convolution for the 3x3, stride 1, pad 1 case as a one-dimensional Winograd F(2, 3) implicit GEMM (csrc/winograd.hip):
 * 2/3 of the multiplies of dp_conv_gemm (4 per 2 outputs x 3 taps along W), input transform at fragment-read time, output transform
 * in the epilogue.  Replaces the same call sites as dp_conv_gemm's 3x3 forward / input-gradient launches
 * (diffusers/models/resnet.py:606,630 conv1 / conv2 and their ConvolutionBackward input gradients;
 * ldm/modules/diffusionmodules/openaimodel.py:214-232 in_layers / out_layers).  Same parameter block and epilogue; A is the
 * operand of dp_pack_weight_wino, U[(ky*4 + pos)*C + c][lda]; batches / a_kc / tile_counters must be unset; ksplit > 1 splits the
 * (channel chunk, kernel row) loop over blockIdx.z with partials in ws and the reduction launch of dp_conv_gemm.
 * dp_conv_wino_supported returns the K-chunk width the kernel would use (16 / 8) or 0 when the shape is not taken
 * (W a power of two in 4..256, channel counts per concat source multiples of 8, 3x3 / stride 1 / pad 1). */
int dp_conv_wino(const dp_conv_gemm_params* p, void* stream);
int dp_conv_wino_supported(const dp_conv_gemm_params* p);
/* the reduction launch of a split-K convolution (ksplit > 1, no tile_counters): out = epilogue(sum_z ws[z][m][pix]), ascending z */
int dp_conv_splitk_epilogue(const dp_conv_gemm_params* p, void* stream);
/* mode 0: forward operand (K = Ci, columns = co); mode 1: input-gradient operand (K = Co, columns = ci, taps flipped).
 * dst holds 12 * K * ld floats. */
int dp_pack_weight_wino(const float* W, int Co, int Ci, int mode, float* dst, int ld, void* stream);

/* The same convolution as a TWO-DIMENSIONAL Winograd F(2x2, 3x3) implicit GEMM (csrc/winograd2d.hip, round 6): 16 multiplies per
 * 2x2 output tile and channel instead of 36 -- 4/9 of dp_conv_gemm, 2/3 of dp_conv_wino.  One workgroup = 64 output channels x 32
 * tiles (128 output pixels = whole image rows) x 16 positions, the four ROWS of the position matrix on the four wavefronts; input
 * transform at fragment-read time, output transform in registers (columns) and through LDS (rows).  Replaces the same call sites as
 * dp_conv_wino (diffusers/models/resnet.py:606,630 and their input gradients; ldm/modules/diffusionmodules/openaimodel.py:214-232).
 * Same parameter block, epilogue operands and split-K contract; A is dp_pack_weight_wino2d's operand U[(pos*K + k)][lda],
 * pos = 4 i + j of U = G g G^T (dst holds 16 * K * ld floats; mode 0 forward, mode 1 input gradient with both tap axes flipped).
 * Takes W a power of two in 4..256 (beyond 64 pixels a block is a 2-row x 64-column segment with a halo tile), H even, channel counts
 * per concat source in multiples of 8, even image strides. */
int dp_conv_wino2d(const dp_conv_gemm_params* p, void* stream);
int dp_conv_wino2d_supported(const dp_conv_gemm_params* p);
int dp_pack_weight_wino2d(const float* W, int Co, int Ci, int mode, float* dst, int ld, void* stream);

/* The same convolution as Winograd F(4, 3) along W (csrc/winograd43.hip): HALF the multiplies of dp_conv_gemm (6 per 4 outputs x 3
 * taps), for the forwards that keep nothing for a backward -- the sampling loops (diffusers/pipelines/ddim/pipeline_ddim.py:101-116,
 * pipelines/ddpm/pipeline_ddpm.py:87-96) and the CFG sampler of the LDM importance pass (ldm_exp/prune_ldm.py:111-118,
 * ldm/models/diffusion/ddim.py:165-203).  fp32 error vs fp64 ~1e-6 (F(2, 3): ~3e-7): not used for scored gradients.  Same parameter
 * block, epilogue and split-K contract as dp_conv_wino; A is dp_pack_weight_wino43's operand U[(ky*6 + pos)*C + c][lda]
 * (forward flavour only; dst holds 18 * Ci * ld floats).  Takes W a power of two in 4..256, channel counts per concat source in
 * multiples of 8, pixel count / image strides in multiples of 4, 16-byte aligned tensors. */
int dp_conv_wino43(const dp_conv_gemm_params* p, void* stream);
int dp_conv_wino43_supported(const dp_conv_gemm_params* p);
int dp_pack_weight_wino43(const float* W, int Co, int Ci, float* dst, int ld, void* stream);

/* D[m][c][tap] = alpha * sum_pix A[m][pix] * X(pix, c, tap)  -- weight gradients (split over pixels, one kernel tap
 * per workgroup) and the k-contiguous batched products of attention (P.V, dQ).  Replaces the weight-gradient half of
 * ConvolutionBackward / AddmmBackward reached from loss.backward() (ddpm_prune.py:102) and torch.bmm
 * (attention_processor.py:446).
 * A element (m, pix=(img,r)) at A + z*a_bs + img*a_img_stride + m*HoWo + r;  NCOLS = number of channels c.
 * batched = 1: blockIdx.z = batch, output out[z*o_bs + m*ldo + c]  (ntaps must be 1);
 * batched = 0: blockIdx.z = split*ntaps + tap, partial sums to out[split*o_bs + m*ldo + c*ntaps + tap]
 *              (reduce with dp_splitk_reduce), or direct (+accumulate) when splits == 1.
 * merge != 0 (few channels on one side, conv_in / conv_out): one tile holds all C*ntaps columns; with bit 1 the plain
 *              rows are the layer INPUT and the gathered operand is dy with mirrored taps (stride-1 'same' convs only).
 * nn.Linear forward y[n][o] = sum_i x[n][i] W[o][i] + b[o] (embeddings.py:192-212, resnet.py:611) is the batched form
 * with one batch: A = x, X1 = W (both row-major, reduction index contiguous), col_bias = b. */
typedef struct dp_nt_gemm_params {
    const float* A; long long a_bs; long long a_img_stride;
    const float* X1; const float* X2; long long x_bs;
    unsigned a_bytes, x1_bytes, x2_bytes, _pad0;   /* readable extent of A / X1 / X2 (per batch), each < 2 GiB */
    dp_conv_geom g;
    int M, C, NCOLS, ntaps, P, batches, splits, p_per_split, tile, batched;   /* tile: 0 = 128x128, 1 = 64x128, 2 = 64x64 */
    float* out; long long o_bs; int ldo; int accumulate;
    float alpha; int merge;                /* merge: bit 0 = taps folded into the columns (NCOLS = C*ntaps), bit 1 = mirrored taps */
    long long ocs;                         /* merge: output element (row, c, tap) at row*ldo + c*ocs + tap */
    long long o_tap_stride; int o_col_stride; int xcd;       /* 0 = defaults (1, ntaps); (M*NCOLS, 1) with ldo = NCOLS gives
                                              tap-major partials [tap][m][c] whose stores are contiguous */
    /* xcd != 0 (fast weight-gradient kernel only): XCD-aware workgroup order, the workgroups of one split share an L2 */
    const float* col_bias;                 /* optional [NCOLS]: added per output column by split 0 (nn.Linear bias), or NULL */
} dp_nt_gemm_params;
int dp_nt_gemm(const dp_nt_gemm_params* p, void* stream);

/* Weight gradient of the same convolutions by the transposed algorithm (3 taps from output pairs: 4 multiplies instead of 6 per
 * pair, kernel row and channel pair), csrc/winograd.hip wgrad_wino_kernel.  Parameter block as for dp_nt_gemm's weight-gradient
 * launches (A = dy, X1 / X2 = the layer input, ntaps = 9, tap-major split-K partials); the K range is counted in 32-pixel tiles
 * over P/32 + 1 tiles, so splits * p_per_split must cover P + 32.  Replaces the ConvolutionBackward weight gradient of
 * diffusers/models/resnet.py:606,630 (conv1 / conv2).  Shapes: 3x3 / stride 1 / pad 1, W a power of two in 8..256, H*W a power of
 * two >= 64, P % 32 == 0, c_split % 64 == 0 with two sources. */
int dp_wgrad_wino(const dp_nt_gemm_params* p, void* stream);
int dp_wgrad_wino_supported(const dp_nt_gemm_params* p);

/* The same weight gradient by the TWO-dimensional transposed algorithm F(3x3, 2x2) (csrc/wgrad2d.hip, round 6): 16 multiplies per
 * (2x2 block of output gradients, m, c) instead of 36 -- 2/3 of dp_wgrad_wino's.  One workgroup = a 64 x 32 (m, c) tile of all 16
 * position matrices over a range of 64-pixel K tiles; the nine taps are folded out of the positions in the epilogue and written as
 * the same tap-major split-K partials (dp_splitk_reduce_taps).  Parameter block as for dp_wgrad_wino; splits * p_per_split must cover
 * P, counted in 64-pixel tiles.  Shapes: W in {8, 16, 32}, H even, H*W a power of two >= 64, P % 64 == 0, c_split % 32 == 0 with two
 * sources.  Replaces the same ConvolutionBackward weight gradients (diffusers/models/resnet.py:606,630). */
int dp_wgrad_wino2d(const dp_nt_gemm_params* p, void* stream);
int dp_wgrad_wino2d_supported(const dp_nt_gemm_params* p);

/* out[i] (+)= sum_s ws[s*stride + i], fixed summation order (deterministic split-K epilogue). */
int dp_splitk_reduce(const float* ws, long long stride, int splits, float* out, long long n, int accumulate, void* stream);
/* same for tap-major partials ws[s][tap][mc] -> out[mc][ntaps] (the torch weight layout) */
int dp_splitk_reduce_taps(const float* ws, long long stride, int splits, float* out, long long mc, int ntaps,
                          int accumulate, void* stream);

/* Weight packing for dp_conv_gemm's A operand.  W is a torch Conv2d/Linear weight [Co][Ci][taps].
 * mode 0 (forward): dst[(tap*Ci + ci)*ld + co] = W[co][ci][tap],            ld = roundup4(Co)
 * mode 1 (dgrad)  : dst[(tap*Co + co)*ld + ci] = W[co][ci][taps-1-tap],     ld = roundup4(Ci)
 * dst must hold taps*K*ld floats; padding columns are written as zeros. */
int dp_pack_weight(const float* W, int Co, int Ci, int taps, int mode, float* dst, int ld, void* stream);

/* Dropout of the finetune step (nn.Dropout in ResnetBlock2D, resnet.py:628, and Attention.to_out[1],
 * attention_processor.py:457; probability set by utils.set_dropout, utils.py:26-29, ddpm_train.py:380-382).
 * The mask is a pure function of (seed, site, step, logical element index) through Philox4x32-10 -- see csrc/dp_common.h --
 * so the backward kernels regenerate it instead of reading a stored mask.  thr24 = ceil(p * 2^24) (0 disables),
 * scale = 1/(1-p), site = a stable id of the layer, step = optimizer step, n_off = global index of the shard's first
 * image (masks do not depend on how the batch is sharded over ranks). */
typedef struct dp_dropout {
    unsigned thr24; float scale; unsigned long long seed; unsigned site; unsigned step; long long n_off;
    const unsigned* step_dev;   /* optional DEVICE counter read instead of `step`: a captured / replayed finetune step must not bake
                                 * the optimizer step into its kernel arguments (dp_set_step_scalars writes it) */
} dp_dropout;

/* Standalone forms: y[i] = x[i] * m(i) (in place allowed; forward and backward are the same map), and the bare mask
 * multipliers m(i) in {0, scale} for logical elements [idx0, idx0 + n) (parity tests export masks through it).
 * x is [N][per_img] with image stride x_img_stride (logical index = (n_off + n) * per_img + r). */
int dp_dropout_apply(const float* x, long long x_img_stride, float* y, long long y_img_stride, int N, long long per_img,
                     const dp_dropout* drop, void* stream);
int dp_dropout_mask(float* m, long long idx0, long long n, const dp_dropout* drop, void* stream);
/* out[i] = standard-normal draw of logical element idx0 + i: Philox4x32-10 on counter (idx >> 2 lo, hi, stream_id, step), key
 * seed, Box-Muller on the word pairs (see csrc/elementwise.hip).  Replaces the device-RNG draws of the LDM importance pass
 * (ldm/models/diffusion/ddim.py:122 `torch.randn(shape, device=device)`, ddpm.py:1023 `torch.randn_like(x_start)`) with a
 * stream that does not depend on how the latents are sharded over ranks. */
int dp_randn_philox(float* out, long long idx0, long long n, unsigned long long seed, unsigned stream_id, unsigned step,
                    void* stream);

/* GroupNorm (+ optional SiLU) (+ optional dropout of the result, drop may be NULL) forward over a (virtually
 * concatenated) NCHW tensor.
 * Replaces F.group_norm + F.silu: resnet.py:596-598,622-628, unet_2d.py:302-303, attention_processor.py:433.
 * Channel c < c_split is read from x1 (image stride x1_img_stride), else from x2.  y is contiguous
 * [N][C][HW] with image stride y_img_stride.  stats[(n*G+g)*2 + {0,1}] = {mean, rstd}. */
int dp_groupnorm_silu_fwd(const float* x1, const float* x2, int c_split, long long x1_img_stride, long long x2_img_stride,
                          const float* gamma, const float* beta, int N, int C, int HW, int G, float eps, int silu,
                          float* y, long long y_img_stride, float* stats, const dp_dropout* drop, void* stream);

/* Backward of the above (drop: the same descriptor as in the forward; dz is masked on the fly).  dz = gradient w.r.t. the (SiLU'd) output, image stride dz_img_stride.
 * dx (image stride dx_img_stride) = gn_backward(dz) (+ add1) (+ add2); add tensors carry their own image
 * strides.  pws[(n*C + c)*2 + {0,1}] = per-image sums {sum dy, sum dy*xhat} (reduce over n with
 * dp_colsum_accum to obtain dbeta / dgamma).  Replaces NativeGroupNormBackward + SiluBackward. */
int dp_groupnorm_silu_bwd(const float* x1, const float* x2, int c_split, long long x1_img_stride, long long x2_img_stride,
                          const float* gamma, const float* beta, const float* stats, const float* dz, long long dz_img_stride,
                          int N, int C, int HW, int G, int silu,
                          float* dx, long long dx_img_stride,
                          const float* add1, long long add1_img_stride, const float* add2, long long add2_img_stride,
                          float* pws, const dp_dropout* drop, float* rows, void* stream);
/* rows (optional, [N][C]): rows[n*C + c] = sum_hw dx[n][c][hw] -- the bias / time-embedding-projection gradient rows of the
 * layer that produced x fall out of the same pass (otherwise a separate dp_rowsum_nc re-reads dx). */

/* The same two operations for FEW, LARGE groups (e.g. 256x256 images at batch 4: N*G = 128 groups of 1 MB): the work unit
 * is one of `slices` equal slices of one channel plane, partial statistics go through ws and are combined in a fixed
 * order (Chan's parallel variance in the forward).  Requires HW % (4*slices) == 0 and 16-byte aligned planes.
 * ws: forward >= N*C*slices*2 floats, backward >= N*C*slices*2 + N*G*2 floats. */
int dp_groupnorm_silu_fwd_split(const float* x1, const float* x2, int c_split, long long x1_img_stride, long long x2_img_stride,
                                const float* gamma, const float* beta, int N, int C, int HW, int G, float eps, int silu,
                                float* y, long long y_img_stride, float* stats, int slices, float* ws,
                                const dp_dropout* drop, void* stream);
int dp_groupnorm_silu_bwd_split(const float* x1, const float* x2, int c_split, long long x1_img_stride, long long x2_img_stride,
                                const float* gamma, const float* beta, const float* stats, const float* dz,
                                long long dz_img_stride, int N, int C, int HW, int G, int silu, float* dx,
                                long long dx_img_stride, const float* add1, long long add1_img_stride, const float* add2,
                                long long add2_img_stride, float* pws, int slices, float* ws, const dp_dropout* drop,
                                void* stream);

/* out[c*ostride] (+)= sum_n ws[(n*C + c)*wstride + woff]   (deterministic, n ascending) */
int dp_colsum_accum(const float* ws, int N, int C, int wstride, int woff, float* out, int accumulate, void* stream);

/* The same for n independent items in one launch (per 80 items): dst[c] (+)= sum_n src[(n*C + c)*wstride + woff].  The host
 * queues the bias / GroupNorm-parameter gradient sums of a whole backward pass and flushes them together.
 * With ld != 0 element (n, c) sits at src[(n*ld + c)*wstride + woff] (a column slice of a wider matrix). */
typedef struct dp_colsum_item {
    const float* src; float* dst; int N, C, wstride, woff, accumulate, ld;   /* ld: row pitch in elements, 0 = C */
} dp_colsum_item;
int dp_colsum_accum_batch(const dp_colsum_item* items, int n, void* stream);

/* rows[n*C + c] = sum_hw x[n*img_stride + c*HW + hw]  (bias / time-embedding-projection gradients) */
int dp_rowsum_nc(const float* x, long long img_stride, int N, int C, int HW, float* rows, void* stream);

/* y = silu(x) ; dx = dy * silu'(x)   (resnet.py:611 nonlinearity(temb), embeddings.py:206 act) */
int dp_silu_fwd(const float* x, float* y, long long n, void* stream);
int dp_silu_bwd(const float* x, const float* dy, float* dx, long long n, int accumulate, void* stream);

/* y = a*x + b*y  (elementwise) */
int dp_axpby(const float* x, float a, float* y, float b, long long n, void* stream);
/* strided plane copy / add: dst[img*d_stride + i] (+)= src[img*s_stride + i], i < per_img */
int dp_copy_strided(const float* src, long long s_stride, float* dst, long long d_stride, int N, long long per_img, int accumulate, void* stream);

/* Row softmax over the last dim (in place allowed).  attention_processor.py:350-353. */
int dp_softmax_fwd(const float* s, float* p, long long rows, int cols, void* stream);
/* Fused attention forward (no score tensor): for every image n < N and head h < heads
 *   o[n][h*dv + c][i] = sum_j v[n][h*dv + c][j] * softmax_j(scale * sum_c' q[n][h*d + c'][i] * k[n][h*d + c'][j]),  i, j < T.
 * Replaces get_attention_scores (baddbmm + softmax) + bmm of attention_processor.py:415-470 / the einsum-softmax-einsum of
 * ldm/modules/attention.py:168-193 for forwards that keep nothing for a backward (sampling).  Tensors are channel-major
 * ([N, C, T], tokens contiguous; head h = channel rows [h*d, (h+1)*d) -- head_to_batch_dim as a view); *_bs = elements between
 * consecutive images (q / k / v may be channel slices of one fused QKV tensor).  d = query / key width per head, dv = value
 * width per head (they differ after pruning), any d, dv >= 1 with dp_attention_fwd_supported(T, d, dv) != 0 (T a multiple of 32,
 * max(d, dv) <= 640); other shapes return hipErrorInvalidValue -- the caller keeps the three-launch path for those. */
typedef struct dp_attention_params {
    const float* q; const float* k; const float* v; float* o;
    long long q_bs, k_bs, v_bs, o_bs;
    int N, heads, d, dv, T;
    float scale;
    int variant;                           /* 0 = library's choice; 1 / 2 force the plain / the software-pipelined schedule
                                              (same arithmetic, different instruction order) */
    int _pad;
} dp_attention_params;
int dp_attention_fwd(const dp_attention_params* p, void* stream);
int dp_attention_fwd_supported(int T, int d, int dv);
/* ds = scale * p * (dp - sum_j p_j dp_j)   (SoftmaxBackward followed by the baddbmm alpha) */
int dp_softmax_bwd(const float* p, const float* dp, float* ds, long long rows, int cols, float scale, void* stream);

/* Sinusoidal timestep embedding, out[b][dim] (embeddings.py:22-62).  t given as float (timesteps.float()). */
int dp_timestep_embedding(const float* t, int B, int dim, int flip_sin_to_cos, float freq_shift, float max_period, float* out, void* stream);

/* noisy = sqrt(acp[t_b]) * x0 + sqrt(1 - acp[t_b]) * noise   (scheduling_ddpm.py:408-429) */
int dp_add_noise(const float* x0, const float* noise, const float* acp, const int64_t* t, int B, long long per_img, float* out, void* stream);

/* loss partial sums + dOut for the eps-prediction loss.
 * dout = gscale * (out - noise);  partial[block] = sum (out-noise)^2 over the block's slice.
 * F.mse_loss (ddpm_prune.py:101): gscale = 2/numel;  sum-CHW/mean-B loss (ddpm_train.py:459): gscale = 2/B. */
int dp_mse_fwd_bwd(const float* out, const float* noise, long long n, float gscale, float* dout, float* partial, int nblocks,
                   const float* stop_state, void* stream);
/* Distillation loss (functions/losses.py:17-31) with S = out (student), T = teacher (frozen teacher's output), e = noise:
 * dout = gscale * (w_kd (S - T) + w_eps (S - e));  partial[block] = sum (S-T)^2, partial[nblocks + block] = sum (S-e)^2 over the
 * block's slice (dp_mse_fwd_bwd's fixed grid and summation order: (w_kd, w_eps) = (0, 1) reproduces it bit for bit).
 * dp_kd_terms: terms[3] = [w_kd kd + w_eps eps, kd, eps], kd / eps = scale * sum of their partials (dp_sum_partials' order). */
int dp_kd_fwd_bwd(const float* out, const float* teacher, const float* noise, long long n, float w_kd, float w_eps, float gscale,
                  float* dout, float* partial, int nblocks, void* stream);
int dp_kd_terms(const float* partial, int nblocks, float w_kd, float w_eps, float scale, float* terms, void* stream);
/* Diff-Pruning early exit kept on the device (ddpm_prune.py:104-106: `if loss > loss_max: loss_max = loss; if loss <
 * loss_max * thr: break`, fp32 as the reference's 0-d tensors).  state = [loss_max, stopped, executed steps] (zero-initialised),
 * losses[k] = loss of executed step k.  Once stopped, dp_mse_fwd_bwd(stop_state = state) produces dOut = 0, so timesteps the
 * host enqueued past the stop are exact no-ops on the accumulated gradients; the host polls `stopped` every few steps.
 * dp_zero_if_stopped cancels an already computed dOut (ddpm_exp flavour: threshold test before the backward pass). */
int dp_early_exit_update(const float* loss, float thr, float* state, float* losses, int max_steps, void* stream);
int dp_zero_if_stopped(float* x, long long n, const float* state, void* stream);
/* The same state machine in the LDM script's form (ldm_exp/prune_ldm.py:104,124-129: `max_loss = -1` -- the caller initialises
 * state[0] = -1 -- `if loss > max_loss: max_loss = loss; if loss / max_loss < thres: break`, the quotient rounded to fp32).
 * thr < 0 never stops (plain Taylor pass: losses are only recorded). */
int dp_early_exit_update_ratio(const float* loss, float thr, float* state, float* losses, int max_steps, void* stream);
/* dst[0] = scale * sum_i partial[i]  (single block, fixed order) */
int dp_sum_partials(const float* partial, int n, float scale, float* dst, void* stream);

/* dx[n][c][h][w] = sum of the 2x2 block of dy (backward of nearest x2 upsampling, resnet.py:155) */
int dp_downsum2x2(const float* dy, long long dy_img_stride, int N, int C, int H, int W, float* dx, long long dx_img_stride, void* stream);

/* y[n][c][2h+i][2w+j] = x[n][c][h][w]: nearest x2 upsampling, materialised (F.interpolate(scale_factor=2.0,
 * mode="nearest") in Upsample2D, diffusers/models/resnet.py:155; openaimodel.py Upsample).  The conv that follows is then a
 * plain stride-1 conv (dp_conv_gemm with ups = 0) instead of the gather form (ups = 1). */
int dp_upsample2x(const float* x, long long x_img_stride, int N, int C, int H, int W, float* y, long long y_img_stride, void* stream);

/* dx[n][c][2i+ph][2j+pw] = q[(2ph+pw)*q_class_stride + n*q_img_stride + (c*Ho+i)*Wo + j] (+ add[n][c][2i+ph][2j+pw]).
 * Assembles the input gradient of a stride-2 3x3 convolution (Downsample2D, diffusers/models/resnet.py:218; openaimodel.py
 * Downsample) from its four parity classes, each of which is a small stride-1 convolution over dy with the 4 / 2 / 2 / 1 taps
 * that can reach that parity (dp_conv_gemm): 9/4 taps per input pixel instead of the 9 of the zero-inserted form.
 * `add` (optional) is the skip-connection gradient the caller adds to dx (ConvolutionBackward + AddBackward in autograd). */
int dp_interleave2x2(const float* q, long long q_class_stride, long long q_img_stride, int N, int C, int Ho, int Wo,
                     const float* add, long long add_img_stride, float* dx, long long dx_img_stride, void* stream);

/* q[(2ph+pw)*q_class_stride + n*q_img_stride + (c*Ho+i)*Wo + j] = y[n][c][2i+ph][2j+pw]: inverse of dp_interleave2x2. */
int dp_deinterleave2x2(const float* y, long long y_img_stride, int N, int C, int Ho, int Wo, float* q,
                       long long q_class_stride, long long q_img_stride, void* stream);

/* Upsample2D = F.interpolate(nearest, x2) + Conv2d(3x3, pad 1) (diffusers/models/resnet.py:131-166; openaimodel.py Upsample)
 * as four 2x2 convolutions on the low-resolution input, one per parity class (ph, pw) of the output position, top / left
 * padding (1 - ph, 1 - pw); mathematically the same function with 16 instead of 36 multiply-adds per low-resolution pixel.
 * dp_ups_weff: weff[4][M][2][2] from w[M][3][3] (M = Cout*Cin), sums of the taps that read the same source pixel;
 * dp_ups_wfold: gw[M][3][3] (+)= the transposed map applied to the class weight gradients gweff[4][M][2][2]. */
int dp_ups_weff(const float* w, long long M, float* weff, void* stream);
int dp_ups_wfold(const float* gweff, long long M, float* gw, int accumulate, void* stream);

/* The same Upsample2D convolution in NINE multiplies per low-resolution pixel and channel pair (csrc/ups9.hip):
 * U = G w G^T per (co, ci), G = [1 0 0; 1 1 1; 0 0 1] (dp_ups9_u: u[M][3][3] from w[M][3][3], M = Cout*Cin).
 * dp_ups9_dgrad: dx[n][ci][i][j] (+)= sum_co sum_{a,b} U[co][ci][a][b] T[a][b], T = R p R^T of the 4x4 patch p of the
 * high-resolution dy[N][K][2H][2W] at rows 2i-1 .. 2i+2 / columns 2j-1 .. 2j+2 (zero outside), R = [0 -1 0 1; 0 1 1 0; 1 0 -1 0]:
 * the gradient w.r.t. the LOW-resolution input, read from dy as it is (no de-interleave pass).
 * U: dp_pack_weight(u, mode 1) -- exactly 9 * K * ldu floats, 16-byte aligned; M = Cin, K = Cout; H, W: the low resolution.
 * dy / dx: contiguous images at dy_img_stride / dx_img_stride floats; dy_bytes: readable extent from dy, below 2 GiB.
 * tile: pixels per workgroup, 0 = 32 (8 channels per K tile), 1 = 64, 2 = 128 (4 channels): one fixed-order sum per output, the
 * same bits from run to run; tiles 1 and 2 sum in the same order, tile 0 in its own.
 * dp_ups9_dgrad returns hipErrorInvalidValue for what dp_ups9_dgrad_supported refuses. */
typedef struct dp_ups9_params {
    const float* U; const float* dy; float* dx;
    long long dy_img_stride, dx_img_stride;
    unsigned u_bytes, dy_bytes;
    int ldu, N, M, K, H, W, accumulate, tile;
} dp_ups9_params;
int dp_ups9_u(const float* w, long long M, float* u, void* stream);
int dp_ups9_dgrad(const dp_ups9_params* p, void* stream);
int dp_ups9_dgrad_supported(const dp_ups9_params* p);
/* dp_ups9_fwd: y[n][co][2i+ph][2j+pw] = (A^T M A)[ph][pw] (+ bias[co]), M[a][b] = sum_ci U[co][ci][a][b] V[a][b], V = the 3x3
 * low-resolution patch of x[N][K][H][W] round (i, j) (zero outside) after (p0 - p1, p1, p2 - p1) along each axis, A = [1 0; 1 1; 0 1]:
 * the forward pass written straight to the high-resolution y[N][M][2H][2W] (no class staging buffer, no interleave pass).
 * U: dp_pack_weight(u, mode 0) -- exactly 9 * K * ldu floats, 16-byte aligned; M = Cout, K = Cin; H, W: the low resolution.
 * x / y: contiguous images at x_img_stride / y_img_stride floats, y 8-byte aligned and y_img_stride even; x_bytes: readable extent
 * from x, below 2 GiB; bias: M floats or NULL.  One workgroup per 64 output channels x 64 pixels, one fixed-order sum per output: the
 * same bits from run to run.  dp_ups9_fwd checks all of this itself and returns hipErrorInvalidValue, launching nothing, for what it does
 * not take (ops.ups9_fwd_shape_ok is the host's restatement of that rule). */
typedef struct dp_ups9_fwd_params {
    const float* U; const float* x; const float* bias; float* y;
    long long x_img_stride, y_img_stride;
    unsigned u_bytes, x_bytes;
    int ldu, N, M, K, H, W;
} dp_ups9_fwd_params;
int dp_ups9_fwd(const dp_ups9_fwd_params* p, void* stream);
/* The WEIGHT gradient of the same convolution in nine products (csrc/ups9_wgrad.hip), two launches:
 * dp_ups9_wgrad: ws[split][a][b][co][ci] = sum over the split's pixels of dM[n][co][a][b][i][j] V[n][ci][a][b][i][j], dM = A D A^T of
 * the 2x2 block D of the high-resolution dy[N][Co][2H][2W] at rows 2i, 2i+1 / columns 2j, 2j+1 (A = [1 0; 1 1; 0 1]), V as in
 * dp_ups9_fwd from the low-resolution x[N][Ci][H][W].  K tiles of 16 low-resolution pixels numbered over all images; split s takes the
 * tiles [s * tiles_per_split, (s + 1) * tiles_per_split): splits * tiles_per_split covers all of them and no split is empty.
 * dp_ups9_wgrad_reduce: dU = the splits added in ascending order, gw[Co][Ci][3][3] (+)= G^T dU G (accumulate != 0: +=).
 * dy / x: contiguous images at dy_img_stride / x_img_stride floats, dy 8-byte aligned and dy_img_stride even; dy_bytes / x_bytes: readable
 * extents, below 2 GiB.  ws: ws_floats >= splits * 9 * Co * ld floats, row pitch ld >= Ci.  No atomics, one fixed-order sum per output:
 * the same bits from run to run.  Both launchers check all of this themselves (dp_ups9_wgrad_supported, csrc/ups9_wgrad.hip) and return
 * hipErrorInvalidValue, launching nothing, for what they do not take (ops.ups9_wgrad_shape_ok is the host's restatement of that rule). */
typedef struct dp_ups9_wgrad_params {
    const float* dy; const float* x; float* ws; float* gw;
    long long dy_img_stride, x_img_stride, ws_floats;
    unsigned dy_bytes, x_bytes;
    int N, Co, Ci, H, W, splits, tiles_per_split, ld, accumulate;
} dp_ups9_wgrad_params;
int dp_ups9_wgrad(const dp_ups9_wgrad_params* p, void* stream);
int dp_ups9_wgrad_reduce(const dp_ups9_wgrad_params* p, void* stream);

/* Taylor-importance reductions  (ddpm_exp/torch_pruning/importance.py:375-434).
 * Weight viewed as [R][C][T]; dim = 0: out[r] = sum_{c,t} f(w*g); dim = 1: out[c] = sum_{r,t} f(w*g);
 * mode 0: f = (w g)^2 (vendored), mode 1: f = |w g| (sum_abs), mode 2: signed sum then |.| (abs_sum),
 * mode 3: out[i] = |w_i g_i| (GroupNorm member; R = channels, C = T = 1),
 * mode 4: f = g^2 (FisherImportance, importance.py:715-781), mode 5: signed sum, no |.| (FullTaylorImportance,
 * importance.py:482-548: the absolute value is taken after the members are summed).
 * out[i] = (accumulate ? out[i] : 0) + value.  `scratch` (>= C*T floats) is required for dim == 1. */
int dp_wg_reduce(const float* w, const float* g, int R, int C, int T, int dim, int mode, float* out, int accumulate,
                 float* scratch, void* stream);

/* dst[i] += src[idx[i]], i < n : adds one member's channel sums into the group score (importance.py:427-428). */
int dp_gather_add(const float* src, const int64_t* idx, int n, float* dst, void* stream);

/* Batched forms for the prune tail (one launch pair per GROUP of coupled layers instead of two or three per member):
 * dp_group_score = the dp_wg_reduce of every member + the dp_axpby / dp_gather_add chain that folds them into the group
 * score (importance.py:375-434), same per-member arithmetic and member order, hence the same bits.  Member i views its
 * weight / gradient as [R][C][T]; dim / mode as in dp_wg_reduce (mode 3 = GroupNorm member, R channels); its per-channel
 * vector lives at scratch[full_off ...] (R or C floats), dim-1 members also need C*T floats at scratch[col_off ...];
 * idx_off >= 0: score[j] += vector[idx[idx_off + j]], idx_off < 0: identity.  blk0 is filled by the launcher.
 * dp_slice_batch = function.py:85-146,168-207,274-302 for every tensor of a group: dst = the kept channels (keep[keep_off ..
 * keep_off + n_keep), ascending) of src along `dim` of its [R][C][T] view.  blk0 / nblk are filled by the launcher. */
typedef struct dp_score_member {
    const float* w; const float* g;
    int R, C, T, dim, mode, blk0;
    long long full_off, col_off, idx_off;
} dp_score_member;
int dp_group_score(const dp_score_member* members, int n, int n0, const int64_t* idx, float* scratch, float* score, void* stream);
typedef struct dp_slice_item {
    const float* src; float* dst;
    int R, C, T, dim, n_keep, blk0, nblk, _pad;
    long long keep_off;
} dp_slice_item;
int dp_slice_batch(const dp_slice_item* items, int n, const int64_t* keep, void* stream);

/* Global pruning (metapruner.py:256-297; csrc/prune_global.hip): every group scored on the unpruned weights, one threshold.
 * dp_score_groups = dp_group_score for ALL groups in one launch pair.  `entries` (host, n of them) is the member table: the
 * members of a group are adjacent, in dp_group_score's member order, and share score_off (the group's offset into the
 * concatenated score vector) and n0; the groups tile scores[0 .. n_scores) in table order.  The launcher checks every offset
 * against idx_len / scratch_len / n_scores, fills m.blk0 and copies the table to table_dev (device, n entries), from where the
 * kernels read it.  scores[score_off + j] has the bits dp_group_score gives score[j] for that group.
 * dp_select_smallest: thres = the k-th smallest (1 <= k <= n) of scores[0 .. n), exactly; -0.0 counts as +0.0 (a zero threshold
 * is returned as +0.0).  group_off (host, groups + 1 ascending offsets, [0] = 0, [groups] = n) cuts the vector into groups.
 * out_dev / out_host: 2 + groups + n ints -- [0] the threshold's bits, [1] the NaN count, [2 + g] the number of positions of
 * group g with score <= thres, [2 + groups + group_off[g] + j] the j-th of them (ascending, relative to the group; the rest of
 * the group's region is 0).  The call copies out_dev to out_host and waits for the stream; any NaN -> hipErrorInvalidValue.
 * `work`: dp_select_smallest_workspace(n, groups) bytes of device memory. */
typedef struct dp_score_entry {
    dp_score_member m;
    long long score_off;
    int n0, _pad;
} dp_score_entry;
int dp_score_groups(dp_score_entry* entries, int n, dp_score_entry* table_dev, const int64_t* idx, long long idx_len,
                    float* scratch, long long scratch_len, float* scores, long long n_scores, void* stream);
long long dp_select_smallest_workspace(long long n, int groups);
int dp_select_smallest(const float* scores, long long n, const long long* group_off, int groups, long long k, void* work,
                       long long work_bytes, int* out_dev, int* out_host, void* stream);

/* The data-free magnitude criteria (importance.py:18-126 MagnitudeImportance, :154-219 LAMPImportance; csrc/magnitude.hip), every
 * group of the network in one launch pair.
 * dp_magnitude_rows: member i views its weight as [R][C][T]; rows[row_off + j], j < n0, = sum |w|^p over the other dimensions of
 * channel idx[idx_off + j] (idx_off < 0: channel j) along `dim`; root != 0: that sum to the power 1 / p (torch.norm(., p)).
 * fold > 1 (needs an index list of n0 * fold entries): value j sums the channels idx[idx_off + j * fold .. + fold), in list order,
 * before the root -- the `view` of importance.py:188-195 for an in-channel member that holds its group's channels `fold` times.
 * p == 1 and p == 2 take |w| and w * w, any other p > 0 the device powf.  `members` (host, n of them) is checked against idx_len
 * and rows_len, gets blk0 filled in and is copied to table_dev (device, n entries), from where the kernel reads it; a channel
 * index outside the layer is clamped into it.  Two calls give the same bits.
 * dp_magnitude_finish: group i owns `members` rows of n0 floats, adjacent from rows[row_off] in member order, and
 * scores[score_off .. score_off + n0); the groups tile scores[0 .. n_scores) in table order.  One workgroup per group:
 *   reduction   0 sum, 1 mean, 2 max, 3 prod, 4 first -- over the rows, in member order;
 *   normalizer  0 none, 1 / sum, 2 (x - min) / (max - min + 1e-8), 3 / mean, 4 / max, 5 (x - mean) / (std + 1e-8), std unbiased,
 *               two passes; IEEE divisions (an all-zero group under 3 gives NaN); min / max return NaN when the group holds one;
 *   lamp        0 off; else a = descending argsort (ties by ascending channel), q = sorted / inclusive scan of sorted (the scan in
 *               index order, as torch.cumsum on the host); 1: scores[j] = q[a[j]] (importance.py:211-219 as vendored),
 *               2: scores[a[k]] = q[k] (the paper's order).
 * n0 > dp_magnitude_max_width() (the LDS the sort needs) is refused with hipErrorInvalidValue. */
typedef struct dp_mag_member {
    const float* w;
    int R, C, T, dim, n0, blk0, fold, _pad;
    long long idx_off, row_off;
} dp_mag_member;
typedef struct dp_mag_group {
    long long row_off, score_off;
    int n0, members;
} dp_mag_group;
int dp_magnitude_max_width(void);
int dp_magnitude_rows(dp_mag_member* members, int n, dp_mag_member* table_dev, const int64_t* idx, long long idx_len,
                      float p, int root, float* rows, long long rows_len, void* stream);
int dp_magnitude_finish(const dp_mag_group* groups, int n, dp_mag_group* table_dev, const float* rows, long long rows_len,
                        int reduction, int normalizer, int lamp, float* scores, long long n_scores, void* stream);

/* Fused finetune update over flat buffers (ddpm_train.py:462-469, training_utils.py:201-216):
 *   g *= clip_coef (clip_coef read from device: min(1, max_norm/(norm+1e-6)));  Adam;  EMA with constant decay. */
int dp_sumsq_partials(const float* x, long long n, float* partial, int nblocks, void* stream);
/* The per-step scalars of a REPLAYED finetune step live on the device: hyper[0..2] = {lr, bc1 = 1 - b1^step, bc2 = 1 - b2^step}
 * (floats, the values the host computes for dp_adam_ema), hyper[3] = the optimizer step as an unsigned (the dropout masks'
 * `step`, read through dp_dropout.step_dev).  dp_set_step_scalars is the ONE launch per step that carries them by value;
 * dp_adam_ema_dev is dp_adam_ema reading {lr, bc1, bc2} from hyper.  (ddpm_train.py:462-469; LR schedule: optimization.py:282) */
int dp_set_step_scalars(float* hyper, float lr, float bc1, float bc2, unsigned step, void* stream);
int dp_adam_ema_dev(float* p, const float* g, float* m, float* v, float* ema, long long n, const float* clip_coef,
                    const float* hyper, float b1, float b2, float eps, float ema_decay, void* stream);
int dp_clip_coef(const float* partial, int n, float max_norm, float* norm_out, float* coef_out, void* stream);
int dp_adam_ema(float* p, const float* g, float* m, float* v, float* ema, long long n, const float* clip_coef,
                float lr, float b1, float b2, float eps, float bc1, float bc2, float ema_decay, void* stream);

/* LDM finetune update (ldm_exp/ldm/models/diffusion/ddpm.py:1372-1381; ldm/modules/ema.py) over flat buffers, one pass:
 *   torch.optim.AdamW, single tensor, in torch's order:  p *= p_scale (= 1 - lr wd);  m += (g - m) one_minus_b1;
 *   v = b2 v + one_minus_b2 g g;  p -= step_size (= lr / bc1) * m / (sqrt(v) / sqrt_bc2 + eps);
 *   then iff ema != NULL LitEma's  s -= (1 - ema_decay) (s - p).  Every scalar is formed by the host in double and rounded to
 *   fp32 once (ema_decay: LitEma's fp32 decay after warm-up).  clip_coef: NULL, or a device scalar the gradient is scaled by.
 *   16-byte accesses when all buffers are 16-byte aligned, 4-byte accesses for the n % 4 tail; any n (long long indexing). */
int dp_adamw_ema(float* p, const float* g, float* m, float* v, float* ema, long long n, const float* clip_coef,
                 float p_scale, float one_minus_b1, float b2, float one_minus_b2, float sqrt_bc2, float eps,
                 float step_size, float ema_decay, void* stream);
/* LitEma's update alone (ldm/modules/ema.py:40-44): s[i] -= one_minus_decay * (s[i] - p[i]), i < n, rounded after every operation --
 * the EMA half of dp_adamw_ema bit for bit (one_minus_decay = the fp32 difference 1 - decay).  For the batches of a gradient-
 * accumulation window that end without an optimizer step.  16-byte accesses when both pointers are 16-byte aligned, 4-byte
 * accesses for the n % 4 tail and for unaligned views; any n (long long indexing, grid-stride under dp_adamw_ema's cap). */
int dp_ema_update(float* s, const float* p, long long n, float one_minus_decay, void* stream);
/* The stage study's snapshot (csrc/stage.hip): out[i] = ((srcs[0][i] + srcs[1][i]) + srcs[2][i]) + srcs[3][i], i < n, for k = 1 .. 4
 * sources: plain fp32 adds in exactly that order, the sum a chain of dp_axpby(src, 1, out, 1) forms.  `srcs`: k device pointers in
 * HOST memory; they are passed on by value in the kernel arguments (nothing is staged, nothing has to outlive the call).  No source
 * is written.  hipErrorInvalidValue when `out` overlaps a source, k is out of range or a pointer is null; n <= 0 is a no-op.
 * 16-byte accesses when `out` and every source are 16-byte aligned and n >= 4, 4-byte accesses for the n % 4 tail and for
 * unaligned views; any n (long long indexing, grid-stride beyond 4096 blocks: dp_ema_update's rule). */
int dp_fold_sum(float* out, const float* const* srcs, int k, long long n, void* stream);
/* Gradient of an embedding lookup: dW[ids[b], :] += dctx[b, :] for b = 0 .. B-1 (B <= 4096), the rows of a repeated id added in
 * ascending b -- bitwise reproducible, no float atomics.  ids: int64, every id in [0, rows of dW) (checked by the caller). */
int dp_embedding_bwd(const long long* ids, const float* dctx, int B, int D, float* dW, void* stream);

/* DDIM update (scheduling_ddim.py:324-370, eta = 0 or with supplied noise):
 *   x0 = clamp((x - sqrt(1-a_t) eps)/sqrt(a_t), +-clip_range);  prev = sqrt(a_prev) x0 + sqrt(1-a_prev-std^2) eps (+ std*noise) */
int dp_ddim_step(const float* x, const float* eps, const float* vnoise, float a_t, float a_prev, float std, int clip,
                 float clip_range, float* out, long long n, void* stream);

/* DDPM ancestral update (scheduling_ddpm.py:312-406, epsilon prediction):
 *   x0 = clamp((x - sqrt_b_t eps)/sqrt_a_t, +-clip_range);  prev = c_x0 * x0 + c_xt * x (+ sigma * noise)
 * The 0-d coefficient arithmetic stays on the host in the reference's own fp32 operation order. */
int dp_ddpm_step(const float* x, const float* eps, const float* vnoise, float sqrt_a_t, float sqrt_b_t, float c_x0,
                 float c_xt, float sigma, int clip, float clip_range, float* out, long long n, void* stream);

/* ---- The head / body / tail access rule of the elementwise step launchers below (dp_denoise_step, dp_cfg_denoise_step,
 * dp_dpm_solver_step, dp_unipc_step, dp_pndm_step, dp_repaint_step, dp_repaint_undo, dp_sigma_step and its two companions, dp_kdpm2_step, dp_lms_step, dp_x0_step and its two companions, dp_deis_step, dp_dpm_single_step; csrc/dp_headtail_plan.h decides, csrc/dp_headtail.h loops).
 * When every pointer in use (a NULL or unread one does not count) shares one 4-byte-aligned phase modulo 16, a scalar head of
 * 0 .. 3 elements brings all of them to 16 bytes: the n4 = (n - head) / 4 groups after it take 16-byte accesses, the head and the
 * n - head - 4 n4 tail elements 4-byte ones.  Otherwise every access is 4 bytes (head = n).  Any n: long long indexing, one lane
 * per group (or per scalar element, whichever are more) in blocks of 256 lanes, grid-stride beyond the launcher's
 * DP_*_MAX_BLOCKS.  The results do not depend on the width. */

/* One update of the ddpm_exp sampler (csrc/sampler.hip; ddpm_exp/functions/denoising.py) over n fp32 elements, one pass:
 *   mode 0, generalized_steps:23-29:  x0 = (x - eps * p0) / p1;              next = p2 * x0 + p3 * z + p4 * eps
 *           (p0 .. p4 = sqrt(1 - a_t), sqrt(a_t), sqrt(a_next), c1, c2; p5 unread)
 *   mode 1, ddpm_steps:53-65:         x0 = clamp(p0 * x - p1 * eps, -1, 1);  next = (p2 * x0 + p3 * x) / p4 + p5 * z
 *           (p0 .. p5 = sqrt(1 / a_t), sqrt(1 / a_t - 1), sqrt(a_next) * beta_t, sqrt(1 - beta_t) * (1 - a_next), 1 - a_t, sigma)
 * every operation rounded separately, in the reference's order, with a true division; the scalars are the host's 0-d fp32
 * arithmetic.  z == NULL: no noise term (eta = 0, where c1 is exactly 0; the t = 0 mask).  x0_out != NULL: the x0 prediction is
 * written in the same pass.  `next` may be `x`; x0_out aliases nothing.  Accesses: the head / body / tail rule above, at most
 * DP_DENOISE_MAX_BLOCKS blocks. */
#define DP_DENOISE_MAX_BLOCKS 4096
int dp_denoise_step(const float* x, const float* eps, const float* z, int mode, float p0, float p1, float p2, float p3, float p4,
                    float p5, float* next, float* x0_out, long long n, void* stream);
/* fp32 x [N][C][H][W] (image stride x_img_stride floats) -> uint8 out [N][H][W][C], the inverse of dp_u8_to_float:
 *   v = rescaled ? clamp((x + 1) / 2, 0, 1) : clamp(x, 0, 1)      (inverse_data_transform, ddpm_exp/datasets/__init__.py:177-186)
 *   out = (unsigned char) clamp(v * 255 + 0.5, 0, 255), the multiply and the add rounded separately: the torch fp32 expression
 *   bit for bit.  torchvision is absent from the build machine and from the reference tree: save_image's formula is recalled,
 *   and parity with torchvision itself is unpinned. */
int dp_image_to_u8(const float* x, long long x_img_stride, int N, int C, int H, int W, int rescaled, unsigned char* out,
                   void* stream);

/* One model evaluation of the ldm_exp samplers (csrc/ldm_sampler.hip; ldm_exp/ldm/models/diffusion/ddim.py:165-203 and
 * plms.py:173-236) over n fp32 elements, one pass, in the reference's operation order:
 *   e_g  = e_u + scale * (e_c - e_u)                 e_c == NULL: the unguided path, e_g = e_u.  With the [2B, C, H, W] eps of
 *                                                    forward_cfg_pair, e_c = e_u + n: both halves are read in place
 *   e'   = e_g                                       order 0
 *        | (3 e_g - h1) / 2                          order 1   (h1 the newest stored guided eps, h3 the oldest)
 *        | (23 e_g - 16 h1 + 5 h2) / 12              order 2
 *        | (55 e_g - 59 h1 + 37 h2 - 9 h3) / 24      order 3
 *        | (h1 + e_g) / 2                            order 4   (PLMS's first step: h1 = e_t, e_g = e_t_next)
 *   x0   = (x - s1m * e') / sqrt_a_t
 *   next = (sqrt_a_prev * x0 + c_dir * e') + (sigma * z) * temperature          z == NULL: no noise term
 * every operation rounded separately, true divisions; the scalars are the host's (ldm_sampler.sampling_tables).  x0_out / eg_out
 * != NULL: the x0 prediction / the guided eps e_g are written in the same pass.  `next` may be `x`; x0_out and eg_out alias
 * nothing.  A history pointer the order does not read may be NULL.  Accesses: the head / body / tail rule above, at most
 * DP_DENOISE_MAX_BLOCKS blocks. */
int dp_cfg_denoise_step(const float* x, const float* e_u, const float* e_c, float scale, int order, const float* h1, const float* h2,
                        const float* h3, float s1m, float sqrt_a_t, float sqrt_a_prev, float c_dir, float sigma, float temperature,
                        const float* z, float* next, float* x0_out, float* eg_out, long long n, void* stream);

/* One step of the multistep DPM-Solver (csrc/dpm_solver.hip; diffusers/schedulers/scheduling_dpmsolver_multistep.py:346-395 epsilon
 * prediction, :420-442, :466-501, :557-589) over n fp32 elements, one pass, in the reference's operation order:
 *   m0 = data_pred ? (x - sigma_s * e) / alpha_s : e              dpmsolver++ (data prediction) | dpmsolver (noise prediction)
 *   order 1:  x' = kx * x - k0 * m0
 *   order 2:  D1 = ir0 * (m0 - m1);                                          x' = (kx * x - k0 * m0) - k1 * D1
 *   order 3:  D10 = ir0 * (m0 - m1); D11 = ir1 * (m1 - m2); d = D10 - D11;
 *             D1 = D10 + q * d; D2 = iq * d;                                 x' = ((kx * x - k0 * m0) - k1 * D1) - k2 * D2
 * every operation rounded separately, a true division; the scalars are the host's 0-d fp32 arithmetic on the alpha_t / sigma_t /
 * lambda_t tables (ir0 = 1 / r0, ir1 = 1 / r1, q = r0 / (r0 + r1), iq = 1 / (r0 + r1)); where the reference ADDS c * D1 (heun, the
 * third-order dpmsolver++) the host passes k1 = -c, which gives the same bits.  Fields an order / algorithm does not read are ignored.
 * m1 (the previous converted output) and m2 (the one before) may be NULL below their order.  m0_out, the converted output of this
 * step, is always written (for dpmsolver it is a copy of e: the history owns its buffers).
 * Aliases: `x_next` may be `x` itself, and `m0_out` may be `m1` or `m2` itself -- the oldest buffer of a ring of solver_order history
 * buffers that this very step still reads: each lane reads every input of its elements before it writes any of them, and no
 * other lane touches them.  Any other overlap between an output and another buffer is hipErrorInvalidValue, as are a null required
 * pointer and an order outside 1 .. 3; n <= 0 is a no-op.
 * Accesses: the head / body / tail rule above, at most DP_DPM_SOLVER_MAX_BLOCKS blocks. */
#define DP_DPM_SOLVER_MAX_BLOCKS 4096
typedef struct dp_dpm_solver_coef {
    float sigma_s, alpha_s;             /* convert (data_pred only) */
    float kx, k0, k1, k2;               /* the update's coefficients */
    float ir0, ir1, q, iq;              /* the difference quotients of orders 2 and 3 */
} dp_dpm_solver_coef;
int dp_dpm_solver_step(const float* x, const float* e, const float* m1, const float* m2, int order, int data_pred,
                       const dp_dpm_solver_coef* coef, float* x_next, float* m0_out, long long n, void* stream);

/* One step of the UniPC multistep scheduler (csrc/unipc.hip; diffusers/schedulers/scheduling_unipc_multistep.py:256-305 epsilon
 * prediction, :307-410 UniP, :412-516 UniC, chained as :518-600 chains them) over n fp32 elements, one pass:
 *   m_new = predict_x0 ? (x_pred - sigma_s * e) / alpha_s : e                       x_pred: the sample handed to `step`, uncorrected
 *   corrector, pc in 0 (absent) .. 3, on the OLD history m0 (newest), m1, m2 and on x_last (the sample before the last predictor):
 *     D_i = (m_i - m0) / c_rk<i>, i = 1 .. pc - 1;   dt = m_new - m0
 *     x_c = (c_cx * x_last - c_c0 * m0) - c_cB * ([c_rho1 * D_1 [+ c_rho2 * D_2]] + c_rho_last * dt)
 *   predictor, pp in 1 .. 3, on the NEW history (m_new, m0, m1), from xs = pc ? x_c : x_pred:
 *     E_1 = (m0 - m_new) / p_rk1;  E_2 = (m1 - m_new) / p_rk2
 *     x_next = (p_cx * xs - p_c0 * m_new) [- p_cB * (p_rho1 * E_1 [+ p_rho2 * E_2])]       (pp 2: the host passes p_rho1 = 0.5)
 * every operation rounded separately, true divisions; the two history products of a third-order sum are added first, left to right,
 * then (corrector) c_rho_last * dt is added to their sum.  The scalars are the host's 0-d fp32 arithmetic on the alpha_t / sigma_t /
 * lambda_t tables.  Fields an instantiation does not read are ignored.
 * Reads: e, x_pred, x_last (pc > 0), and the first max(pc, pp - 1) of m0, m1, m2; the others may be NULL.  Writes: m_new (always; a
 * copy of e without predict_x0: the history owns its buffers), x_c (pc > 0: the next step's last_sample; may be NULL at pc 0), x_next.
 * Aliases: `m_new` may be `m0`, `m1` or `m2` itself (the oldest buffer of a ring of solver_order history buffers, which this very
 * step may still read), `x_c` may be `x_last` itself, `x_next` may be `x_pred` itself: each lane reads every input of its elements
 * before it writes any of them, and no other lane touches them.  Any other overlap between an output and another buffer is
 * hipErrorInvalidValue, as are a null required pointer, pc outside 0 .. 3 and pp outside 1 .. 3: nothing is launched.  n <= 0 is a no-op.
 * Accesses: the head / body / tail rule above, at most DP_UNIPC_MAX_BLOCKS blocks. */
#define DP_UNIPC_MAX_BLOCKS 4096
typedef struct dp_unipc_coef {
    float sigma_s, alpha_s;             /* convert (predict_x0 only) */
    float c_cx, c_c0, c_cB;             /* corrector: the first-order part and the factor of the sum */
    float c_rk1, c_rk2, c_rho1, c_rho2, c_rho_last;
    float p_cx, p_c0, p_cB;             /* predictor */
    float p_rk1, p_rk2, p_rho1, p_rho2;
} dp_unipc_coef;
int dp_unipc_step(const float* e, const float* x_pred, const float* x_last, const float* m0, const float* m1, const float* m2,
                  int pc, int pp, int predict_x0, const dp_unipc_coef* coef, float* m_new, float* x_c, float* x_next, long long n,
                  void* stream);

/* One step of the PNDM scheduler (csrc/pndm.hip; diffusers/schedulers/scheduling_pndm.py:251-270 step_prk, :314-337 step_plms,
 * :358-399 _get_prev_sample) over n fp32 elements, one pass, in the reference's operation order.  e: the model output, x: the state
 * the update starts from (cur_sample in the Runge-Kutta stages), acc: the Runge-Kutta accumulator, h1 .. h3: older model outputs,
 * newest first.  The combined output m of each mode, and what the mode writes beside x_next:
 *   DP_PNDM_PRK0      m = e;  acc = c6 * e + 0;  hist_out = e        (the reference adds to a Python 0: -0 becomes +0)
 *   DP_PNDM_PRK1/2    m = e;  acc = acc + c3 * e                     (in place)
 *   DP_PNDM_PRK3      m = acc + c6 * e                               (acc is read only: the host forgets it)
 *   DP_PNDM_PLMS1     m = e;  hist_out = e
 *   DP_PNDM_PLMS_AVG  m = (e + h1) / 2                               (skip_prk_steps, the second call: e is not appended)
 *   DP_PNDM_PLMS2     m = (3 * e - h1) / 2;  hist_out = e
 *   DP_PNDM_PLMS3     m = ((23 * e - 16 * h1) + 5 * h2) / 12;  hist_out = e
 *   DP_PNDM_PLMS4     m = c24 * (((55 * e - 59 * h1) + 37 * h2) - 9 * h3);  hist_out = e
 * then, v_pred != 0:  m = sa * m + sb * x;  and always  x_next = sc * x - (d * m) / den.
 * Every operation rounded separately, true divisions; sa .. den are the host's 0-d fp32 arithmetic on the alphas_cumprod table
 * (sa = alpha_prod_t ** 0.5, sb = beta_prod_t ** 0.5, sc = sample_coeff, d = alpha_prod_t_prev - alpha_prod_t,
 * den = model_output_denom_coeff), c6 / c3 / c24 the doubles 1/6, 1/3, 1/24 rounded to fp32 once.  hist_out is a copy of e: the
 * caller's history owns its buffers.  A pointer the mode neither reads nor writes is ignored and may be NULL.
 * Aliases: `x_next` may be `x` itself, `acc` is one buffer updated in place, and `hist_out` may be `h1`, `h2` or `h3` itself -- the
 * oldest buffer of the caller's ring, which this very step may still read: each lane reads every input of its elements before it
 * writes any of them, and no other lane touches them.  Any other overlap between an output and another buffer is
 * hipErrorInvalidValue, as are a null pointer that the mode reads or writes and a mode outside 0 .. 8: nothing is launched.
 * n <= 0 is a no-op.  Accesses: the head / body / tail rule above, at most DP_PNDM_MAX_BLOCKS blocks. */
#define DP_PNDM_MAX_BLOCKS 4096
#define DP_PNDM_PRK0 0
#define DP_PNDM_PRK1 1
#define DP_PNDM_PRK2 2
#define DP_PNDM_PRK3 3
#define DP_PNDM_PLMS1 4
#define DP_PNDM_PLMS_AVG 5
#define DP_PNDM_PLMS2 6
#define DP_PNDM_PLMS3 7
#define DP_PNDM_PLMS4 8
typedef struct dp_pndm_coef {
    float sa, sb;                       /* the v-conversion (v_pred only) */
    float sc, d, den;                   /* formula (9) */
    float c6, c3, c24;                  /* fp32(1/6), fp32(1/3), fp32(1/24) */
} dp_pndm_coef;
int dp_pndm_step(const float* x, const float* e, float* acc, const float* h1, const float* h2, const float* h3, int mode, int v_pred,
                 const dp_pndm_coef* coef, float* x_next, float* hist_out, long long n, void* stream);

/* The two kernels of the RePaint scheduler (csrc/repaint.hip; diffusers/schedulers/scheduling_repaint.py:250-293 step, :303-318
 * undo_step) over n fp32 elements, one pass each, in the reference's operation order.
 * dp_repaint_step: x the state, e the model output, z the noise of this step, o the original image, m the mask (1 = known):
 *   x0  = (x - sb * e) / sa                       clamped to [-1, 1] when clip != 0; written to x0_out when that is not NULL
 *   u   = (sap * x0 + cd * e) + (noise != 0 ? sd * z : 0)      (the reference adds a Python 0: -0 becomes +0)
 *   k   = sap * o + s1 * z
 *   out = m * k + (1 - m) * u
 * Every operation rounded separately, a true division; the scalars are the host's 0-d fp32 arithmetic on the alphas_cumprod table
 * (sa = alpha_prod_t ** 0.5, sb = beta_prod_t ** 0.5, sap = alpha_prod_t_prev ** 0.5, s1 = (1 - alpha_prod_t_prev) ** 0.5,
 * cd = (1 - alpha_prod_t_prev - std_dev_t ** 2) ** 0.5, sd = std_dev_t = eta * variance ** 0.5).
 * The mask is not materialised: element i reads m[(i / m_outer) * m_stride + (i % m_inner)], 1 <= m_inner <= m_outer,
 * m_outer % m_inner == 0, m_stride >= 0 (and, with more than one image, m_stride == 0 or m_stride >= m_inner).  For data [B,C,H,W]:
 * a mask of the data's shape (n, 0, n); [B,1,H,W] (CHW, HW, HW); [1,1,H,W] (n, 0, HW); [1,C,H,W] (n, 0, CHW).  m_inner >= n is the
 * FULL form (16-byte loads of the mask, its pointer takes part in the head / body / tail rule above); any other is read with 4-byte
 * loads, also where a 16-byte group of the data straddles a plane or an image.
 * Aliases: `out` may be `x` itself.  Any other overlap between an output and another buffer (the mask's
 * ((n - 1) / m_outer) * m_stride + m_inner elements included), a null pointer other than x0_out and a mask geometry outside the above
 * are hipErrorInvalidValue: nothing is launched.  n <= 0 is a no-op.  At most DP_REPAINT_MAX_BLOCKS blocks.
 * dp_repaint_undo: x = a[i] * x + b[i] * z[i] for i = 0 .. k - 1 (a[i] = (1 - beta) ** 0.5, b[i] = beta ** 0.5), chained in registers,
 * each product and sum rounded separately: x is read once and written once.  1 <= k <= DP_REPAINT_UNDO_MAX; entries from k on are
 * ignored.  `out` may be `x` itself; any other overlap of `out` with `x` or a z[i], a null pointer among those read and k outside
 * the range are hipErrorInvalidValue. */
#define DP_REPAINT_MAX_BLOCKS 4096
#define DP_REPAINT_UNDO_MAX 8
typedef struct dp_repaint_coef {
    float sa, sb;                       /* the x0 prediction */
    float sap, s1;                      /* alpha_prod_t_prev ** 0.5, (1 - alpha_prod_t_prev) ** 0.5 */
    float cd, sd;                       /* the direction's factor, std_dev_t */
} dp_repaint_coef;
typedef struct dp_repaint_undo_coef {
    const float* z[DP_REPAINT_UNDO_MAX];
    float a[DP_REPAINT_UNDO_MAX];
    float b[DP_REPAINT_UNDO_MAX];
} dp_repaint_undo_coef;
int dp_repaint_step(const float* x, const float* e, const float* z, const float* o, const float* m, long long m_outer,
                    long long m_stride, long long m_inner, int clip, int noise, const dp_repaint_coef* coef, float* out,
                    float* x0_out, long long n, void* stream);
int dp_repaint_undo(const float* x, const dp_repaint_undo_coef* coef, int k, float* out, long long n, void* stream);

/* The three kernels of the sigma-space (k-diffusion) schedulers (csrc/sigma.hip; diffusers/schedulers/scheduling_euler_discrete.py
 * :305-349, scheduling_euler_ancestral_discrete.py:233-273, scheduling_heun_discrete.py:261-318) over n fp32 elements, one pass each,
 * in the reference's operation order.  The state is carried at scale sigma (up to 157 for the CIFAR schedule).
 * dp_sigma_step: x the sample, e the model output, z the noise, d1 the derivative DP_SIGMA_HEUN1 wrote, xs the sample it was handed.
 *   x0 from xh:  DP_SIGMA_EPSILON  xh - sig * e;   DP_SIGMA_V  e * c_out + xh / c_den;   DP_SIGMA_SAMPLE (EULER only)  e
 *   DP_SIGMA_EULER      xh = z ? x + (z * s_noise) * k : x;  d = (xh - x0) / sig;  x_next = xh + d * dt;             aux_out = x0
 *   DP_SIGMA_ANCESTRAL  xh = x;  d = (x - x0) / sig;  x_next = (x + d * dt) + z * sigma_up;                           aux_out = x0
 *   DP_SIGMA_HEUN1      xh = x;  d = (x - x0) / sig;  x_next = x + d * dt;                                            aux_out = d
 *   DP_SIGMA_HEUN2      xh = x;  d2 = (x - x0) / sig;  d = (d1 + d2) / 2;  x_next = xs + d * dt                       (no aux_out)
 * Every operation rounded separately, true divisions; the scalars are the host's 0-d fp32 arithmetic on the sigma table: sig =
 * sigma_hat (EULER, HEUN1), sigma (ANCESTRAL), sigma_next (HEUN2); k = (sigma_hat^2 - sigma^2) ** 0.5; c_out = -s / (s^2 + 1) ** 0.5
 * and c_den = s^2 + 1 for s = sig (EULER: s = sigma, also with churn, as the reference has it); dt; sigma_up.  z == NULL in EULER: no
 * churn.  A pointer the mode neither reads nor writes is ignored and may be NULL.
 * Aliases: `x_next` may be `x` itself, and in HEUN2 `xs` itself: each lane reads every input of its elements before it writes any
 * of them, and no other lane touches them.  Any other overlap between an output and another buffer is hipErrorInvalidValue, as are
 * a null pointer that the mode reads or writes, a mode outside 0 .. 3, a type outside 0 .. 2 and DP_SIGMA_SAMPLE outside EULER:
 * nothing is launched.  n <= 0 is a no-op.
 * dp_sigma_scale: out = x / c (scale_model_input; c = (sigma^2 + 1) ** 0.5 from the host).  `out` may be `x` itself.
 * dp_sigma_add_noise: out[b][i] = x0[b][i] + z[b][i] * sigma[b] for B images of `per` elements, sigma a device vector of B fp32
 * values; `out` overlaps nothing.
 * Accesses: the head / body / tail rule above, at most DP_SIGMA_MAX_BLOCKS blocks. */
#define DP_SIGMA_MAX_BLOCKS 4096
#define DP_SIGMA_EULER 0
#define DP_SIGMA_ANCESTRAL 1
#define DP_SIGMA_HEUN1 2
#define DP_SIGMA_HEUN2 3
#define DP_SIGMA_EPSILON 0
#define DP_SIGMA_V 1
#define DP_SIGMA_SAMPLE 2
typedef struct dp_sigma_coef {
    float s_noise, k;                   /* the churn (EULER with z) */
    float sig;                          /* the sigma of the conversion and of the derivative */
    float c_out, c_den;                 /* the v-conversion (DP_SIGMA_V only) */
    float dt, sigma_up;                 /* the update; sigma_up: ANCESTRAL only */
} dp_sigma_coef;
int dp_sigma_step(const float* x, const float* e, const float* z, const float* d1, const float* xs, int mode, int pred,
                  const dp_sigma_coef* coef, float* x_next, float* aux_out, long long n, void* stream);
int dp_sigma_scale(const float* x, float c, float* out, long long n, void* stream);
int dp_sigma_add_noise(const float* x0, const float* z, const float* sigma, long long B, long long per, float* out, void* stream);

/* The step kernels of the rest of the sigma-space family (csrc/kdiff.hip; diffusers/schedulers/scheduling_k_dpm_2_discrete.py
 * :252-305, scheduling_k_dpm_2_ancestral_discrete.py:264-324, scheduling_lms_discrete.py:299-330) over n fp32 elements, one pass each,
 * in the reference's operation order.  x the sample, e the model output.
 *   x0:  DP_KDIFF_EPSILON  x - sig * e;   DP_KDIFF_V  e * c_out + x / c_den;   DP_KDIFF_SAMPLE (dp_lms_step only)  e
 * dp_kdpm2_step: one call of KDPM2DiscreteScheduler or KDPM2AncestralDiscreteScheduler.  xs: the sample the first-order call was
 * handed, NULL in first-order state; z: the noise, given only for the ancestral class's second-order call.
 *   d = (x - x0) / sig;  r = (xs ? xs : x) + d * dt;  x_next = z ? r + z * sigma_up : r
 * Three shapes (first, second, second + noise) x two types: six instantiations.  It writes no derivative and no x0: 4 streams read at
 * most, 1 written.  sig = sigma_hat in first-order state, sigma_interpol in second-order state; c_out = -sig / (sig^2 + 1) ** 0.5 and
 * c_den = sig^2 + 1; dt = sigma_interpol - sigma_hat, then sigma_next (ancestral: sigma_down) - sigma_hat.
 * Aliases: `x_next` may be `x` itself or `xs` itself.  Any other overlap, a null x, e, coef or x_next, z without xs and a type outside
 * 0 .. 1 are hipErrorInvalidValue: nothing is launched.
 * dp_lms_step: one linear-multistep call.  d1 .. d3: the previous derivatives, newest first; those beyond `order` are not read and may
 * be NULL.
 *   d = (x - x0) / sig;  acc = c0 * d;  acc = acc + c1 * d1;  ... (`order` terms, in that order);  x_next = x + acc
 *   d_new = d;  x0_out = x0
 * Orders 1 .. 4 x three types: twelve instantiations.  c0 .. c3: the host's integrals of the Lagrange basis over [sigma, sigma_next],
 * each rounded to fp32 once.
 * Aliases: `x_next` may be `x` itself.  d_new and x0_out overlap nothing that the call reads, nor each other, nor x_next.  Any other
 * overlap, a null pointer that the order reads or writes, an order outside 1 .. 4 and a type outside 0 .. 2 are
 * hipErrorInvalidValue: nothing is launched.
 * Both: every operation rounded separately, true divisions, n <= 0 is a no-op.
 * Accesses: the head / body / tail rule above, at most DP_KDIFF_MAX_BLOCKS blocks. */
#define DP_KDIFF_MAX_BLOCKS 4096
#define DP_KDIFF_EPSILON 0
#define DP_KDIFF_V 1
#define DP_KDIFF_SAMPLE 2
typedef struct dp_kdpm2_coef {
    float sig;                          /* the sigma of the conversion and of the derivative */
    float c_out, c_den;                 /* the v-conversion (DP_KDIFF_V only) */
    float dt, sigma_up;                 /* the update; sigma_up: with z only */
} dp_kdpm2_coef;
typedef struct dp_lms_coef {
    float sig;                          /* the sigma of the conversion and of the derivative */
    float c_out, c_den;                 /* the v-conversion (DP_KDIFF_V only) */
    float c0, c1, c2, c3;               /* the multistep coefficients, newest derivative first; those beyond `order` are not read */
} dp_lms_coef;
int dp_kdpm2_step(const float* x, const float* e, const float* xs, const float* z, int pred, const dp_kdpm2_coef* coef,
                  float* x_next, long long n, void* stream);
int dp_lms_step(const float* x, const float* e, const float* d1, const float* d2, const float* d3, int order, int pred,
                const dp_lms_coef* coef, float* x_next, float* d_new, float* x0_out, long long n, void* stream);

/* x0 forming, dynamic thresholding and the DDPM / DDIM update for epsilon, sample and v-prediction models (csrc/threshold.hip;
 * diffusers/schedulers/scheduling_ddpm.py:278-310, :355-401, scheduling_ddim.py:205-237, :334-385) over B images of n fp32 elements.
 * sa, sb: the host's fp32 alpha_prod_t ** 0.5 and beta_prod_t ** 0.5.
 *   model DP_X0_PRED_EPSILON: x0 = (x - sb m) / sa, eps = m;  _SAMPLE: x0 = m, eps = (x - sa x0) / sb from the untreated x0;
 *   _V: x0 = sa x - sb m, eps = sa m + sb x.  Every operation rounded on its own, true divisions.
 *
 * dp_x0_abs_quantile: stats[b] = (v_lo, v_hi, quantile, s) of image b: v_lo, v_hi the order statistics lo and hi (0-based,
 * hi = lo or lo + 1 < n) of the row's |x0|, exact (-0 counts as +0, a NaN as the largest key); quantile = fma(w, v_hi - v_lo, v_lo)
 * for w < 0.5, fma(w - 1, v_hi - v_lo, v_hi) otherwise (torch.quantile's lerp; lo, hi, w: the rank the host formed as torch does),
 * NaN for a row that holds a NaN; s = clamp(quantile, 1, max_value) as torch.clamp (a NaN stays, max_value < 1 gives max_value).
 * route DP_X0_ROUTE_LDS: one workgroup per image, the row in LDS, n <= DP_THRESHOLD_LDS_MAX; _MULTI: any n < 2^31, per-image digit
 * histograms in ws (dp_x0_abs_quantile_workspace(B, n) bytes), x0 recomputed in each of the five passes over x and m; _AUTO: by n.
 * x may be NULL for a sample model.  Nothing is read back; two calls give the same bits.
 *
 * dp_x0_step: one pass.  x0 treated as DP_X0_TREAT_NONE | _CLIP (clamp(x0, -range, range)) | _THRESHOLD (clamp(x0, -s, s) / s with
 * s = stats[b][3]); reclip: eps = (x - sa x0) / sb from the treated x0;
 *   DP_X0_MODE_DDIM: prev = c0 x0 + c1 eps [+ cz z];  _DDPM: prev = (c0 x0 + c1 x) + (cz z, or 0 without z);
 *   _CONVERT: prev = the treated x0 (z and x0_out must be NULL; x may be NULL for a sample model).
 * x0_out (optional) takes the treated x0.  prev may be x itself; any other overlap between an output (or stats) and another buffer is
 * hipErrorInvalidValue.  Accesses: the head / body / tail rule above within every row when n % 4 == 0 (then every row has the
 * first one's phase), 4-byte accesses otherwise; at most DP_X0_STEP_MAX_BLOCKS blocks of 256 lanes, strided over rows and images beyond.
 *
 * dp_x0_threshold_step: the LDS route of the quantile with the thresholded step applied by the same workgroup, ONE launch for
 * n <= DP_THRESHOLD_LDS_MAX; writes prev, x0_out (optional) and stats; the bits of dp_x0_abs_quantile followed by dp_x0_step. */
#define DP_THRESHOLD_LDS_MAX 16384
#define DP_X0_STEP_MAX_BLOCKS 4096
#define DP_X0_PRED_EPSILON 0
#define DP_X0_PRED_SAMPLE 1
#define DP_X0_PRED_V 2
#define DP_X0_TREAT_NONE 0
#define DP_X0_TREAT_CLIP 1
#define DP_X0_TREAT_THRESHOLD 2
#define DP_X0_MODE_DDIM 0
#define DP_X0_MODE_DDPM 1
#define DP_X0_MODE_CONVERT 2
#define DP_X0_ROUTE_AUTO 0
#define DP_X0_ROUTE_LDS 1
#define DP_X0_ROUTE_MULTI 2
typedef struct dp_x0_coef {
    float sa, sb;                       /* forming x0 and eps */
    float range;                        /* DP_X0_TREAT_CLIP */
    float c0, c1, cz;                   /* the update: factors of x0, of eps (DDIM) or x (DDPM), of z */
} dp_x0_coef;
long long dp_x0_abs_quantile_workspace(long long B, long long n);
int dp_x0_abs_quantile(const float* x, const float* m, long long B, long long n, int pred, float sa, float sb, long long lo,
                       long long hi, float w, float max_value, int route, void* ws, float* stats, void* stream);
int dp_x0_step(const float* x, const float* m, const float* z, const float* stats, int mode, int pred, int treat, int reclip,
               const dp_x0_coef* coef, float* prev, float* x0_out, long long B, long long n, void* stream);
int dp_x0_threshold_step(const float* x, const float* m, const float* z, int mode, int pred, int reclip, const dp_x0_coef* coef,
                         long long lo, long long hi, float w, float max_value, float* prev, float* x0_out, float* stats,
                         long long B, long long n, void* stream);

/* One step of the DEIS multistep scheduler and of the singlestep DPM-Solver (csrc/deis.hip; diffusers/schedulers/
 * scheduling_deis_multistep.py:240-405 and scheduling_dpmsolver_singlestep.py:291-519) for epsilon, sample and v-prediction models,
 * one pass, in the reference's operation order.  m: the model's output; sa, sb: alpha_t and sigma_t of the step's timestep.
 *   x0 = DP_X0_PRED_EPSILON: (x - sb m) / sa;  _SAMPLE: m;  _V: sa x - sb m          (the x0 of dp_x0_abs_quantile, bit for bit)
 *   stats != NULL: the data is [B, n] and x0 = clamp(x0, -s, s) / s with s = stats[4 b + 3], as dp_x0_abs_quantile wrote it;
 *   stats == NULL: no treatment, and the data is B n flat elements.
 * dp_deis_step keeps m0 = (x - sa x0) / sb -- always, for an epsilon model too (the reference converts there and back), and
 *   order 1:  x' = kx x - k0 m0
 *   order 2:  x' = at ((x / as0 + c1 m0) + c2 m1)
 *   order 3:  x' = at (((x / as0 + c1 m0) + c2 m1) + c3 m2)
 * dp_dpm_single_step keeps, data_pred (dpmsolver++): m0 = the treated x0;  !data_pred (dpmsolver; stats must be NULL):
 *   _EPSILON: m0 = m;  _SAMPLE: m0 = (x - sa m) / sb;  _V: m0 = sa m + sb x.   The conversion reads this call's x, the update the
 *   saved sample xs of the order-1 step this one completes (x itself at order 1):
 *   order 1:  x' = kx x - k0 m0
 *   order 2:  D1 = ir0 (m0 - m1);                                              x' = (kx xs - k0 m1) - k1 D1
 *   order 3:  D1_0 = ir1 (m1 - m2); D1_1 = ir0 (m0 - m2);           midpoint:  x' = (kx xs - k0 m2) - k1 D1_1
 *             heun: D1 = (r0 D1_0 - r1 D1_1) / dr; D2 = (2 (D1_1 - D1_0)) / dr; x' = ((kx xs - k0 m2) - k1 D1) - k2 D2
 * every operation rounded separately, true divisions; the scalars are the host's 0-d fp32 arithmetic (ir0 = 1 / r0, ir1 = 1 / r1,
 * dr = r0 - r1); where the reference ADDS c * D1 the host passes k1 = -c, which gives the same bits.  Fields an order does not read
 * are ignored.  m1 (the previous converted output) and m2 (the one before) may be NULL below their order; an input the step does
 * not read is not loaded and may be NULL: xs at order 1, and above order 1 x for an epsilon model under dpmsolver or a sample
 * model under dpmsolver++.  m0_out is always written.
 * Aliases: `x_next` may be `x` itself (dp_dpm_single_step: or `xs` itself), and `m0_out` may be the oldest history buffer the step
 * reads (m1 at order 2, m2 at order 3): each lane reads every input of its elements before it writes any of them, and no other lane
 * touches them.  Any other overlap between an output and another buffer (stats included) is hipErrorInvalidValue, as are a null
 * required pointer and an order outside 1 .. 3; B <= 0 or n <= 0 is a no-op.
 * Accesses: the head / body / tail rule above -- with stats within every row when n % 4 == 0 (then every row has the first one's
 * phase), 4-byte accesses otherwise; at most DP_DEIS_MAX_BLOCKS blocks of 256 lanes, strided over rows and images beyond. */
#define DP_DEIS_MAX_BLOCKS 4096
typedef struct dp_deis_coef {
    float sa, sb;                       /* convert */
    float kx, k0;                       /* order 1 */
    float at, as0, c1, c2, c3;          /* orders 2 and 3 */
} dp_deis_coef;
typedef struct dp_dpm_single_coef {
    float sa, sb;                       /* convert */
    float kx, k0, k1, k2;               /* the update's coefficients */
    float ir0, ir1, r0, r1, dr;         /* the difference quotients of orders 2 and 3 */
} dp_dpm_single_coef;
int dp_deis_step(const float* x, const float* m, const float* m1, const float* m2, const float* stats, int order, int pred,
                 const dp_deis_coef* coef, float* x_next, float* m0_out, long long B, long long n, void* stream);
int dp_dpm_single_step(const float* x, const float* xs, const float* m, const float* m1, const float* m2, const float* stats,
                       int order, int pred, int data_pred, int heun, const dp_dpm_single_coef* coef, float* x_next, float* m0_out,
                       long long B, long long n, void* stream);

/* ---- LDM (CompVis) transformer-block glue on channel-major tokens x[n][c][t]  (ldm_exp/ldm/modules/attention.py) ---- */
/* LayerNorm over the C channels of every token (attention.py:200-212 norm1/2/3); stats[(n*T+t)*2+{0,1}] = {mean, rstd}. */
int dp_layernorm_fwd(const float* x, long long x_img_stride, const float* gamma, const float* beta, int N, int C, int T,
                     float eps, float* y, long long y_img_stride, float* stats, void* stream);
/* dx = layernorm_backward(dy) (+ add);  pws[(n*C+c)*2+{0,1}] = {sum_t dy, sum_t dy*xhat} (reduce over n: dp_colsum_accum). */
int dp_layernorm_bwd(const float* x, long long x_img_stride, const float* gamma, const float* stats, const float* dy,
                     long long dy_img_stride, int N, int C, int T, float* dx, long long dx_img_stride, const float* add,
                     long long add_img_stride, float* pws, void* stream);
/* GEGLU (attention.py:37-46): in [N][2D][T] -> out [N][D][T] = in[:, :D] * gelu(in[:, D:]); half_plane = D*T. */
int dp_geglu_fwd(const float* in, int N, long long half_plane, float* out, void* stream);
int dp_geglu_bwd(const float* in, const float* dout, int N, long long half_plane, float* din, void* stream);
/* out[n][c][t] = x[n][c][t] + v[n*C + c]  (cross-attention over a single context token, attention.py:168-193) */
int dp_add_rowvec(const float* x, long long x_img_stride, const float* v, int N, int C, int T, float* out,
                  long long o_img_stride, void* stream);

/* q_sample with precomputed fp32 sqrt tables (ldm_exp/ldm/models/diffusion/ddpm.py q_sample / extract_into_tensor) */
int dp_q_sample(const float* x0, const float* noise, const float* sqrt_acp, const float* sqrt_1m_acp, const int64_t* t,
                int B, long long per_img, float* out, void* stream);
/* classifier-free guidance: out = e_uncond + scale * (e_cond - e_uncond)  (ldm_exp/ldm/models/diffusion/ddim.py:178-183) */
int dp_cfg_combine(const float* e_uncond, const float* e_cond, float scale, float* out, long long n, void* stream);

/* version / build info (smoke-tested by the CPU suite: library loads, symbols resolve) */
/* ---- FID / SSIM evaluation: fid_score.py:100-322, inception.py:16-340, compute_ssim.py:14-53 ---- */
/* k x k pooling, symmetric padding; mode 0: F.max_pool2d, mode 1: F.avg_pool2d(count_include_pad=False) (inception.py:238,266,300,333) */
int dp_pool2d(const float* x, long long x_img_stride, int N, int C, int H, int W, int k, int stride, int pad, int mode,
              float* y, long long y_img_stride, void* stream);
/* y = a * bilinear_resize(x -> Ho x Wo, align_corners = False) + b   (inception.py:147-154: 299 x 299, then 2x - 1) */
int dp_resize_bilinear(const float* x, long long x_img_stride, int N, int C, int H, int W, int Ho, int Wo, float a, float b,
                       float* y, void* stream);
/* out[n] = SSIM(x_n, y_n) as pytorch_msssim.ssim(x, y, data_range, size_average=False) (compute_ssim.py:43): 11-tap Gaussian,
 * sigma 1.5, valid filtering per channel, mean over the map, mean over channels.  x, y contiguous [N][C][H][W];
 * part: workspace of dp_ssim_workspace(N, C, H, W) floats.  dp_mse_per_image: compute_ssim.py:45. */
int dp_ssim(const float* x, const float* y, int N, int C, int H, int W, float data_range, float* part, float* out, void* stream);
long long dp_ssim_workspace(int N, int C, int H, int W);
int dp_mse_per_image(const float* a, const float* b, int N, long long per, float* out, void* stream);

/* ---- Inception Score / KID / precision-recall reductions (csrc/evalmetrics.hip; metrics.py calculate_metrics restates the
 * reference's ldm_exp/test_diffusion.py, a torch_fidelity.calculate_metrics call).  G is a block of a Gram matrix X . Y^T written by
 * dp_nt_gemm: `rows` x `cols` fp32 with row stride ldg floats (any alignment: 16-byte loads between a scalar head and tail per row).
 * Squared distances are d2_ij = max(xn_i + yn_j - 2 G_ij, 0), formed in double from the double norms of dp_em_row_norms2 and
 * rounded to fp32.  No atomics; every sum has a fixed order (two calls give the same bits).
 * dp_em_row_norms2: out[i] = sum_c x[i * ld + c]^2 in double.
 * dp_em_knn_merge: best [rows][k] fp32, ascending: replaced by the k smallest of its old contents (ignored when first != 0) and
 *   the block's d2_i*.  Fewer than k values so far leave +inf at the end.  1 <= k <= DP_EM_MAX_K, else hipErrorNotSupported.
 * dp_em_inside_ball: hit[i] |= any_j (d2_ij <= r2[j]); hit is int32 [rows], 0 / 1, initialised by the caller.
 * dp_em_poly_sums: out[0] = sum_ij (gamma g_ij + coef0)^degree and out[1] = the same over i == j, in double, where
 *   g_ij = sum_s G[s * slab_stride + i * ldg + j] over `slabs` partial Gram matrices (products over slices of the feature
 *   dimension), added in double in slab order; part is a workspace of 2 * nblocks doubles (nblocks workgroups take the rows
 *   round-robin, 1 <= nblocks <= 65536, degree >= 1).
 * dp_em_isc_rows: per row of the fp32 logits [n][c] (row stride ld), in double: lse[i] = log sum_c exp(l_ic) and
 *   h[i] = sum_c p_ic (l_ic - lse[i]), p = softmax.
 * dp_em_isc_colmeans: q[c] = mean over rows lo <= i < hi of exp(l_ic - lse[i]), in double. */
#define DP_EM_MAX_K 9
int dp_em_row_norms2(const float* x, long long n, int d, long long ld, double* out, void* stream);
int dp_em_knn_merge(const float* G, long long rows, long long cols, long long ldg, const double* xn, const double* yn, int k,
                    int first, float* best, void* stream);
int dp_em_inside_ball(const float* G, long long rows, long long cols, long long ldg, const double* xn, const double* yn,
                      const float* r2, int* hit, void* stream);
int dp_em_poly_sums(const float* G, int slabs, long long slab_stride, long long rows, long long cols, long long ldg, double gamma,
                    double coef0, int degree, double* part, int nblocks, double* out, void* stream);
int dp_em_isc_rows(const float* logits, long long n, int c, long long ld, double* lse, double* h, void* stream);
int dp_em_isc_colmeans(const float* logits, long long ld, const double* lse, long long lo, long long hi, int c, double* q,
                       void* stream);

/* Input pipeline (utils.py:8-58 get_dataset transforms; ddpm_exp/datasets/__init__.py:176-192 data_transform): decoded
 * uint8 images -> fp32 NCHW batch: x/255 (ToTensor), horizontal flip of image n with probability flip_thr24 / 2^24
 * (RandomHorizontalFlip; Philox decision on counter (n_off + n, 0, rng.site, rng.step), key rng.seed), mode 1:
 * (v - 0.5)/0.5 (Normalize(0.5, 0.5)), mode 2: 2v - 1 (rescaled), mode 0: none; dequant != 0: v/256*255 + u/256 first.
 * hwc != 0: src is [N][H][W][C], else [N][C][H][W].  rng: only seed / site / step / n_off are read. */
int dp_u8_to_float(const unsigned char* src, int hwc, int N, int C, int H, int W, float* out, long long out_img_stride,
                   int mode, unsigned flip_thr24, int dequant, const dp_dropout* rng, void* stream);

/* Nearest-codebook vector quantizer (csrc/vq.hip; diffusers VectorQuantizer.forward, vae.py:332-364, legacy=True, remap=None).
 * z [N][D][H][W] channel-major (image stride z_bs floats, HW = H * W, P = N * HW pixels), codebook E [K][D] row-major.
 * idx[p] = argmin_k sum_d (z[p,d] - E[k,d])^2 in the direct form, the lowest k among equal fp32 distances;
 * zq[p,d] = z[p,d] + (E[idx,d] - z[p,d]) in two fp32 roundings (image stride zq_bs); idx (int64 [P]) and partial (fp64
 * [dp_vq_blocks(P)]: per-block sums of (E[idx,d] - z[p,d])^2) may be NULL.  1 <= D <= 16 (else hipErrorNotSupported), K >= 1.
 * dp_vq_loss: loss[0] = (float)(scale * sum of the partials) in a fixed order -- (1 + beta) / (P * D) gives the reference's
 * mean + beta * mean.  Plain vector stores, no atomics: deterministic. */
int dp_vq_blocks(long long P);
int dp_vq_quantize(const float* z, long long z_bs, int D, int HW, long long P, const float* E, int K, float* zq, long long zq_bs,
                   long long* idx, double* partial, void* stream);
int dp_vq_loss(const double* partial, int nblocks, double scale, float* loss, void* stream);

/* The posterior of the KL autoencoder (csrc/vae.hip; diffusers DiagonalGaussianDistribution, vae.py:384-428) in one pass over the
 * moments [N][2 chw]: per image (image stride m_stride floats) the first chw floats are the mean, the next chw the log-variance.
 *   lv = clamp(logvar, -30, 20) (a NaN stays a NaN);  std = exp(0.5 lv);  var = exp(lv);
 *   z = scale * (mean + std * noise), each operation rounded on its own, the multiply by scale skipped when scale == 1;
 *   kl[n] = (float)(0.5 * sum_i (mean^2 + var - 1 - lv)), summed in double in a fixed order (two calls give the same bits).
 * Outputs logvar / std / var / z [N][chw] (contiguous) and kl [N] are optional: a NULL pointer skips one.  z needs noise [N][chw];
 * kl needs kl_ws, dp_gaussian_posterior_ws(N, chw) doubles (per-block partial sums, combined by a second launch).
 * No output may overlap an input or another output, except that z may be noise itself (a lane reads its elements before it writes
 * them): any other overlap is hipErrorInvalidValue and nothing is launched.  16-byte accesses when chw % 4 == 0, m_stride % 4 == 0 and
 * every pointer in use is 16-byte aligned, 4-byte accesses otherwise; at most DP_VAE_MAX_BLOCKS blocks of 256 lanes, grid-stride beyond. */
#define DP_VAE_MAX_BLOCKS 4096
long long dp_gaussian_posterior_ws(int N, long long chw);
int dp_gaussian_posterior(const float* moments, long long m_stride, int N, long long chw, const float* noise, float scale,
                          float* logvar, float* std, float* var, float* z, float* kl, double* kl_ws, void* stream);

/* One tile of a tiled encode / decode blended into its neighbours and cropped into the canvas, in one launch (csrc/vae.hip;
 * AutoencoderKL.blend_v, blend_h, the crop and the two torch.cat of autoencoder_kl.py:198-208, 236-249, 285-298).
 * b [planes][Hb][Wb] is updated in place; a [planes][Ha][Wb] is the (already blended) tile above, l [planes][Hb][Wl] the one to the
 * left, either may be NULL.  With ev / eh the blend extents the host formed (min(Ha, Hb, extent), min(Wl, Wb, extent)):
 *   v = b[y][x]
 *   a and y < ev:  v = a[Ha - ev + y][x] * w0(y, ev) + v * w1(y, ev)
 *   l and x < eh:  v = l[y][Wl - eh + x] * w0(x, eh) + v * w1(x, eh)
 * w1(k, e) = (float)(k / e) and w0(k, e) = (float)(1 - k / e) evaluated in double; every product and sum rounded on its own.
 * v is stored to b[y][x] and, where y < row_limit and x < row_limit, to out[plane][oy + y][ox + x] of the canvas
 * [planes][Hout][Wout] (out may be NULL).  A crop that leaves the canvas, an extent outside its tiles or b overlapping another
 * buffer is hipErrorInvalidValue and nothing is launched. */
int dp_tile_blend(float* b, int planes, int Hb, int Wb, const float* a, int Ha, int ev, const float* l, int Wl, int eh,
                  float* out, int Hout, int Wout, int oy, int ox, int row_limit, void* stream);

/* Native replay list (csrc/replay.hip): re-issue the kernels / memsets of a stream-captured step from a C loop.  The
 * reference's loop re-launches ~700 ATen kernels per timestep from Python (ddpm_prune.py:94-106); here one timestep is captured
 * once into a hipGraph (never instantiated: hipGraphLaunch of these graphs costs more host time than eager launches on this
 * stack), its nodes are read back, list-scheduled onto two streams along the captured dependency edges, and
 * dp_replay_launch re-issues them with hipLaunchKernel.  `graph`: hipGraph_t; it must outlive the list.
 * info[8] = nodes, kernels, memsets, memcpys, empty nodes, cross-stream waits, nodes on the side stream, events. */
int dp_replay_build(void* graph, void** out_handle);
int dp_replay_launch(void* handle, void* main_stream, void* side_stream);
int dp_replay_info(void* handle, int* info8);
int dp_replay_free(void* handle);

/* dp_pack_weight for many layers in one launch (blk0 / nblk are filled by the launcher).  mode 0 / 1 as dp_pack_weight;
 * mode 2 / 3: the dp_pack_weight_wino operand (mode - 2) of a 3x3 weight (taps = 9, dst holds 12 * K * ld floats);
 * mode 4 / 5: the dp_pack_weight_wino2d operand (mode - 4) of a 3x3 weight (taps = 9, dst holds 16 * K * ld floats). */
typedef struct dp_pack_item {
    const float* W; float* dst;
    int Co, Ci, taps, mode, ld, blk0, nblk, _pad;
} dp_pack_item;
int dp_pack_weight_batch(const dp_pack_item* items, int n, void* stream);

int dp_version(void);
/* Number of kernel launches this library has issued since it was loaded (host counter; bench.py reports launches per step).
 * Returned in place of an error code. */
long long dp_launch_count(void);
/* Names of the most recent kernel launches, oldest first: writes min(cap, launches so far, 256) pointers to static strings (the
 * kernel expression of the launch site with its template arguments, e.g. "(gn_bwd_wave_kernel<8, false, false>)",
 * "rowsum_kernel<true>") into out and returns how many.  With dp_launch_count() before and after a call, the last (after - before)
 * names are the launches of that call.  Host-side ring next to the counter; like the counter it is not thread-safe.
 * Returned in place of an error code. */
int dp_recent_launches(const char** out, int cap);

#ifdef __cplusplus
}
#endif
#endif
