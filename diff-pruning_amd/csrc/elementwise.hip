// HBM-bound elementwise / small-reduction kernels of the sweep: SiLU, softmax, timestep embedding,
// add_noise, eps-loss (+gradient), nearest-upsample backward, strided copies, DDIM update.
// All are grid-stride, coalesced (consecutive lanes -> consecutive floats), wave-shuffle reductions.
#include "dp_common.h"

unsigned long long dp_launches = 0;
const char* dp_launch_names[DP_LAUNCH_RING] = {};
extern "C" long long dp_launch_count(void) { return (long long)dp_launches; }
extern "C" int dp_recent_launches(const char** out, int cap) {
    unsigned long long have = dp_launches < DP_LAUNCH_RING ? dp_launches : DP_LAUNCH_RING;
    if (cap < 0) cap = 0;
    if (have > (unsigned long long)cap) have = (unsigned long long)cap;
    for (unsigned long long i = 0; i < have; ++i) out[i] = dp_launch_names[(dp_launches - have + i) & (DP_LAUNCH_RING - 1)];
    return (int)have;
}

static inline unsigned dp_grid(long long n, int per_block = 256, unsigned cap = 8192) {
    long long nb = (n + per_block - 1) / per_block;
    if (nb > cap) nb = cap;
    if (nb < 1) nb = 1;
    return (unsigned)nb;
}

#define GS_LOOP(i, n) for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (long long)gridDim.x * blockDim.x)

__global__ void silu_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, long long n) {
    GS_LOOP(i, n) y[i] = dp_silu(x[i]);
}
__global__ void silu_bwd_kernel(const float* __restrict__ x, const float* __restrict__ dy, float* __restrict__ dx, long long n,
                                int accumulate) {
    GS_LOOP(i, n) {
        const float v = dy[i] * dp_silu_grad(x[i]);
        dx[i] = accumulate ? dx[i] + v : v;
    }
}
extern "C" int dp_silu_fwd(const float* x, float* y, long long n, void* stream) {
    if (n <= 0) return 0;
    DP_LAUNCH(silu_fwd_kernel, dim3(dp_grid(n)), dim3(256), 0, (hipStream_t)stream, x, y, n);
    return DP_LAUNCH_CHECK();
}
extern "C" int dp_silu_bwd(const float* x, const float* dy, float* dx, long long n, int accumulate, void* stream) {
    if (n <= 0) return 0;
    DP_LAUNCH(silu_bwd_kernel, dim3(dp_grid(n)), dim3(256), 0, (hipStream_t)stream, x, dy, dx, n, accumulate);
    return DP_LAUNCH_CHECK();
}

__global__ void axpby_kernel(const float* __restrict__ x, float a, float* __restrict__ y, float b, long long n) {
    GS_LOOP(i, n) y[i] = (b == 0.f) ? a * x[i] : a * x[i] + b * y[i];
}
extern "C" int dp_axpby(const float* x, float a, float* y, float b, long long n, void* stream) {
    if (n <= 0) return 0;
    DP_LAUNCH(axpby_kernel, dim3(dp_grid(n)), dim3(256), 0, (hipStream_t)stream, x, a, y, b, n);
    return DP_LAUNCH_CHECK();
}

__global__ void copy_strided_kernel(const float* __restrict__ src, long long s_stride, float* __restrict__ dst,
                                    long long d_stride, int N, long long per_img, int accumulate) {
    const long long total = (long long)N * per_img;
    GS_LOOP(i, total) {
        const long long img = i / per_img;
        const long long r = i - img * per_img;
        const float v = src[img * s_stride + r];
        float* d = dst + img * d_stride + r;
        *d = accumulate ? *d + v : v;
    }
}
extern "C" int dp_copy_strided(const float* src, long long s_stride, float* dst, long long d_stride, int N,
                               long long per_img, int accumulate, void* stream) {
    if ((long long)N * per_img <= 0) return 0;
    DP_LAUNCH(copy_strided_kernel, dim3(dp_grid((long long)N * per_img)), dim3(256), 0, (hipStream_t)stream, src,
                       s_stride, dst, d_stride, N, per_img, accumulate);
    return DP_LAUNCH_CHECK();
}

// ---------------------------------------------------------------------------------------------
// softmax over the last dimension, one wavefront per row (cols = 16 ... 1024 in this model family)
// ---------------------------------------------------------------------------------------------
#define SM_CACHE 16
__global__ __launch_bounds__(256) void softmax_fwd_kernel(const float* __restrict__ s, float* __restrict__ p, long long rows,
                                                          int cols) {
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    const float* sr = s + row * cols;
    float* pr = p + row * cols;
    if (cols <= 64 * SM_CACHE) {
        float v[SM_CACHE];
        float mx = -INFINITY;
#pragma unroll
        for (int i = 0; i < SM_CACHE; ++i) {
            const int j = lane + 64 * i;
            v[i] = (j < cols) ? sr[j] : -INFINITY;
            mx = fmaxf(mx, v[i]);
        }
        mx = dp_wave_max(mx);
        float sum = 0.f;
#pragma unroll
        for (int i = 0; i < SM_CACHE; ++i) {
            const int j = lane + 64 * i;
            v[i] = (j < cols) ? expf(v[i] - mx) : 0.f;
            sum += v[i];
        }
        sum = dp_wave_sum(sum);
        const float inv = 1.0f / sum;
#pragma unroll
        for (int i = 0; i < SM_CACHE; ++i) {
            const int j = lane + 64 * i;
            if (j < cols) pr[j] = v[i] * inv;
        }
    } else {
        float mx = -INFINITY;
        for (int j = lane; j < cols; j += 64) mx = fmaxf(mx, sr[j]);
        mx = dp_wave_max(mx);
        float sum = 0.f;
        for (int j = lane; j < cols; j += 64) sum += expf(sr[j] - mx);
        sum = dp_wave_sum(sum);
        const float inv = 1.0f / sum;
        for (int j = lane; j < cols; j += 64) pr[j] = expf(sr[j] - mx) * inv;
    }
}
extern "C" int dp_softmax_fwd(const float* s, float* p, long long rows, int cols, void* stream) {
    if (rows <= 0) return 0;
    DP_LAUNCH(softmax_fwd_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, s, p, rows,
                       cols);
    return DP_LAUNCH_CHECK();
}

__global__ __launch_bounds__(256) void softmax_bwd_kernel(const float* __restrict__ p, const float* __restrict__ dp,
                                                          float* __restrict__ ds, long long rows, int cols, float scale) {
    const long long row = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int lane = threadIdx.x & 63;
    const float* pr = p + row * cols;
    const float* dr = dp + row * cols;
    float* o = ds + row * cols;
    float dot = 0.f;
    for (int j = lane; j < cols; j += 64) dot += pr[j] * dr[j];
    dot = dp_wave_sum(dot);
    for (int j = lane; j < cols; j += 64) o[j] = scale * pr[j] * (dr[j] - dot);
}
extern "C" int dp_softmax_bwd(const float* p, const float* dp, float* ds, long long rows, int cols, float scale,
                              void* stream) {
    if (rows <= 0) return 0;
    DP_LAUNCH(softmax_bwd_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, (hipStream_t)stream, p, dp, ds,
                       rows, cols, scale);
    return DP_LAUNCH_CHECK();
}

// ---------------------------------------------------------------------------------------------
// timestep embedding (embeddings.py:22-62): out[b][i] = sin/cos(t_b * exp(-ln(P) * k / (half - shift)))
// ---------------------------------------------------------------------------------------------
__global__ void temb_kernel(const float* __restrict__ t, int B, int dim, int flip, float freq_shift, float log_period,
                            float* __restrict__ out) {
    const int half = dim / 2;
    const long long total = (long long)B * dim;
    GS_LOOP(i, total) {
        const int b = (int)(i / dim);
        const int j = (int)(i - (long long)b * dim);
        float v = 0.f;
        if (j < 2 * half) {
            const bool second = j >= half;
            const int k = second ? j - half : j;
            float e = -log_period * (float)k;
            e = e / ((float)half - freq_shift);
            const float arg = t[b] * expf(e);
            const bool use_cos = flip ? !second : second;
            v = use_cos ? cosf(arg) : sinf(arg);
        }
        out[i] = v;
    }
}
extern "C" int dp_timestep_embedding(const float* t, int B, int dim, int flip_sin_to_cos, float freq_shift, float max_period,
                                     float* out, void* stream) {
    if (B <= 0) return 0;
    DP_LAUNCH(temb_kernel, dim3(dp_grid((long long)B * dim)), dim3(256), 0, (hipStream_t)stream, t, B, dim,
                       flip_sin_to_cos, freq_shift, logf(max_period), out);
    return DP_LAUNCH_CHECK();
}

// ---------------------------------------------------------------------------------------------
// add_noise (scheduling_ddpm.py:408-429)
// ---------------------------------------------------------------------------------------------
__global__ void add_noise_kernel(const float* __restrict__ x0, const float* __restrict__ noise, const float* __restrict__ acp,
                                 const int64_t* __restrict__ t, int B, long long per_img, float* __restrict__ out) {
    const long long total = (long long)B * per_img;
    GS_LOOP(i, total) {
        const int b = (int)(i / per_img);
        const float a = acp[t[b]];
        const float sa = sqrtf(a);
        const float sb = sqrtf(1.0f - a);
        out[i] = sa * x0[i] + sb * noise[i];
    }
}
extern "C" int dp_add_noise(const float* x0, const float* noise, const float* acp, const int64_t* t, int B,
                            long long per_img, float* out, void* stream) {
    if ((long long)B * per_img <= 0) return 0;
    DP_LAUNCH(add_noise_kernel, dim3(dp_grid((long long)B * per_img)), dim3(256), 0, (hipStream_t)stream, x0, noise,
                       acp, t, B, per_img, out);
    return DP_LAUNCH_CHECK();
}

// ---------------------------------------------------------------------------------------------
// eps-loss: partial[blk] = sum (out-noise)^2 over a fixed contiguous slice, dout = gscale*(out-noise)
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mse_kernel(const float* __restrict__ out, const float* __restrict__ noise, long long n,
                                                  float gscale, float* __restrict__ dout, float* __restrict__ partial,
                                                  const float* __restrict__ stop_state) {
    __shared__ float red[4];
    // Diff-Pruning early exit kept on the device (dp_early_exit_update): once the sweep has stopped, later timesteps that the
    // host had already enqueued get dOut = 0 -- every gradient of such a step is an exact zero and the += epilogues add
    // nothing, so overshoot steps are exact no-ops and the host need not read the loss after every step.
    if (stop_state && stop_state[1] != 0.f) gscale = 0.f;
    const long long per = (n + gridDim.x - 1) / gridDim.x;
    const long long lo = (long long)blockIdx.x * per;
    long long hi = lo + per;
    if (hi > n) hi = n;
    float s = 0.f;
    for (long long i = lo + threadIdx.x; i < hi; i += 256) {
        const float d = out[i] - noise[i];
        s += d * d;
        if (dout) dout[i] = gscale * d;
    }
    s = dp_block_sum_256(s, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}
extern "C" int dp_mse_fwd_bwd(const float* out, const float* noise, long long n, float gscale, float* dout, float* partial,
                              int nblocks, const float* stop_state, void* stream) {
    if (n <= 0 || nblocks <= 0) return (int)hipErrorInvalidValue;
    DP_LAUNCH(mse_kernel, dim3(nblocks), dim3(256), 0, (hipStream_t)stream, out, noise, n, gscale, dout, partial, stop_state);
    return DP_LAUNCH_CHECK();
}

// ---------------------------------------------------------------------------------------------
// distillation loss (functions/losses.py:17-31): S = student output, T = frozen teacher output, e = noise
//   dout = gscale * (w_kd (S - T) + w_eps (S - e));  partial[blk] = sum (S-T)^2,  partial[nblocks + blk] = sum (S-e)^2
// Same fixed grid, contiguous per-block slice and per-thread summation order as mse_kernel: the eps partial of (w_kd, w_eps) =
// (0, 1) is mse_kernel's partial bit for bit.  KD_UNROLL strided elements per thread per round: their 3 x KD_UNROLL loads are
// issued before the first use (indices clamped into the slice, so every load is unconditional); the out-of-slice lanes of the
// last round add an exact +0 to both sums and store nothing.
// ---------------------------------------------------------------------------------------------
#define KD_UNROLL 4
__global__ __launch_bounds__(256) void kd_kernel(const float* __restrict__ S, const float* __restrict__ T,
                                                 const float* __restrict__ E, long long n, float w_kd, float w_eps, float gscale,
                                                 float* __restrict__ dout, float* __restrict__ partial) {
    __shared__ float red[4];
    const long long per = (n + gridDim.x - 1) / gridDim.x;
    const long long lo = (long long)blockIdx.x * per;
    long long hi = lo + per;
    if (hi > n) hi = n;
    float sk = 0.f, se = 0.f;
    for (long long base = lo + threadIdx.x; base < hi; base += 256 * KD_UNROLL) {
        float s[KD_UNROLL], t[KD_UNROLL], e[KD_UNROLL];
#pragma unroll
        for (int u = 0; u < KD_UNROLL; ++u) {
            const long long i = base + (long long)u * 256;
            const long long j = i < hi ? i : hi - 1;          // hi > lo here: the slice is not empty
            s[u] = S[j];
            t[u] = T[j];
            e[u] = E[j];
        }
#pragma unroll
        for (int u = 0; u < KD_UNROLL; ++u) {
            const long long i = base + (long long)u * 256;
            const bool ok = i < hi;
            const float dk = ok ? s[u] - t[u] : 0.f;
            const float de = ok ? s[u] - e[u] : 0.f;
            sk = fmaf(dk, dk, sk);                              // mse_kernel's `s += d * d` compiles to this fma: written
            se = fmaf(de, de, se);                              // out so that the vectoriser cannot split it here
            if (ok) dout[i] = gscale * (w_kd * dk + w_eps * de);
        }
    }
    sk = dp_block_sum_256(sk, red);
    se = dp_block_sum_256(se, red);
    if (threadIdx.x == 0) {
        partial[blockIdx.x] = sk;
        partial[gridDim.x + blockIdx.x] = se;
    }
}
extern "C" int dp_kd_fwd_bwd(const float* out, const float* teacher, const float* noise, long long n, float w_kd, float w_eps,
                             float gscale, float* dout, float* partial, int nblocks, void* stream) {
    if (n <= 0 || nblocks <= 0 || !dout || !partial) return (int)hipErrorInvalidValue;
    DP_LAUNCH(kd_kernel, dim3(nblocks), dim3(256), 0, (hipStream_t)stream, out, teacher, noise, n, w_kd, w_eps, gscale, dout,
              partial);
    return DP_LAUNCH_CHECK();
}

// terms = [w_kd * kd + w_eps * eps, kd, eps] with kd / eps = scale * (sum of their nblocks partials), each summed in
// sum_partials_kernel's order (so eps == dp_sum_partials of the same partials, and loss == eps for (0, 1))
__global__ __launch_bounds__(256) void kd_terms_kernel(const float* __restrict__ partial, int n, float w_kd, float w_eps,
                                                       float scale, float* __restrict__ terms) {
    __shared__ float red[4];
    float a = 0.f, b = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) {
        a += partial[i];
        b += partial[n + i];
    }
    a = dp_block_sum_256(a, red);
    b = dp_block_sum_256(b, red);
    if (threadIdx.x == 0) {
        const float kd = a * scale, eps = b * scale;
        terms[0] = w_kd * kd + w_eps * eps;
        terms[1] = kd;
        terms[2] = eps;
    }
}
extern "C" int dp_kd_terms(const float* partial, int nblocks, float w_kd, float w_eps, float scale, float* terms, void* stream) {
    if (nblocks <= 0) return (int)hipErrorInvalidValue;
    DP_LAUNCH(kd_terms_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partial, nblocks, w_kd, w_eps, scale, terms);
    return DP_LAUNCH_CHECK();
}

// ---------------------------------------------------------------------------------------------
// Diff-Pruning early exit on the device (ddpm_prune.py:104-106 / ddpm_exp/prune.py:249-256), fp32 like the reference's
// 0-d tensors:  if (loss > loss_max) loss_max = loss;  if (loss < loss_max * thr) stop.
// state = [loss_max, stopped (0/1), executed steps]; the loss of executed step k is kept in losses[k].
// ---------------------------------------------------------------------------------------------
__global__ void early_exit_update_kernel(const float* __restrict__ loss, float thr, float* __restrict__ state,
                                         float* __restrict__ losses, int max_steps) {
    if (threadIdx.x != 0 || blockIdx.x != 0 || state[1] != 0.f) return;
    const float l = loss[0];
    const int k = (int)state[2];
    if (k < max_steps) losses[k] = l;
    state[2] = (float)(k + 1);
    float mx = state[0];
    if (l > mx) mx = l;
    state[0] = mx;
    if (l < __fmul_rn(mx, thr)) state[1] = 1.f;
}
extern "C" int dp_early_exit_update(const float* loss, float thr, float* state, float* losses, int max_steps, void* stream) {
    DP_LAUNCH(early_exit_update_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, loss, thr, state, losses, max_steps);
    return DP_LAUNCH_CHECK();
}

// The LDM script's form of the same test (ldm_exp/prune_ldm.py:104,124-129): `max_loss = -1` initially (the host writes -1 into
// state[0]), `if loss > max_loss: max_loss = loss;  if loss / max_loss < thres: break` -- the quotient rounded to fp32 as the
// division of two fp32 0-d tensors is.  thr < 0 never fires (plain Taylor: only the losses are recorded).
__global__ void early_exit_update_ratio_kernel(const float* __restrict__ loss, float thr, float* __restrict__ state,
                                               float* __restrict__ losses, int max_steps) {
    if (threadIdx.x != 0 || blockIdx.x != 0 || state[1] != 0.f) return;
    const float l = loss[0];
    const int k = (int)state[2];
    if (k < max_steps) losses[k] = l;
    state[2] = (float)(k + 1);
    float mx = state[0];
    if (l > mx) mx = l;
    state[0] = mx;
    if (__fdiv_rn(l, mx) < thr) state[1] = 1.f;
}
extern "C" int dp_early_exit_update_ratio(const float* loss, float thr, float* state, float* losses, int max_steps,
                                          void* stream) {
    DP_LAUNCH(early_exit_update_ratio_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, loss, thr, state, losses, max_steps);
    return DP_LAUNCH_CHECK();
}

// x *= (stopped ? 0 : 1): the ddpm_exp flavour tests the threshold BEFORE the backward pass, so dOut of the breaking step
// itself has to be cancelled after the state update
__global__ void scale_if_stopped_kernel(float* __restrict__ x, long long n, const float* __restrict__ state) {
    if (state[1] == 0.f) return;
    GS_LOOP(i, n) x[i] = 0.f;
}
extern "C" int dp_zero_if_stopped(float* x, long long n, const float* state, void* stream) {
    if (n <= 0) return 0;
    DP_LAUNCH(scale_if_stopped_kernel, dim3(dp_grid(n)), dim3(256), 0, (hipStream_t)stream, x, n, state);
    return DP_LAUNCH_CHECK();
}

__global__ __launch_bounds__(256) void sum_partials_kernel(const float* __restrict__ partial, int n, float scale,
                                                           float* __restrict__ dst) {
    __shared__ float red[4];
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) s += partial[i];
    s = dp_block_sum_256(s, red);
    if (threadIdx.x == 0) dst[0] = s * scale;
}
extern "C" int dp_sum_partials(const float* partial, int n, float scale, float* dst, void* stream) {
    DP_LAUNCH(sum_partials_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partial, n, scale, dst);
    return DP_LAUNCH_CHECK();
}

// ---------------------------------------------------------------------------------------------
// backward of nearest x2 upsampling: dx[h][w] = sum of the 2x2 block of dy
// ---------------------------------------------------------------------------------------------
__global__ void downsum_kernel(const float* __restrict__ dy, long long dy_img_stride, int N, int C, int H, int W,
                               float* __restrict__ dx, long long dx_img_stride) {
    const long long per = (long long)C * H * W;
    const long long total = (long long)N * per;
    GS_LOOP(i, total) {
        const long long n = i / per;
        const long long r = i - n * per;
        const int w = (int)(r % W);
        const long long ch = r / W;             // c*H + h
        const int h = (int)(ch % H);
        const long long c = ch / H;
        const float* s = dy + n * dy_img_stride + (c * (2 * H) + 2 * h) * (long long)(2 * W) + 2 * w;
        dx[n * dx_img_stride + r] = (s[0] + s[1]) + (s[2 * W] + s[2 * W + 1]);
    }
}
extern "C" int dp_downsum2x2(const float* dy, long long dy_img_stride, int N, int C, int H, int W, float* dx,
                             long long dx_img_stride, void* stream) {
    const long long total = (long long)N * C * H * W;
    if (total <= 0) return 0;
    DP_LAUNCH(downsum_kernel, dim3(dp_grid(total)), dim3(256), 0, (hipStream_t)stream, dy, dy_img_stride, N, C, H, W,
                       dx, dx_img_stride);
    return DP_LAUNCH_CHECK();
}

// ---------------------------------------------------------------------------------------------
// nearest x2 upsampling, materialised (F.interpolate(scale_factor=2.0, mode="nearest"), resnet.py:155): one thread per 4
// consecutive output pixels (= 2 source pixels) when W is even, per output pixel otherwise.  The upsample convolution then
// is a plain stride-1 convolution and runs on the LDS-DMA kernels; the gather form stays for foreign callers.
// ---------------------------------------------------------------------------------------------
__global__ void upsample2x_kernel(const float* __restrict__ x, long long x_img_stride, int N, int C, int H, int W,
                                  float* __restrict__ y, long long y_img_stride, int vec) {
    const int Wo = 2 * W, Ho = 2 * H;
    if (vec) {
        const int W4 = Wo / 4;
        const long long per = (long long)C * Ho * W4;
        const long long total = (long long)N * per;
        GS_LOOP(i, total) {
            const long long n = i / per;
            const long long r = i - n * per;
            const int w4 = (int)(r % W4);
            const long long ch = r / W4;            // c*Ho + ho
            const int ho = (int)(ch % Ho);
            const long long c = ch / Ho;
            const float2 s = *reinterpret_cast<const float2*>(x + n * x_img_stride + (c * H + (ho >> 1)) * (long long)W + 2 * w4);
            *reinterpret_cast<float4*>(y + n * y_img_stride + ch * Wo + 4 * w4) = make_float4(s.x, s.x, s.y, s.y);
        }
    } else {
        const long long per = (long long)C * Ho * Wo;
        const long long total = (long long)N * per;
        GS_LOOP(i, total) {
            const long long n = i / per;
            const long long r = i - n * per;
            const int wo = (int)(r % Wo);
            const long long ch = r / Wo;
            const int ho = (int)(ch % Ho);
            const long long c = ch / Ho;
            y[n * y_img_stride + r] = x[n * x_img_stride + (c * H + (ho >> 1)) * (long long)W + (wo >> 1)];
        }
    }
}
extern "C" int dp_upsample2x(const float* x, long long x_img_stride, int N, int C, int H, int W, float* y,
                             long long y_img_stride, void* stream) {
    const int vec = (W % 2 == 0) && (x_img_stride % 2 == 0) && (y_img_stride % 4 == 0) && ((uintptr_t)x % 8 == 0) &&
                    ((uintptr_t)y % 16 == 0);
    const long long total = (long long)N * C * (2 * H) * (vec ? W / 2 : 2 * W);
    if (total <= 0) return 0;
    DP_LAUNCH(upsample2x_kernel, dim3(dp_grid(total)), dim3(256), 0, (hipStream_t)stream, x, x_img_stride, N, C, H, W, y,
                       y_img_stride, vec);
    return DP_LAUNCH_CHECK();
}

// ---------------------------------------------------------------------------------------------
// Input gradient of a stride-2 3x3 convolution, assembled from its four parity classes: dx[2i+ph][2j+pw] = q[2ph+pw][i][j]
// (+ add: the skip-connection gradient that the caller would otherwise add in a second pass).  See ops.conv_dgrad_s2.
// ---------------------------------------------------------------------------------------------
__global__ void interleave2x2_kernel(const float* __restrict__ q, long long q_class_stride, long long q_img_stride, int N, int C,
                                     int Ho, int Wo, const float* __restrict__ add, long long add_img_stride,
                                     float* __restrict__ dx, long long dx_img_stride, int vec) {
    const int W = 2 * Wo, H = 2 * Ho;
    if (vec) {                                   // one thread: 4 consecutive output pixels of one row = 2 + 2 class elements
        const int W4 = W / 4;
        const long long per = (long long)C * H * W4;
        const long long total = (long long)N * per;
        GS_LOOP(t, total) {
            const long long n = t / per;
            const long long r = t - n * per;
            const int w4 = (int)(r % W4);
            const long long ch = r / W4;            // c*H + h
            const int h = (int)(ch % H);
            const long long c = ch / H;
            const float* qb = q + (long long)(2 * (h & 1)) * q_class_stride + n * q_img_stride + (c * Ho + (h >> 1)) * (long long)Wo + 2 * w4;
            const float2 a = *reinterpret_cast<const float2*>(qb);
            const float2 b = *reinterpret_cast<const float2*>(qb + q_class_stride);
            float4 o = make_float4(a.x, b.x, a.y, b.y);
            const long long oi = ch * W + 4 * w4;
            if (add) {
                const float4 s = *reinterpret_cast<const float4*>(add + n * add_img_stride + oi);
                o.x += s.x; o.y += s.y; o.z += s.z; o.w += s.w;
            }
            *reinterpret_cast<float4*>(dx + n * dx_img_stride + oi) = o;
        }
    } else {
        const long long per = (long long)C * H * W;
        const long long total = (long long)N * per;
        GS_LOOP(t, total) {
            const long long n = t / per;
            const long long r = t - n * per;
            const int w = (int)(r % W);
            const long long ch = r / W;
            const int h = (int)(ch % H);
            const long long c = ch / H;
            float v = q[(long long)(2 * (h & 1) + (w & 1)) * q_class_stride + n * q_img_stride + (c * Ho + (h >> 1)) * (long long)Wo + (w >> 1)];
            if (add) v += add[n * add_img_stride + r];
            dx[n * dx_img_stride + r] = v;
        }
    }
}
// q[2ph+pw][n][c][i][j] = y[n][c][2i+ph][2j+pw]: the inverse of interleave2x2 (the four parity classes of an output gradient).
__global__ void deinterleave2x2_kernel(const float* __restrict__ y, long long y_img_stride, int N, int C, int Ho, int Wo,
                                       float* __restrict__ q, long long q_class_stride, long long q_img_stride, int vec) {
    const int W = 2 * Wo, H = 2 * Ho;
    if (vec) {
        const int W4 = W / 4;
        const long long per = (long long)C * H * W4;
        const long long total = (long long)N * per;
        GS_LOOP(t, total) {
            const long long n = t / per;
            const long long r = t - n * per;
            const int w4 = (int)(r % W4);
            const long long ch = r / W4;
            const int h = (int)(ch % H);
            const long long c = ch / H;
            const float4 v = *reinterpret_cast<const float4*>(y + n * y_img_stride + ch * W + 4 * w4);
            float* qb = q + (long long)(2 * (h & 1)) * q_class_stride + n * q_img_stride + (c * Ho + (h >> 1)) * (long long)Wo + 2 * w4;
            *reinterpret_cast<float2*>(qb) = make_float2(v.x, v.z);
            *reinterpret_cast<float2*>(qb + q_class_stride) = make_float2(v.y, v.w);
        }
    } else {
        const long long per = (long long)C * H * W;
        const long long total = (long long)N * per;
        GS_LOOP(t, total) {
            const long long n = t / per;
            const long long r = t - n * per;
            const int w = (int)(r % W);
            const long long ch = r / W;
            const int h = (int)(ch % H);
            const long long c = ch / H;
            q[(long long)(2 * (h & 1) + (w & 1)) * q_class_stride + n * q_img_stride + (c * Ho + (h >> 1)) * (long long)Wo + (w >> 1)] =
                y[n * y_img_stride + r];
        }
    }
}
extern "C" int dp_deinterleave2x2(const float* y, long long y_img_stride, int N, int C, int Ho, int Wo, float* q,
                                  long long q_class_stride, long long q_img_stride, void* stream) {
    const int vec = (Wo % 2 == 0) && (q_class_stride % 2 == 0) && (q_img_stride % 2 == 0) && (y_img_stride % 4 == 0) &&
                    ((uintptr_t)q % 8 == 0) && ((uintptr_t)y % 16 == 0);
    const long long total = (long long)N * C * (2 * Ho) * (vec ? Wo / 2 : 2 * Wo);
    if (total <= 0) return 0;
    DP_LAUNCH(deinterleave2x2_kernel, dim3(dp_grid(total)), dim3(256), 0, (hipStream_t)stream, y, y_img_stride, N, C, Ho, Wo, q,
                       q_class_stride, q_img_stride, vec);
    return DP_LAUNCH_CHECK();
}

// ---------------------------------------------------------------------------------------------
// Nearest-x2 upsampling followed by a 3x3 'same' convolution == four 2x2 convolutions on the LOW-resolution input, one per
// parity class (ph, pw) of the output position: output row 2i+ph reads upsampled rows 2i+ph+ky-1, i.e. source rows
//   ph = 0:  i-1 (ky = 0),  i (ky = 1, 2)        ph = 1:  i (ky = 0, 1),  i+1 (ky = 2)
// so the class kernel has 2 taps per dimension whose weights are SUMS of the 3x3 taps that land on the same source pixel
// (top / left padding 1 - ph / 1 - pw).  16 multiply-adds per low-resolution pixel and channel pair instead of 36.
//   weff[2ph+pw][m][ty][tx] = sum_{ky in S(ph,ty)} sum_{kx in S(pw,tx)} w[m][ky][kx],  S(0,0) = {0}, S(0,1) = {1,2},
//                                                                                    S(1,0) = {0,1}, S(1,1) = {2}
// and the weight gradient folds back with the transposed map:  gw[m][ky][kx] (+)= sum_classes gweff[class][m][ty(ph,ky)][tx(pw,kx)].
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ int dp_ups_t(int parity, int k) { return parity == 0 ? (k == 0 ? 0 : 1) : (k == 2 ? 1 : 0); }

__global__ void ups_weff_kernel(const float* __restrict__ w, long long M, float* __restrict__ weff) {
    GS_LOOP(m, M) {
        float k[9];
#pragma unroll
        for (int t = 0; t < 9; ++t) k[t] = w[m * 9 + t];
#pragma unroll
        for (int cls = 0; cls < 4; ++cls) {
            const int ph = cls >> 1, pw = cls & 1;
            float e[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ky = 0; ky < 3; ++ky)
#pragma unroll
                for (int kx = 0; kx < 3; ++kx) e[dp_ups_t(ph, ky) * 2 + dp_ups_t(pw, kx)] += k[ky * 3 + kx];
#pragma unroll
            for (int t = 0; t < 4; ++t) weff[((long long)cls * M + m) * 4 + t] = e[t];
        }
    }
}
extern "C" int dp_ups_weff(const float* w, long long M, float* weff, void* stream) {
    if (M <= 0) return 0;
    DP_LAUNCH(ups_weff_kernel, dim3(dp_grid(M)), dim3(256), 0, (hipStream_t)stream, w, M, weff);
    return DP_LAUNCH_CHECK();
}

__global__ void ups_wfold_kernel(const float* __restrict__ gweff, long long M, float* __restrict__ gw, int accumulate) {
    GS_LOOP(m, M) {
        float e[4][4];
#pragma unroll
        for (int cls = 0; cls < 4; ++cls)
#pragma unroll
            for (int t = 0; t < 4; ++t) e[cls][t] = gweff[((long long)cls * M + m) * 4 + t];
#pragma unroll
        for (int ky = 0; ky < 3; ++ky)
#pragma unroll
            for (int kx = 0; kx < 3; ++kx) {
                float s = 0.f;
#pragma unroll
                for (int cls = 0; cls < 4; ++cls) s += e[cls][dp_ups_t(cls >> 1, ky) * 2 + dp_ups_t(cls & 1, kx)];
                float* o = gw + m * 9 + ky * 3 + kx;
                *o = accumulate ? *o + s : s;
            }
    }
}
extern "C" int dp_ups_wfold(const float* gweff, long long M, float* gw, int accumulate, void* stream) {
    if (M <= 0) return 0;
    DP_LAUNCH(ups_wfold_kernel, dim3(dp_grid(M)), dim3(256), 0, (hipStream_t)stream, gweff, M, gw, accumulate);
    return DP_LAUNCH_CHECK();
}

extern "C" int dp_interleave2x2(const float* q, long long q_class_stride, long long q_img_stride, int N, int C, int Ho, int Wo,
                                const float* add, long long add_img_stride, float* dx, long long dx_img_stride, void* stream) {
    const int vec = (Wo % 2 == 0) && (q_class_stride % 2 == 0) && (q_img_stride % 2 == 0) && (dx_img_stride % 4 == 0) &&
                    (add_img_stride % 4 == 0) && ((uintptr_t)q % 8 == 0) && ((uintptr_t)dx % 16 == 0) && ((uintptr_t)add % 16 == 0);
    const long long total = (long long)N * C * (2 * Ho) * (vec ? Wo / 2 : 2 * Wo);
    if (total <= 0) return 0;
    DP_LAUNCH(interleave2x2_kernel, dim3(dp_grid(total)), dim3(256), 0, (hipStream_t)stream, q, q_class_stride, q_img_stride, N,
                       C, Ho, Wo, add, add_img_stride, dx, dx_img_stride, vec);
    return DP_LAUNCH_CHECK();
}

// ---------------------------------------------------------------------------------------------
// DDIM update (scheduling_ddim.py:324-370)
// ---------------------------------------------------------------------------------------------
__global__ void ddim_step_kernel(const float* __restrict__ x, const float* __restrict__ eps, const float* __restrict__ vn,
                                 float sqrt_a_t, float sqrt_b_t, float sqrt_a_prev, float dir_coef, float stdv, int clip,
                                 float clip_range, float* __restrict__ out, long long n) {
    GS_LOOP(i, n) {
        const float e = eps[i];
        float x0 = (x[i] - sqrt_b_t * e) / sqrt_a_t;
        if (clip) x0 = fminf(fmaxf(x0, -clip_range), clip_range);
        float v = sqrt_a_prev * x0 + dir_coef * e;
        if (vn) v += stdv * vn[i];
        out[i] = v;
    }
}
extern "C" int dp_ddim_step(const float* x, const float* eps, const float* vnoise, float a_t, float a_prev, float stdv,
                            int clip, float clip_range, float* out, long long n, void* stream) {
    if (n <= 0) return 0;
    // coefficient arithmetic in fp32, in the reference's operation order (0-d fp32 tensors there)
    const float b_t = 1.0f - a_t;
    const float sqrt_a_t = powf(a_t, 0.5f);
    const float sqrt_b_t = powf(b_t, 0.5f);
    const float sqrt_a_prev = powf(a_prev, 0.5f);
    const float dir_coef = powf(1.0f - a_prev - stdv * stdv, 0.5f);
    DP_LAUNCH(ddim_step_kernel, dim3(dp_grid(n)), dim3(256), 0, (hipStream_t)stream, x, eps, vnoise, sqrt_a_t,
                       sqrt_b_t, sqrt_a_prev, dir_coef, stdv, clip, clip_range, out, n);
    return DP_LAUNCH_CHECK();
}

// ---------------------------------------------------------------------------------------------
// DDPM ancestral update (scheduling_ddpm.py:360-401): coefficients arrive from the host (0-d fp32 arithmetic there)
// ---------------------------------------------------------------------------------------------
__global__ void ddpm_step_kernel(const float* __restrict__ x, const float* __restrict__ eps, const float* __restrict__ vn,
                                 float sqrt_a_t, float sqrt_b_t, float c_x0, float c_xt, float sigma, int clip,
                                 float clip_range, float* __restrict__ out, long long n) {
    GS_LOOP(i, n) {
        const float xi = x[i];
        float x0 = (xi - sqrt_b_t * eps[i]) / sqrt_a_t;
        if (clip) x0 = fminf(fmaxf(x0, -clip_range), clip_range);
        float v = c_x0 * x0 + c_xt * xi;
        if (vn) v += sigma * vn[i];
        out[i] = v;
    }
}
extern "C" int dp_ddpm_step(const float* x, const float* eps, const float* vnoise, float sqrt_a_t, float sqrt_b_t, float c_x0,
                            float c_xt, float sigma, int clip, float clip_range, float* out, long long n, void* stream) {
    if (n <= 0) return 0;
    DP_LAUNCH(ddpm_step_kernel, dim3(dp_grid(n)), dim3(256), 0, (hipStream_t)stream, x, eps, vnoise, sqrt_a_t,
                       sqrt_b_t, c_x0, c_xt, sigma, clip, clip_range, out, n);
    return DP_LAUNCH_CHECK();
}

// ---------------------------------------------------------------------------------------------
// Dropout, standalone forms (Attention.to_out[1]; mask export for the parity tests).  Philox masks: dp_common.h.
// ---------------------------------------------------------------------------------------------
__global__ void dropout_apply_kernel(const float* __restrict__ x, long long xs, float* __restrict__ y, long long ys, int N,
                                     long long per_img, DpDrop drop) {
    const long long total = (long long)N * per_img;
    GS_LOOP(i, total) {
        const long long n = i / per_img;
        const long long r = i - n * per_img;
        y[n * ys + r] = x[n * xs + r] * dp_drop1(drop, (drop.n_off + n) * per_img + r);
    }
}
extern "C" int dp_dropout_apply(const float* x, long long x_img_stride, float* y, long long y_img_stride, int N,
                                long long per_img, const dp_dropout* drop, void* stream) {
    if ((long long)N * per_img <= 0) return 0;
    if (!drop || !drop->thr24) return (int)hipErrorInvalidValue;
    DP_LAUNCH(dropout_apply_kernel, dim3(dp_grid((long long)N * per_img)), dim3(256), 0, (hipStream_t)stream, x,
                       x_img_stride, y, y_img_stride, N, per_img, dp_drop_host(drop));
    return DP_LAUNCH_CHECK();
}

__global__ void dropout_mask_kernel(float* __restrict__ m, long long idx0, long long n, DpDrop drop) {
    GS_LOOP(i, n) m[i] = dp_drop1(drop, idx0 + i);
}
extern "C" int dp_dropout_mask(float* m, long long idx0, long long n, const dp_dropout* drop, void* stream) {
    if (n <= 0) return 0;
    if (!drop || !drop->thr24) return (int)hipErrorInvalidValue;
    DP_LAUNCH(dropout_mask_kernel, dim3(dp_grid(n)), dim3(256), 0, (hipStream_t)stream, m, idx0, n,
                       dp_drop_host(drop));
    return DP_LAUNCH_CHECK();
}

// ---------------------------------------------------------------------------------------------
// Standard-normal draws as a pure function of (seed, stream, step, logical element index): Philox4x32-10 on counter
// (idx4 lo, idx4 hi, stream, step), key = seed; the four words give two Box-Muller pairs
//   u = w * 2^-32 + 2^-33 in (0, 1],  r = sqrt(-2 ln u_a),  (r cos 2 pi u_b, r sin 2 pi u_b).
// Element idx takes output idx & 3 (0: r0 cos, 1: r0 sin, 2: r1 cos, 3: r1 sin).  The LDM importance pass draws x_T and the
// loss noise with it (the reference draws both from the device RNG: ddim.py `torch.randn(shape, device=device)`,
// ddpm.py p_losses `torch.randn_like(x_start)`): idx is the GLOBAL index of the latent element, so a rank's shard holds
// exactly its slice of the one-process draw.  Restated in oracle/philox_ref.py.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float dp_u01(unsigned w) { return fmaf((float)w, 2.3283064365386963e-10f, 1.1641532182693481e-10f); }
__global__ void randn_philox_kernel(float* __restrict__ out, long long idx0, long long n, unsigned seed_lo, unsigned seed_hi,
                                    unsigned stream_id, unsigned step) {
    const long long q0 = idx0 >> 2;
    const long long nq = ((idx0 + n + 3) >> 2) - q0;
    GS_LOOP(j, nq) {
        const unsigned long long q = (unsigned long long)(q0 + j);
        const uint4 r = dp_philox4x32_10(make_uint4((unsigned)q, (unsigned)(q >> 32), stream_id, step), seed_lo, seed_hi);
        const float ra = sqrtf(-2.f * logf(dp_u01(r.x))), rb = sqrtf(-2.f * logf(dp_u01(r.z)));
        const float ta = 6.2831853071795865f * dp_u01(r.y), tb = 6.2831853071795865f * dp_u01(r.w);
        const float v[4] = {ra * cosf(ta), ra * sinf(ta), rb * cosf(tb), rb * sinf(tb)};
        const long long base = (long long)(q << 2) - idx0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const long long i = base + e;
            if (i >= 0 && i < n) out[i] = v[e];
        }
    }
}
extern "C" int dp_randn_philox(float* out, long long idx0, long long n, unsigned long long seed, unsigned stream_id,
                               unsigned step, void* stream) {
    if (n <= 0) return 0;
    if (idx0 < 0) return (int)hipErrorInvalidValue;
    DP_LAUNCH(randn_philox_kernel, dim3(dp_grid((n + 3) / 4 + 1)), dim3(256), 0, (hipStream_t)stream, out, idx0, n,
              (unsigned)(seed & 0xffffffffull), (unsigned)(seed >> 32), stream_id, step);
    return DP_LAUNCH_CHECK();
}

// ---------------------------------------------------------------------------------------------
// LDM glue: q_sample with precomputed sqrt tables (ldm/models/diffusion/ddpm.py q_sample) and the classifier-free
// guidance combination e = e_u + s (e_c - e_u) (ldm/models/diffusion/ddim.py:178-183)
// ---------------------------------------------------------------------------------------------
__global__ void q_sample_kernel(const float* __restrict__ x0, const float* __restrict__ noise, const float* __restrict__ sa,
                                const float* __restrict__ sb, const int64_t* __restrict__ t, int B, long long per_img,
                                float* __restrict__ out) {
    const long long total = (long long)B * per_img;
    GS_LOOP(i, total) {
        const int b = (int)(i / per_img);
        out[i] = sa[t[b]] * x0[i] + sb[t[b]] * noise[i];
    }
}
extern "C" int dp_q_sample(const float* x0, const float* noise, const float* sqrt_acp, const float* sqrt_1m_acp,
                           const int64_t* t, int B, long long per_img, float* out, void* stream) {
    if ((long long)B * per_img <= 0) return 0;
    DP_LAUNCH(q_sample_kernel, dim3(dp_grid((long long)B * per_img)), dim3(256), 0, (hipStream_t)stream, x0, noise,
                       sqrt_acp, sqrt_1m_acp, t, B, per_img, out);
    return DP_LAUNCH_CHECK();
}

__global__ void cfg_combine_kernel(const float* __restrict__ eu, const float* __restrict__ ec, float s, float* __restrict__ out,
                                   long long n) {
    GS_LOOP(i, n) {
        const float u = eu[i];
        out[i] = u + s * (ec[i] - u);
    }
}
extern "C" int dp_cfg_combine(const float* e_uncond, const float* e_cond, float scale, float* out, long long n, void* stream) {
    if (n <= 0) return 0;
    DP_LAUNCH(cfg_combine_kernel, dim3(dp_grid(n)), dim3(256), 0, (hipStream_t)stream, e_uncond, e_cond, scale, out, n);
    return DP_LAUNCH_CHECK();
}


// ---------------------------------------------------------------------------------------------
// Input pipeline on the device (utils.py:8-58, ddpm_exp/datasets/__init__.py:30-60,176-192): decoded uint8 images ->
// fp32 NCHW training batch in one pass:  ToTensor (x / 255)  ->  RandomHorizontalFlip(p)  ->  Normalize(0.5, 0.5)
// [(v - 0.5) / 0.5, the reference's two roundings] or data_transform's `2 v - 1`, optional uniform dequantization
// (v / 256 * 255 + u / 256).  The flip decision of image n and the dequantization noise are Philox functions of
// (seed, stream id, step, global image / element index): reproducible on the host and independent of the sharding.
// src layout: hwc = 1 -> [N][H][W][C] (PIL / image folders), 0 -> [N][C][H][W] (CIFAR-10 python batches).
// ---------------------------------------------------------------------------------------------
__global__ void u8_to_float_kernel(const unsigned char* __restrict__ src, int hwc, int N, int C, int H, int W,
                                   float* __restrict__ out, long long out_img_stride, int mode, unsigned flip_thr24,
                                   int dequant, DpDrop rng) {
    const long long per = (long long)C * H * W;
    const long long total = (long long)N * per;
    GS_LOOP(i, total) {
        const long long n = i / per;
        const long long r = i - n * per;
        const int w = (int)(r % W);
        const long long ch = r / W;
        const int h = (int)(ch % H);
        const int c = (int)(ch / H);
        int ws = w;
        if (flip_thr24) {
            const unsigned long long gi = (unsigned long long)(rng.n_off + n);
            const uint4 d = dp_philox4x32_10(make_uint4((unsigned)gi, (unsigned)(gi >> 32), rng.site, rng.step), rng.seed_lo, rng.seed_hi);
            if ((d.x >> 8) < flip_thr24) ws = W - 1 - w;
        }
        const long long si = hwc ? (((n * H + h) * W + ws) * C + c) : (((n * C + c) * H + h) * (long long)W + ws);
        float v = (float)src[si] / 255.0f;
        if (dequant) {
            const unsigned long long e = (unsigned long long)((rng.n_off + n) * per + r);
            const unsigned long long q = e >> 2;
            const uint4 d = dp_philox4x32_10(make_uint4((unsigned)q, (unsigned)(q >> 32), rng.site ^ 0x9E3779B9u, rng.step), rng.seed_lo, rng.seed_hi);
            const unsigned word = (e & 3) == 0 ? d.x : (e & 3) == 1 ? d.y : (e & 3) == 2 ? d.z : d.w;
            v = v / 256.0f * 255.0f + ((float)(word >> 8) * (1.0f / 16777216.0f)) / 256.0f;
        }
        if (mode == 1) v = (v - 0.5f) / 0.5f;            // transforms.Normalize(mean=0.5, std=0.5)
        else if (mode == 2) v = 2.0f * v - 1.0f;         // data_transform: rescaled
        out[n * out_img_stride + r] = v;
    }
}
extern "C" int dp_u8_to_float(const unsigned char* src, int hwc, int N, int C, int H, int W, float* out,
                              long long out_img_stride, int mode, unsigned flip_thr24, int dequant, const dp_dropout* rng,
                              void* stream) {
    const long long total = (long long)N * C * H * W;
    if (total <= 0) return 0;
    if ((flip_thr24 || dequant) && !rng) return (int)hipErrorInvalidValue;
    DpDrop d{};
    if (rng) {
        d.seed_lo = (unsigned)(rng->seed & 0xffffffffull);
        d.seed_hi = (unsigned)(rng->seed >> 32);
        d.site = rng->site;
        d.step = rng->step;
        d.n_off = rng->n_off;
    }
    DP_LAUNCH(u8_to_float_kernel, dim3(dp_grid(total)), dim3(256), 0, (hipStream_t)stream, src, hwc, N, C, H, W, out,
              out_img_stride, mode, flip_thr24, dequant, d);
    return DP_LAUNCH_CHECK();
}


// ---------------------------------------------------------------------------------------------
// FID / SSIM evaluation glue (fid_score.py:100-322, inception.py:16-340, ddpm_exp/compute_ssim.py:14-53)
// ---------------------------------------------------------------------------------------------
// 3x3-style pooling over NCHW planes: mode 0 = max (padding excluded, as F.max_pool2d), mode 1 = average over the VALID taps
// only (F.avg_pool2d(..., count_include_pad=False), the TensorFlow behaviour the FID Inception patches in).
__global__ void pool2d_kernel(const float* __restrict__ x, long long x_img_stride, int N, int C, int H, int W, int k, int stride,
                              int pad, int mode, int Ho, int Wo, float* __restrict__ y, long long y_img_stride) {
    const long long per = (long long)C * Ho * Wo;
    const long long total = (long long)N * per;
    GS_LOOP(i, total) {
        const long long n = i / per;
        const long long r = i - n * per;
        const int wo = (int)(r % Wo);
        const long long ch = r / Wo;
        const int ho = (int)(ch % Ho);
        const long long c = ch / Ho;
        const float* xp = x + n * x_img_stride + c * (long long)H * W;
        float acc = mode == 0 ? -INFINITY : 0.f;
        int cnt = 0;
        for (int ky = 0; ky < k; ++ky) {
            const int h = ho * stride + ky - pad;
            if ((unsigned)h >= (unsigned)H) continue;
            for (int kx = 0; kx < k; ++kx) {
                const int w = wo * stride + kx - pad;
                if ((unsigned)w >= (unsigned)W) continue;
                const float v = xp[(long long)h * W + w];
                acc = mode == 0 ? fmaxf(acc, v) : acc + v;
                ++cnt;
            }
        }
        y[n * y_img_stride + r] = mode == 0 ? acc : acc / (float)cnt;
    }
}
extern "C" int dp_pool2d(const float* x, long long x_img_stride, int N, int C, int H, int W, int k, int stride, int pad, int mode,
                         float* y, long long y_img_stride, void* stream) {
    const int Ho = (H + 2 * pad - k) / stride + 1, Wo = (W + 2 * pad - k) / stride + 1;
    const long long total = (long long)N * C * Ho * Wo;
    if (total <= 0) return 0;
    DP_LAUNCH(pool2d_kernel, dim3(dp_grid(total)), dim3(256), 0, (hipStream_t)stream, x, x_img_stride, N, C, H, W, k, stride, pad,
              mode, Ho, Wo, y, y_img_stride);
    return DP_LAUNCH_CHECK();
}

// F.interpolate(x, size=(Ho, Wo), mode='bilinear', align_corners=False) followed by y = a * v + b (inception.py:147-154:
// resize to 299x299, then 2x - 1).  Source index arithmetic in fp32 exactly as ATen's area_pixel_compute_source_index.
__global__ void resize_bilinear_kernel(const float* __restrict__ x, long long x_img_stride, int N, int C, int H, int W, int Ho,
                                       int Wo, float a, float b, float* __restrict__ y) {
    const float sh = (float)H / (float)Ho, sw = (float)W / (float)Wo;
    const long long per = (long long)C * Ho * Wo;
    const long long total = (long long)N * per;
    GS_LOOP(i, total) {
        const long long n = i / per;
        const long long r = i - n * per;
        const int wo = (int)(r % Wo);
        const long long ch = r / Wo;
        const int ho = (int)(ch % Ho);
        const long long c = ch / Ho;
        float fh = sh * ((float)ho + 0.5f) - 0.5f;
        float fw = sw * ((float)wo + 0.5f) - 0.5f;
        if (fh < 0.f) fh = 0.f;
        if (fw < 0.f) fw = 0.f;
        const int h0 = (int)fh, w0 = (int)fw;
        const int h1 = h0 + (h0 < H - 1 ? 1 : 0), w1 = w0 + (w0 < W - 1 ? 1 : 0);
        const float lh1 = fh - (float)h0, lw1 = fw - (float)w0;
        const float lh0 = 1.f - lh1, lw0 = 1.f - lw1;
        const float* xp = x + n * x_img_stride + c * (long long)H * W;
        const float v = lh0 * (lw0 * xp[(long long)h0 * W + w0] + lw1 * xp[(long long)h0 * W + w1]) +
                        lh1 * (lw0 * xp[(long long)h1 * W + w0] + lw1 * xp[(long long)h1 * W + w1]);
        y[i] = a * v + b;
    }
}
extern "C" int dp_resize_bilinear(const float* x, long long x_img_stride, int N, int C, int H, int W, int Ho, int Wo, float a,
                                  float b, float* y, void* stream) {
    const long long total = (long long)N * C * Ho * Wo;
    if (total <= 0) return 0;
    DP_LAUNCH(resize_bilinear_kernel, dim3(dp_grid(total)), dim3(256), 0, (hipStream_t)stream, x, x_img_stride, N, C, H, W, Ho, Wo,
              a, b, y);
    return DP_LAUNCH_CHECK();
}

// SSIM (Wang et al. 2004 as implemented by pytorch_msssim.ssim, which compute_ssim.py:43 calls with data_range = 1,
// size_average = False): 11-tap Gaussian (sigma 1.5) "valid" filtering of x, y, x^2, y^2, xy per channel plane, then the mean of
// the SSIM map.  One workgroup per (plane, 16x16 output tile): the (16+10)^2 input patch of x and y sits in LDS, the
// horizontal pass writes 5 maps of 26x16 to LDS, the vertical pass produces the tile's SSIM values and their sum.
// part[(plane * tiles) + tile] = sum of the tile's SSIM values; sq[...] = sum of squared differences of the whole tile patch
// core (for the per-image MSE of compute_ssim.py:45).  Reduced in a fixed order by ssim_finish_kernel.
#define SSIM_T 16
#define SSIM_K 11
__constant__ float dp_ssim_win[SSIM_K];
__global__ __launch_bounds__(256) void ssim_tile_kernel(const float* __restrict__ x, const float* __restrict__ y, int H, int W,
                                                        int tiles_x, float C1, float C2, float* __restrict__ part) {
    constexpr int P = SSIM_T + SSIM_K - 1;                 // 26
    __shared__ float sx[P][P + 1], sy[P][P + 1];
    __shared__ float hm[5][P][SSIM_T + 1];
    __shared__ float red[4];
    const int plane = blockIdx.y;
    const int ty = blockIdx.x / tiles_x, tx = blockIdx.x - ty * tiles_x;
    const int Ho = H - SSIM_K + 1, Wo = W - SSIM_K + 1;
    const int h0 = ty * SSIM_T, w0 = tx * SSIM_T;
    const float* xp = x + (long long)plane * H * W;
    const float* yp = y + (long long)plane * H * W;
    for (int e = threadIdx.x; e < P * P; e += 256) {
        const int r = e / P, c = e - r * P;
        const int h = h0 + r, w = w0 + c;
        const bool v = h < H && w < W;
        sx[r][c] = v ? xp[(long long)h * W + w] : 0.f;
        sy[r][c] = v ? yp[(long long)h * W + w] : 0.f;
    }
    __syncthreads();
    for (int e = threadIdx.x; e < P * SSIM_T; e += 256) {          // horizontal pass
        const int r = e / SSIM_T, c = e - r * SSIM_T;
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, a4 = 0.f;
#pragma unroll
        for (int k = 0; k < SSIM_K; ++k) {
            const float g = dp_ssim_win[k], u = sx[r][c + k], v = sy[r][c + k];
            a0 += g * u; a1 += g * v; a2 += g * (u * u); a3 += g * (v * v); a4 += g * (u * v);
        }
        hm[0][r][c] = a0; hm[1][r][c] = a1; hm[2][r][c] = a2; hm[3][r][c] = a3; hm[4][r][c] = a4;
    }
    __syncthreads();
    float s = 0.f;
    {
        const int r = threadIdx.x / SSIM_T, c = threadIdx.x - r * SSIM_T;      // 256 threads = 16 x 16 outputs
        if (h0 + r < Ho && w0 + c < Wo) {
            float m[5] = {0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int k = 0; k < SSIM_K; ++k) {
                const float g = dp_ssim_win[k];
#pragma unroll
                for (int q = 0; q < 5; ++q) m[q] += g * hm[q][r + k][c];
            }
            const float mu1 = m[0], mu2 = m[1];
            const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
            const float s1 = m[2] - mu1_sq, s2 = m[3] - mu2_sq, s12 = m[4] - mu12;
            const float cs = (2.f * s12 + C2) / (s1 + s2 + C2);
            s = ((2.f * mu12 + C1) / (mu1_sq + mu2_sq + C1)) * cs;
        }
    }
    s = dp_block_sum_256(s, red);
    if (threadIdx.x == 0) part[(long long)plane * gridDim.x + blockIdx.x] = s;
}
// out[n] = mean_c ( sum_tiles part / (Ho*Wo) )
__global__ void ssim_finish_kernel(const float* __restrict__ part, int N, int C, int tiles, float inv_cnt, float* __restrict__ out) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    float acc = 0.f;
    for (int c = 0; c < C; ++c) {
        float s = 0.f;
        for (int t = 0; t < tiles; ++t) s += part[((long long)n * C + c) * tiles + t];
        acc += s * inv_cnt;
    }
    out[n] = acc / (float)C;
}
extern "C" int dp_ssim(const float* x, const float* y, int N, int C, int H, int W, float data_range, float* part, float* out,
                       void* stream) {
    if (N <= 0) return 0;
    if (H < SSIM_K || W < SSIM_K) return (int)hipErrorInvalidValue;
    static bool win_set = false;
    if (!win_set) {                                  // pytorch_msssim._fspecial_gauss_1d(11, 1.5): exp(-x^2 / (2 sigma^2)), normalised
        float g[SSIM_K], tot = 0.f;
        for (int i = 0; i < SSIM_K; ++i) { const float d = (float)(i - SSIM_K / 2); g[i] = expf(-(d * d) / (2.f * 1.5f * 1.5f)); tot += g[i]; }
        for (int i = 0; i < SSIM_K; ++i) g[i] /= tot;
        if (hipMemcpyToSymbol(HIP_SYMBOL(dp_ssim_win), g, sizeof(g)) != hipSuccess) return (int)hipGetLastError();
        win_set = true;
    }
    const int Ho = H - SSIM_K + 1, Wo = W - SSIM_K + 1;
    const int tx = (Wo + SSIM_T - 1) / SSIM_T, ty = (Ho + SSIM_T - 1) / SSIM_T;
    const float C1 = (0.01f * data_range) * (0.01f * data_range), C2 = (0.03f * data_range) * (0.03f * data_range);
    DP_LAUNCH(ssim_tile_kernel, dim3(tx * ty, N * C), dim3(256), 0, (hipStream_t)stream, x, y, H, W, tx, C1, C2, part);
    DP_LAUNCH(ssim_finish_kernel, dim3((N + 63) / 64), dim3(64), 0, (hipStream_t)stream, part, N, C, tx * ty,
              1.0f / (float)(Ho * Wo), out);
    return DP_LAUNCH_CHECK();
}
extern "C" long long dp_ssim_workspace(int N, int C, int H, int W) {
    const int Ho = H - SSIM_K + 1, Wo = W - SSIM_K + 1;
    if (Ho <= 0 || Wo <= 0) return 0;
    return (long long)N * C * ((Wo + SSIM_T - 1) / SSIM_T) * ((Ho + SSIM_T - 1) / SSIM_T);
}

// out[n] = mean over the image of (a - b)^2   (compute_ssim.py:45: mse_loss(reduction='none').mean(dim=(1,2,3)))
__global__ __launch_bounds__(256) void mse_per_image_kernel(const float* __restrict__ a, const float* __restrict__ b, long long per,
                                                            float* __restrict__ out) {
    __shared__ float red[4];
    const float* ap = a + (long long)blockIdx.x * per;
    const float* bp = b + (long long)blockIdx.x * per;
    float s = 0.f;
    for (long long i = threadIdx.x; i < per; i += 256) { const float d = ap[i] - bp[i]; s += d * d; }
    s = dp_block_sum_256(s, red);
    if (threadIdx.x == 0) out[blockIdx.x] = s / (float)per;
}
extern "C" int dp_mse_per_image(const float* a, const float* b, int N, long long per, float* out, void* stream) {
    if (N <= 0 || per <= 0) return 0;
    DP_LAUNCH(mse_per_image_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, a, b, per, out);
    return DP_LAUNCH_CHECK();
}


// ---------------------------------------------------------------------------------------------
// dp_pack_weight for MANY layers in one launch (same element map as pack_weight_kernel in gemm.hip): a finetune step re-packs
// every convolution weight in both operand layouts after each optimizer update (~190 launches of ~6 us on the pruned CIFAR
// UNet, ddpm_train.py:426-471); the packed operands are the "A" inputs of dp_conv_gemm (forward: [(tap, ci)][Cout], input
// gradient: [(flipped tap, co)][Cin]).
// ---------------------------------------------------------------------------------------------
#define DP_PACK_BATCH 64
struct PackBatch {
    int n;
    dp_pack_item it[DP_PACK_BATCH];
};
// One thread per (k, m) element of the operand: it reads the layer's taps for that (output, input) channel pair ONCE (36 bytes for a
// 3x3 weight) and writes every tap / Winograd position of it -- the stores of a wavefront are m-contiguous for each of them.  (Round
// 6: the first version ran one thread per OUTPUT element and re-read the nine taps for each of the 12 / 16 positions: 114 us per
// launch of 64 layers of the pruned CIFAR UNet.)  The expressions per output are those of pack_weight_kernel (gemm.hip),
// pack_weight_wino_kernel (winograd.hip) and pack_weight_wino2d_kernel (winograd2d.hip): same bits.
__global__ __launch_bounds__(256) void pack_weight_batch_kernel(const PackBatch b) {
    int i = 0;
    while (i + 1 < b.n && (int)blockIdx.x >= b.it[i + 1].blk0) ++i;
    const dp_pack_item& it = b.it[i];
    const long long step = (long long)it.nblk * 256;
    const int wm = it.mode & 1, kind = it.mode >> 1;             // kind 0: taps as they are, 1: F(2, 3) operand, 2: F(2x2, 3x3) operand
    const int K = wm == 0 ? it.Ci : it.Co, Mv = wm == 0 ? it.Co : it.Ci;
    const int ld = it.ld, taps = it.taps;
    const long long nkm = (long long)K * ld;
    float* __restrict__ dst = it.dst;
    for (long long e = (long long)((int)blockIdx.x - it.blk0) * 256 + threadIdx.x; e < nkm; e += step) {
        const int m = (int)(e % ld);
        const int k = (int)(e / ld);
        const bool ok = m < Mv;
        const float* w = it.W + (wm == 0 ? ((long long)m * it.Ci + k) : ((long long)k * it.Ci + m)) * taps;
        if (kind == 0) {
            for (int tap = 0; tap < taps; ++tap)
                dst[((long long)tap * K + k) * ld + m] = ok ? (wm == 0 ? w[tap] : w[taps - 1 - tap]) : 0.f;
            continue;
        }
        float g[9];
#pragma unroll
        for (int t = 0; t < 9; ++t) g[t] = ok ? w[t] : 0.f;
        if (kind == 1) {
#pragma unroll
            for (int ky = 0; ky < 3; ++ky) {
                const int r = wm == 0 ? ky : 2 - ky;
                const float g0 = wm == 0 ? g[r * 3] : g[r * 3 + 2], g1 = g[r * 3 + 1], g2 = wm == 0 ? g[r * 3 + 2] : g[r * 3];
                const float v[4] = {g0, ((g0 + g1) + g2) * 0.5f, ((g0 - g1) + g2) * 0.5f, g2};
#pragma unroll
                for (int pos = 0; pos < 4; ++pos) dst[((long long)(ky * 4 + pos) * K + k) * ld + m] = ok ? v[pos] : 0.f;
            }
            continue;
        }
        float gg[3][3];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int c = 0; c < 3; ++c) gg[a][c] = wm == 0 ? g[a * 3 + c] : g[(2 - a) * 3 + (2 - c)];
#pragma unroll
        for (int ii = 0; ii < 4; ++ii) {
            float t[3];
#pragma unroll
            for (int c = 0; c < 3; ++c)
                t[c] = ii == 0 ? gg[0][c] : ii == 1 ? ((gg[0][c] + gg[1][c]) + gg[2][c]) * 0.5f : ii == 2 ? ((gg[0][c] - gg[1][c]) + gg[2][c]) * 0.5f : gg[2][c];
            const float v[4] = {t[0], ((t[0] + t[1]) + t[2]) * 0.5f, ((t[0] - t[1]) + t[2]) * 0.5f, t[2]};
#pragma unroll
            for (int j = 0; j < 4; ++j) dst[((long long)(ii * 4 + j) * K + k) * ld + m] = ok ? v[j] : 0.f;
        }
    }
}
extern "C" int dp_pack_weight_batch(const dp_pack_item* items, int n, void* stream) {
    for (int lo = 0; lo < n; lo += DP_PACK_BATCH) {
        PackBatch b;
        b.n = (n - lo < DP_PACK_BATCH) ? n - lo : DP_PACK_BATCH;
        int blocks = 0;
        for (int i = 0; i < b.n; ++i) {
            b.it[i] = items[lo + i];
            dp_pack_item& it = b.it[i];
            if (it.Co <= 0 || it.Ci <= 0 || it.taps <= 0 || it.ld <= 0 || it.mode < 0 || it.mode > 5) return (int)hipErrorInvalidValue;
            if (it.mode >= 2 && it.taps != 9) return (int)hipErrorInvalidValue;
            const long long total = (long long)((it.mode & 1) == 0 ? it.Ci : it.Co) * it.ld;        // one thread per (k, m)
            long long nb = (total + 255) / 256;
            if (nb > 1024) nb = 1024;
            it.blk0 = blocks;
            it.nblk = (int)nb;
            blocks += (int)nb;
        }
        DP_LAUNCH(pack_weight_batch_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, b);
    }
    return DP_LAUNCH_CHECK();
}
