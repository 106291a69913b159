// Fused finetune update over flat parameter / gradient / moment / EMA buffers (HBM-bound, one pass):
//   global-norm clip (ddpm_train.py:462) -> Adam (ddpm_train.py:331-337,463; torch.optim.Adam, wd = 0)
//   -> EMA with constant decay (diffusers/training_utils.py:201,215-216).
#include "dp_common.h"

__global__ __launch_bounds__(256) void sumsq_kernel(const float* __restrict__ x, long long n, float* __restrict__ partial) {
    __shared__ float red[4];
    const long long per = (n + gridDim.x - 1) / gridDim.x;
    const long long lo = (long long)blockIdx.x * per;
    long long hi = lo + per;
    if (hi > n) hi = n;
    float s = 0.f;
    for (long long i = lo + threadIdx.x; i < hi; i += 256) s += x[i] * x[i];
    s = dp_block_sum_256(s, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = s;
}
extern "C" int dp_sumsq_partials(const float* x, long long n, float* partial, int nblocks, void* stream) {
    if (nblocks <= 0) return (int)hipErrorInvalidValue;
    DP_LAUNCH(sumsq_kernel, dim3(nblocks), dim3(256), 0, (hipStream_t)stream, x, n, partial);
    return DP_LAUNCH_CHECK();
}

__global__ __launch_bounds__(256) void clip_coef_kernel(const float* __restrict__ partial, int n, float max_norm,
                                                        float* __restrict__ norm_out, float* __restrict__ coef_out) {
    __shared__ float red[4];
    float s = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) s += partial[i];
    s = dp_block_sum_256(s, red);
    if (threadIdx.x == 0) {
        const float nrm = sqrtf(s);
        norm_out[0] = nrm;
        const float c = max_norm / (nrm + 1e-6f);
        coef_out[0] = c < 1.0f ? c : 1.0f;
    }
}
extern "C" int dp_clip_coef(const float* partial, int n, float max_norm, float* norm_out, float* coef_out, void* stream) {
    DP_LAUNCH(clip_coef_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partial, n, max_norm, norm_out, coef_out);
    return DP_LAUNCH_CHECK();
}

// The Adam + EMA pass both launch variants run: they differ in where {lr, bc1, bc2} come from only.
__device__ __forceinline__ void adam_ema_pass(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                              float* __restrict__ v, float* __restrict__ ema, long long n,
                                              const float* __restrict__ clip_coef, float lr, float b1, float b2, float eps,
                                              float bc1, float bc2, float ema_decay) {
    const float coef = clip_coef ? clip_coef[0] : 1.0f;
    const float step_size = lr / bc1;
    const float inv_sqrt_bc2 = 1.0f / sqrtf(bc2);
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const float gi = g[i] * coef;
        const float mi = b1 * m[i] + (1.0f - b1) * gi;
        const float vi = b2 * v[i] + (1.0f - b2) * gi * gi;
        m[i] = mi;
        v[i] = vi;
        const float denom = sqrtf(vi) * inv_sqrt_bc2 + eps;
        const float pi = p[i] - step_size * (mi / denom);
        p[i] = pi;
        if (ema) ema[i] = (1.0f - ema_decay) * pi + ema_decay * ema[i];
    }
}

__global__ __launch_bounds__(256) void adam_ema_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                       float* __restrict__ v, float* __restrict__ ema, long long n,
                                                       const float* __restrict__ clip_coef, float lr, float b1, float b2,
                                                       float eps, float bc1, float bc2, float ema_decay) {
    adam_ema_pass(p, g, m, v, ema, n, clip_coef, lr, b1, b2, eps, bc1, bc2, ema_decay);
}
extern "C" int dp_adam_ema(float* p, const float* g, float* m, float* v, float* ema, long long n, const float* clip_coef,
                           float lr, float b1, float b2, float eps, float bc1, float bc2, float ema_decay, void* stream) {
    if (n <= 0) return 0;
    long long nb = (n + 255) / 256;
    if (nb > 8192) nb = 8192;
    DP_LAUNCH(adam_ema_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, p, g, m, v, ema, n, clip_coef,
                       lr, b1, b2, eps, bc1, bc2, ema_decay);
    return DP_LAUNCH_CHECK();
}

// ---- the same update with the per-step scalars on the device (a captured finetune step replays with unchanged kernel arguments)
__global__ void set_step_scalars_kernel(float* __restrict__ hyper, float lr, float bc1, float bc2, unsigned step) {
    hyper[0] = lr;
    hyper[1] = bc1;
    hyper[2] = bc2;
    reinterpret_cast<unsigned*>(hyper)[3] = step;
}
extern "C" int dp_set_step_scalars(float* hyper, float lr, float bc1, float bc2, unsigned step, void* stream) {
    DP_LAUNCH(set_step_scalars_kernel, dim3(1), dim3(1), 0, (hipStream_t)stream, hyper, lr, bc1, bc2, step);
    return DP_LAUNCH_CHECK();
}

__global__ __launch_bounds__(256) void adam_ema_dev_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                           float* __restrict__ v, float* __restrict__ ema, long long n,
                                                           const float* __restrict__ clip_coef, const float* __restrict__ hyper,
                                                           float b1, float b2, float eps, float ema_decay) {
    adam_ema_pass(p, g, m, v, ema, n, clip_coef, hyper[0], b1, b2, eps, hyper[1], hyper[2], ema_decay);
}
extern "C" int dp_adam_ema_dev(float* p, const float* g, float* m, float* v, float* ema, long long n, const float* clip_coef,
                               const float* hyper, float b1, float b2, float eps, float ema_decay, void* stream) {
    if (n <= 0) return 0;
    if (!hyper) return (int)hipErrorInvalidValue;
    long long nb = (n + 255) / 256;
    if (nb > 8192) nb = 8192;
    DP_LAUNCH(adam_ema_dev_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, p, g, m, v, ema, n, clip_coef, hyper,
                       b1, b2, eps, ema_decay);
    return DP_LAUNCH_CHECK();
}


// ---- LDM finetune update (ldm_exp/ldm/models/diffusion/ddpm.py:1372-1381, ldm/modules/ema.py): torch.optim.AdamW (single tensor,
// amsgrad = False, maximize = False) in torch's order of operations, then LitEma's `s -= (1 - decay) (s - p)`.  The host forms
// p_scale = 1 - lr wd, step_size = lr / bc1 and sqrt_bc2 in double and rounds them to fp32 once, as torch does; `decay` is
// LitEma's fp32 decay after its warm-up.  28 B per element (36 with the shadow) and nothing else: 16-byte accesses per lane,
// the n % 4 tail (or buffers that are not 16-byte aligned) by 4-byte accesses.
struct adamw_scalars {
    float p_scale, omb1, b2, omb2, sqrt_bc2, eps, step_size, decay;
};

__device__ __forceinline__ void adamw_one(float& p, float g, float& m, float& v, float& s, bool has_ema, const adamw_scalars& c) {
#pragma clang fp contract(off)      // torch's AdamW rounds after every operation: no fused multiply-add across them
    float pi = p * c.p_scale;                            // param.mul_(1 - lr * weight_decay)
    const float mi = m + (g - m) * c.omb1;               // exp_avg.lerp_(grad, 1 - beta1), weight < 0.5
    const float vi = v * c.b2 + c.omb2 * g * g;          // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
    const float denom = sqrtf(vi) / c.sqrt_bc2 + c.eps;
    pi = pi - c.step_size * (mi / denom);                // param.addcdiv_(exp_avg, denom, value=-step_size)
    p = pi;
    m = mi;
    v = vi;
    if (has_ema) s = dp_lit_ema(s, pi, 1.0f - c.decay);  // shadow.sub_(one_minus_decay * (shadow - param))
}

template <bool VEC>
__global__ __launch_bounds__(256) void adamw_ema_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                        float* __restrict__ v, float* __restrict__ ema, long long n,
                                                        const float* __restrict__ clip_coef, adamw_scalars c) {
    const float coef = clip_coef ? clip_coef[0] : 1.0f;
    const bool has_ema = ema != nullptr;
    const long long tid = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long stride = (long long)gridDim.x * 256;
    const long long n4 = VEC ? n / 4 : 0;
    if (VEC) {
        float4* p4 = reinterpret_cast<float4*>(p);
        const float4* g4 = reinterpret_cast<const float4*>(g);
        float4* m4 = reinterpret_cast<float4*>(m);
        float4* v4 = reinterpret_cast<float4*>(v);
        float4* s4 = reinterpret_cast<float4*>(ema);
        for (long long i = tid; i < n4; i += stride) {
            float4 pi = p4[i], gi = g4[i], mi = m4[i], vi = v4[i];
            float4 si = has_ema ? s4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
            if (clip_coef) { gi.x *= coef; gi.y *= coef; gi.z *= coef; gi.w *= coef; }
            adamw_one(pi.x, gi.x, mi.x, vi.x, si.x, has_ema, c);
            adamw_one(pi.y, gi.y, mi.y, vi.y, si.y, has_ema, c);
            adamw_one(pi.z, gi.z, mi.z, vi.z, si.z, has_ema, c);
            adamw_one(pi.w, gi.w, mi.w, vi.w, si.w, has_ema, c);
            p4[i] = pi;
            m4[i] = mi;
            v4[i] = vi;
            if (has_ema) s4[i] = si;
        }
    }
    for (long long i = 4 * n4 + tid; i < n; i += stride) {       // the scalar tail (everything when !VEC)
        float pi = p[i], mi = m[i], vi = v[i], si = has_ema ? ema[i] : 0.f;
        const float gi = clip_coef ? g[i] * coef : g[i];
        adamw_one(pi, gi, mi, vi, si, has_ema, c);
        p[i] = pi;
        m[i] = mi;
        v[i] = vi;
        if (has_ema) ema[i] = si;
    }
}
extern "C" int dp_adamw_ema(float* p, const float* g, float* m, float* v, float* ema, long long n, const float* clip_coef,
                            float p_scale, float one_minus_b1, float b2, float one_minus_b2, float sqrt_bc2, float eps,
                            float step_size, float ema_decay, void* stream) {
    if (n <= 0) return 0;
    if (!p || !g || !m || !v) return (int)hipErrorInvalidValue;
    const adamw_scalars c = {p_scale, one_minus_b1, b2, one_minus_b2, sqrt_bc2, eps, step_size, ema_decay};
    bool vec;
    const unsigned nb = dp_flat_grid((uintptr_t)p | (uintptr_t)g | (uintptr_t)m | (uintptr_t)v | (uintptr_t)ema, n, &vec);
    if (vec)
        DP_LAUNCH(adamw_ema_kernel<true>, dim3(nb), dim3(256), 0, (hipStream_t)stream, p, g, m, v, ema, n, clip_coef, c);
    else
        DP_LAUNCH(adamw_ema_kernel<false>, dim3(nb), dim3(256), 0, (hipStream_t)stream, p, g, m, v, ema, n, clip_coef, c);
    return DP_LAUNCH_CHECK();
}

// ---- gradient of the class-embedding lookup (ldm/modules/encoders/modules.py:21-33 under autograd):
// dW[ids[b], :] += dctx[b, :], rows of one id added in ascending b, without float atomics.  One wave per batch row b: it
// builds the bit mask of the rows that carry its id (one ballot per 64 rows), leaves if an earlier row does (that row's wave
// owns the id), else walks the mask upwards, each lane keeping its columns of the sum in a register.  Ids are range-checked
// by the caller; B <= 4096.
__global__ __launch_bounds__(64) void embedding_bwd_kernel(const long long* __restrict__ ids, const float* __restrict__ dctx,
                                                           int B, int D, float* __restrict__ dW) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const long long id = ids[b];
    const int words = (B + 63) >> 6;
    __shared__ unsigned long long mask[64];
    for (int w = 0; w < words; ++w) {
        const int j = (w << 6) + lane;
        const unsigned long long bal = __ballot(j < B && ids[j] == id);
        if (lane == 0) mask[w] = bal;
    }
    __syncthreads();
    const int wb = b >> 6;
    for (int w = 0; w < wb; ++w)
        if (mask[w]) return;                             // an earlier row holds this id
    if (mask[wb] & ((1ull << (b & 63)) - 1ull)) return;
    float* __restrict__ row = dW + id * (long long)D;
    for (int d = lane; d < D; d += 64) {
        float acc = row[d];
        for (int w = wb; w < words; ++w) {
            unsigned long long bits = mask[w];
            while (bits) {
                const int j = (w << 6) + __ffsll((long long)bits) - 1;
                bits &= bits - 1ull;
                acc += dctx[(long long)j * D + d];
            }
        }
        row[d] = acc;
    }
}
extern "C" int dp_embedding_bwd(const long long* ids, const float* dctx, int B, int D, float* dW, void* stream) {
    if (B <= 0 || D <= 0) return 0;
    if (B > 4096 || !ids || !dctx || !dW) return (int)hipErrorInvalidValue;
    DP_LAUNCH(embedding_bwd_kernel, dim3((unsigned)B), dim3(64), 0, (hipStream_t)stream, ids, dctx, B, D, dW);
    return DP_LAUNCH_CHECK();
}
