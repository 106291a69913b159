// The elementwise kernel of the ldm_exp samplers (ldm_exp/ldm/models/diffusion/ddim.py:165-203, plms.py:173-236):
//   dp_cfg_denoise_step  classifier-free guidance, the PLMS extrapolation of eps, the x0 prediction and the DDIM update in ONE
//                        pass per model evaluation.  It reads the [2B, C, H, W] eps of forward_cfg_pair in place (unconditional
//                        half at e_u, conditional half at e_c = e_u + n: no chunk copies) and writes the next state and, when
//                        asked for, the x0 prediction the reference logs and the guided eps that PLMS keeps as history.
// It is memory bound and small beside the UNet forward of a sampling step (four tensors, 9.8 MB, at [50, 3, 64, 64] beside
// a 100-row forward), exactly as sampler.hip says of its own kernels.  Its value is not speed: it is one pass instead of
// the two launches of dp_cfg_combine + dp_ddim_step, the reference's rounding, and the x0 prediction for free.
//
// Rounding: every operation of the reference's expressions is rounded separately (clang fp contract(off): hipcc would otherwise
// fuse a * b + c into one v_fma_f32), the divisions are true IEEE divisions, and the five per-step scalars arrive from the host
// (ldm_sampler.sampling_tables), which forms them as the reference's torch.full((b, 1, 1, 1), table[index]) and the fp32 ops
// that follow it do.  dp_cfg_combine / dp_ddim_step (elementwise.hip) share no device code with this file and are unchanged.
#include "dp_headtail.h"

struct CfgDenoiseCoef {
    float scale, s1m, sqrt_a_t, sqrt_a_prev, c_dir, sigma, temperature;
};

// ORDER: how e' is formed from the guided eps e_g and the history h1 (newest) .. h3 (oldest)
//   0  e' = e_g                                        DDIM; the first of the two evaluations of PLMS's first step
//   1  e' = (3 e_g - h1) / 2                           plms.py:226
//   2  e' = (23 e_g - 16 h1 + 5 h2) / 12               plms.py:229
//   3  e' = (55 e_g - 59 h1 + 37 h2 - 9 h3) / 24       plms.py:232
//   4  e' = (h1 + e_g) / 2                             plms.py:223 (h1 = the stored e_t, e_g = e_t_next)
template <int ORDER>
__device__ __forceinline__ float cfg_extrapolate(float eg, float h1, float h2, float h3) {
#pragma clang fp contract(off)
    if (ORDER == 1) {
        const float a = 3.0f * eg;
        return (a - h1) / 2.0f;
    }
    if (ORDER == 2) {
        const float a = 23.0f * eg;
        const float b = 16.0f * h1;
        const float c = 5.0f * h2;
        const float s = a - b;
        return (s + c) / 12.0f;
    }
    if (ORDER == 3) {
        const float a = 55.0f * eg;
        const float b = 59.0f * h1;
        const float c = 37.0f * h2;
        const float d = 9.0f * h3;
        const float s = a - b;
        const float t = s + c;
        return (t - d) / 24.0f;
    }
    if (ORDER == 4) return (h1 + eg) / 2.0f;
    return eg;
}

// e_g = e_u + scale * (e_c - e_u)                   ddim.py:177 (GUIDED; otherwise e_g = e_u, the model's one output)
// x0  = (x - s1m * e') / sqrt_a_t                   ddim.py:194
// dir = c_dir * e'                                  ddim.py:198
// nz  = (sigma * z) * temperature                   ddim.py:199 (absent when z is null)
// nxt = (sqrt_a_prev * x0 + dir) + nz               ddim.py:202
template <int ORDER, bool GUIDED>
__device__ __forceinline__ float cfg_denoise_one(float x, float eu, float ec, float h1, float h2, float h3, float z, bool has_z,
                                                 const CfgDenoiseCoef& c, float& x0, float& eg) {
#pragma clang fp contract(off)
    eg = eu;
    if (GUIDED) {
        const float d = ec - eu;
        const float m = c.scale * d;
        eg = eu + m;
    }
    const float ep = cfg_extrapolate<ORDER>(eg, h1, h2, h3);
    const float se = c.s1m * ep;
    x0 = (x - se) / c.sqrt_a_t;
    const float dir = c.c_dir * ep;
    const float ax = c.sqrt_a_prev * x0;
    float v = ax + dir;
    if (has_z) {
        const float sz = c.sigma * z;
        const float nz = sz * c.temperature;
        v = v + nz;
    }
    return v;
}

// The head / body / tail loop of dp_headtail.h (all scalar with e_c = e_u + n and n % 4 != 0, for one).  `next` may be `x` itself
// (no __restrict__ on the two): an element is read and written by the same lane, in that order.  x0_out and eg_out alias nothing.
// A history pointer ORDER does not read is never touched.
template <int ORDER, bool GUIDED>
__global__ __launch_bounds__(256) void cfg_denoise_step_kernel(const float* x, const float* __restrict__ e_u,
                                                               const float* __restrict__ e_c, const float* __restrict__ h1,
                                                               const float* __restrict__ h2, const float* __restrict__ h3,
                                                               const float* __restrict__ z, CfgDenoiseCoef c, float* next,
                                                               float* __restrict__ x0_out, float* __restrict__ eg_out, long long n,
                                                               long long head) {
    constexpr bool H1 = ORDER >= 1, H2 = ORDER == 2 || ORDER == 3, H3 = ORDER == 3;
    const bool has_z = z != nullptr;
    dp_ht_for(
        n, head, (long long)blockIdx.x * 256 + threadIdx.x, (long long)gridDim.x * 256,
        [&](long long at) {
            const float4 xv = dp_ld4(x, at, true), uv = dp_ld4(e_u, at, true), cv = dp_ld4(e_c, at, GUIDED);
            const float4 av = dp_ld4(h1, at, H1), bv = dp_ld4(h2, at, H2), dv = dp_ld4(h3, at, H3), zv = dp_ld4(z, at, has_z);
            float4 ov, pv, gv;
            ov.x = cfg_denoise_one<ORDER, GUIDED>(xv.x, uv.x, cv.x, av.x, bv.x, dv.x, zv.x, has_z, c, pv.x, gv.x);
            ov.y = cfg_denoise_one<ORDER, GUIDED>(xv.y, uv.y, cv.y, av.y, bv.y, dv.y, zv.y, has_z, c, pv.y, gv.y);
            ov.z = cfg_denoise_one<ORDER, GUIDED>(xv.z, uv.z, cv.z, av.z, bv.z, dv.z, zv.z, has_z, c, pv.z, gv.z);
            ov.w = cfg_denoise_one<ORDER, GUIDED>(xv.w, uv.w, cv.w, av.w, bv.w, dv.w, zv.w, has_z, c, pv.w, gv.w);
            dp_st4(next, at, ov);
            if (x0_out) dp_st4(x0_out, at, pv);
            if (eg_out) dp_st4(eg_out, at, gv);
        },
        [&](long long i) {
            float p, g;
            const float v = cfg_denoise_one<ORDER, GUIDED>(x[i], e_u[i], dp_ld1(e_c, i, GUIDED), dp_ld1(h1, i, H1), dp_ld1(h2, i, H2),
                                                           dp_ld1(h3, i, H3), dp_ld1(z, i, has_z), has_z, c, p, g);
            next[i] = v;
            if (x0_out) x0_out[i] = p;
            if (eg_out) eg_out[i] = g;
        });
}

// literal template arguments, so that the name DP_LAUNCH records says which instantiation ran
#define CFG_DENOISE_CASE(ORDER)                                                                                                  \
    case ORDER:                                                                                                                  \
        if (e_c)                                                                                                                 \
            DP_LAUNCH((cfg_denoise_step_kernel<ORDER, true>), dim3(grid), dim3(256), 0, s, x, e_u, e_c, h1, h2, h3, z, c, next,  \
                      x0_out, eg_out, n, head);                                                                                  \
        else                                                                                                                     \
            DP_LAUNCH((cfg_denoise_step_kernel<ORDER, false>), dim3(grid), dim3(256), 0, s, x, e_u, e_c, h1, h2, h3, z, c, next, \
                      x0_out, eg_out, n, head);                                                                                  \
        break;

extern "C" int dp_cfg_denoise_step(const float* x, const float* e_u, const float* e_c, float scale, int order, const float* h1,
                                   const float* h2, const float* h3, float s1m, float sqrt_a_t, float sqrt_a_prev, float c_dir,
                                   float sigma, float temperature, const float* z, float* next, float* x0_out, float* eg_out,
                                   long long n, void* stream) {
    if (n <= 0) return 0;
    if (!x || !e_u || !next || order < 0 || order > 4) return (int)hipErrorInvalidValue;
    const bool need1 = order >= 1, need2 = order == 2 || order == 3, need3 = order == 3;
    if ((need1 && !h1) || (need2 && !h2) || (need3 && !h3)) return (int)hipErrorInvalidValue;
    // only the pointers that are read or written count: a history pointer the order does not read is left out
    const void* ptrs[10] = {x, e_u, next, e_c, need1 ? h1 : nullptr, need2 ? h2 : nullptr, need3 ? h3 : nullptr, z, x0_out, eg_out};
    const long long head = dp_ht_head(n, ptrs, 10);
    const unsigned grid = dp_ht_blocks(n, head, DP_DENOISE_MAX_BLOCKS);
    const CfgDenoiseCoef c{scale, s1m, sqrt_a_t, sqrt_a_prev, c_dir, sigma, temperature};
    const hipStream_t s = (hipStream_t)stream;
    switch (order) {
        CFG_DENOISE_CASE(0)
        CFG_DENOISE_CASE(1)
        CFG_DENOISE_CASE(2)
        CFG_DENOISE_CASE(3)
        CFG_DENOISE_CASE(4)
    }
    return DP_LAUNCH_CHECK();
}
