// The elementwise kernels of the sigma-space (k-diffusion) schedulers (diffusers/schedulers/scheduling_euler_discrete.py,
// scheduling_euler_ancestral_discrete.py, scheduling_heun_discrete.py):
//   dp_sigma_step       one scheduler call in ONE pass: the optional churn, the conversion of the model output to x0, the ODE
//                       derivative and the update; x, e (and the noise, the saved derivative and sample where the mode has them) are
//                       read once, x' and the mode's second output written once.  The reference runs six to ten elementwise launches.
//   dp_sigma_scale      scale_model_input: out = x / c, c = (sigma^2 + 1) ** 0.5 from the host
//   dp_sigma_add_noise  add_noise: out = x0 + noise * sigma[b], one fp32 sigma per image
// x: the sample, e: the model output, z: the noise, d1: the derivative HEUN1 stored, xs: the sample HEUN1 was handed.  sig is
// sigma_hat (EULER, HEUN1), sigma (ANCESTRAL) or sigma_next (HEUN2); c_out and c_den belong to the same sigma (EULER: to sigma).
//   x0        EPSILON  xh - sig * e;   V  e * c_out + xh / c_den;   SAMPLE  e
//   EULER     xh = z ? x + (z * s_noise) * k : x;  d = (xh - x0) / sig;  x' = xh + d * dt;                 aux = x0
//   ANCESTRAL xh = x;  d = (x - x0) / sig;  x' = (x + d * dt) + z * sigma_up;                               aux = x0
//   HEUN1     xh = x;  d = (x - x0) / sig;  x' = x + d * dt;                                                aux = d
//   HEUN2     xh = x;  d2 = (x - x0) / sig;  d = (d1 + d2) / 2;  x' = xs + d * dt
//
// Rounding: every operation above is rounded separately (clang fp contract(off): hipcc would otherwise fuse a * b + c into one
// v_fma_f32), the divisions are true IEEE divisions, and the scalars arrive from the host, which forms them with 0-d fp32 torch ops in
// the reference's order (diffusion._SigmaSchedulerBase).
//
// Memory bound: at most 4 x (4 reads + 1 write) B per element (HEUN2), 16-byte accesses, nothing else.  Plain vector loads and stores.
#include "dp_headtail.h"

// The launch macro of this file: the body of the library's own (dp_common.h) under a name of its own, so that the launch sites of
// this file are tabled by this file's test module (tests/test_sigma_gpu.py), as pndm.hip and repaint.hip do.
#define SG_LAUNCH(k, ...) do { dp_launch_names[dp_launches++ & (DP_LAUNCH_RING - 1)] = #k; hipLaunchKernelGGL(k, __VA_ARGS__); } while (0)

template <int MODE, int PRED>
__device__ __forceinline__ float sigma_one(float x, float e, float z, float d1, float xs, bool churn, const dp_sigma_coef& c, float& aux) {
#pragma clang fp contract(off)
    float xh = x;
    if (MODE == DP_SIGMA_EULER && churn) {
        const float eps = z * c.s_noise;
        const float t = eps * c.k;
        xh = x + t;
    }
    float x0;
    if (PRED == DP_SIGMA_EPSILON) {
        const float t = c.sig * e;
        x0 = xh - t;
    } else if (PRED == DP_SIGMA_V) {
        const float p = e * c.c_out;
        const float q = xh / c.c_den;
        x0 = p + q;
    } else {
        x0 = e;
    }
    const float diff = xh - x0;
    float d = diff / c.sig;
    aux = MODE == DP_SIGMA_HEUN1 ? d : x0;
    if (MODE == DP_SIGMA_HEUN2) {
        const float s = d1 + d;
        d = s / 2.f;
        xh = xs;
    }
    const float step = d * c.dt;
    float r = xh + step;
    if (MODE == DP_SIGMA_ANCESTRAL) {
        const float t = z * c.sigma_up;
        r = r + t;
    }
    return r;
}

// The head / body / tail loop of dp_headtail.h.  `next` may be `x` itself (in HEUN2 `xs` itself), so neither carries __restrict__: a
// lane reads every input of its elements before it writes any of them, and no other lane touches them.
template <int MODE, int PRED>
__global__ __launch_bounds__(256) void sigma_step_kernel(const float* x, const float* __restrict__ e, const float* __restrict__ z,
                                                         const float* __restrict__ d1, const float* xs, dp_sigma_coef c, float* next,
                                                         float* __restrict__ aux, long long n, long long head) {
    constexpr bool Z = MODE == DP_SIGMA_EULER || MODE == DP_SIGMA_ANCESTRAL, H2 = MODE == DP_SIGMA_HEUN2;
    const bool noisy = Z && z != nullptr;
    dp_ht_for(
        n, head, (long long)blockIdx.x * 256 + threadIdx.x, (long long)gridDim.x * 256,
        [&](long long at) {
            const float4 xv = dp_ld4(x, at, true), ev = dp_ld4(e, at, true), zv = dp_ld4(z, at, noisy);
            const float4 dv = dp_ld4(d1, at, H2), sv = dp_ld4(xs, at, H2);
            float4 ov, av;
            ov.x = sigma_one<MODE, PRED>(xv.x, ev.x, zv.x, dv.x, sv.x, noisy, c, av.x);
            ov.y = sigma_one<MODE, PRED>(xv.y, ev.y, zv.y, dv.y, sv.y, noisy, c, av.y);
            ov.z = sigma_one<MODE, PRED>(xv.z, ev.z, zv.z, dv.z, sv.z, noisy, c, av.z);
            ov.w = sigma_one<MODE, PRED>(xv.w, ev.w, zv.w, dv.w, sv.w, noisy, c, av.w);
            dp_st4(next, at, ov);                                    // after every load of this lane's elements
            if (!H2) dp_st4(aux, at, av);
        },
        [&](long long i) {
            const float xx = x[i], ee = e[i], zz = dp_ld1(z, i, noisy), dd = dp_ld1(d1, i, H2), ss = dp_ld1(xs, i, H2);
            float a;
            const float v = sigma_one<MODE, PRED>(xx, ee, zz, dd, ss, noisy, c, a);
            next[i] = v;
            if (!H2) aux[i] = a;
        });
}

// out may be x itself
__global__ __launch_bounds__(256) void sigma_scale_kernel(const float* x, float c, float* out, long long n, long long head) {
    dp_ht_for(
        n, head, (long long)blockIdx.x * 256 + threadIdx.x, (long long)gridDim.x * 256,
        [&](long long at) {
            const float4 v = dp_ld4(x, at, true);
            dp_st4(out, at, make_float4(v.x / c, v.y / c, v.z / c, v.w / c));
        },
        [&](long long i) { out[i] = x[i] / c; });
}

__device__ __forceinline__ float sigma_noised(float x0, float z, float s) {
#pragma clang fp contract(off)
    const float t = z * s;
    return x0 + t;
}

// element i belongs to image i / per: a 16-byte group may straddle two or more images (per is any positive number)
__global__ __launch_bounds__(256) void sigma_add_noise_kernel(const float* __restrict__ x0, const float* __restrict__ z,
                                                              const float* __restrict__ sigma, long long per, float* __restrict__ out,
                                                              long long n, long long head) {
    dp_ht_for(
        n, head, (long long)blockIdx.x * 256 + threadIdx.x, (long long)gridDim.x * 256,
        [&](long long at) {
            const float4 xv = dp_ld4(x0, at, true), zv = dp_ld4(z, at, true);
            const long long b = at / per, left = per - (at - b * per);       // elements of image b from `at` on: >= 1
            const float s0 = sigma[b];
            float4 ov;
            if (left >= 4) {
                ov = make_float4(sigma_noised(xv.x, zv.x, s0), sigma_noised(xv.y, zv.y, s0), sigma_noised(xv.z, zv.z, s0),
                                 sigma_noised(xv.w, zv.w, s0));
            } else {                                                         // at + 3 < n: every index below is inside sigma[B]
                ov.x = sigma_noised(xv.x, zv.x, s0);
                ov.y = sigma_noised(xv.y, zv.y, sigma[(at + 1) / per]);
                ov.z = sigma_noised(xv.z, zv.z, sigma[(at + 2) / per]);
                ov.w = sigma_noised(xv.w, zv.w, sigma[(at + 3) / per]);
            }
            dp_st4(out, at, ov);
        },
        [&](long long i) { out[i] = sigma_noised(x0[i], z[i], sigma[i / per]); });
}

extern "C" int dp_sigma_step(const float* x, const float* e, const float* z, const float* d1, const float* xs, int mode, int pred,
                             const dp_sigma_coef* coef, float* x_next, float* aux_out, long long n, void* stream) {
    if (n <= 0) return 0;
    if (!x || !e || !coef || !x_next || mode < DP_SIGMA_EULER || mode > DP_SIGMA_HEUN2) return (int)hipErrorInvalidValue;
    if (pred < DP_SIGMA_EPSILON || pred > DP_SIGMA_SAMPLE || (pred == DP_SIGMA_SAMPLE && mode != DP_SIGMA_EULER)) return (int)hipErrorInvalidValue;
    if (mode != DP_SIGMA_EULER && mode != DP_SIGMA_ANCESTRAL) z = nullptr;       // not read by this mode
    if (mode != DP_SIGMA_HEUN2) d1 = xs = nullptr;
    if (mode == DP_SIGMA_HEUN2) aux_out = nullptr;                               // not written by this mode
    if ((mode == DP_SIGMA_ANCESTRAL && !z) || (mode == DP_SIGMA_HEUN2 && (!d1 || !xs)) || (mode != DP_SIGMA_HEUN2 && !aux_out))
        return (int)hipErrorInvalidValue;
    // the aliases the kernel is written for: x_next == x, and in HEUN2 x_next == xs.  Everything else is disjoint: no output shares a
    // byte with the other output or with an input that is not itself.
    const unsigned long long len = 4ull * (unsigned long long)n;
    const auto hit = [len](const void* a, const void* b) { return dp_bytes_overlap(a, len, b, len); };
    if ((x_next != x && hit(x_next, x)) || (x_next != xs && hit(x_next, xs))) return (int)hipErrorInvalidValue;
    if (hit(x_next, e) || hit(x_next, z) || hit(x_next, d1) || hit(x_next, aux_out)) return (int)hipErrorInvalidValue;
    if (hit(aux_out, x) || hit(aux_out, e) || hit(aux_out, z)) return (int)hipErrorInvalidValue;
    const void* ptrs[7] = {x, e, z, d1, xs, x_next, aux_out};
    const long long head = dp_ht_head(n, ptrs, 7);
    const unsigned grid = dp_ht_blocks(n, head, DP_SIGMA_MAX_BLOCKS);
    const dp_sigma_coef c = *coef;
    const hipStream_t st = (hipStream_t)stream;
#define SG_ARGS dim3(grid), dim3(256), 0, st, x, e, z, d1, xs, c, x_next, aux_out, n, head
    // one site per instantiation: the launch ring keeps the stringised kernel expression of the site that launched
    switch (3 * mode + pred) {
        case 0: SG_LAUNCH((sigma_step_kernel<DP_SIGMA_EULER, DP_SIGMA_EPSILON>), SG_ARGS); break;
        case 1: SG_LAUNCH((sigma_step_kernel<DP_SIGMA_EULER, DP_SIGMA_V>), SG_ARGS); break;
        case 2: SG_LAUNCH((sigma_step_kernel<DP_SIGMA_EULER, DP_SIGMA_SAMPLE>), SG_ARGS); break;
        case 3: SG_LAUNCH((sigma_step_kernel<DP_SIGMA_ANCESTRAL, DP_SIGMA_EPSILON>), SG_ARGS); break;
        case 4: SG_LAUNCH((sigma_step_kernel<DP_SIGMA_ANCESTRAL, DP_SIGMA_V>), SG_ARGS); break;
        case 6: SG_LAUNCH((sigma_step_kernel<DP_SIGMA_HEUN1, DP_SIGMA_EPSILON>), SG_ARGS); break;
        case 7: SG_LAUNCH((sigma_step_kernel<DP_SIGMA_HEUN1, DP_SIGMA_V>), SG_ARGS); break;
        case 9: SG_LAUNCH((sigma_step_kernel<DP_SIGMA_HEUN2, DP_SIGMA_EPSILON>), SG_ARGS); break;
        case 10: SG_LAUNCH((sigma_step_kernel<DP_SIGMA_HEUN2, DP_SIGMA_V>), SG_ARGS); break;
        default: return (int)hipErrorInvalidValue;
    }
#undef SG_ARGS
    return DP_LAUNCH_CHECK();
}

extern "C" int dp_sigma_scale(const float* x, float c, float* out, long long n, void* stream) {
    if (n <= 0) return 0;
    if (!x || !out) return (int)hipErrorInvalidValue;
    const unsigned long long len = 4ull * (unsigned long long)n;
    if (out != x && dp_bytes_overlap(out, len, x, len)) return (int)hipErrorInvalidValue;
    const void* ptrs[2] = {x, out};
    const long long head = dp_ht_head(n, ptrs, 2);
    SG_LAUNCH(sigma_scale_kernel, dim3(dp_ht_blocks(n, head, DP_SIGMA_MAX_BLOCKS)), dim3(256), 0, (hipStream_t)stream, x, c, out, n, head);
    return DP_LAUNCH_CHECK();
}

extern "C" int dp_sigma_add_noise(const float* x0, const float* z, const float* sigma, long long B, long long per, float* out,
                                  void* stream) {
    if (B <= 0 || per <= 0) return 0;
    if (!x0 || !z || !sigma || !out || B > (long long)(0x7fffffffffffffffLL / 4) / per) return (int)hipErrorInvalidValue;
    const long long n = B * per;
    const unsigned long long len = 4ull * (unsigned long long)n;
    if (dp_bytes_overlap(out, len, x0, len) || dp_bytes_overlap(out, len, z, len) || dp_bytes_overlap(out, len, sigma, 4ull * (unsigned long long)B))
        return (int)hipErrorInvalidValue;
    const void* ptrs[3] = {x0, z, out};
    const long long head = dp_ht_head(n, ptrs, 3);
    SG_LAUNCH(sigma_add_noise_kernel, dim3(dp_ht_blocks(n, head, DP_SIGMA_MAX_BLOCKS)), dim3(256), 0, (hipStream_t)stream, x0, z, sigma, per, out,
              n, head);
    return DP_LAUNCH_CHECK();
}
