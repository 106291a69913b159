// The step kernels of the rest of the sigma-space (k-diffusion) family (diffusers/schedulers/scheduling_lms_discrete.py,
// scheduling_k_dpm_2_discrete.py, scheduling_k_dpm_2_ancestral_discrete.py), on the pattern of sigma.hip:
//   dp_kdpm2_step  one call of either KDPM2 class in ONE pass: the conversion of the model output to x0, the ODE derivative and the
//                  update from the sample of this call (first-order state) or from the saved one (second-order state), the ancestral
//                  noise where it is handed one.  At most 4 streams read, 1 written.  The reference runs five to eight launches.
//   dp_lms_step    one linear-multistep call in ONE pass: the conversion, the derivative, the sum over up to four derivatives and the
//                  update; x', the new derivative and x0 written once.  The reference runs about 12 launches at order 4.
// x: the sample, e: the model output, xs: the sample the first-order call was handed, z: the noise, d1 .. d3: the previous
// derivatives, newest first.  sig is the sigma of the conversion and of the derivative (sigma_hat in first-order state, sigma_interpol
// in second-order state); c_out and c_den belong to the same sigma.
//   x0     EPSILON  x - sig * e;   V  e * c_out + x / c_den;   SAMPLE (LMS only)  e
//   KDPM2  d = (x - x0) / sig;  r = (xs ? xs : x) + d * dt;  x' = z ? r + z * sigma_up : r
//   LMS    d = (x - x0) / sig;  acc = c0 * d;  acc = acc + c1 * d1;  ... (order terms);  x' = x + acc;  d_new = d;  x0_out = x0
//
// Rounding: every operation above is rounded separately (clang fp contract(off): hipcc would otherwise fuse a * b + c into one
// v_fma_f32), the divisions are true IEEE divisions, and the scalars arrive from the host, which forms them with 0-d fp32 torch ops in
// the reference's order (diffusion._KDPM2Tables, diffusion.LMSDiscreteScheduler).
//
// Memory bound: at most 4 x (4 reads + 1 write) B per element (KDPM2) and 4 x (5 reads + 3 writes) B (LMS at order 4), 16-byte
// accesses, nothing else.  Plain vector loads and stores.
#include "dp_headtail.h"

// The launch macro of this file: the body of the library's own (dp_common.h) under a name of its own, so that the launch sites of
// this file are tabled by this file's test module (tests/test_kdiff_gpu.py), as sigma.hip does.
#define KD_LAUNCH(k, ...) do { dp_launch_names[dp_launches++ & (DP_LAUNCH_RING - 1)] = #k; hipLaunchKernelGGL(k, __VA_ARGS__); } while (0)

template <int PRED>
__device__ __forceinline__ float kd_x0(float x, float e, float sig, float c_out, float c_den) {
#pragma clang fp contract(off)
    if (PRED == DP_KDIFF_EPSILON) {
        const float t = sig * e;
        return x - t;
    }
    if (PRED == DP_KDIFF_V) {
        const float p = e * c_out;
        const float q = x / c_den;
        return p + q;
    }
    return e;
}

// SHAPE: 0 the first-order call (base x), 1 the second-order call (base xs), 2 the second-order call with noise
template <int SHAPE, int PRED>
__device__ __forceinline__ float kdpm2_one(float x, float e, float xs, float z, const dp_kdpm2_coef& c) {
#pragma clang fp contract(off)
    const float x0 = kd_x0<PRED>(x, e, c.sig, c.c_out, c.c_den);
    const float diff = x - x0;
    const float d = diff / c.sig;
    const float step = d * c.dt;
    float r = (SHAPE == 0 ? x : xs) + step;
    if (SHAPE == 2) {
        const float t = z * c.sigma_up;
        r = r + t;
    }
    return r;
}

// The head / body / tail loop of dp_headtail.h.  `next` may be `x` itself or `xs` itself, so none of the three carries __restrict__:
// a lane reads every input of its elements before it writes any of them, and no other lane touches them.
template <int SHAPE, int PRED>
__global__ __launch_bounds__(256) void kdpm2_step_kernel(const float* x, const float* __restrict__ e, const float* xs,
                                                         const float* __restrict__ z, dp_kdpm2_coef c, float* next, long long n,
                                                         long long head) {
    constexpr bool S = SHAPE != 0, Z = SHAPE == 2;
    dp_ht_for(
        n, head, (long long)blockIdx.x * 256 + threadIdx.x, (long long)gridDim.x * 256,
        [&](long long at) {
            const float4 xv = dp_ld4(x, at, true), ev = dp_ld4(e, at, true), sv = dp_ld4(xs, at, S), zv = dp_ld4(z, at, Z);
            float4 ov;
            ov.x = kdpm2_one<SHAPE, PRED>(xv.x, ev.x, sv.x, zv.x, c);
            ov.y = kdpm2_one<SHAPE, PRED>(xv.y, ev.y, sv.y, zv.y, c);
            ov.z = kdpm2_one<SHAPE, PRED>(xv.z, ev.z, sv.z, zv.z, c);
            ov.w = kdpm2_one<SHAPE, PRED>(xv.w, ev.w, sv.w, zv.w, c);
            dp_st4(next, at, ov);                                    // after every load of this lane's elements
        },
        [&](long long i) {
            const float xx = x[i], ee = e[i], ss = dp_ld1(xs, i, S), zz = dp_ld1(z, i, Z);
            next[i] = kdpm2_one<SHAPE, PRED>(xx, ee, ss, zz, c);
        });
}

template <int ORDER, int PRED>
__device__ __forceinline__ float lms_one(float x, float e, float d1, float d2, float d3, const dp_lms_coef& c, float& d, float& x0) {
#pragma clang fp contract(off)
    x0 = kd_x0<PRED>(x, e, c.sig, c.c_out, c.c_den);
    const float diff = x - x0;
    d = diff / c.sig;
    float acc = c.c0 * d;
    if (ORDER > 1) {
        const float t = c.c1 * d1;
        acc = acc + t;
    }
    if (ORDER > 2) {
        const float t = c.c2 * d2;
        acc = acc + t;
    }
    if (ORDER > 3) {
        const float t = c.c3 * d3;
        acc = acc + t;
    }
    return x + acc;
}

// `next` may be `x` itself; d_new and x0_out overlap nothing the kernel reads.
template <int ORDER, int PRED>
__global__ __launch_bounds__(256) void lms_step_kernel(const float* x, const float* __restrict__ e, const float* __restrict__ d1,
                                                       const float* __restrict__ d2, const float* __restrict__ d3, dp_lms_coef c,
                                                       float* next, float* __restrict__ d_new, float* __restrict__ x0_out, long long n,
                                                       long long head) {
    dp_ht_for(
        n, head, (long long)blockIdx.x * 256 + threadIdx.x, (long long)gridDim.x * 256,
        [&](long long at) {
            const float4 xv = dp_ld4(x, at, true), ev = dp_ld4(e, at, true);
            const float4 av = dp_ld4(d1, at, ORDER > 1), bv = dp_ld4(d2, at, ORDER > 2), cv = dp_ld4(d3, at, ORDER > 3);
            float4 ov, dv, pv;
            ov.x = lms_one<ORDER, PRED>(xv.x, ev.x, av.x, bv.x, cv.x, c, dv.x, pv.x);
            ov.y = lms_one<ORDER, PRED>(xv.y, ev.y, av.y, bv.y, cv.y, c, dv.y, pv.y);
            ov.z = lms_one<ORDER, PRED>(xv.z, ev.z, av.z, bv.z, cv.z, c, dv.z, pv.z);
            ov.w = lms_one<ORDER, PRED>(xv.w, ev.w, av.w, bv.w, cv.w, c, dv.w, pv.w);
            dp_st4(next, at, ov);                                    // after every load of this lane's elements
            dp_st4(d_new, at, dv);
            dp_st4(x0_out, at, pv);
        },
        [&](long long i) {
            const float xx = x[i], ee = e[i], aa = dp_ld1(d1, i, ORDER > 1), bb = dp_ld1(d2, i, ORDER > 2), cc = dp_ld1(d3, i, ORDER > 3);
            float d, p;
            const float v = lms_one<ORDER, PRED>(xx, ee, aa, bb, cc, c, d, p);
            next[i] = v;
            d_new[i] = d;
            x0_out[i] = p;
        });
}

extern "C" int dp_kdpm2_step(const float* x, const float* e, const float* xs, const float* z, int pred, const dp_kdpm2_coef* coef,
                             float* x_next, long long n, void* stream) {
    if (n <= 0) return 0;
    if (!x || !e || !coef || !x_next || pred < DP_KDIFF_EPSILON || pred > DP_KDIFF_V) return (int)hipErrorInvalidValue;
    if (z && !xs) return (int)hipErrorInvalidValue;                              // the noise belongs to the second-order call
    // the aliases the kernel is written for: x_next == x and x_next == xs.  Everything else is disjoint.
    const unsigned long long len = 4ull * (unsigned long long)n;
    const auto hit = [len](const void* a, const void* b) { return dp_bytes_overlap(a, len, b, len); };
    if ((x_next != x && hit(x_next, x)) || (x_next != xs && hit(x_next, xs))) return (int)hipErrorInvalidValue;
    if (hit(x_next, e) || hit(x_next, z)) return (int)hipErrorInvalidValue;
    const void* ptrs[5] = {x, e, xs, z, x_next};
    const long long head = dp_ht_head(n, ptrs, 5);
    const unsigned grid = dp_ht_blocks(n, head, DP_KDIFF_MAX_BLOCKS);
    const dp_kdpm2_coef c = *coef;
    const hipStream_t st = (hipStream_t)stream;
#define KD_ARGS dim3(grid), dim3(256), 0, st, x, e, xs, z, c, x_next, n, head
    // one site per instantiation: the launch ring keeps the stringised kernel expression of the site that launched
    switch (2 * (xs ? (z ? 2 : 1) : 0) + pred) {
        case 0: KD_LAUNCH((kdpm2_step_kernel<0, DP_KDIFF_EPSILON>), KD_ARGS); break;
        case 1: KD_LAUNCH((kdpm2_step_kernel<0, DP_KDIFF_V>), KD_ARGS); break;
        case 2: KD_LAUNCH((kdpm2_step_kernel<1, DP_KDIFF_EPSILON>), KD_ARGS); break;
        case 3: KD_LAUNCH((kdpm2_step_kernel<1, DP_KDIFF_V>), KD_ARGS); break;
        case 4: KD_LAUNCH((kdpm2_step_kernel<2, DP_KDIFF_EPSILON>), KD_ARGS); break;
        case 5: KD_LAUNCH((kdpm2_step_kernel<2, DP_KDIFF_V>), KD_ARGS); break;
        default: return (int)hipErrorInvalidValue;
    }
#undef KD_ARGS
    return DP_LAUNCH_CHECK();
}

extern "C" int dp_lms_step(const float* x, const float* e, const float* d1, const float* d2, const float* d3, int order, int pred,
                           const dp_lms_coef* coef, float* x_next, float* d_new, float* x0_out, long long n, void* stream) {
    if (n <= 0) return 0;
    if (!x || !e || !coef || !x_next || !d_new || !x0_out || order < 1 || order > 4) return (int)hipErrorInvalidValue;
    if (pred < DP_KDIFF_EPSILON || pred > DP_KDIFF_SAMPLE) return (int)hipErrorInvalidValue;
    if (order < 4) d3 = nullptr;                                                 // not read at this order
    if (order < 3) d2 = nullptr;
    if (order < 2) d1 = nullptr;
    if ((order > 1 && !d1) || (order > 2 && !d2) || (order > 3 && !d3)) return (int)hipErrorInvalidValue;
    // the alias the kernel is written for: x_next == x.  The three outputs share no byte with each other, and none with an input
    // that is not x_next's own x.
    const unsigned long long len = 4ull * (unsigned long long)n;
    const auto hit = [len](const void* a, const void* b) { return dp_bytes_overlap(a, len, b, len); };
    if (x_next != x && hit(x_next, x)) return (int)hipErrorInvalidValue;
    if (hit(x_next, e) || hit(x_next, d1) || hit(x_next, d2) || hit(x_next, d3)) return (int)hipErrorInvalidValue;
    if (hit(d_new, x_next) || hit(x0_out, x_next) || hit(d_new, x0_out)) return (int)hipErrorInvalidValue;
    const float* outs[2] = {d_new, x0_out};
    for (const float* o : outs)
        if (hit(o, x) || hit(o, e) || hit(o, d1) || hit(o, d2) || hit(o, d3)) return (int)hipErrorInvalidValue;
    const void* ptrs[8] = {x, e, d1, d2, d3, x_next, d_new, x0_out};
    const long long head = dp_ht_head(n, ptrs, 8);
    const unsigned grid = dp_ht_blocks(n, head, DP_KDIFF_MAX_BLOCKS);
    const dp_lms_coef c = *coef;
    const hipStream_t st = (hipStream_t)stream;
#define KD_ARGS dim3(grid), dim3(256), 0, st, x, e, d1, d2, d3, c, x_next, d_new, x0_out, n, head
    switch (3 * (order - 1) + pred) {
        case 0: KD_LAUNCH((lms_step_kernel<1, DP_KDIFF_EPSILON>), KD_ARGS); break;
        case 1: KD_LAUNCH((lms_step_kernel<1, DP_KDIFF_V>), KD_ARGS); break;
        case 2: KD_LAUNCH((lms_step_kernel<1, DP_KDIFF_SAMPLE>), KD_ARGS); break;
        case 3: KD_LAUNCH((lms_step_kernel<2, DP_KDIFF_EPSILON>), KD_ARGS); break;
        case 4: KD_LAUNCH((lms_step_kernel<2, DP_KDIFF_V>), KD_ARGS); break;
        case 5: KD_LAUNCH((lms_step_kernel<2, DP_KDIFF_SAMPLE>), KD_ARGS); break;
        case 6: KD_LAUNCH((lms_step_kernel<3, DP_KDIFF_EPSILON>), KD_ARGS); break;
        case 7: KD_LAUNCH((lms_step_kernel<3, DP_KDIFF_V>), KD_ARGS); break;
        case 8: KD_LAUNCH((lms_step_kernel<3, DP_KDIFF_SAMPLE>), KD_ARGS); break;
        case 9: KD_LAUNCH((lms_step_kernel<4, DP_KDIFF_EPSILON>), KD_ARGS); break;
        case 10: KD_LAUNCH((lms_step_kernel<4, DP_KDIFF_V>), KD_ARGS); break;
        case 11: KD_LAUNCH((lms_step_kernel<4, DP_KDIFF_SAMPLE>), KD_ARGS); break;
        default: return (int)hipErrorInvalidValue;
    }
#undef KD_ARGS
    return DP_LAUNCH_CHECK();
}
