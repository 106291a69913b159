// The elementwise kernel of the multistep DPM-Solver (diffusers/schedulers/scheduling_dpmsolver_multistep.py):
//   dp_dpm_solver_step  one scheduler step in ONE pass: convert_model_output (:346-395, epsilon prediction) and the first-, second-
//                       or third-order update (:420-442, :466-501, :557-589).  The reference runs about a dozen elementwise
//                       launches per step; here x, e and the history are read once, the next state and the converted output are
//                       written once.
//   convert  DATA (dpmsolver++):  m0 = (x - sigma_s * e) / alpha_s          !DATA (dpmsolver):  m0 = e
//   order 1  x' = kx * x - k0 * m0
//   order 2  D1 = ir0 * (m0 - m1);                                              x' = (kx * x - k0 * m0) - k1 * D1
//   order 3  D10 = ir0 * (m0 - m1); D11 = ir1 * (m1 - m2); d = D10 - D11;
//            D1 = D10 + q * d; D2 = iq * d;                                     x' = ((kx * x - k0 * m0) - k1 * D1) - k2 * D2
// Where the reference adds a term (`+ c * D1`: heun, third-order dpmsolver++) the host passes k1 = -c: a - (-c) * D and a + c * D are
// the same bits.  m0 is written in the !DATA case too: the caller's history owns its copy (a captured forward reuses its output buffer).
//
// Rounding: every operation above is rounded separately (clang fp contract(off): hipcc would otherwise fuse a * b + c into one
// v_fma_f32), the division is a true IEEE division, and the scalars arrive from the host, which forms them with 0-d fp32 torch ops in
// the reference's order (diffusion.DPMSolverMultistepScheduler) -- the way dp_denoise_step takes its coefficients.
//
// Memory bound: 4 (order + 1) B read and 8 B written per element, 16-byte accesses, nothing else.  Plain vector loads and stores.
#include "dp_headtail.h"

// The launch macro of this file: the body of the library's own (dp_common.h) under a name of its own, so that the launch sites of
// this file are tabled by this file's test module (tests/test_dpm_solver_gpu.py), as stage.hip, evalmetrics.hip and prune_global.hip do.
#define DS_LAUNCH(k, ...) do { dp_launch_names[dp_launches++ & (DP_LAUNCH_RING - 1)] = #k; hipLaunchKernelGGL(k, __VA_ARGS__); } while (0)

template <int ORDER, bool DATA>
__device__ __forceinline__ float dpm_solver_one(float x, float e, float m1, float m2, const dp_dpm_solver_coef& c, float& m0) {
#pragma clang fp contract(off)
    if (DATA) {
        const float se = c.sigma_s * e;
        m0 = (x - se) / c.alpha_s;
    } else {
        m0 = e;
    }
    const float a = c.kx * x;
    const float b = c.k0 * m0;
    float v = a - b;
    if (ORDER == 2) {
        const float D1 = c.ir0 * (m0 - m1);
        const float t1 = c.k1 * D1;
        v = v - t1;
    } else if (ORDER == 3) {
        const float D10 = c.ir0 * (m0 - m1);
        const float D11 = c.ir1 * (m1 - m2);
        const float d = D10 - D11;
        const float qd = c.q * d;
        const float D1 = D10 + qd;
        const float D2 = c.iq * d;
        const float t1 = c.k1 * D1;
        v = v - t1;
        const float t2 = c.k2 * D2;
        v = v - t2;
    }
    return v;
}

// The head / body / tail loop of dp_headtail.h.  `next` may be `x` itself and `m0_out` may be `m1` or `m2` itself (no __restrict__ on
// those): a lane reads every input of its elements before it writes any of them, and no other lane touches them.  e aliases nothing.
template <int ORDER, bool DATA>
__global__ __launch_bounds__(256) void dpm_solver_step_kernel(const float* x, const float* __restrict__ e, const float* m1, const float* m2,
                                                              dp_dpm_solver_coef c, float* next, float* m0_out, long long n, long long head) {
    dp_ht_for(
        n, head, (long long)blockIdx.x * 256 + threadIdx.x, (long long)gridDim.x * 256,
        [&](long long at) {
            const float4 xv = dp_ld4(x, at, true), ev = dp_ld4(e, at, true);
            const float4 av = dp_ld4(m1, at, ORDER >= 2), bv = dp_ld4(m2, at, ORDER >= 3);
            float4 ov, mv;
            ov.x = dpm_solver_one<ORDER, DATA>(xv.x, ev.x, av.x, bv.x, c, mv.x);
            ov.y = dpm_solver_one<ORDER, DATA>(xv.y, ev.y, av.y, bv.y, c, mv.y);
            ov.z = dpm_solver_one<ORDER, DATA>(xv.z, ev.z, av.z, bv.z, c, mv.z);
            ov.w = dpm_solver_one<ORDER, DATA>(xv.w, ev.w, av.w, bv.w, c, mv.w);
            dp_st4(next, at, ov);                                    // after every load of this lane's elements
            dp_st4(m0_out, at, mv);
        },
        [&](long long i) {
            const float xs = x[i], es = e[i];
            const float as = dp_ld1(m1, i, ORDER >= 2), bs = dp_ld1(m2, i, ORDER >= 3);
            float m;
            const float v = dpm_solver_one<ORDER, DATA>(xs, es, as, bs, c, m);
            next[i] = v;
            m0_out[i] = m;
        });
}

extern "C" int dp_dpm_solver_step(const float* x, const float* e, const float* m1, const float* m2, int order, int data_pred,
                                  const dp_dpm_solver_coef* coef, float* x_next, float* m0_out, long long n, void* stream) {
    if (n <= 0) return 0;
    if (!x || !e || !coef || !x_next || !m0_out || order < 1 || order > 3) return (int)hipErrorInvalidValue;
    if (order < 3) m2 = nullptr;                                                 // not read below their order
    if (order < 2) m1 = nullptr;
    if ((order >= 2 && !m1) || (order >= 3 && !m2)) return (int)hipErrorInvalidValue;
    // the aliases the kernel is written for: x_next == x, m0_out == m1, m0_out == m2.  Everything else is disjoint.
    const unsigned long long len = 4ull * (unsigned long long)n;
    const auto hit = [len](const void* a, const void* b) { return dp_bytes_overlap(a, len, b, len); };
    if ((x_next != x && hit(x_next, x)) || hit(x_next, e) || hit(x_next, m0_out)) return (int)hipErrorInvalidValue;
    if (hit(m0_out, x) || hit(m0_out, e)) return (int)hipErrorInvalidValue;
    if (hit(x_next, m1) || (m0_out != m1 && hit(m0_out, m1))) return (int)hipErrorInvalidValue;
    if (hit(x_next, m2) || (m0_out != m2 && hit(m0_out, m2))) return (int)hipErrorInvalidValue;
    const void* ptrs[6] = {x, e, x_next, m0_out, m1, m2};
    const long long head = dp_ht_head(n, ptrs, 6);
    const unsigned grid = dp_ht_blocks(n, head, DP_DPM_SOLVER_MAX_BLOCKS);
    const dp_dpm_solver_coef c = *coef;
    const hipStream_t st = (hipStream_t)stream;
    // one site per instantiation: the launch ring keeps the stringised kernel expression of the site that launched
    switch (2 * order + (data_pred ? 1 : 0)) {
        case 2: DS_LAUNCH((dpm_solver_step_kernel<1, false>), dim3(grid), dim3(256), 0, st, x, e, m1, m2, c, x_next, m0_out, n, head); break;
        case 3: DS_LAUNCH((dpm_solver_step_kernel<1, true>), dim3(grid), dim3(256), 0, st, x, e, m1, m2, c, x_next, m0_out, n, head); break;
        case 4: DS_LAUNCH((dpm_solver_step_kernel<2, false>), dim3(grid), dim3(256), 0, st, x, e, m1, m2, c, x_next, m0_out, n, head); break;
        case 5: DS_LAUNCH((dpm_solver_step_kernel<2, true>), dim3(grid), dim3(256), 0, st, x, e, m1, m2, c, x_next, m0_out, n, head); break;
        case 6: DS_LAUNCH((dpm_solver_step_kernel<3, false>), dim3(grid), dim3(256), 0, st, x, e, m1, m2, c, x_next, m0_out, n, head); break;
        default: DS_LAUNCH((dpm_solver_step_kernel<3, true>), dim3(grid), dim3(256), 0, st, x, e, m1, m2, c, x_next, m0_out, n, head); break;
    }
    return DP_LAUNCH_CHECK();
}
