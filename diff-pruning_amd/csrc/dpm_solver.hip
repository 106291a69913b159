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
#include "dp_common.h"

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

// Elements [0, head) and [head + 4 * n4, n) take 4-byte accesses, the n4 = (n - head) / 4 groups between them 16-byte ones.  The
// launcher chooses head so that every pointer + head is 16-byte aligned, or head = n when the pointers do not share one alignment.
// `next` may be `x` itself and `m0_out` may be `m1` or `m2` itself (no __restrict__ on those): a lane reads every input of its
// elements before it writes any of them, and no other lane touches them.  e aliases nothing.
template <int ORDER, bool DATA>
__global__ __launch_bounds__(256) void dpm_solver_step_kernel(const float* x, const float* __restrict__ e, const float* m1, const float* m2,
                                                              dp_dpm_solver_coef c, float* next, float* m0_out, long long n, long long head) {
    const long long tid = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long stride = (long long)gridDim.x * 256;
    const long long n4 = (n - head) / 4;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    for (long long i = tid; i < n4; i += stride) {
        const long long at = head + 4 * i;
        const float4 xv = *reinterpret_cast<const float4*>(x + at);
        const float4 ev = *reinterpret_cast<const float4*>(e + at);
        const float4 av = ORDER >= 2 ? *reinterpret_cast<const float4*>(m1 + at) : zero;
        const float4 bv = ORDER >= 3 ? *reinterpret_cast<const float4*>(m2 + at) : zero;
        float4 ov, mv;
        ov.x = dpm_solver_one<ORDER, DATA>(xv.x, ev.x, av.x, bv.x, c, mv.x);
        ov.y = dpm_solver_one<ORDER, DATA>(xv.y, ev.y, av.y, bv.y, c, mv.y);
        ov.z = dpm_solver_one<ORDER, DATA>(xv.z, ev.z, av.z, bv.z, c, mv.z);
        ov.w = dpm_solver_one<ORDER, DATA>(xv.w, ev.w, av.w, bv.w, c, mv.w);
        *reinterpret_cast<float4*>(next + at) = ov;                  // after every load of this lane's elements
        *reinterpret_cast<float4*>(m0_out + at) = mv;
    }
    const long long ns = n - 4 * n4;                  // the scalar head and tail (everything when head == n)
    for (long long j = tid; j < ns; j += stride) {
        const long long i = j < head ? j : 4 * n4 + j;
        const float xs = x[i], es = e[i];
        const float as = ORDER >= 2 ? m1[i] : 0.f;
        const float bs = ORDER >= 3 ? m2[i] : 0.f;
        float m;
        const float v = dpm_solver_one<ORDER, DATA>(xs, es, as, bs, c, m);
        next[i] = v;
        m0_out[i] = m;
    }
}

// [a, a + 4 n) and [b, b + 4 n) share a byte without being the same buffer
static inline bool ds_partial_overlap(const void* a, const void* b, long long n) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b, len = 4ull * (unsigned long long)n;
    return a0 != b0 && a0 < b0 + len && b0 < a0 + len;
}

static inline bool ds_overlap(const void* a, const void* b, long long n) {
    return a == b || ds_partial_overlap(a, b, n);
}

extern "C" int dp_dpm_solver_step(const float* x, const float* e, const float* m1, const float* m2, int order, int data_pred,
                                  const dp_dpm_solver_coef* coef, float* x_next, float* m0_out, long long n, void* stream) {
    if (n <= 0) return 0;
    if (!x || !e || !coef || !x_next || !m0_out || order < 1 || order > 3) return (int)hipErrorInvalidValue;
    if (order < 3) m2 = nullptr;                                                 // not read below their order
    if (order < 2) m1 = nullptr;
    if ((order >= 2 && !m1) || (order >= 3 && !m2)) return (int)hipErrorInvalidValue;
    // the aliases the kernel is written for: x_next == x, m0_out == m1, m0_out == m2.  Everything else is disjoint.
    if (ds_partial_overlap(x_next, x, n) || ds_overlap(x_next, e, n) || ds_overlap(x_next, m0_out, n)) return (int)hipErrorInvalidValue;
    if (ds_overlap(m0_out, x, n) || ds_overlap(m0_out, e, n)) return (int)hipErrorInvalidValue;
    if (m1 && (ds_overlap(x_next, m1, n) || ds_partial_overlap(m0_out, m1, n))) return (int)hipErrorInvalidValue;
    if (m2 && (ds_overlap(x_next, m2, n) || ds_partial_overlap(m0_out, m2, n))) return (int)hipErrorInvalidValue;
    // one alignment for every pointer -> a scalar head of 0 .. 3 elements brings all of them to 16 bytes; otherwise all scalar
    const uintptr_t a = (uintptr_t)x & 15;
    bool same = (a & 3) == 0 && ((uintptr_t)e & 15) == a && ((uintptr_t)x_next & 15) == a && ((uintptr_t)m0_out & 15) == a;
    if (m1) same = same && ((uintptr_t)m1 & 15) == a;
    if (m2) same = same && ((uintptr_t)m2 & 15) == a;
    long long head = same ? (long long)(((16 - a) & 15) / 4) : n;
    if (head > n) head = n;
    const long long n4 = (n - head) / 4;
    const long long work = n4 > n - 4 * n4 ? n4 : n - 4 * n4;
    const long long nb = (work + 255) / 256;
    const unsigned grid = (unsigned)(nb > DP_DPM_SOLVER_MAX_BLOCKS ? DP_DPM_SOLVER_MAX_BLOCKS : nb < 1 ? 1 : nb);
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
