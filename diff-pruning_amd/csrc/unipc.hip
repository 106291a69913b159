// The elementwise kernel of the UniPC multistep scheduler (diffusers/schedulers/scheduling_unipc_multistep.py):
//   dp_unipc_step  one scheduler step for an epsilon model in ONE pass: convert_model_output (:256-305), the UniC corrector of the
//                  PREVIOUS step's order (:412-516) and the UniP predictor of this step's order (:307-410), as `step` (:518-600)
//                  chains them.  The reference runs about forty elementwise launches for a third-order step; here every input is
//                  read once and the converted output, the corrected sample and the next sample are written once.
//   convert    X0:  m_new = (x_pred - sigma_s * e) / alpha_s        !X0:  m_new = e          (x_pred: the UNcorrected sample)
//   corrector  PC in {0 (absent), 1, 2, 3}, on the OLD history m0 (newest), m1, m2 and on x_last:
//                D_i = (m_i - m0) / c_rk<i>   (i = 1 .. PC - 1);    dt = m_new - m0
//                x_c = (c_cx * x_last - c_c0 * m0) - c_cB * (S + c_rho_last * dt)
//                S: absent (PC 1) | c_rho1 * D_1 (PC 2) | c_rho1 * D_1 + c_rho2 * D_2 (PC 3)
//   predictor  PP in {1, 2, 3}, on the NEW history (m_new, m0, m1), from xs = x_c (PC > 0) or x_pred (PC 0):
//                E_1 = (m0 - m_new) / p_rk1;  E_2 = (m1 - m_new) / p_rk2
//                x_next = (p_cx * xs - p_c0 * m_new) [ - p_cB * T ]
//                T: absent (PP 1) | p_rho1 * E_1 (PP 2, the host passes the fixed 0.5) | p_rho1 * E_1 + p_rho2 * E_2 (PP 3)
// m_new is written in the !X0 case too: the caller's history owns its copy (a captured forward reuses its output buffer).
//
// Rounding: every operation above is rounded separately (clang fp contract(off): hipcc would otherwise fuse a * b + c into one
// v_fma_f32) and the divisions are true IEEE divisions; the scalars arrive from the host, which forms them with 0-d fp32 torch ops in
// the reference's order (diffusion.UniPCMultistepScheduler).  The order of the up-to-two history terms of a sum is this kernel's
// own: the two products are added first, left to right (c_rho1 * D_1 + c_rho2 * D_2), and the corrector then adds
// c_rho_last * dt to that sum.  The reference leaves that order to torch.einsum, so a third-order sum is not held to its bits.
//
// Aliases: m_new may be m0, m1 or m2 itself (the oldest buffer of the caller's ring, which this very step may still read), x_c may be
// x_last itself and x_next may be x_pred itself: a lane reads every input of its elements before it writes any of them, and no other
// lane touches them.  Every other overlap between an output and another buffer is refused (hipErrorInvalidValue, nothing launched).
//
// Memory bound: 4 (2 + [PC > 0] + max(PC, PP - 1)) B read and 4 (2 + [PC > 0]) B written per element, 16-byte accesses, nothing else.
// Plain vector loads and stores.
#include "dp_headtail.h"

// The launch macro of this file: the body of the library's own (dp_common.h) under a name of its own, so that the launch sites of
// this file are tabled by this file's test module (tests/test_unipc_gpu.py), as dpm_solver.hip, stage.hip and evalmetrics.hip do.
#define UP_LAUNCH(k, ...) do { dp_launch_names[dp_launches++ & (DP_LAUNCH_RING - 1)] = #k; hipLaunchKernelGGL(k, __VA_ARGS__); } while (0)

template <int PC, int PP, bool X0>
__device__ __forceinline__ void unipc_one(float e, float xp, float xl, float m0, float m1, float m2, const dp_unipc_coef& c,
                                          float& mn, float& xc, float& xn) {
#pragma clang fp contract(off)
    if (X0) {
        const float se = c.sigma_s * e;
        mn = (xp - se) / c.alpha_s;
    } else {
        mn = e;
    }
    float xs = xp;
    xc = 0.f;
    if (PC > 0) {
        const float a = c.c_cx * xl;
        const float b = c.c_c0 * m0;
        const float base = a - b;
        const float dt = mn - m0;
        float inner = c.c_rho_last * dt;
        if (PC == 2) {
            const float D1 = (m1 - m0) / c.c_rk1;
            const float s = c.c_rho1 * D1;
            inner = s + inner;
        } else if (PC == 3) {
            const float D1 = (m1 - m0) / c.c_rk1;
            const float D2 = (m2 - m0) / c.c_rk2;
            const float s1 = c.c_rho1 * D1;
            const float s2 = c.c_rho2 * D2;
            const float s = s1 + s2;
            inner = s + inner;
        }
        const float t = c.c_cB * inner;
        xs = base - t;
        xc = xs;
    }
    const float a = c.p_cx * xs;
    const float b = c.p_c0 * mn;
    float v = a - b;
    if (PP == 2) {
        const float E1 = (m0 - mn) / c.p_rk1;
        const float s = c.p_rho1 * E1;
        const float t = c.p_cB * s;
        v = v - t;
    } else if (PP == 3) {
        const float E1 = (m0 - mn) / c.p_rk1;
        const float E2 = (m1 - mn) / c.p_rk2;
        const float s1 = c.p_rho1 * E1;
        const float s2 = c.p_rho2 * E2;
        const float s = s1 + s2;
        const float t = c.p_cB * s;
        v = v - t;
    }
    xn = v;
}

// The head / body / tail loop of dp_headtail.h.  No __restrict__ on the pointers that may alias (header); e aliases no output.  NH = max(PC, PP - 1) history buffers are read,
// x_last only when PC > 0; x_c is written only when PC > 0.
template <int PC, int PP, bool X0>
__global__ __launch_bounds__(256) void unipc_step_kernel(const float* __restrict__ e, const float* x_pred, const float* x_last,
                                                         const float* m0, const float* m1, const float* m2, dp_unipc_coef c,
                                                         float* m_new, float* x_c, float* x_next, long long n, long long head) {
    constexpr int NH = PC > PP - 1 ? PC : PP - 1;
    dp_ht_for(
        n, head, (long long)blockIdx.x * 256 + threadIdx.x, (long long)gridDim.x * 256,
        [&](long long at) {
            const float4 ev = dp_ld4(e, at, true), pv = dp_ld4(x_pred, at, true), lv = dp_ld4(x_last, at, PC > 0);
            const float4 av = dp_ld4(m0, at, NH >= 1), bv = dp_ld4(m1, at, NH >= 2), cv = dp_ld4(m2, at, NH >= 3);
            float4 mv, xc, xn;
            unipc_one<PC, PP, X0>(ev.x, pv.x, lv.x, av.x, bv.x, cv.x, c, mv.x, xc.x, xn.x);
            unipc_one<PC, PP, X0>(ev.y, pv.y, lv.y, av.y, bv.y, cv.y, c, mv.y, xc.y, xn.y);
            unipc_one<PC, PP, X0>(ev.z, pv.z, lv.z, av.z, bv.z, cv.z, c, mv.z, xc.z, xn.z);
            unipc_one<PC, PP, X0>(ev.w, pv.w, lv.w, av.w, bv.w, cv.w, c, mv.w, xc.w, xn.w);
            dp_st4(m_new, at, mv);                                   // after every load of this lane's elements
            if (PC > 0) dp_st4(x_c, at, xc);
            dp_st4(x_next, at, xn);
        },
        [&](long long i) {
            const float es = e[i], ps = x_pred[i], ls = dp_ld1(x_last, i, PC > 0);
            const float as = dp_ld1(m0, i, NH >= 1), bs = dp_ld1(m1, i, NH >= 2), cs = dp_ld1(m2, i, NH >= 3);
            float mn, xc, xn;
            unipc_one<PC, PP, X0>(es, ps, ls, as, bs, cs, c, mn, xc, xn);
            m_new[i] = mn;
            if (PC > 0) x_c[i] = xc;
            x_next[i] = xn;
        });
}

extern "C" int dp_unipc_step(const float* e, const float* x_pred, const float* x_last, const float* m0, const float* m1,
                             const float* m2, int pc, int pp, int predict_x0, const dp_unipc_coef* coef, float* m_new, float* x_c,
                             float* x_next, long long n, void* stream) {
    if (n <= 0) return 0;
    if (!e || !x_pred || !coef || !m_new || !x_next || pc < 0 || pc > 3 || pp < 1 || pp > 3) return (int)hipErrorInvalidValue;
    const int nh = pc > pp - 1 ? pc : pp - 1;
    const float* hist[3] = {nh >= 1 ? m0 : nullptr, nh >= 2 ? m1 : nullptr, nh >= 3 ? m2 : nullptr};   // not read above nh
    for (int i = 0; i < nh; i++)
        if (!hist[i]) return (int)hipErrorInvalidValue;
    if (pc == 0) { x_last = nullptr; x_c = nullptr; }                            // neither read nor written without a corrector
    else if (!x_last || !x_c) return (int)hipErrorInvalidValue;
    // the aliases the kernel is written for: m_new == m0 | m1 | m2, x_c == x_last, x_next == x_pred.  Everything else is disjoint.
    const void* ins[6] = {e, x_pred, x_last, hist[0], hist[1], hist[2]};
    const void* outs[3] = {m_new, x_c, x_next};
    const unsigned long long len = 4ull * (unsigned long long)n;
    for (int o = 0; o < 3; o++) {
        for (int p = o + 1; p < 3; p++)
            if (dp_bytes_overlap(outs[o], len, outs[p], len)) return (int)hipErrorInvalidValue;
        for (int i = 0; i < 6; i++) {
            if (!dp_bytes_overlap(outs[o], len, ins[i], len)) continue;
            const bool allowed = outs[o] == ins[i] && ((o == 0 && i >= 3) || (o == 1 && i == 2) || (o == 2 && i == 1));
            if (!allowed) return (int)hipErrorInvalidValue;
        }
    }
    const void* ptrs[9] = {e, x_pred, x_last, hist[0], hist[1], hist[2], m_new, x_c, x_next};
    const long long head = dp_ht_head(n, ptrs, 9);
    const unsigned grid = dp_ht_blocks(n, head, DP_UNIPC_MAX_BLOCKS);
    const dp_unipc_coef c = *coef;
    const hipStream_t st = (hipStream_t)stream;
    m0 = hist[0]; m1 = hist[1]; m2 = hist[2];
#define UP_ARGS dim3(grid), dim3(256), 0, st, e, x_pred, x_last, m0, m1, m2, c, m_new, x_c, x_next, n, head
    // one site per instantiation: the launch ring keeps the stringised kernel expression of the site that launched
    switch ((pc * 3 + (pp - 1)) * 2 + (predict_x0 ? 1 : 0)) {
        case 0: UP_LAUNCH((unipc_step_kernel<0, 1, false>), UP_ARGS); break;
        case 1: UP_LAUNCH((unipc_step_kernel<0, 1, true>), UP_ARGS); break;
        case 2: UP_LAUNCH((unipc_step_kernel<0, 2, false>), UP_ARGS); break;
        case 3: UP_LAUNCH((unipc_step_kernel<0, 2, true>), UP_ARGS); break;
        case 4: UP_LAUNCH((unipc_step_kernel<0, 3, false>), UP_ARGS); break;
        case 5: UP_LAUNCH((unipc_step_kernel<0, 3, true>), UP_ARGS); break;
        case 6: UP_LAUNCH((unipc_step_kernel<1, 1, false>), UP_ARGS); break;
        case 7: UP_LAUNCH((unipc_step_kernel<1, 1, true>), UP_ARGS); break;
        case 8: UP_LAUNCH((unipc_step_kernel<1, 2, false>), UP_ARGS); break;
        case 9: UP_LAUNCH((unipc_step_kernel<1, 2, true>), UP_ARGS); break;
        case 10: UP_LAUNCH((unipc_step_kernel<1, 3, false>), UP_ARGS); break;
        case 11: UP_LAUNCH((unipc_step_kernel<1, 3, true>), UP_ARGS); break;
        case 12: UP_LAUNCH((unipc_step_kernel<2, 1, false>), UP_ARGS); break;
        case 13: UP_LAUNCH((unipc_step_kernel<2, 1, true>), UP_ARGS); break;
        case 14: UP_LAUNCH((unipc_step_kernel<2, 2, false>), UP_ARGS); break;
        case 15: UP_LAUNCH((unipc_step_kernel<2, 2, true>), UP_ARGS); break;
        case 16: UP_LAUNCH((unipc_step_kernel<2, 3, false>), UP_ARGS); break;
        case 17: UP_LAUNCH((unipc_step_kernel<2, 3, true>), UP_ARGS); break;
        case 18: UP_LAUNCH((unipc_step_kernel<3, 1, false>), UP_ARGS); break;
        case 19: UP_LAUNCH((unipc_step_kernel<3, 1, true>), UP_ARGS); break;
        case 20: UP_LAUNCH((unipc_step_kernel<3, 2, false>), UP_ARGS); break;
        case 21: UP_LAUNCH((unipc_step_kernel<3, 2, true>), UP_ARGS); break;
        case 22: UP_LAUNCH((unipc_step_kernel<3, 3, false>), UP_ARGS); break;
        default: UP_LAUNCH((unipc_step_kernel<3, 3, true>), UP_ARGS); break;
    }
#undef UP_ARGS
    return DP_LAUNCH_CHECK();
}
