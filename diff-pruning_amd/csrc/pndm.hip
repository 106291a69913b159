// The elementwise kernel of the PNDM scheduler (diffusers/schedulers/scheduling_pndm.py):
//   dp_pndm_step  one scheduler step in ONE pass: the Runge-Kutta accumulation of step_prk (:251-270) or the linear multistep
//                 combination of step_plms (:314-337), the optional v-conversion and formula (9) of _get_prev_sample (:358-399).
//                 The reference runs about a dozen elementwise launches per step; here x, e, the accumulator and the history are
//                 read once, the next state (and, where the mode has one, the accumulator or the history entry) written once.
//   e: the model output, x: the state the update starts from, acc: the Runge-Kutta accumulator, h1 .. h3: older outputs, newest first
//   PRK0      m = e;  acc = c6 * e + 0;  hist_out = e            (the reference adds to a Python 0: a negative zero turns positive)
//   PRK1/2    m = e;  acc = acc + c3 * e
//   PRK3      m = acc + c6 * e
//   PLMS1     m = e;  hist_out = e
//   PLMS_AVG  m = (e + h1) / 2                                   (e is not appended)
//   PLMS2     m = (3 * e - h1) / 2;  hist_out = e
//   PLMS3     m = ((23 * e - 16 * h1) + 5 * h2) / 12;  hist_out = e
//   PLMS4     m = c24 * (((55 * e - 59 * h1) + 37 * h2) - 9 * h3);  hist_out = e
//   V         m = sa * m + sb * x                                (v_prediction)
//   always    x' = sc * x - (d * m) / den
// hist_out is a copy of e: the caller's history owns its buffers (a captured forward reuses its output buffer).
//
// Rounding: every operation above is rounded separately (clang fp contract(off): hipcc would otherwise fuse a * b + c into one
// v_fma_f32), the divisions are true IEEE divisions, and the scalars arrive from the host, which forms them with 0-d fp32 torch ops in
// the reference's order (diffusion.PNDMScheduler); c6, c3, c24 are the doubles 1/6, 1/3, 1/24 rounded to fp32 once.
//
// Memory bound: at most 4 x (5 reads + 2 writes) B per element (PLMS4), 16-byte accesses, nothing else.  Plain vector loads and stores.
#include "dp_headtail.h"

// The launch macro of this file: the body of the library's own (dp_common.h) under a name of its own, so that the launch sites of
// this file are tabled by this file's test module (tests/test_pndm_gpu.py), as dpm_solver.hip and unipc.hip do.
#define PN_LAUNCH(k, ...) do { dp_launch_names[dp_launches++ & (DP_LAUNCH_RING - 1)] = #k; hipLaunchKernelGGL(k, __VA_ARGS__); } while (0)

// what a mode (DP_PNDM_*, include/dp_hip.h) reads and writes beside x, e and x'
__host__ __device__ constexpr bool pn_reads_acc(int m) { return m == DP_PNDM_PRK1 || m == DP_PNDM_PRK2 || m == DP_PNDM_PRK3; }
__host__ __device__ constexpr bool pn_writes_acc(int m) { return m == DP_PNDM_PRK0 || m == DP_PNDM_PRK1 || m == DP_PNDM_PRK2; }
__host__ __device__ constexpr int pn_history(int m) { return m == DP_PNDM_PLMS_AVG || m == DP_PNDM_PLMS2 ? 1 : m == DP_PNDM_PLMS3 ? 2 : m == DP_PNDM_PLMS4 ? 3 : 0; }
__host__ __device__ constexpr bool pn_writes_hist(int m) { return m == DP_PNDM_PRK0 || m == DP_PNDM_PLMS1 || m >= DP_PNDM_PLMS2; }

template <int MODE, bool V>
__device__ __forceinline__ float pndm_one(float x, float e, float a, float h1, float h2, float h3, const dp_pndm_coef& c, float& acc) {
#pragma clang fp contract(off)
    float m = e;
    acc = 0.f;
    if (MODE == DP_PNDM_PRK0) {
        const float t = c.c6 * e;
        acc = t + 0.f;
    } else if (MODE == DP_PNDM_PRK1 || MODE == DP_PNDM_PRK2) {
        const float t = c.c3 * e;
        acc = a + t;
    } else if (MODE == DP_PNDM_PRK3) {
        const float t = c.c6 * e;
        m = a + t;
    } else if (MODE == DP_PNDM_PLMS_AVG) {
        m = (e + h1) / 2.f;
    } else if (MODE == DP_PNDM_PLMS2) {
        const float t = 3.f * e;
        m = (t - h1) / 2.f;
    } else if (MODE == DP_PNDM_PLMS3) {
        const float t0 = 23.f * e;
        const float t1 = 16.f * h1;
        const float t2 = 5.f * h2;
        m = ((t0 - t1) + t2) / 12.f;
    } else if (MODE == DP_PNDM_PLMS4) {
        const float t0 = 55.f * e;
        const float t1 = 59.f * h1;
        const float t2 = 37.f * h2;
        const float t3 = 9.f * h3;
        m = c.c24 * (((t0 - t1) + t2) - t3);
    }
    if (V) {
        const float p = c.sa * m;
        const float q = c.sb * x;
        m = p + q;
    }
    const float s = c.sc * x;
    const float dm = c.d * m;
    const float r = dm / c.den;
    return s - r;
}

// The head / body / tail loop of dp_headtail.h.  `next` may be `x` itself, `acc` is updated in place and `hist_out` may be one of
// h1 .. h3 itself (no __restrict__ on those): a lane reads every input of its elements before it writes any of them, and no
// other lane touches them.  e aliases nothing.
template <int MODE, bool V>
__global__ __launch_bounds__(256) void pndm_step_kernel(const float* x, const float* __restrict__ e, float* acc, const float* h1,
                                                        const float* h2, const float* h3, dp_pndm_coef c, float* next,
                                                        float* hist_out, long long n, long long head) {
    constexpr int H = pn_history(MODE);
    dp_ht_for(
        n, head, (long long)blockIdx.x * 256 + threadIdx.x, (long long)gridDim.x * 256,
        [&](long long at) {
            const float4 xv = dp_ld4(x, at, true), ev = dp_ld4(e, at, true), av = dp_ld4(acc, at, pn_reads_acc(MODE));
            const float4 h1v = dp_ld4(h1, at, H >= 1), h2v = dp_ld4(h2, at, H >= 2), h3v = dp_ld4(h3, at, H >= 3);
            float4 ov, cv;
            ov.x = pndm_one<MODE, V>(xv.x, ev.x, av.x, h1v.x, h2v.x, h3v.x, c, cv.x);
            ov.y = pndm_one<MODE, V>(xv.y, ev.y, av.y, h1v.y, h2v.y, h3v.y, c, cv.y);
            ov.z = pndm_one<MODE, V>(xv.z, ev.z, av.z, h1v.z, h2v.z, h3v.z, c, cv.z);
            ov.w = pndm_one<MODE, V>(xv.w, ev.w, av.w, h1v.w, h2v.w, h3v.w, c, cv.w);
            dp_st4(next, at, ov);                                    // after every load of this lane's elements
            if (pn_writes_acc(MODE)) dp_st4(acc, at, cv);
            if (pn_writes_hist(MODE)) dp_st4(hist_out, at, ev);
        },
        [&](long long i) {
            const float xs = x[i], es = e[i], as = dp_ld1(acc, i, pn_reads_acc(MODE));
            const float h1s = dp_ld1(h1, i, H >= 1), h2s = dp_ld1(h2, i, H >= 2), h3s = dp_ld1(h3, i, H >= 3);
            float cs;
            const float v = pndm_one<MODE, V>(xs, es, as, h1s, h2s, h3s, c, cs);
            next[i] = v;
            if (pn_writes_acc(MODE)) acc[i] = cs;
            if (pn_writes_hist(MODE)) hist_out[i] = es;
        });
}

extern "C" int dp_pndm_step(const float* x, const float* e, float* acc, const float* h1, const float* h2, const float* h3, int mode,
                            int v_pred, const dp_pndm_coef* coef, float* x_next, float* hist_out, long long n, void* stream) {
    if (n <= 0) return 0;
    if (!x || !e || !coef || !x_next || mode < DP_PNDM_PRK0 || mode > DP_PNDM_PLMS4) return (int)hipErrorInvalidValue;
    const int H = pn_history(mode);
    if (H < 3) h3 = nullptr;                                                     // not read by this mode
    if (H < 2) h2 = nullptr;
    if (H < 1) h1 = nullptr;
    if (!pn_reads_acc(mode) && !pn_writes_acc(mode)) acc = nullptr;
    if (!pn_writes_hist(mode)) hist_out = nullptr;
    if ((H >= 1 && !h1) || (H >= 2 && !h2) || (H >= 3 && !h3)) return (int)hipErrorInvalidValue;
    if (((pn_reads_acc(mode) || pn_writes_acc(mode)) && !acc) || (pn_writes_hist(mode) && !hist_out)) return (int)hipErrorInvalidValue;
    // the aliases the kernel is written for: x_next == x, hist_out == h1 / h2 / h3 (acc is one buffer, in place).  Everything else is
    // disjoint: no output shares a byte with another output or with an input that is not itself.
    const unsigned long long len = 4ull * (unsigned long long)n;
    const auto hit = [len](const void* a, const void* b) { return dp_bytes_overlap(a, len, b, len); };
    if ((x_next != x && hit(x_next, x)) || hit(x_next, e) || hit(x_next, acc) || hit(x_next, hist_out)) return (int)hipErrorInvalidValue;
    if (hit(x_next, h1) || hit(x_next, h2) || hit(x_next, h3)) return (int)hipErrorInvalidValue;
    if (hit(acc, x) || hit(acc, e) || hit(acc, hist_out) || hit(acc, h1) || hit(acc, h2) || hit(acc, h3)) return (int)hipErrorInvalidValue;
    if (hit(hist_out, x) || hit(hist_out, e)) return (int)hipErrorInvalidValue;
    if ((hist_out != h1 && hit(hist_out, h1)) || (hist_out != h2 && hit(hist_out, h2)) || (hist_out != h3 && hit(hist_out, h3)))
        return (int)hipErrorInvalidValue;
    const void* ptrs[8] = {x, e, acc, h1, h2, h3, x_next, hist_out};
    const long long head = dp_ht_head(n, ptrs, 8);
    const unsigned grid = dp_ht_blocks(n, head, DP_PNDM_MAX_BLOCKS);
    const dp_pndm_coef c = *coef;
    const hipStream_t st = (hipStream_t)stream;
#define PN_ARGS dim3(grid), dim3(256), 0, st, x, e, acc, h1, h2, h3, c, x_next, hist_out, n, head
    // one site per instantiation: the launch ring keeps the stringised kernel expression of the site that launched
    switch (2 * mode + (v_pred ? 1 : 0)) {
        case 0: PN_LAUNCH((pndm_step_kernel<DP_PNDM_PRK0, false>), PN_ARGS); break;
        case 1: PN_LAUNCH((pndm_step_kernel<DP_PNDM_PRK0, true>), PN_ARGS); break;
        case 2: PN_LAUNCH((pndm_step_kernel<DP_PNDM_PRK1, false>), PN_ARGS); break;
        case 3: PN_LAUNCH((pndm_step_kernel<DP_PNDM_PRK1, true>), PN_ARGS); break;
        case 4: PN_LAUNCH((pndm_step_kernel<DP_PNDM_PRK2, false>), PN_ARGS); break;
        case 5: PN_LAUNCH((pndm_step_kernel<DP_PNDM_PRK2, true>), PN_ARGS); break;
        case 6: PN_LAUNCH((pndm_step_kernel<DP_PNDM_PRK3, false>), PN_ARGS); break;
        case 7: PN_LAUNCH((pndm_step_kernel<DP_PNDM_PRK3, true>), PN_ARGS); break;
        case 8: PN_LAUNCH((pndm_step_kernel<DP_PNDM_PLMS1, false>), PN_ARGS); break;
        case 9: PN_LAUNCH((pndm_step_kernel<DP_PNDM_PLMS1, true>), PN_ARGS); break;
        case 10: PN_LAUNCH((pndm_step_kernel<DP_PNDM_PLMS_AVG, false>), PN_ARGS); break;
        case 11: PN_LAUNCH((pndm_step_kernel<DP_PNDM_PLMS_AVG, true>), PN_ARGS); break;
        case 12: PN_LAUNCH((pndm_step_kernel<DP_PNDM_PLMS2, false>), PN_ARGS); break;
        case 13: PN_LAUNCH((pndm_step_kernel<DP_PNDM_PLMS2, true>), PN_ARGS); break;
        case 14: PN_LAUNCH((pndm_step_kernel<DP_PNDM_PLMS3, false>), PN_ARGS); break;
        case 15: PN_LAUNCH((pndm_step_kernel<DP_PNDM_PLMS3, true>), PN_ARGS); break;
        case 16: PN_LAUNCH((pndm_step_kernel<DP_PNDM_PLMS4, false>), PN_ARGS); break;
        default: PN_LAUNCH((pndm_step_kernel<DP_PNDM_PLMS4, true>), PN_ARGS); break;
    }
#undef PN_ARGS
    return DP_LAUNCH_CHECK();
}
