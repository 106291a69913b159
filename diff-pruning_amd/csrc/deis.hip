// The elementwise kernels of the two remaining exponential-integrator solvers (diffusers/schedulers/scheduling_deis_multistep.py and
// scheduling_dpmsolver_singlestep.py), for epsilon, `sample` and `v_prediction` models, with or without dynamic thresholding:
//   dp_deis_step        one DEISMultistepScheduler.step in ONE pass: convert_model_output (:240-276) and the first-, second- or
//                       third-order log-rho update (:278-405)
//   dp_dpm_single_step  one DPMSolverSinglestepScheduler.step in ONE pass: convert_model_output (:291-355) and the first-, second- or
//                       third-order singlestep update (:357-519)
// The reference runs about a dozen elementwise launches per step and, with thresholding, a full sort per image; here every input is
// read once and the next state and the converted output are written once.  The per-image s of a thresholded step comes from
// dp_x0_abs_quantile (threshold.hip), whose (pred, sa, sb) form exactly the x0 formed below.
//
//   convert, ONE routine for both entry points (de_convert):
//     x0    epsilon: (x - sb m) / sa       sample: m                      v_prediction: sa x - sb m           (as threshold.hip forms it)
//     treat (stats != NULL)  x0 = clamp(x0, -s, s) / s,  s = stats[4 b + 3] of the element's image b
//     kept  DE_KEEP_DEIS: m0 = (x - sa x0) / sb, always -- for an epsilon model too: the reference converts there and back
//           DE_KEEP_X0   (singlestep dpmsolver++): m0 = the treated x0
//           DE_KEEP_EPS  (singlestep dpmsolver, never treated): epsilon: m;  sample: (x - sa m) / sb;  v_prediction: sa m + sb x
//   dp_deis_step
//     order 1  x' = kx x - k0 m0
//     order 2  x' = at ((x / as0 + c1 m0) + c2 m1)
//     order 3  x' = at (((x / as0 + c1 m0) + c2 m1) + c3 m2)
//   dp_dpm_single_step   (the conversion reads this call's x, the update the saved sample xs -- x itself at order 1)
//     order 1  x' = kx x - k0 m0
//     order 2  D1 = ir0 (m0 - m1);                                                  x' = (kx xs - k0 m1) - k1 D1
//     order 3  D1_0 = ir1 (m1 - m2); D1_1 = ir0 (m0 - m2);               midpoint:  x' = (kx xs - k0 m2) - k1 D1_1
//              heun: D1 = (r0 D1_0 - r1 D1_1) / dr; D2 = (2 (D1_1 - D1_0)) / dr;    x' = ((kx xs - k0 m2) - k1 D1) - k2 D2
// Where the reference adds a term (`+ c * D1`) the host passes k1 = -c: a - (-c) * D and a + c * D are the same bits.
//
// Rounding: every operation above is rounded separately (clang fp contract(off): hipcc would otherwise fuse a * b + c into one
// v_fma_f32), the divisions are true IEEE divisions, and every scalar arrives from the host in a coefficient struct, formed there with
// 0-d fp32 torch ops in the reference's order.
//
// Memory bound: 4 B per input the step reads and 8 B written per element, 16-byte accesses, nothing else.  An input the step does not
// read is not loaded.  Plain vector loads and stores, 64-bit element indices.
#include "dp_headtail.h"

// The launch macro of this file: the body of the library's own (dp_common.h) under a name of its own, so that the launch sites of
// this file are tabled by this file's test module (tests/test_deis_gpu.py), as dpm_solver.hip, unipc.hip and threshold.hip do.
#define DE_LAUNCH(k, ...) do { dp_launch_names[dp_launches++ & (DP_LAUNCH_RING - 1)] = #k; hipLaunchKernelGGL(k, __VA_ARGS__); } while (0)

enum { DE_KEEP_DEIS = 0, DE_KEEP_X0 = 1, DE_KEEP_EPS = 2 };

// What the conversion needs beside the data: uniform over the launch.
struct DeConv {
    int pred, keep, treat;
    float sa, sb;
};

static inline bool de_convert_reads_x(int pred, int keep) {
    if (keep == DE_KEEP_DEIS) return true;
    return keep == DE_KEEP_X0 ? pred != DP_X0_PRED_SAMPLE : pred != DP_X0_PRED_EPSILON;
}

// torch.clamp: a NaN value stays a NaN (both comparisons are false).  Selects only: no bit of v is changed.
__device__ __forceinline__ float de_clamp(float v, float lo, float hi) {
    const float t = v < lo ? lo : v;
    return t > hi ? hi : t;
}

// The value the history keeps for one element: the ONE copy, so that every instantiation of both kernels sees the same bits.
__device__ __forceinline__ float de_convert(const DeConv& p, float x, float m, float s) {
#pragma clang fp contract(off)
    if (p.keep == DE_KEEP_EPS) {
        if (p.pred == DP_X0_PRED_EPSILON) return m;
        if (p.pred == DP_X0_PRED_SAMPLE) {
            const float t = p.sa * m;
            return (x - t) / p.sb;
        }
        const float c = p.sa * m, d = p.sb * x;
        return c + d;
    }
    float x0;
    if (p.pred == DP_X0_PRED_EPSILON) {
        const float t = p.sb * m;
        x0 = (x - t) / p.sa;
    } else if (p.pred == DP_X0_PRED_SAMPLE) {
        x0 = m;
    } else {
        const float a = p.sa * x, b = p.sb * m;
        x0 = a - b;
    }
    if (p.treat) x0 = de_clamp(x0, -s, s) / s;            // a NaN s: the division makes every element NaN, as the reference's does
    if (p.keep == DE_KEEP_X0) return x0;
    const float t = p.sa * x0;
    return (x - t) / p.sb;
}

template <int ORDER>
__device__ __forceinline__ float deis_one(float x, float m0, float m1, float m2, const dp_deis_coef& c) {
#pragma clang fp contract(off)
    if (ORDER == 1) {
        const float a = c.kx * x, b = c.k0 * m0;
        return a - b;
    }
    float v = x / c.as0;
    const float t0 = c.c1 * m0;
    v = v + t0;
    const float t1 = c.c2 * m1;
    v = v + t1;
    if (ORDER == 3) {
        const float t2 = c.c3 * m2;
        v = v + t2;
    }
    return c.at * v;
}

// u: the sample the update starts from (x at order 1, the saved sample above it).
template <int ORDER, bool HEUN>
__device__ __forceinline__ float single_one(float u, float m0, float m1, float m2, const dp_dpm_single_coef& c) {
#pragma clang fp contract(off)
    const float a = c.kx * u;
    if (ORDER == 1) {
        const float b = c.k0 * m0;
        return a - b;
    }
    if (ORDER == 2) {
        const float D1 = c.ir0 * (m0 - m1);
        const float b = c.k0 * m1;
        const float v = a - b;
        const float t1 = c.k1 * D1;
        return v - t1;
    }
    const float D10 = c.ir1 * (m1 - m2);
    const float D11 = c.ir0 * (m0 - m2);
    const float b = c.k0 * m2;
    float v = a - b;
    if (!HEUN) {
        const float t1 = c.k1 * D11;
        return v - t1;
    }
    const float p = c.r0 * D10, q = c.r1 * D11;
    const float D1 = (p - q) / c.dr;
    const float d = D11 - D10;
    const float D2 = (2.0f * d) / c.dr;
    const float t1 = c.k1 * D1;
    v = v - t1;
    const float t2 = c.k2 * D2;
    return v - t2;
}

// The head / body / tail loop of dp_headtail.h over the rows of [B, n] (B = 1: flat data); grid (blocks along a row, rows), both
// strided.  `next` may be `x` (or `u`) itself and `m0_out` may be the oldest history buffer the step reads (no __restrict__ on those):
// a lane reads every input of its elements before it writes any of them, and no other lane touches them.  m aliases nothing.
// upd(u, m0, m1, m2) is the update of one element; READ_U: it starts from `u`, a buffer of its own, and not from x.
template <int ORDER, bool READ_U, typename F>
__device__ __forceinline__ void de_rows(const float* x, const float* u, const float* __restrict__ m, const float* m1, const float* m2,
                                        const float* __restrict__ stats, const DeConv& p, bool conv_x, float* next, float* m0_out, long long B,
                                        long long n, long long head, F&& upd) {
    const long long tid = (long long)blockIdx.x * 256 + threadIdx.x, stride = (long long)gridDim.x * 256;
    const bool need_x = conv_x || !READ_U;
    for (long long b = blockIdx.y; b < B; b += gridDim.y) {
        const float s = p.treat ? stats[4 * b + 3] : 1.0f;
        const long long off = b * n;
        const float* xr = need_x ? x + off : nullptr;
        const float* ur = READ_U ? u + off : nullptr;
        const float* mr = m + off;
        const float* ar = ORDER >= 2 ? m1 + off : nullptr;
        const float* br = ORDER >= 3 ? m2 + off : nullptr;
        float* nr = next + off;
        float* qr = m0_out + off;
        dp_ht_for(
            n, head, tid, stride,
            [&](long long at) {
                const float4 xv = dp_ld4(xr, at, need_x), uv = dp_ld4(ur, at, READ_U), mv = dp_ld4(mr, at, true);
                const float4 av = dp_ld4(ar, at, ORDER >= 2), bv = dp_ld4(br, at, ORDER >= 3);
                float4 q, o;
                q.x = de_convert(p, xv.x, mv.x, s);
                q.y = de_convert(p, xv.y, mv.y, s);
                q.z = de_convert(p, xv.z, mv.z, s);
                q.w = de_convert(p, xv.w, mv.w, s);
                o.x = upd(READ_U ? uv.x : xv.x, q.x, av.x, bv.x);
                o.y = upd(READ_U ? uv.y : xv.y, q.y, av.y, bv.y);
                o.z = upd(READ_U ? uv.z : xv.z, q.z, av.z, bv.z);
                o.w = upd(READ_U ? uv.w : xv.w, q.w, av.w, bv.w);
                dp_st4(nr, at, o);                                   // after every load of this lane's elements
                dp_st4(qr, at, q);
            },
            [&](long long i) {
                const float xs = dp_ld1(xr, i, need_x), us = dp_ld1(ur, i, READ_U), ms = mr[i];
                const float as = dp_ld1(ar, i, ORDER >= 2), bs = dp_ld1(br, i, ORDER >= 3);
                const float q = de_convert(p, xs, ms, s);
                const float o = upd(READ_U ? us : xs, q, as, bs);
                nr[i] = o;
                qr[i] = q;
            });
    }
}

template <int ORDER>
__global__ __launch_bounds__(256) void deis_step_kernel(const float* x, const float* __restrict__ m, const float* m1, const float* m2,
                                                        const float* __restrict__ stats, DeConv p, dp_deis_coef c, float* next, float* m0_out,
                                                        long long B, long long n, long long head) {
    de_rows<ORDER, false>(x, nullptr, m, m1, m2, stats, p, true, next, m0_out, B, n, head,
                          [&](float u, float m0, float a, float b) { return deis_one<ORDER>(u, m0, a, b, c); });
}

template <int ORDER, bool HEUN>
__global__ __launch_bounds__(256) void dpm_single_step_kernel(const float* x, const float* xs, const float* __restrict__ m, const float* m1,
                                                              const float* m2, const float* __restrict__ stats, DeConv p, int conv_x,
                                                              dp_dpm_single_coef c, float* next, float* m0_out, long long B, long long n,
                                                              long long head) {
    de_rows<ORDER, (ORDER > 1)>(x, xs, m, m1, m2, stats, p, conv_x != 0, next, m0_out, B, n, head,
                                [&](float u, float m0, float a, float b) { return single_one<ORDER, HEUN>(u, m0, a, b, c); });
}

// ---------------------------------------------------------------------------------------------------- launchers
// blocks along a row (`work` lanes wanted) and rows for a strided two-dimensional grid of at most DP_DEIS_MAX_BLOCKS blocks
static inline dim3 de_grid(long long work, long long B) {
    const long long cap = DP_DEIS_MAX_BLOCKS;
    const long long by = B > cap ? cap : B;
    long long bx = (work + 255) / 256;
    const long long room = cap / by;
    if (bx > room) bx = room;
    if (bx < 1) bx = 1;
    return dim3((unsigned)bx, (unsigned)by);
}

// What both entry points check: the buffers the step reads are there, and no output shares a byte with anything except through the
// aliases the kernels are written for -- x_next == x, x_next == xs, m0_out == `oldest` (the oldest history buffer the step reads).
// The caller has already set the pointers the step does not read to null.
static int de_check(const float* x, const float* xs, const float* m, const float* m1, const float* m2, const float* stats,
                    const float* oldest, const float* x_next, const float* m0_out, long long B, long long n) {
    const unsigned long long len = 4ull * (unsigned long long)B * (unsigned long long)n, slen = 16ull * (unsigned long long)B;
    const auto hit = [len](const void* a, const void* b) { return dp_bytes_overlap(a, len, b, len); };
    if ((x_next != x && hit(x_next, x)) || (x_next != xs && hit(x_next, xs))) return (int)hipErrorInvalidValue;
    if (hit(x_next, m) || hit(x_next, m1) || hit(x_next, m2) || hit(x_next, m0_out)) return (int)hipErrorInvalidValue;
    if (hit(m0_out, x) || hit(m0_out, xs) || hit(m0_out, m)) return (int)hipErrorInvalidValue;
    if ((m0_out != m1 || m1 != oldest) && hit(m0_out, m1)) return (int)hipErrorInvalidValue;
    if ((m0_out != m2 || m2 != oldest) && hit(m0_out, m2)) return (int)hipErrorInvalidValue;
    if (dp_bytes_overlap(stats, slen, x_next, len) || dp_bytes_overlap(stats, slen, m0_out, len)) return (int)hipErrorInvalidValue;
    return 0;
}

// The scalar head of every row: dp_ht_head's when n % 4 == 0 or the data is flat (then every row has the phase of the first), else n
// (all scalar) -- the per-row rule of dp_x0_step.
static inline long long de_row_head(long long B, long long n, const void* const* ptrs, int count) {
    return B > 1 && n % 4 != 0 ? n : dp_ht_head(n, ptrs, count);
}

extern "C" int dp_deis_step(const float* x, const float* m, const float* m1, const float* m2, const float* stats, int order, int pred,
                            const dp_deis_coef* coef, float* x_next, float* m0_out, long long B, long long n, void* stream) {
    if (B <= 0 || n <= 0) return 0;
    if (!x || !m || !coef || !x_next || !m0_out || order < 1 || order > 3) return (int)hipErrorInvalidValue;
    if (pred < DP_X0_PRED_EPSILON || pred > DP_X0_PRED_V) return (int)hipErrorInvalidValue;
    if (order < 3) m2 = nullptr;                                                 // not read below their order
    if (order < 2) m1 = nullptr;
    if ((order >= 2 && !m1) || (order >= 3 && !m2)) return (int)hipErrorInvalidValue;
    if (!stats) {                                                                // without stats the data is flat
        n *= B;
        B = 1;
    }
    const int bad = de_check(x, nullptr, m, m1, m2, stats, order == 3 ? m2 : m1, x_next, m0_out, B, n);
    if (bad) return bad;
    const void* ptrs[6] = {x, m, m1, m2, x_next, m0_out};
    const long long head = de_row_head(B, n, ptrs, 6);
    const dim3 grid = de_grid(dp_ht_work(n, head), B);
    const DeConv p = {pred, DE_KEEP_DEIS, stats ? 1 : 0, coef->sa, coef->sb};
    const dp_deis_coef c = *coef;
    const hipStream_t st = (hipStream_t)stream;
    // one site per instantiation: the launch ring keeps the stringised kernel expression of the site that launched
    switch (order) {
        case 1: DE_LAUNCH((deis_step_kernel<1>), grid, dim3(256), 0, st, x, m, m1, m2, stats, p, c, x_next, m0_out, B, n, head); break;
        case 2: DE_LAUNCH((deis_step_kernel<2>), grid, dim3(256), 0, st, x, m, m1, m2, stats, p, c, x_next, m0_out, B, n, head); break;
        default: DE_LAUNCH((deis_step_kernel<3>), grid, dim3(256), 0, st, x, m, m1, m2, stats, p, c, x_next, m0_out, B, n, head); break;
    }
    return DP_LAUNCH_CHECK();
}

extern "C" int dp_dpm_single_step(const float* x, const float* xs, const float* m, const float* m1, const float* m2, const float* stats,
                                  int order, int pred, int data_pred, int heun, const dp_dpm_single_coef* coef, float* x_next,
                                  float* m0_out, long long B, long long n, void* stream) {
    if (B <= 0 || n <= 0) return 0;
    if (!m || !coef || !x_next || !m0_out || order < 1 || order > 3) return (int)hipErrorInvalidValue;
    if (pred < DP_X0_PRED_EPSILON || pred > DP_X0_PRED_V) return (int)hipErrorInvalidValue;
    if (stats && !data_pred) return (int)hipErrorInvalidValue;                   // the reference thresholds on the dpmsolver++ branch only
    const int keep = data_pred ? DE_KEEP_X0 : DE_KEEP_EPS;
    const bool conv_x = de_convert_reads_x(pred, keep);
    if (order == 1) xs = nullptr;                                                // the update starts from x itself
    if (order > 1 && !conv_x) x = nullptr;                                       // neither the conversion nor the update reads it
    if (order < 3) m2 = nullptr;
    if (order < 2) m1 = nullptr;
    if ((order == 1 || conv_x) && !x) return (int)hipErrorInvalidValue;
    if ((order >= 2 && (!xs || !m1)) || (order >= 3 && !m2)) return (int)hipErrorInvalidValue;
    if (!stats) {
        n *= B;
        B = 1;
    }
    const int bad = de_check(x, xs, m, m1, m2, stats, order == 3 ? m2 : m1, x_next, m0_out, B, n);
    if (bad) return bad;
    const void* ptrs[7] = {x, xs, m, m1, m2, x_next, m0_out};
    const long long head = de_row_head(B, n, ptrs, 7);
    const dim3 grid = de_grid(dp_ht_work(n, head), B);
    const DeConv p = {pred, keep, stats ? 1 : 0, coef->sa, coef->sb};
    const int cx = conv_x ? 1 : 0;
    const dp_dpm_single_coef c = *coef;
    const hipStream_t st = (hipStream_t)stream;
    // one site per instantiation; heun differs from midpoint in the kernel at order 3 only (below it in the host's k1)
    switch (order == 3 && heun ? 4 : order) {
        case 1: DE_LAUNCH((dpm_single_step_kernel<1, false>), grid, dim3(256), 0, st, x, xs, m, m1, m2, stats, p, cx, c, x_next, m0_out, B, n, head); break;
        case 2: DE_LAUNCH((dpm_single_step_kernel<2, false>), grid, dim3(256), 0, st, x, xs, m, m1, m2, stats, p, cx, c, x_next, m0_out, B, n, head); break;
        case 3: DE_LAUNCH((dpm_single_step_kernel<3, false>), grid, dim3(256), 0, st, x, xs, m, m1, m2, stats, p, cx, c, x_next, m0_out, B, n, head); break;
        default: DE_LAUNCH((dpm_single_step_kernel<3, true>), grid, dim3(256), 0, st, x, xs, m, m1, m2, stats, p, cx, c, x_next, m0_out, B, n, head); break;
    }
    return DP_LAUNCH_CHECK();
}
