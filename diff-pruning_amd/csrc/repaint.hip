// The two elementwise kernels of the RePaint scheduler (diffusers/schedulers/scheduling_repaint.py):
//   dp_repaint_step  one scheduler step in ONE pass (:250-293): the x0 prediction with its clip, the DDIM update of the unknown region,
//                    the re-noised original image of the known region and the blend by the mask.  The reference runs about fifteen
//                    elementwise launches; here x, e, z, o and the mask are read once and the next state (and, when asked for, the
//                    x0 prediction) written once.
//   dp_repaint_undo  up to DP_REPAINT_UNDO_MAX re-noising steps of undo_step (:303-318) chained in registers: x is read once and
//                    written once, each noise tensor read once.  The reference runs three launches per re-noising step.
//   x: the state, e: the model output, z: the noise of this step, o: the original image, m: the mask (1 = known)
//   x0  = (x - sb * e) / sa                        clamped to [-1, 1] with CLIP
//   u   = (sap * x0 + cd * e) + (NOISE ? sd * z : 0)                (the reference adds a Python 0: a negative zero turns positive)
//   k   = sap * o + s1 * z
//   out = m * k + (1 - m) * u
//   undo: x = a_i * x + b_i * z_i, i = 0 .. k - 1
//
// Rounding: every operation above is rounded separately (clang fp contract(off): hipcc would otherwise fuse a * b + c into one
// v_fma_f32), the division is a true IEEE division, and the scalars arrive from the host, which forms them with 0-d fp32 torch ops in
// the reference's order (diffusion.RePaintScheduler).  The clamp is two compares: a NaN stays a NaN, as in torch.clamp.
//
// The mask is read where it lies: element i of the data reads m[(i / outer) * mstride + (i % inner)], which covers a mask of the
// data's own shape (FULL: 16-byte loads, the pointer takes part in the head rule) and the broadcast ones -- [B,1,H,W], [1,1,H,W],
// [1,C,H,W] -- with 4-byte loads (BROADCAST: a 16-byte group of the data may straddle a plane or an image).  One division pair per
// group, in 32 bits when n and outer allow it; the four elements of a group step the pair forward.
//
// Memory bound: 4 x (4 reads + 1 write) B per element + the mask's bytes, 16-byte accesses of the data.  Plain vector loads and stores.
#include "dp_headtail.h"

// The launch macro of this file: the body of the library's own (dp_common.h) under a name of its own, so that the launch sites of
// this file are tabled by this file's test module (tests/test_repaint_gpu.py), as dpm_solver.hip, unipc.hip and pndm.hip do.
#define RP_LAUNCH(k, ...) do { dp_launch_names[dp_launches++ & (DP_LAUNCH_RING - 1)] = #k; hipLaunchKernelGGL(k, __VA_ARGS__); } while (0)

template <bool CLIP, bool NOISE>
__device__ __forceinline__ float repaint_one(float x, float e, float z, float o, float m, const dp_repaint_coef& c, float& x0) {
#pragma clang fp contract(off)
    const float t = c.sb * e;
    float p = (x - t) / c.sa;
    if (CLIP) {
        p = p < -1.f ? -1.f : p;
        p = p > 1.f ? 1.f : p;
    }
    x0 = p;
    const float dir = c.cd * e;
    const float a = c.sap * p;
    const float ad = a + dir;
    float var = 0.f;
    if (NOISE) var = c.sd * z;
    const float u = ad + var;
    const float k1 = c.sap * o;
    const float k2 = c.s1 * z;
    const float k = k1 + k2;
    const float mk = m * k;
    const float im = 1.f - m;
    const float mu = im * u;
    return mk + mu;
}

// where element i of the data finds its mask value: (image index q, offset r inside the image's `outer` elements, r % inner)
struct rp_mask_pos {
    long long q, r, s;
};

__device__ __forceinline__ rp_mask_pos rp_mask_at(long long i, long long outer, long long inner, bool small) {
    rp_mask_pos p;
    if (small) {                                                          // n, outer < 2^31: two 32-bit divisions
        const unsigned iu = (unsigned)i, ou = (unsigned)outer, nu = (unsigned)inner;
        const unsigned q = iu / ou, r = iu - q * ou;
        p.q = q, p.r = r, p.s = r % nu;
    } else {
        p.q = i / outer;
        p.r = i - p.q * outer;
        p.s = p.r % inner;
    }
    return p;
}

// the mask value at p, then p one element on (inner divides outer: an image boundary is a period boundary too)
__device__ __forceinline__ float rp_mask_next(const float* m, rp_mask_pos& p, long long outer, long long mstride, long long inner) {
    const float v = m[p.q * mstride + p.s];
    ++p.r, ++p.s;
    if (p.s == inner) p.s = 0;
    if (p.r == outer) p.r = 0, p.s = 0, ++p.q;
    return v;
}

// The head / body / tail loop of dp_headtail.h.  `out` may be `x` itself (no __restrict__ on those): a lane reads every input of its
// elements before it writes any of them, and no other lane touches them.  Nothing else aliases.
template <bool CLIP, bool NOISE, bool FULL, bool X0>
__global__ __launch_bounds__(256) void repaint_step_kernel(const float* x, const float* __restrict__ e, const float* __restrict__ z,
                                                           const float* __restrict__ o, const float* __restrict__ m, long long outer,
                                                           long long mstride, long long inner, dp_repaint_coef c, float* out,
                                                           float* __restrict__ x0_out, long long n, long long head) {
    const bool small = n < (1ll << 31) && outer < (1ll << 31);
    dp_ht_for(
        n, head, (long long)blockIdx.x * 256 + threadIdx.x, (long long)gridDim.x * 256,
        [&](long long at) {
            const float4 xv = dp_ld4(x, at, true), ev = dp_ld4(e, at, true), zv = dp_ld4(z, at, true), ov = dp_ld4(o, at, true);
            float4 mv;
            if (FULL) {
                mv = dp_ld4(m, at, true);
            } else {
                rp_mask_pos p = rp_mask_at(at, outer, inner, small);
                mv.x = rp_mask_next(m, p, outer, mstride, inner);
                mv.y = rp_mask_next(m, p, outer, mstride, inner);
                mv.z = rp_mask_next(m, p, outer, mstride, inner);
                mv.w = rp_mask_next(m, p, outer, mstride, inner);
            }
            float4 r, pv;
            r.x = repaint_one<CLIP, NOISE>(xv.x, ev.x, zv.x, ov.x, mv.x, c, pv.x);
            r.y = repaint_one<CLIP, NOISE>(xv.y, ev.y, zv.y, ov.y, mv.y, c, pv.y);
            r.z = repaint_one<CLIP, NOISE>(xv.z, ev.z, zv.z, ov.z, mv.z, c, pv.z);
            r.w = repaint_one<CLIP, NOISE>(xv.w, ev.w, zv.w, ov.w, mv.w, c, pv.w);
            dp_st4(out, at, r);                                      // after every load of this lane's elements
            if (X0) dp_st4(x0_out, at, pv);
        },
        [&](long long i) {
            const float xs = x[i], es = e[i], zs = z[i], os = o[i];
            float ms;
            if (FULL) {
                ms = m[i];
            } else {
                rp_mask_pos p = rp_mask_at(i, outer, inner, small);
                ms = m[p.q * mstride + p.s];
            }
            float ps;
            const float v = repaint_one<CLIP, NOISE>(xs, es, zs, os, ms, c, ps);
            out[i] = v;
            if (X0) x0_out[i] = ps;
        });
}

__device__ __forceinline__ float undo_one(float a, float x, float b, float z) {
#pragma clang fp contract(off)
    const float p = a * x;
    const float q = b * z;
    return p + q;
}

// K re-noising steps in registers.  `out` may be `x` itself; the noise tensors alias neither.
template <int K>
__global__ __launch_bounds__(256) void repaint_undo_kernel(const float* x, dp_repaint_undo_coef c, float* out, long long n, long long head) {
    dp_ht_for(
        n, head, (long long)blockIdx.x * 256 + threadIdx.x, (long long)gridDim.x * 256,
        [&](long long at) {
            float4 v = dp_ld4(x, at, true);
#pragma unroll
            for (int j = 0; j < K; ++j) {
                const float4 zv = dp_ld4(c.z[j], at, true);
                v.x = undo_one(c.a[j], v.x, c.b[j], zv.x);
                v.y = undo_one(c.a[j], v.y, c.b[j], zv.y);
                v.z = undo_one(c.a[j], v.z, c.b[j], zv.z);
                v.w = undo_one(c.a[j], v.w, c.b[j], zv.w);
            }
            dp_st4(out, at, v);
        },
        [&](long long i) {
            float v = x[i];
#pragma unroll
            for (int j = 0; j < K; ++j) v = undo_one(c.a[j], v, c.b[j], c.z[j][i]);
            out[i] = v;
        });
}

extern "C" int dp_repaint_step(const float* x, const float* e, const float* z, const float* o, const float* m, long long m_outer,
                               long long m_stride, long long m_inner, int clip, int noise, const dp_repaint_coef* coef, float* out,
                               float* x0_out, long long n, void* stream) {
    if (n <= 0) return 0;
    if (!x || !e || !z || !o || !m || !coef || !out) return (int)hipErrorInvalidValue;
    // the mask's geometry: a period `inner` that divides the image length `outer`, images a non-negative stride apart
    if (m_inner < 1 || m_outer < m_inner || m_outer % m_inner != 0 || m_stride < 0) return (int)hipErrorInvalidValue;
    const bool full = m_inner >= n;                                             // then i / outer == 0 and i % inner == i
    const long long images = (n - 1) / m_outer + 1;
    if (!full && m_stride != 0 && m_stride < m_inner && images > 1) return (int)hipErrorInvalidValue;   // images of the mask overlap
    // the one alias the kernel is written for: out == x.  Everything else is disjoint: no output shares a byte with the other
    // output or with an input that is not itself.
    const unsigned long long len = 4ull * (unsigned long long)n;
    const unsigned long long mlen = full ? len : 4ull * (unsigned long long)((images - 1) * m_stride + m_inner);
    const auto hit = [len](const void* a, const void* b) { return dp_bytes_overlap(a, len, b, len); };
    if ((out != x && hit(out, x)) || hit(out, e) || hit(out, z) || hit(out, o) || dp_bytes_overlap(out, len, m, mlen))
        return (int)hipErrorInvalidValue;
    if (hit(x0_out, x) || hit(x0_out, e) || hit(x0_out, z) || hit(x0_out, o) || hit(x0_out, out) || dp_bytes_overlap(x0_out, len, m, mlen))
        return (int)hipErrorInvalidValue;
    const void* ptrs[7] = {x, e, z, o, out, x0_out, full ? m : nullptr};        // a broadcast mask is read 4 bytes at a time
    const long long head = dp_ht_head(n, ptrs, 7);
    const unsigned grid = dp_ht_blocks(n, head, DP_REPAINT_MAX_BLOCKS);
    const dp_repaint_coef c = *coef;
    const hipStream_t st = (hipStream_t)stream;
#define RP_ARGS dim3(grid), dim3(256), 0, st, x, e, z, o, m, m_outer, m_stride, m_inner, c, out, x0_out, n, head
    // one site per instantiation: the launch ring keeps the stringised kernel expression of the site that launched
    switch ((clip ? 8 : 0) + (noise ? 4 : 0) + (full ? 2 : 0) + (x0_out ? 1 : 0)) {
        case 0: RP_LAUNCH((repaint_step_kernel<false, false, false, false>), RP_ARGS); break;
        case 1: RP_LAUNCH((repaint_step_kernel<false, false, false, true>), RP_ARGS); break;
        case 2: RP_LAUNCH((repaint_step_kernel<false, false, true, false>), RP_ARGS); break;
        case 3: RP_LAUNCH((repaint_step_kernel<false, false, true, true>), RP_ARGS); break;
        case 4: RP_LAUNCH((repaint_step_kernel<false, true, false, false>), RP_ARGS); break;
        case 5: RP_LAUNCH((repaint_step_kernel<false, true, false, true>), RP_ARGS); break;
        case 6: RP_LAUNCH((repaint_step_kernel<false, true, true, false>), RP_ARGS); break;
        case 7: RP_LAUNCH((repaint_step_kernel<false, true, true, true>), RP_ARGS); break;
        case 8: RP_LAUNCH((repaint_step_kernel<true, false, false, false>), RP_ARGS); break;
        case 9: RP_LAUNCH((repaint_step_kernel<true, false, false, true>), RP_ARGS); break;
        case 10: RP_LAUNCH((repaint_step_kernel<true, false, true, false>), RP_ARGS); break;
        case 11: RP_LAUNCH((repaint_step_kernel<true, false, true, true>), RP_ARGS); break;
        case 12: RP_LAUNCH((repaint_step_kernel<true, true, false, false>), RP_ARGS); break;
        case 13: RP_LAUNCH((repaint_step_kernel<true, true, false, true>), RP_ARGS); break;
        case 14: RP_LAUNCH((repaint_step_kernel<true, true, true, false>), RP_ARGS); break;
        default: RP_LAUNCH((repaint_step_kernel<true, true, true, true>), RP_ARGS); break;
    }
#undef RP_ARGS
    return DP_LAUNCH_CHECK();
}

extern "C" int dp_repaint_undo(const float* x, const dp_repaint_undo_coef* coef, int k, float* out, long long n, void* stream) {
    if (n <= 0) return 0;
    if (!x || !coef || !out || k < 1 || k > DP_REPAINT_UNDO_MAX) return (int)hipErrorInvalidValue;
    const unsigned long long len = 4ull * (unsigned long long)n;
    if (out != x && dp_bytes_overlap(out, len, x, len)) return (int)hipErrorInvalidValue;
    dp_repaint_undo_coef c = *coef;
    const void* ptrs[2 + DP_REPAINT_UNDO_MAX] = {x, out};
    for (int j = 0; j < DP_REPAINT_UNDO_MAX; ++j) {
        if (j >= k) {                                                            // not read by this launch
            c.z[j] = nullptr, c.a[j] = 0.f, c.b[j] = 0.f;
            continue;
        }
        if (!c.z[j] || dp_bytes_overlap(out, len, c.z[j], len)) return (int)hipErrorInvalidValue;
        ptrs[2 + j] = c.z[j];
    }
    const long long head = dp_ht_head(n, ptrs, 2 + k);
    const unsigned grid = dp_ht_blocks(n, head, DP_REPAINT_MAX_BLOCKS);
    const hipStream_t st = (hipStream_t)stream;
#define RP_ARGS dim3(grid), dim3(256), 0, st, x, c, out, n, head
    switch (k) {
        case 1: RP_LAUNCH((repaint_undo_kernel<1>), RP_ARGS); break;
        case 2: RP_LAUNCH((repaint_undo_kernel<2>), RP_ARGS); break;
        case 3: RP_LAUNCH((repaint_undo_kernel<3>), RP_ARGS); break;
        case 4: RP_LAUNCH((repaint_undo_kernel<4>), RP_ARGS); break;
        case 5: RP_LAUNCH((repaint_undo_kernel<5>), RP_ARGS); break;
        case 6: RP_LAUNCH((repaint_undo_kernel<6>), RP_ARGS); break;
        case 7: RP_LAUNCH((repaint_undo_kernel<7>), RP_ARGS); break;
        default: RP_LAUNCH((repaint_undo_kernel<8>), RP_ARGS); break;
    }
#undef RP_ARGS
    return DP_LAUNCH_CHECK();
}
