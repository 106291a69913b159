// x0 forming, dynamic thresholding and the DDPM / DDIM update for the three model types (diffusers/schedulers/scheduling_ddpm.py:278-310,
// :355-401; scheduling_ddim.py:205-237, :334-385):
//   dp_x0_abs_quantile    per image b of [B, n]: the order statistics lo and hi of |x0|, EXACT (a radix select over the bit patterns of
//                         the non-negative floats; -0 counts as +0, a NaN as the largest key), torch.quantile's lerp between them with
//                         ONE fused multiply-add, and s = clamp(quantile, 1, sample_max_value).  stats[b] = (v_lo, v_hi, quantile, s).
//                         Two routes: the row in LDS (one workgroup per image, n <= DP_THRESHOLD_LDS_MAX) and a multi-block one with
//                         per-image digit histograms in a workspace.  The reference sorts every image (torch.quantile).
//   dp_x0_step            one pass over [B, n]: form (x0, eps), treat x0 (none | clip | threshold with the image's s), optionally
//                         re-derive eps from the treated x0, update (DDIM | DDPM | CONVERT), write.
//   dp_x0_threshold_step  the LDS route with the apply stage switched on: the workgroup that selected an image's s applies it.  ONE launch,
//                         the same bits as dp_x0_abs_quantile followed by dp_x0_step.
//
//   model         x0                   eps
//   epsilon       (x - sb m) / sa      m
//   sample        m                    (x - sa x0) / sb     from the x0 BEFORE its treatment
//   v_prediction  sa x - sb m          sa m + sb x
//   clip: x0 = clamp(x0, -range, range);  threshold: x0 = clamp(x0, -s, s) / s;  reclip: eps = (x - sa x0) / sb from the treated x0
//   DDIM: prev = c0 x0 + c1 eps [+ cz z];  DDPM: prev = (c0 x0 + c1 x) + (cz z | 0);  CONVERT: the treated x0 alone
//
// Rounding: every operation is rounded separately (clang fp contract(off)), the divisions are true IEEE divisions, the scalars arrive
// from the host.  The ONE contraction is the explicit fmaf of the quantile's lerp, as torch's lerp has it.  The counters of the select are
// integers: the order in which they are accumulated does not change them, and no floating-point value depends on scheduling.
// Plain vector loads and stores, 64-bit element indices.
#include "dp_headtail.h"

// The launch macro of this file: the body of the library's own (dp_common.h) under a name of its own, so that the launch sites of
// this file are tabled by this file's test module (tests/test_threshold_gpu.py), as dpm_solver.hip and unipc.hip do.
#define TH_LAUNCH(k, ...) do { dp_launch_names[dp_launches++ & (DP_LAUNCH_RING - 1)] = #k; hipLaunchKernelGGL(k, __VA_ARGS__); } while (0)

#define TH_LDS_THREADS 1024
#define TH_WS_STRIDE 264                 // unsigned words of workspace per image: 256 histogram bins, then the TH_* state words
enum { TH_PREFIX = 256, TH_K = 257, TH_NAN = 258, TH_MINABOVE = 259, TH_NEED = 260 };
#define TH_NAN_KEY 0x7f800000u           // keys above it are NaNs

// The rank of the quantile as the host formed it (torch.quantile: r = fp32(q) * fp32(n - 1), lo = floor r, hi = ceil r, w = r - lo).
struct ThRank {
    unsigned lo, hi;
    float w, max_value;
};

// What the apply stage needs beside the data.
struct ThStep {
    int mode, pred, treat, reclip;
    dp_x0_coef c;
};

// ---------------------------------------------------------------------------------------------------- the arithmetic, one copy each
// The x0 prediction and the epsilon prediction of one element: the ONE copy, so that every kernel of this file sees the same bits.
__device__ __forceinline__ void th_form(int pred, float x, float m, float sa, float sb, float& x0, float& eps) {
#pragma clang fp contract(off)
    if (pred == DP_X0_PRED_EPSILON) {
        const float t = sb * m;
        x0 = (x - t) / sa;
        eps = m;
    } else if (pred == DP_X0_PRED_SAMPLE) {
        x0 = m;
        const float t = sa * m;
        eps = (x - t) / sb;
    } else {
        const float a = sa * x, b = sb * m;
        x0 = a - b;
        const float c = sa * m, d = sb * x;
        eps = c + d;
    }
}

// torch.clamp: a NaN value stays a NaN (both comparisons are false), lo > hi gives hi.  Selects only: no bit of v is changed.
__device__ __forceinline__ float th_clamp(float v, float lo, float hi) {
    const float t = v < lo ? lo : v;
    return t > hi ? hi : t;
}

// treatment, eps re-derivation and update of one element.  Returns prev (CONVERT: the treated x0); x0 leaves treated.
__device__ __forceinline__ float th_update(const ThStep& p, float x, float z, bool has_z, float s, float& x0, float eps) {
#pragma clang fp contract(off)
    if (p.treat == DP_X0_TREAT_CLIP) {
        x0 = th_clamp(x0, -p.c.range, p.c.range);
    } else if (p.treat == DP_X0_TREAT_THRESHOLD) {
        x0 = th_clamp(x0, -s, s) / s;                 // a NaN s: the division makes every element NaN, as the reference's does
    }
    if (p.mode == DP_X0_MODE_CONVERT) return x0;
    if (p.reclip) {
        const float t = p.c.sa * x0;
        eps = (x - t) / p.c.sb;
    }
    const float a = p.c.c0 * x0;
    float prev;
    if (p.mode == DP_X0_MODE_DDIM) {
        const float b = p.c.c1 * eps;
        prev = a + b;
        if (has_z) {
            const float n = p.c.cz * z;
            prev = prev + n;
        }
    } else {
        const float b = p.c.c1 * x;
        prev = a + b;
        const float n = has_z ? p.c.cz * z : 0.0f;    // the reference adds its `variance = 0` at t == 0 too: -0 + 0 = +0
        prev = prev + n;
    }
    return prev;
}

__device__ __forceinline__ unsigned th_key(float x0) { return __float_as_uint(x0) & 0x7fffffffu; }

// (v_lo, v_hi, quantile, s) of one image from its two order statistics: torch's lerp with ONE fma, torch's clamp.
__device__ __forceinline__ void th_finish(unsigned lo_key, unsigned hi_key, bool has_nan, const ThRank& r, float* out4) {
#pragma clang fp contract(off)
    const float vl = __uint_as_float(lo_key), vh = __uint_as_float(hi_key);
    const float d = vh - vl;
    float q = r.w < 0.5f ? fmaf(r.w, d, vl) : fmaf(r.w - 1.0f, d, vh);
    if (has_nan) q = __uint_as_float(0x7fc00000u);
    out4[0] = vl;
    out4[1] = vh;
    out4[2] = q;
    out4[3] = th_clamp(q, 1.0f, r.max_value);
}

// One wave picks the digit of the k-th smallest (0-based) key from a 256-bin histogram (LDS or global): lane l owns bins 4 l .. 4 l + 3,
// an inclusive scan over the lanes finds the lane, the lane finds its bin.  Every lane returns the same (digit, keys below the digit,
// keys in it).  k < the histogram's total, so exactly one lane holds the crossing.
__device__ __forceinline__ void th_pick(const unsigned* hist, unsigned k, unsigned& digit, unsigned& below, unsigned& count) {
    const int lane = threadIdx.x & 63;
    const unsigned c0 = hist[4 * lane], c1 = hist[4 * lane + 1], c2 = hist[4 * lane + 2], c3 = hist[4 * lane + 3];
    const unsigned mine = c0 + c1 + c2 + c3;
    unsigned incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
    }
    const unsigned excl = incl - mine;
    const bool here = excl <= k && k < incl;
    unsigned d = 0, b = 0, c = 0;
    if (here) {
        const unsigned r = k - excl;
        if (r < c0) { d = 0; b = 0; c = c0; }
        else if (r < c0 + c1) { d = 1; b = c0; c = c1; }
        else if (r < c0 + c1 + c2) { d = 2; b = c0 + c1; c = c2; }
        else { d = 3; b = c0 + c1 + c2; c = c3; }
        d += 4 * lane;
        b += excl;
    }
    const unsigned long long who = __ballot(here);
    const int src = who ? __ffsll((long long)who) - 1 : 0;
    digit = __shfl(d, src, 64);
    below = __shfl(b, src, 64);
    count = __shfl(c, src, 64);
}

// f(i, x0) for the elements i of one row that the strided lanes (tid, stride) own, in the head / body / tail loop of dp_headtail.h (the
// launcher chooses head so that the row pointers + head are 16-byte aligned in every row, or head = n).  xr is not read for a `sample`
// model.
template <typename F>
__device__ __forceinline__ void th_row_x0(const float* __restrict__ xr, const float* __restrict__ mr, long long n, long long head, int pred,
                                          float sa, float sb, long long tid, long long stride, F&& f) {
    const bool need_x = pred != DP_X0_PRED_SAMPLE;
    dp_ht_for(
        n, head, tid, stride,
        [&](long long at) {
            const float4 mv = dp_ld4(mr, at, true), xv = dp_ld4(xr, at, need_x);
            float a, b, c, d, e;
            th_form(pred, xv.x, mv.x, sa, sb, a, e);
            th_form(pred, xv.y, mv.y, sa, sb, b, e);
            th_form(pred, xv.z, mv.z, sa, sb, c, e);
            th_form(pred, xv.w, mv.w, sa, sb, d, e);
            f(at, a);
            f(at + 1, b);
            f(at + 2, c);
            f(at + 3, d);
        },
        [&](long long i) {
            float a, e;
            th_form(pred, dp_ld1(xr, i, need_x), mr[i], sa, sb, a, e);
            f(i, a);
        });
}

// The treated-x0 update of the elements of one row that the strided lanes (tid, stride) own, in the same loop: form (x0, eps), treat x0
// with s, update, write pr and (optional) qr.  ROW: x0 is not formed again but read from `row`, where th_row_x0's caller put it (the
// same bits).  pr may be xr (no __restrict__ on either): a lane reads every input of its elements before it writes any of them, and
// no other lane touches them.  xr is not read where neither the model nor the update needs x.
template <bool ROW>
__device__ __forceinline__ void th_row_update(const ThStep& p, float s, const float* xr, const float* __restrict__ mr, const float* __restrict__ zr,
                                              const float* row, float* pr, float* __restrict__ qr, long long n, long long head, long long tid,
                                              long long stride) {
    const bool need_x = !(p.mode == DP_X0_MODE_CONVERT && p.pred == DP_X0_PRED_SAMPLE);
    const bool has_z = zr != nullptr;
    dp_ht_for(
        n, head, tid, stride,
        [&](long long at) {
            const float4 xv = dp_ld4(xr, at, need_x), mv = dp_ld4(mr, at, true), zv = dp_ld4(zr, at, has_z);
            float4 q, e, o;
            th_form(p.pred, xv.x, mv.x, p.c.sa, p.c.sb, q.x, e.x);
            th_form(p.pred, xv.y, mv.y, p.c.sa, p.c.sb, q.y, e.y);
            th_form(p.pred, xv.z, mv.z, p.c.sa, p.c.sb, q.z, e.z);
            th_form(p.pred, xv.w, mv.w, p.c.sa, p.c.sb, q.w, e.w);
            if (ROW) q = dp_ld4(row, at, true);
            o.x = th_update(p, xv.x, zv.x, has_z, s, q.x, e.x);
            o.y = th_update(p, xv.y, zv.y, has_z, s, q.y, e.y);
            o.z = th_update(p, xv.z, zv.z, has_z, s, q.z, e.z);
            o.w = th_update(p, xv.w, zv.w, has_z, s, q.w, e.w);
            dp_st4(pr, at, o);                                       // after every load of this lane's elements
            if (qr) dp_st4(qr, at, q);
        },
        [&](long long i) {
            const float xs = dp_ld1(xr, i, need_x), zs = dp_ld1(zr, i, has_z);
            float q, e;
            th_form(p.pred, xs, mr[i], p.c.sa, p.c.sb, q, e);
            if (ROW) q = row[i];
            const float o = th_update(p, xs, zs, has_z, s, q, e);
            pr[i] = o;
            if (qr) qr[i] = q;
        });
}

// ---------------------------------------------------------------------------------------------------- the row in LDS
// One workgroup per image.  x0 is written once into LDS; four 8-bit digits of the key are selected most significant first with an LDS
// histogram each; v_hi is v_lo itself when more than hi keys are <= v_lo, else the smallest key above v_lo.  APPLY: the workgroup goes
// on to the update of its image: x0 from LDS, x, m and z re-read.  `prev` may be `x` (no __restrict__ on either): the rows of two
// workgroups are disjoint, a barrier separates the select's reads of the row from the apply stage, and in that stage a lane reads
// its elements before it writes them.
template <bool APPLY>
__global__ __launch_bounds__(TH_LDS_THREADS) void th_lds_kernel(const float* x, const float* __restrict__ m, const float* __restrict__ z,
                                                                ThStep p, ThRank r, float* prev, float* __restrict__ x0_out,
                                                                float* __restrict__ stats, long long n, long long head) {
    __shared__ __attribute__((aligned(16))) float row_store[DP_THRESHOLD_LDS_MAX + 4];
    __shared__ unsigned hist[256];
    __shared__ unsigned sh[8];                      // 0 prefix, 1 k, 2 NaN seen, 3 smallest key above v_lo, 4 keys <= v_lo; 5 s (APPLY)
    const long long b = blockIdx.x;
    const int tid = threadIdx.x;
    const float* xr = x ? x + b * n : nullptr;
    const float* mr = m + b * n;
    // LDS index = row index + pad, so that the 16-byte groups of the row are 16-byte groups of LDS as well
    float* row = row_store + ((4 - (head & 3)) & 3);
    if (tid < 8) sh[tid] = tid == 1 ? r.lo : tid == 3 ? 0xffffffffu : 0u;
    bool nan = false;
    th_row_x0(xr, mr, n, head, p.pred, p.c.sa, p.c.sb, tid, TH_LDS_THREADS, [&](long long i, float v) {
        row[i] = v;
        nan = nan || th_key(v) > TH_NAN_KEY;
    });
    __syncthreads();
    if (nan) sh[2] = 1u;                            // every writer stores the same word
    unsigned prefix = 0, mask = 0, eq = 0;
    for (int shift = 24; shift >= 0; shift -= 8) {
        if (tid < 256) hist[tid] = 0u;
        __syncthreads();
        for (long long i = tid; i < n; i += TH_LDS_THREADS) {
            const unsigned key = th_key(row[i]);
            if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (tid < 64) {
            unsigned digit, below, count;
            th_pick(hist, sh[1], digit, below, count);
            if (tid == 0) {
                sh[0] = prefix | (digit << shift);
                sh[1] -= below;
                sh[4] = count;
            }
        }
        __syncthreads();
        prefix = sh[0];
        eq = sh[4];
        mask |= 255u << shift;
    }
    // keys below v_lo: lo - k; keys <= v_lo: that + eq
    const unsigned lo_key = prefix;
    const bool need = r.lo - sh[1] + eq <= r.hi;
    if (need) {
        unsigned best = 0xffffffffu;
        for (long long i = tid; i < n; i += TH_LDS_THREADS) {
            const unsigned key = th_key(row[i]);
            if (key > lo_key && key < best) best = key;
        }
        if (best != 0xffffffffu) atomicMin(&sh[3], best);
        __syncthreads();
    }
    if (tid == 0) {
        float out4[4];
        th_finish(lo_key, need ? sh[3] : lo_key, sh[2] != 0u, r, out4);
        stats[4 * b] = out4[0];
        stats[4 * b + 1] = out4[1];
        stats[4 * b + 2] = out4[2];
        stats[4 * b + 3] = out4[3];
        sh[5] = __float_as_uint(out4[3]);
    }
    if (!APPLY) return;
    __syncthreads();
    const float s = __uint_as_float(sh[5]);
    th_row_update<true>(p, s, xr, mr, z ? z + b * n : nullptr, row, prev + b * n, x0_out ? x0_out + b * n : nullptr, n, head, tid,
                        TH_LDS_THREADS);
}

// ---------------------------------------------------------------------------------------------------- the multi-block route
// x0 is recomputed from x and m in every pass (8 B read per element and pass, no key buffer of B n words to write and keep).
// ws: TH_WS_STRIDE words per image.  th_init zeroes them; th_hist adds one digit's histogram of the keys under the image's prefix
// (an LDS histogram per block, then at most 256 integer atomics per block and image); th_pick, one wave per image, narrows the prefix
// and zeroes the bins for the next pass; th_minabove finds the smallest key above v_lo where v_hi is not v_lo; th_stats finishes.
__global__ __launch_bounds__(256) void th_init_kernel(unsigned* __restrict__ ws, ThRank r, long long B) {
    for (long long b = blockIdx.x; b < B; b += gridDim.x) {
        unsigned* w = ws + b * TH_WS_STRIDE;
        for (int i = threadIdx.x; i < TH_WS_STRIDE; i += 256) w[i] = i == TH_K ? r.lo : i == TH_MINABOVE ? 0xffffffffu : 0u;
    }
}

__global__ __launch_bounds__(256) void th_hist_kernel(const float* __restrict__ x, const float* __restrict__ m, int pred, float sa, float sb,
                                                      unsigned* ws, long long B, long long n, long long head, int shift) {
    __shared__ unsigned hist[256];
    const unsigned mask = shift == 24 ? 0u : 0xffffffffu << (shift + 8);
    const long long tid = (long long)blockIdx.x * 256 + threadIdx.x, stride = (long long)gridDim.x * 256;
    for (long long b = blockIdx.y; b < B; b += gridDim.y) {
        unsigned* w = ws + b * TH_WS_STRIDE;
        const unsigned prefix = w[TH_PREFIX];
        hist[threadIdx.x] = 0u;
        __syncthreads();
        bool nan = false;
        th_row_x0(x ? x + b * n : nullptr, m + b * n, n, head, pred, sa, sb, tid, stride, [&](long long, float v) {
            const unsigned key = th_key(v);
            nan = nan || key > TH_NAN_KEY;
            if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
        });
        __syncthreads();
        const unsigned c = hist[threadIdx.x];
        if (c) atomicAdd(&w[threadIdx.x], c);
        if (nan && shift == 24) w[TH_NAN] = 1u;     // every writer stores the same word
        __syncthreads();
    }
}

__global__ __launch_bounds__(64) void th_pick_kernel(unsigned* ws, ThRank r, long long B, int shift) {
    for (long long b = blockIdx.x; b < B; b += gridDim.x) {
        unsigned* w = ws + b * TH_WS_STRIDE;
        unsigned digit, below, count;
        const unsigned k = w[TH_K];
        th_pick(w, k, digit, below, count);
        const int lane = threadIdx.x;
        w[4 * lane] = 0u;
        w[4 * lane + 1] = 0u;
        w[4 * lane + 2] = 0u;
        w[4 * lane + 3] = 0u;
        if (lane == 0) {
            w[TH_PREFIX] |= digit << shift;
            w[TH_K] = k - below;
            if (shift == 0) w[TH_NEED] = r.lo - (k - below) + count <= r.hi ? 1u : 0u;
        }
    }
}

__global__ __launch_bounds__(256) void th_minabove_kernel(const float* __restrict__ x, const float* __restrict__ m, int pred, float sa, float sb,
                                                          unsigned* ws, long long B, long long n, long long head) {
    __shared__ unsigned best_s;
    const long long tid = (long long)blockIdx.x * 256 + threadIdx.x, stride = (long long)gridDim.x * 256;
    for (long long b = blockIdx.y; b < B; b += gridDim.y) {
        unsigned* w = ws + b * TH_WS_STRIDE;
        if (!w[TH_NEED]) continue;                  // uniform over the block
        const unsigned lo_key = w[TH_PREFIX];
        if (threadIdx.x == 0) best_s = 0xffffffffu;
        __syncthreads();
        unsigned best = 0xffffffffu;
        th_row_x0(x ? x + b * n : nullptr, m + b * n, n, head, pred, sa, sb, tid, stride, [&](long long, float v) {
            const unsigned key = th_key(v);
            if (key > lo_key && key < best) best = key;
        });
        if (best != 0xffffffffu) atomicMin(&best_s, best);
        __syncthreads();
        if (threadIdx.x == 0 && best_s != 0xffffffffu) atomicMin(&w[TH_MINABOVE], best_s);
        __syncthreads();
    }
}

__global__ __launch_bounds__(256) void th_stats_kernel(const unsigned* __restrict__ ws, ThRank r, float* __restrict__ stats, long long B) {
    for (long long b = (long long)blockIdx.x * 256 + threadIdx.x; b < B; b += (long long)gridDim.x * 256) {
        const unsigned* w = ws + b * TH_WS_STRIDE;
        float out4[4];
        th_finish(w[TH_PREFIX], w[TH_NEED] ? w[TH_MINABOVE] : w[TH_PREFIX], w[TH_NAN] != 0u, r, out4);
        stats[4 * b] = out4[0];
        stats[4 * b + 1] = out4[1];
        stats[4 * b + 2] = out4[2];
        stats[4 * b + 3] = out4[3];
    }
}

// ---------------------------------------------------------------------------------------------------- the step
// grid (blocks along a row, images), both strided.  `prev` may be `x` (no __restrict__ on either): a lane reads every input of its
// elements before it writes any of them, and no other lane touches them.
__global__ __launch_bounds__(256) void th_step_kernel(const float* x, const float* __restrict__ m, const float* __restrict__ z,
                                                      const float* __restrict__ stats, ThStep p, float* prev, float* __restrict__ x0_out,
                                                      long long B, long long n, long long head) {
    const long long tid = (long long)blockIdx.x * 256 + threadIdx.x, stride = (long long)gridDim.x * 256;
    for (long long b = blockIdx.y; b < B; b += gridDim.y) {
        const float s = p.treat == DP_X0_TREAT_THRESHOLD ? stats[4 * b + 3] : 1.0f;
        th_row_update<false>(p, s, x ? x + b * n : nullptr, m + b * n, z ? z + b * n : nullptr, nullptr, prev + b * n,
                             x0_out ? x0_out + b * n : nullptr, n, head, tid, stride);
    }
}

// ---------------------------------------------------------------------------------------------------- launchers
// The scalar head of every row: dp_ht_head's when n % 4 == 0 (then every row has the phase of the first), else n (all scalar).
static inline long long th_row_head(long long n, const void* const* ptrs, int count) {
    return n % 4 != 0 ? n : dp_ht_head(n, ptrs, count);
}

static inline bool th_rank_ok(long long n, long long lo, long long hi, float w) {
    return lo >= 0 && hi >= lo && hi <= lo + 1 && hi < n && w >= 0.f && w < 1.f;
}

static inline bool th_step_ok(int mode, int pred, int treat) {
    return mode >= DP_X0_MODE_DDIM && mode <= DP_X0_MODE_CONVERT && pred >= DP_X0_PRED_EPSILON && pred <= DP_X0_PRED_V &&
           treat >= DP_X0_TREAT_NONE && treat <= DP_X0_TREAT_THRESHOLD;
}

// blocks along a row (`work` lanes wanted) and images for a strided two-dimensional grid of at most `cap` blocks
static inline dim3 th_grid(long long work, long long B, long long cap) {
    const long long by = B > cap ? cap : B;
    long long bx = (work + 255) / 256;
    const long long room = cap / by;
    if (bx > room) bx = room;
    if (bx < 1) bx = 1;
    return dim3((unsigned)bx, (unsigned)by);
}

extern "C" long long dp_x0_abs_quantile_workspace(long long B, long long n) {
    (void)n;
    return B <= 0 ? 0 : B * TH_WS_STRIDE * (long long)sizeof(unsigned);
}

extern "C" int dp_x0_abs_quantile(const float* x, const float* m, long long B, long long n, int pred, float sa, float sb, long long lo,
                                  long long hi, float w, float max_value, int route, void* ws, float* stats, void* stream) {
    if (B <= 0) return 0;
    if (!m || !stats || n < 1 || n > 0x7fffffffll || pred < DP_X0_PRED_EPSILON || pred > DP_X0_PRED_V) return (int)hipErrorInvalidValue;
    if ((pred != DP_X0_PRED_SAMPLE && !x) || !th_rank_ok(n, lo, hi, w)) return (int)hipErrorInvalidValue;
    if (route == DP_X0_ROUTE_AUTO) route = n <= DP_THRESHOLD_LDS_MAX ? DP_X0_ROUTE_LDS : DP_X0_ROUTE_MULTI;
    if (route != DP_X0_ROUTE_LDS && route != DP_X0_ROUTE_MULTI) return (int)hipErrorInvalidValue;
    if (route == DP_X0_ROUTE_LDS && n > DP_THRESHOLD_LDS_MAX) return (int)hipErrorInvalidValue;
    if (route == DP_X0_ROUTE_MULTI && !ws) return (int)hipErrorInvalidValue;
    if (pred == DP_X0_PRED_SAMPLE) x = nullptr;
    const unsigned long long bytes = 4ull * (unsigned long long)B * (unsigned long long)n, sbytes = 16ull * (unsigned long long)B;
    const unsigned long long wbytes = (unsigned long long)dp_x0_abs_quantile_workspace(B, n);
    if (dp_bytes_overlap(stats, sbytes, x, bytes) || dp_bytes_overlap(stats, sbytes, m, bytes)) return (int)hipErrorInvalidValue;
    if (route == DP_X0_ROUTE_MULTI && (dp_bytes_overlap(ws, wbytes, x, bytes) || dp_bytes_overlap(ws, wbytes, m, bytes) || dp_bytes_overlap(ws, wbytes, stats, sbytes)))
        return (int)hipErrorInvalidValue;
    const void* ptrs[2] = {x, m};
    const long long head = th_row_head(n, ptrs, 2);
    const ThRank r = {(unsigned)lo, (unsigned)hi, w, max_value};
    const hipStream_t st = (hipStream_t)stream;
    if (route == DP_X0_ROUTE_LDS) {
        ThStep p = {};
        p.pred = pred;
        p.c.sa = sa;
        p.c.sb = sb;
        TH_LAUNCH((th_lds_kernel<false>), dim3((unsigned)B), dim3(TH_LDS_THREADS), 0, st, x, m, (const float*)nullptr, p, r, (float*)nullptr,
                  (float*)nullptr, stats, n, head);
        return DP_LAUNCH_CHECK();
    }
    unsigned* w32 = (unsigned*)ws;
    const unsigned per_image = (unsigned)(B > DP_X0_STEP_MAX_BLOCKS ? DP_X0_STEP_MAX_BLOCKS : B);
    const dim3 grid = th_grid((n + 15) / 16, B, DP_X0_STEP_MAX_BLOCKS);          // 16 elements a lane: a block covers 4096 of a row
    TH_LAUNCH(th_init_kernel, dim3(per_image), dim3(256), 0, st, w32, r, B);
    for (int shift = 24; shift >= 0; shift -= 8) {
        TH_LAUNCH(th_hist_kernel, grid, dim3(256), 0, st, x, m, pred, sa, sb, w32, B, n, head, shift);
        TH_LAUNCH(th_pick_kernel, dim3(per_image), dim3(64), 0, st, w32, r, B, shift);
    }
    TH_LAUNCH(th_minabove_kernel, grid, dim3(256), 0, st, x, m, pred, sa, sb, w32, B, n, head);
    TH_LAUNCH(th_stats_kernel, dim3((unsigned)((per_image + 255) / 256)), dim3(256), 0, st, (const unsigned*)w32, r, stats, B);
    return DP_LAUNCH_CHECK();
}

// the checks the step and the fused form share.  stats is an input of the step and an output of the fused form: disjoint from
// everything either way.
static int th_check_step(const float* x, const float* m, const float* z, const float* stats, int mode, int pred, int treat,
                         const dp_x0_coef* coef, const float* prev, const float* x0_out, long long B, long long n, bool* need_x) {
    if (!m || !coef || !prev || n < 1 || !th_step_ok(mode, pred, treat)) return (int)hipErrorInvalidValue;
    *need_x = !(mode == DP_X0_MODE_CONVERT && pred == DP_X0_PRED_SAMPLE);
    if (*need_x && !x) return (int)hipErrorInvalidValue;
    if (treat == DP_X0_TREAT_THRESHOLD && !stats) return (int)hipErrorInvalidValue;
    if (mode == DP_X0_MODE_CONVERT && (z || x0_out)) return (int)hipErrorInvalidValue;
    const unsigned long long bytes = 4ull * (unsigned long long)B * (unsigned long long)n, sbytes = 16ull * (unsigned long long)B;
    // the alias the kernels are written for: prev == x.  Everything else is disjoint.
    if (*need_x && prev != x && dp_bytes_overlap(prev, bytes, x, bytes)) return (int)hipErrorInvalidValue;
    if (dp_bytes_overlap(prev, bytes, m, bytes) || dp_bytes_overlap(prev, bytes, z, bytes) || dp_bytes_overlap(prev, bytes, x0_out, bytes)) return (int)hipErrorInvalidValue;
    if (dp_bytes_overlap(x0_out, bytes, m, bytes) || dp_bytes_overlap(x0_out, bytes, z, bytes)) return (int)hipErrorInvalidValue;
    if (*need_x && dp_bytes_overlap(x0_out, bytes, x, bytes)) return (int)hipErrorInvalidValue;
    if (stats && treat == DP_X0_TREAT_THRESHOLD) {
        if (dp_bytes_overlap(stats, sbytes, prev, bytes) || dp_bytes_overlap(stats, sbytes, x0_out, bytes) || dp_bytes_overlap(stats, sbytes, m, bytes) ||
            dp_bytes_overlap(stats, sbytes, z, bytes) || (*need_x && dp_bytes_overlap(stats, sbytes, x, bytes)))
            return (int)hipErrorInvalidValue;
    }
    return 0;
}

extern "C" int dp_x0_step(const float* x, const float* m, const float* z, const float* stats, int mode, int pred, int treat, int reclip,
                          const dp_x0_coef* coef, float* prev, float* x0_out, long long B, long long n, void* stream) {
    if (B <= 0) return 0;
    bool need_x = true;
    const int bad = th_check_step(x, m, z, stats, mode, pred, treat, coef, prev, x0_out, B, n, &need_x);
    if (bad) return bad;
    if (!need_x) x = nullptr;
    if (treat != DP_X0_TREAT_THRESHOLD) stats = nullptr;
    const void* ptrs[5] = {x, m, z, prev, x0_out};
    const long long head = th_row_head(n, ptrs, 5);
    ThStep p = {mode, pred, treat, reclip ? 1 : 0, *coef};
    TH_LAUNCH(th_step_kernel, th_grid(dp_ht_work(n, head), B, DP_X0_STEP_MAX_BLOCKS), dim3(256), 0, (hipStream_t)stream, x, m, z, stats, p, prev, x0_out, B, n,
              head);
    return DP_LAUNCH_CHECK();
}

extern "C" int dp_x0_threshold_step(const float* x, const float* m, const float* z, int mode, int pred, int reclip, const dp_x0_coef* coef,
                                    long long lo, long long hi, float w, float max_value, float* prev, float* x0_out, float* stats,
                                    long long B, long long n, void* stream) {
    if (B <= 0) return 0;
    bool need_x = true;
    const int bad = th_check_step(x, m, z, stats, mode, pred, DP_X0_TREAT_THRESHOLD, coef, prev, x0_out, B, n, &need_x);
    if (bad) return bad;
    if (n > DP_THRESHOLD_LDS_MAX || !th_rank_ok(n, lo, hi, w)) return (int)hipErrorInvalidValue;
    if (!need_x) x = nullptr;
    const void* ptrs[5] = {x, m, z, prev, x0_out};
    const long long head = th_row_head(n, ptrs, 5);
    ThStep p = {mode, pred, DP_X0_TREAT_THRESHOLD, reclip ? 1 : 0, *coef};
    const ThRank r = {(unsigned)lo, (unsigned)hi, w, max_value};
    TH_LAUNCH((th_lds_kernel<true>), dim3((unsigned)B), dim3(TH_LDS_THREADS), 0, (hipStream_t)stream, x, m, z, p, r, prev, x0_out, stats, n,
              head);
    return DP_LAUNCH_CHECK();
}
