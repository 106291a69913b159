// The data-free magnitude criteria (ddpm_exp/torch_pruning/importance.py:18-126 MagnitudeImportance, :154-219 LAMPImportance) for
// EVERY group of the network in one launch pair.
//   dp_magnitude_rows    per member of every group one row of n0 floats: sum |w|^p over the member's other dimensions for the group's
//                        channels, in the member's index order (with `root`: that sum to the power 1/p = torch.norm(., p), LAMP).  Rows
//                        are kept apart -- the 'max' / 'prod' / 'first' reductions need them.  One pass over every weight (4 bytes per
//                        parameter), no atomics, one fixed summation order per member.
//   dp_magnitude_finish  one workgroup per group: the member reduction over the group's rows in member order, the segment statistics
//                        of the normaliser (sum, min, max, mean, the unbiased standard deviation in two passes around the mean), the
//                        normalisation in place, and for LAMP a descending key-index sort of the group in LDS, the inclusive scan, the
//                        division and the scatter in the vendored or the paper's order.  Output: the concatenated score vector.
#include "dp_common.h"
#include <limits.h>
#include <math.h>

// The launch macro of this file: the body of the library's own (dp_common.h) -- the ring store, the count, the launch -- under a
// name of its own, so that the launch sites of this file are tabled by this file's test module (tests/test_magnitude_family_gpu.py).
#define MG_LAUNCH(k, ...) do { dp_launch_names[dp_launches++ & (DP_LAUNCH_RING - 1)] = #k; hipLaunchKernelGGL(k, __VA_ARGS__); } while (0)

#define MG_MAX_BLOCKS 2097152          // grid-stride beyond
// Widest group dp_magnitude_finish takes.  The LAMP sort holds per channel one 64-bit (key, index) word and one float in LDS:
// 4096 * (8 + 4) = 48 KiB of the 64 KiB a workgroup may declare statically (160 KiB per CU: three groups stay resident).
#define MG_MAX_WIDTH 4096
#define MG_TILE_T 16                   // taps up to which an in-order dim-1 member is read in 256-byte segments (16 KiB of LDS)

extern "C" int dp_magnitude_max_width(void) { return MG_MAX_WIDTH; }

// ------------------------------------------------------------------------------------------------ dp_magnitude_rows
template <int PM>      // 1: |w|, 2: w * w, 0: powf(|w|, p)
static __device__ __forceinline__ float mg_f(float w, float p) {
    if (PM == 1) return fabsf(w);
    if (PM == 2) return w * w;
    return powf(fabsf(w), p);
}

static __device__ __forceinline__ float mg_root(float s, float p, int pm) {
    if (pm == 1) return s;
    if (pm == 2) return sqrtf(s);
    return powf(s, 1.0f / p);
}

// dim-0 member: one wave per channel.  The channel's C * T weights are contiguous; lane l sums elements l, l + 64, ... (as float4
// l, l + 64, ... where the row starts on 16 bytes and its length is a multiple of 4), then the wave folds its 64 partial sums in
// the fixed xor order.  Loads are clamped and unconditional, four in flight per lane.
template <int PM>
static __device__ __forceinline__ float mg_row_sum(const float* __restrict__ wr, long long inner, float p, int lane) {
    float s = 0.f;
    if ((((uintptr_t)wr) & 15) == 0 && (inner & 3) == 0) {
        const long long n4 = inner >> 2;
        const float4* w4 = (const float4*)wr;
        for (long long e0 = lane; e0 < n4; e0 += 256) {
            float4 v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const long long e = e0 + 64 * k;
                v[k] = w4[e < n4 ? e : n4 - 1];
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bool ok = e0 + 64 * k < n4;
                const float a = (mg_f<PM>(v[k].x, p) + mg_f<PM>(v[k].y, p)) + (mg_f<PM>(v[k].z, p) + mg_f<PM>(v[k].w, p));
                s += ok ? a : 0.f;
            }
        }
    } else {
        for (long long e0 = lane; e0 < inner; e0 += 256) {
            float v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const long long e = e0 + 64 * k;
                v[k] = wr[e < inner ? e : inner - 1];
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) s += e0 + 64 * k < inner ? mg_f<PM>(v[k], p) : 0.f;
        }
    }
    return dp_wave_sum(s);
}

// dim-1 member read through an index list (or with more than MG_TILE_T taps): 64 channels per block, lane = channel.  Wave v sums
// rows v, v + 4, ... (all T taps of its channel in each), the four wave sums are added in wave order.  The in-order form, which
// reads whole 256-byte segments, is in the kernel body.
template <int PM>
static __device__ __forceinline__ float mg_col_sum(const float* __restrict__ w, int R, long long CT, int T, long long c, bool live,
                                                   float p, int wave) {
    float s = 0.f;
    const float* wc = w + c * T;
    for (int r0 = wave; r0 < R; r0 += 16) {
        for (int t = 0; t < T; ++t) {
            float v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int r = r0 + 4 * k;
                v[k] = wc[(long long)(r < R ? r : R - 1) * CT + t];
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) s += (live && r0 + 4 * k < R) ? mg_f<PM>(v[k], p) : 0.f;
        }
    }
    return s;
}

// One work unit: 4 channels of a dim-0 member (one per wave) or 64 channels of a dim-1 member.  tab[i].blk0 = first unit of member i
// (ascending, every member has >= 1 unit).  A channel index outside the layer is clamped into it (the host refuses such a list).
template <int PM>
__global__ __launch_bounds__(256) void mg_rows_kernel(const dp_mag_member* __restrict__ tab, int n, long long units,
                                                      const int64_t* __restrict__ idx, float p, int root, float* __restrict__ rows) {
    __shared__ float part[4][64];
    __shared__ float tile[4][64 * MG_TILE_T];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (long long u = blockIdx.x; u < units; u += gridDim.x) {                   // block-uniform
        int lo = 0, hi = n - 1;
        while (lo < hi) {                                                        // last member whose first unit is <= u
            const int mid = (lo + hi + 1) >> 1;
            if ((long long)tab[mid].blk0 <= u) lo = mid; else hi = mid - 1;
        }
        const dp_mag_member m = tab[lo];
        const int blk = (int)(u - m.blk0);
        if (m.dim == 0) {
            const int j = blk * 4 + wave;                                        // wave-uniform
            const int jc = j < m.n0 ? j : m.n0 - 1;
            const long long inner = (long long)m.C * m.T;
            float s = 0.f;
            for (int f = 0; f < m.fold; ++f) {                                   // fold > 1: the channels idx[j * fold ...] in list order
                long long c = m.idx_off >= 0 ? (long long)idx[m.idx_off + (long long)jc * m.fold + f] : jc;
                c = c < 0 ? 0 : c >= m.R ? m.R - 1 : c;
                s += mg_row_sum<PM>(m.w + c * inner, inner, p, lane);
            }
            if (lane == 0 && j < m.n0) rows[m.row_off + j] = root ? mg_root(s, p, PM) : s;
            continue;
        }
        if (m.idx_off < 0 && m.T <= MG_TILE_T) {
            // Channels in order: the 64 * T weights of the block's channels are contiguous in every row.  Wave v sums rows v, v + 4, ...
            // of 64 consecutive floats at a time (one 256-byte segment per load), the four wave sums are added in wave order into a
            // [64 * T] tile, and lane = channel folds its T taps in tap order.
            const long long CT = (long long)m.C * m.T;
            const long long e_base = (long long)blk * 64 * m.T;
            const int j = blk * 64 + lane;
            const int width = ((m.n0 - blk * 64) < 64 ? (m.n0 - blk * 64) : 64) * m.T;      // floats of this block per row
            for (int q = 0; q < m.T; ++q) {
                const int e = q * 64 + lane;
                const long long ec = e_base + (e < width ? e : width - 1);
                float s = 0.f;
                for (int r0 = wave; r0 < m.R; r0 += 16) {
                    float v[4];
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int r = r0 + 4 * k;
                        v[k] = m.w[(long long)(r < m.R ? r : m.R - 1) * CT + ec];
                    }
#pragma unroll
                    for (int k = 0; k < 4; ++k) s += (e < width && r0 + 4 * k < m.R) ? mg_f<PM>(v[k], p) : 0.f;
                }
                tile[wave][e] = s;
            }
            __syncthreads();
            for (int e = tid; e < width; e += 256) tile[0][e] = (tile[0][e] + tile[1][e]) + (tile[2][e] + tile[3][e]);
            __syncthreads();
            if (wave == 0 && j < m.n0) {
                float s = 0.f;
                for (int t = 0; t < m.T; ++t) s += tile[0][lane * m.T + t];
                rows[m.row_off + j] = root ? mg_root(s, p, PM) : s;
            }
            __syncthreads();                                                     // `tile` is written again by the next unit
            continue;
        }
        const int j = blk * 64 + lane;
        const int jc = j < m.n0 ? j : m.n0 - 1;
        float sc = 0.f;
        for (int f = 0; f < m.fold; ++f) {
            long long c = m.idx_off >= 0 ? (long long)idx[m.idx_off + (long long)jc * m.fold + f] : jc;
            c = c < 0 ? 0 : c >= m.C ? m.C - 1 : c;
            sc += mg_col_sum<PM>(m.w, m.R, (long long)m.C * m.T, m.T, c, j < m.n0, p, wave);
        }
        part[wave][lane] = sc;
        __syncthreads();
        if (wave == 0 && j < m.n0) {
            const float s = (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
            rows[m.row_off + j] = root ? mg_root(s, p, PM) : s;
        }
        __syncthreads();                                                         // `part` is written again by the next unit
    }
}

extern "C" int dp_magnitude_rows(dp_mag_member* members, int n, dp_mag_member* table_dev, const int64_t* idx, long long idx_len,
                                 float p, int root, float* rows, long long rows_len, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (n <= 0) return 0;
    if (!members || !table_dev || !rows || !(p > 0.f) || rows_len <= 0) return (int)hipErrorInvalidValue;
    long long units = 0;
    for (int i = 0; i < n; ++i) {
        dp_mag_member& m = members[i];
        if (m.R <= 0 || m.C <= 0 || m.T <= 0 || (m.dim != 0 && m.dim != 1) || m.n0 <= 0 || !m.w) return (int)hipErrorInvalidValue;
        if (m.row_off < 0 || m.row_off + m.n0 > rows_len) return (int)hipErrorInvalidValue;
        if (m.fold < 1 || (m.fold > 1 && m.idx_off < 0)) return (int)hipErrorInvalidValue;
        if (m.idx_off >= 0 ? (!idx || m.idx_off + (long long)m.n0 * m.fold > idx_len) : m.n0 > (m.dim == 0 ? m.R : m.C))
            return (int)hipErrorInvalidValue;
        m.blk0 = (int)units;
        units += m.dim == 0 ? (m.n0 + 3) / 4 : (m.n0 + 63) / 64;
        if (units > INT_MAX) return (int)hipErrorInvalidValue;
    }
    int e = (int)hipMemcpyAsync(table_dev, members, sizeof(dp_mag_member) * (size_t)n, hipMemcpyHostToDevice, st);
    if (e) return e;
    const dim3 grid((unsigned)(units < MG_MAX_BLOCKS ? units : MG_MAX_BLOCKS));
    if (p == 1.f)
        MG_LAUNCH((mg_rows_kernel<1>), grid, dim3(256), 0, st, (const dp_mag_member*)table_dev, n, units, idx, p, root, rows);
    else if (p == 2.f)
        MG_LAUNCH((mg_rows_kernel<2>), grid, dim3(256), 0, st, (const dp_mag_member*)table_dev, n, units, idx, p, root, rows);
    else
        MG_LAUNCH((mg_rows_kernel<0>), grid, dim3(256), 0, st, (const dp_mag_member*)table_dev, n, units, idx, p, root, rows);
    return DP_LAUNCH_CHECK();
}

// ------------------------------------------------------------------------------------------------ dp_magnitude_finish
// torch's min / max return NaN when the segment holds one
static __device__ __forceinline__ float mg_max(float a, float b) { return (a != a || b != b) ? NAN : (a > b ? a : b); }
static __device__ __forceinline__ float mg_min(float a, float b) { return (a != a || b != b) ? NAN : (a < b ? a : b); }

// Block-wide fold for 256 threads in one fixed order: xor butterfly inside the wave, then the four waves as (0 . 1) . (2 . 3).
template <int OP>      // 0 sum, 1 max, 2 min
static __device__ __forceinline__ float mg_block_fold(float v, float* sm) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float t = __shfl_xor(v, o, 64);
        v = OP == 0 ? v + t : OP == 1 ? mg_max(v, t) : mg_min(v, t);
    }
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    if (OP == 0) return (sm[0] + sm[1]) + (sm[2] + sm[3]);
    if (OP == 1) return mg_max(mg_max(sm[0], sm[1]), mg_max(sm[2], sm[3]));
    return mg_min(mg_min(sm[0], sm[1]), mg_min(sm[2], sm[3]));
}

// Order-preserving image of a float (prune_global.hip pg_key): a < b <=> key(a) < key(b); both zeros share the key of +0.0.
static __device__ __forceinline__ unsigned mg_key(float f) {
    unsigned u = __float_as_uint(f);
    if ((u & 0x7fffffffu) == 0u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
static __device__ __forceinline__ float mg_unkey(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// reduction: 0 sum, 1 mean, 2 max, 3 prod, 4 first.  normalizer: 0 none, 1 sum, 2 standarization, 3 mean, 4 max, 5 gaussian.
// lamp: 0 off, 1 the vendored scatter (out[j] = q[a[j]]), 2 the paper's (out[a[k]] = q[k]); a = descending argsort, q = sorted / cumsum.
__global__ __launch_bounds__(256) void mg_finish_kernel(const dp_mag_group* __restrict__ tab, const float* __restrict__ rows,
                                                        int reduction, int normalizer, int lamp, float* __restrict__ scores) {
    __shared__ float s[MG_MAX_WIDTH];
    __shared__ unsigned long long comp[MG_MAX_WIDTH];
    __shared__ float red[4];
    const dp_mag_group g = tab[blockIdx.x];
    const int tid = threadIdx.x, n0 = g.n0, M = g.members;
    const float* r0 = rows + g.row_off;
    for (int j = tid; j < n0; j += 256) {                                        // the member reduction, in member order
        float acc = r0[j];
        if (reduction != 4)
            for (int i = 1; i < M; ++i) {
                const float v = r0[(long long)i * n0 + j];
                acc = reduction == 2 ? mg_max(acc, v) : reduction == 3 ? acc * v : acc + v;
            }
        if (reduction == 1) acc = acc / (float)M;
        s[j] = acc;
    }
    __syncthreads();
    if (normalizer != 0) {
        float sum = 0.f, mx = -INFINITY, mn = INFINITY;
        for (int j = tid; j < n0; j += 256) {
            const float v = s[j];
            sum += v;
            mx = mg_max(mx, v);
            mn = mg_min(mn, v);
        }
        float sub = 0.f, div = 1.f;
        if (normalizer == 1) div = mg_block_fold<0>(sum, red);
        else if (normalizer == 3) div = mg_block_fold<0>(sum, red) / (float)n0;
        else if (normalizer == 4) div = mg_block_fold<1>(mx, red);
        else if (normalizer == 2) {
            mx = mg_block_fold<1>(mx, red);
            sub = mg_block_fold<2>(mn, red);
            div = (mx - sub) + 1e-8f;
        } else {
            sub = mg_block_fold<0>(sum, red) / (float)n0;
            float dm = 0.f;                                                      // the largest |x - mean|: the squares are taken of
            for (int j = tid; j < n0; j += 256) dm = mg_max(dm, fabsf(s[j] - sub));   // (x - mean) / dm, which cannot overflow
            dm = mg_block_fold<1>(dm, red);                                      // (a 'prod' of five members reaches 1e20: its square is inf)
            const float scale = dm > 0.f ? dm : 1.f;
            float sq = 0.f;
            for (int j = tid; j < n0; j += 256) {
                const float d = (s[j] - sub) / scale;
                sq += d * d;
            }
            div = scale * sqrtf(mg_block_fold<0>(sq, red) / (float)(n0 - 1)) + 1e-8f;     // one channel: 0 / 0, as torch.std gives NaN
        }
        __syncthreads();
        for (int j = tid; j < n0; j += 256) s[j] = (s[j] - sub) / div;
        __syncthreads();
    }
    float* out = scores + g.score_off;
    if (lamp == 0) {
        for (int j = tid; j < n0; j += 256) out[j] = s[j];
        return;
    }
    int P = 1;
    while (P < n0) P <<= 1;
    // descending by score, ties by ascending channel: one 64-bit word (key, ~index) sorted descending; the padding (0) sorts last
    for (int j = tid; j < P; j += 256)
        comp[j] = j < n0 ? ((unsigned long long)mg_key(s[j]) << 32) | (unsigned long long)(0xffffffffu - (unsigned)j) : 0ull;
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int h = k >> 1; h > 0; h >>= 1) {
            for (int i = tid; i < P; i += 256) {
                const int o = i ^ h;
                if (o > i) {
                    const unsigned long long a = comp[i], b = comp[o];
                    if ((a < b) == ((i & k) == 0)) { comp[i] = b; comp[o] = a; }
                }
            }
            __syncthreads();
        }
    for (int k = tid; k < n0; k += 256) s[k] = mg_unkey((unsigned)(comp[k] >> 32));      // the sorted scores (a zero as +0.0)
    __syncthreads();
    if (tid == 0) {                                                              // torch.cumsum's order on the host: c[k] = c[k-1] + s[k]
        float c = 0.f;
        for (int k = 0; k < n0; ++k) {
            const float v = s[k];
            c = k == 0 ? v : c + v;
            s[k] = v / c;
        }
    }
    __syncthreads();
    for (int k = tid; k < n0; k += 256) {
        const int a = (int)(0xffffffffu - (unsigned)(comp[k] & 0xffffffffull));
        if (lamp == 1) out[k] = s[a]; else out[a] = s[k];
    }
}

extern "C" int dp_magnitude_finish(const dp_mag_group* groups, int n, dp_mag_group* table_dev, const float* rows, long long rows_len,
                                   int reduction, int normalizer, int lamp, float* scores, long long n_scores, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (n <= 0) return 0;
    if (!groups || !table_dev || !rows || !scores || reduction < 0 || reduction > 4 || normalizer < 0 || normalizer > 5 ||
        lamp < 0 || lamp > 2 || n > MG_MAX_BLOCKS)
        return (int)hipErrorInvalidValue;
    long long next_off = 0;
    for (int i = 0; i < n; ++i) {
        const dp_mag_group& g = groups[i];
        if (g.n0 <= 0 || g.n0 > MG_MAX_WIDTH || g.members <= 0) return (int)hipErrorInvalidValue;      // wider: the caller's torch path
        if (g.row_off < 0 || g.row_off + (long long)g.members * g.n0 > rows_len) return (int)hipErrorInvalidValue;
        if (g.score_off != next_off) return (int)hipErrorInvalidValue;           // the groups tile the score vector in table order
        next_off += g.n0;
    }
    if (next_off != n_scores) return (int)hipErrorInvalidValue;
    int e = (int)hipMemcpyAsync(table_dev, groups, sizeof(dp_mag_group) * (size_t)n, hipMemcpyHostToDevice, st);
    if (e) return e;
    MG_LAUNCH(mg_finish_kernel, dim3((unsigned)n), dim3(256), 0, st, (const dp_mag_group*)table_dev, rows, reduction, normalizer, lamp,
              scores);
    return DP_LAUNCH_CHECK();
}
