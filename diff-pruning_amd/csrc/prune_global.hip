// Global pruning (ddpm_exp/torch_pruning/pruner/algorithms/metapruner.py:256-297): every group of the network is scored on the
// UNPRUNED weights, the scores are concatenated and ONE threshold -- the k-th smallest of all of them -- decides every group's mask.
//   dp_score_groups     the scores of ALL groups in one launch pair.  The member descriptors live in a device-memory table (any
//                       number of members, no 24-member batches by value); per-member arithmetic, work split and member order are
//                       those of dp_group_score (importance.hip), so each group's scores have dp_group_score's bits.  One pass over
//                       every weight and gradient (8 bytes per parameter), no atomics, fixed summation order.
//   dp_select_smallest  the exact k-th smallest of the concatenated scores (radix select over the order-preserving integer image of
//                       the floats, four 8-bit passes, integer counters only) and, per group, the ascending positions with
//                       score <= threshold, compacted on the device; threshold, counts and positions reach the host in one copy.
#include "dp_common.h"
#include <limits.h>

// The launch macro of this file: the body of the library's own (dp_common.h) -- the ring store, the count, the launch -- under a
// name of its own, so that the launch sites of this file are tabled by this file's test module (tests/test_prune_global_gpu.py).
#define PG_LAUNCH(k, ...) do { dp_launch_names[dp_launches++ & (DP_LAUNCH_RING - 1)] = #k; hipLaunchKernelGGL(k, __VA_ARGS__); } while (0)

#define PG_MAX_BLOCKS 2097152          // the cap of the library's other one-block-per-unit launchers; grid-stride beyond

// ------------------------------------------------------------------------------------------------ dp_score_groups
// f(w, g) of dp_wg_reduce (importance.hip wg_f): the same expression, so the compiler contracts it the same way.
static __device__ __forceinline__ float pg_wg_f(float w, float g, int mode) {
    const float p = w * g;
    if (mode == 0) { const float a = fabsf(p); return a * a; }
    if (mode == 1) return fabsf(p);
    if (mode == 4) return g * g;
    return p;
}

// One work unit = one block of group_score_part_kernel: a row of a dim-0 member, 64 (c, t) columns of a dim-1 member, 256
// channels of a GroupNorm member.  tab[i].m.blk0 = first unit of member i (ascending, every member has >= 1 unit).
// Loads are CLAMPED and unconditional (lanes past the end re-read the last element and contribute +0, which leaves the fp32
// partial sum unchanged): four weight and four gradient loads are in flight per thread instead of one dependent pair.
__global__ __launch_bounds__(256) void pg_score_part_kernel(const dp_score_entry* __restrict__ tab, int n, long long units,
                                                            float* __restrict__ scratch) {
    __shared__ float red[4];
    __shared__ float part[4][64];
    const int tid = threadIdx.x;
    for (long long u = blockIdx.x; u < units; u += gridDim.x) {                   // block-uniform
        int lo = 0, hi = n - 1;
        while (lo < hi) {                                                        // last member whose first unit is <= u
            const int mid = (lo + hi + 1) >> 1;
            if ((long long)tab[mid].m.blk0 <= u) lo = mid; else hi = mid - 1;
        }
        const dp_score_member m = tab[lo].m;
        const int blk = (int)(u - m.blk0);
        const int mode = m.mode;
        if (mode == 3) {                                                         // GroupNorm member: |w g| per channel
            const int c = blk * 256 + tid;
            const int cc = c < m.R ? c : m.R - 1;
            const float v = fabsf(m.w[cc] * m.g[cc]);
            if (c < m.R) scratch[m.full_off + c] = v;
            continue;
        }
        if (m.dim == 0) {                                                        // wg_rows_kernel: thread t sums t, t + 256, ...
            const long long inner = (long long)m.C * m.T;
            const float* wr = m.w + (long long)blk * inner;
            const float* gr = m.g + (long long)blk * inner;
            float s = 0.f;
            for (long long e0 = tid; e0 < inner; e0 += 1024) {
                float wv[4], gv[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const long long e = e0 + 256 * k;
                    const long long ec = e < inner ? e : inner - 1;
                    wv[k] = wr[ec];
                    gv[k] = gr[ec];
                }
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const bool ok = e0 + 256 * k < inner;
                    s += pg_wg_f(ok ? wv[k] : 0.f, ok ? gv[k] : 0.f, mode);
                }
            }
            s = dp_block_sum_256(s, red);
            if (tid == 0) scratch[m.full_off + blk] = (mode == 2) ? fabsf(s) : s;
            continue;
        }
        const long long CT = (long long)m.C * m.T;                               // wg_cols_ct_kernel: wave w sums rows w, w + 4, ...
        const int lane = tid & 63;
        const int wave = tid >> 6;
        const long long col = (long long)blk * 64 + lane;
        const long long colc = col < CT ? col : CT - 1;
        float s = 0.f;
        for (int r0 = wave; r0 < m.R; r0 += 16) {
            float wv[4], gv[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int r = r0 + 4 * k;
                const long long o = (long long)(r < m.R ? r : m.R - 1) * CT + colc;
                wv[k] = m.w[o];
                gv[k] = m.g[o];
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bool ok = r0 + 4 * k < m.R && col < CT;
                s += pg_wg_f(ok ? wv[k] : 0.f, ok ? gv[k] : 0.f, mode);
            }
        }
        part[wave][lane] = s;
        __syncthreads();
        if (wave == 0 && col < CT) scratch[m.col_off + col] = (part[0][lane] + part[1][lane]) + (part[2][lane] + part[3][lane]);
        __syncthreads();                                                         // `part` is written again by the next unit
    }
}

// scores[score_off + j] = ((0 + m_1[j]) + m_2[j]) + ... over the members of the group, in table order
// (group_score_combine_kernel; a group's members are adjacent in the table and share score_off / n0).
__global__ __launch_bounds__(256) void pg_score_combine_kernel(const dp_score_entry* __restrict__ tab, int n,
                                                               const float* __restrict__ scratch, const int64_t* __restrict__ idx,
                                                               long long total, float* __restrict__ scores) {
    const long long step = (long long)gridDim.x * 256;
    for (long long p = (long long)blockIdx.x * 256 + threadIdx.x; p < total; p += step) {
        int lo = 0, hi = n - 1;
        while (lo < hi) {                                                        // first member whose group's range ends after p
            const int mid = (lo + hi) >> 1;
            if (tab[mid].score_off + tab[mid].n0 > p) hi = mid; else lo = mid + 1;
        }
        const long long off = tab[lo].score_off;
        const long long j = p - off;
        float acc = 0.f;
        for (int i = lo; i < n && tab[i].score_off == off; ++i) {
            const dp_score_member m = tab[i].m;
            const long long c = m.idx_off >= 0 ? (long long)idx[m.idx_off + j] : j;
            float v;
            if (m.mode != 3 && m.dim == 1) {                                     // wg_fold_taps_kernel
                float s = 0.f;
                for (int t = 0; t < m.T; ++t) s += scratch[m.col_off + c * m.T + t];
                v = (m.mode == 2) ? fabsf(s) : s;
            } else {
                v = scratch[m.full_off + c];
            }
            acc = acc + v;
        }
        scores[p] = acc;
    }
}

extern "C" int dp_score_groups(dp_score_entry* entries, int n, dp_score_entry* table_dev, const int64_t* idx, long long idx_len,
                               float* scratch, long long scratch_len, float* scores, long long n_scores, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (n <= 0 || n_scores <= 0) return 0;
    if (!entries || !table_dev || !scratch || !scores) return (int)hipErrorInvalidValue;
    long long units = 0, next_off = 0;
    for (int i = 0; i < n; ++i) {
        dp_score_entry& e = entries[i];
        dp_score_member& m = e.m;
        if (m.R <= 0 || m.C <= 0 || m.T <= 0 || (m.dim != 0 && m.dim != 1) || m.mode < 0 || m.mode > 5 || e.n0 <= 0 || !m.w || !m.g)
            return (int)hipErrorInvalidValue;
        const bool cols = m.mode != 3 && m.dim == 1;
        const long long n_full = cols ? m.C : m.R;
        const long long CT = (long long)m.C * m.T;
        if (m.mode == 3 && (m.C != 1 || m.T != 1)) return (int)hipErrorInvalidValue;
        if (cols ? (m.col_off < 0 || m.col_off + CT > scratch_len) : (m.full_off < 0 || m.full_off + n_full > scratch_len))
            return (int)hipErrorInvalidValue;
        if (m.idx_off >= 0 ? (!idx || m.idx_off + e.n0 > idx_len) : e.n0 > n_full) return (int)hipErrorInvalidValue;
        // groups tile the score vector in table order: a member either continues its predecessor's group or opens the next one
        const bool same = i > 0 && e.score_off == entries[i - 1].score_off && e.n0 == entries[i - 1].n0;
        if (!same) {
            if (e.score_off != next_off) return (int)hipErrorInvalidValue;
            next_off = e.score_off + e.n0;
        }
        m.blk0 = (int)units;
        units += m.mode == 3 ? (m.R + 255) / 256 : m.dim == 0 ? m.R : (CT + 63) / 64;
        if (units > INT_MAX) return (int)hipErrorInvalidValue;
    }
    if (next_off != n_scores) return (int)hipErrorInvalidValue;
    int e = (int)hipMemcpyAsync(table_dev, entries, sizeof(dp_score_entry) * (size_t)n, hipMemcpyHostToDevice, st);
    if (e) return e;
    const long long cb = (n_scores + 255) / 256;
    PG_LAUNCH(pg_score_part_kernel, dim3((unsigned)(units < PG_MAX_BLOCKS ? units : PG_MAX_BLOCKS)), dim3(256), 0, st,
              (const dp_score_entry*)table_dev, n, units, scratch);
    PG_LAUNCH(pg_score_combine_kernel, dim3((unsigned)(cb < PG_MAX_BLOCKS ? cb : PG_MAX_BLOCKS)), dim3(256), 0, st,
              (const dp_score_entry*)table_dev, n, (const float*)scratch, idx, n_scores, scores);
    return DP_LAUNCH_CHECK();
}

// ------------------------------------------------------------------------------------------------ dp_select_smallest
#define PG_HIST_BLOCKS 1024            // upper bound of the histogram grid (grid-stride beyond)
#define PG_HIST_ROW 257                // 256 digit counters + the block's NaN count
#define PG_CHUNK 2048                  // elements per compaction chunk: 256 threads x 8 consecutive elements
#define PG_CHUNK_BLOCKS 65536

// Order-preserving image of a float: a < b  <=>  key(a) < key(b) (unsigned); -0.0 is counted as +0.0, as torch compares them.
// Integer operations only (denormals included, whatever the float mode), and every later comparison is made on the keys.
static __device__ __forceinline__ unsigned pg_key(float f) {
    unsigned u = __float_as_uint(f);
    if ((u & 0x7fffffffu) == 0u) u = 0u;
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
static __device__ __forceinline__ bool pg_is_nan(float f) { return (__float_as_uint(f) & 0x7fffffffu) > 0x7f800000u; }
static __device__ __forceinline__ float pg_unkey(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// state[0] = key prefix found so far, state[1] = rank still looked for among the keys that share it (1-based),
// state[2] = NaN count (saturated), state[3] = number of positions with score <= threshold
__global__ void pg_sel_init_kernel(unsigned* __restrict__ state, unsigned k) {
    if (threadIdx.x == 0) { state[0] = 0u; state[1] = k; state[2] = 0u; state[3] = 0u; }
}

// pass `shift` (24, 16, 8, 0): digit histogram of the keys whose higher bits equal the prefix; one row per block, no global atomics
__global__ __launch_bounds__(256) void pg_sel_hist_kernel(const float* __restrict__ x, long long n, const unsigned* __restrict__ state,
                                                          int shift, unsigned* __restrict__ partial) {
    __shared__ unsigned h[PG_HIST_ROW];
    for (int i = threadIdx.x; i < PG_HIST_ROW; i += 256) h[i] = 0u;
    __syncthreads();
    const unsigned prefix = state[0];
    const unsigned himask = shift == 24 ? 0u : ~0u << (shift + 8);
    const long long step = (long long)gridDim.x * 256;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < n; i += step) {
        const float f = x[i];
        if (pg_is_nan(f)) { atomicAdd(&h[256], 1u); continue; }                        // integer LDS counters: order-independent
        const unsigned key = pg_key(f);
        if ((key & himask) == (prefix & himask)) atomicAdd(&h[(key >> shift) & 255u], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < PG_HIST_ROW; i += 256) partial[(long long)blockIdx.x * PG_HIST_ROW + i] = h[i];
}

// one block: add the rows, find the digit that holds the wanted rank, extend the prefix
__global__ __launch_bounds__(256) void pg_sel_pick_kernel(const unsigned* __restrict__ partial, int rows, int shift,
                                                          unsigned* __restrict__ state, int* __restrict__ out) {
    __shared__ unsigned h[256];
    unsigned s = 0u;
    for (int b = 0; b < rows; ++b) s += partial[(long long)b * PG_HIST_ROW + threadIdx.x];
    h[threadIdx.x] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned nan = 0u;
        for (int b = 0; b < rows; ++b) { const unsigned v = partial[(long long)b * PG_HIST_ROW + 256]; nan = nan + v < nan ? ~0u : nan + v; }
        unsigned want = state[1], d = 0u;
        while (d < 255u && h[d] < want) { want -= h[d]; ++d; }
        const unsigned prefix = state[0] | (d << shift);
        state[0] = prefix;
        state[1] = want;
        if (shift == 24) state[2] = nan;
        if (shift == 0) {
            out[0] = (int)__float_as_uint(pg_unkey(prefix));
            out[1] = (int)(state[2] > (unsigned)INT_MAX ? (unsigned)INT_MAX : state[2]);
        }
    }
}

// chunk_count[c] = number of positions of chunk c with score <= threshold
__global__ __launch_bounds__(256) void pg_sel_count_kernel(const float* __restrict__ x, long long n, const unsigned* __restrict__ state,
                                                           long long chunks, unsigned* __restrict__ chunk_count) {
    __shared__ unsigned red[4];
    const unsigned thres = state[0];                                             // the key of the k-th smallest
    for (long long c = blockIdx.x; c < chunks; c += gridDim.x) {
        const long long base = c * PG_CHUNK + (long long)threadIdx.x * 8;
        unsigned cnt = 0u;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const long long i = base + k;
            const float f = x[i < n ? i : n - 1];
            cnt += (i < n && !pg_is_nan(f) && pg_key(f) <= thres) ? 1u : 0u;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o, 64);
        __syncthreads();
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = cnt;
        __syncthreads();
        if (threadIdx.x == 0) chunk_count[c] = red[0] + red[1] + red[2] + red[3];
    }
}

// one block: chunk_base[c] = sum of chunk_count[0 .. c) (exclusive), state[3] = the total
__global__ __launch_bounds__(256) void pg_sel_scan_kernel(const unsigned* __restrict__ chunk_count, long long chunks,
                                                          unsigned* __restrict__ chunk_base, unsigned* __restrict__ state) {
    __shared__ unsigned sm[256];
    __shared__ unsigned carry;
    if (threadIdx.x == 0) carry = 0u;
    __syncthreads();
    for (long long c0 = 0; c0 < chunks; c0 += 256) {
        const long long c = c0 + threadIdx.x;
        const unsigned v = c < chunks ? chunk_count[c] : 0u;
        sm[threadIdx.x] = v;
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {                                      // inclusive scan of the strip
            const unsigned a = threadIdx.x >= o ? sm[threadIdx.x - o] : 0u;
            __syncthreads();
            sm[threadIdx.x] += a;
            __syncthreads();
        }
        if (c < chunks) chunk_base[c] = carry + sm[threadIdx.x] - v;
        __syncthreads();
        if (threadIdx.x == 255) carry += sm[255];
        __syncthreads();
    }
    if (threadIdx.x == 0) state[3] = carry;
}

// sel[r] = the r-th position (ascending) with score <= threshold; fstart[g] = how many such positions lie before group g
__global__ __launch_bounds__(256) void pg_sel_compact_kernel(const float* __restrict__ x, long long n,
                                                             long long chunks, const unsigned* __restrict__ chunk_base,
                                                             const long long* __restrict__ goff, int G, const unsigned* __restrict__ state,
                                                             int* __restrict__ sel, unsigned* __restrict__ fstart) {
    __shared__ unsigned sm[256];
    const unsigned thres = state[0];
    if (blockIdx.x == 0 && threadIdx.x == 0) fstart[G] = state[3];
    for (long long c = blockIdx.x; c < chunks; c += gridDim.x) {
        const long long base = c * PG_CHUNK + (long long)threadIdx.x * 8;
        unsigned flags = 0u, cnt = 0u;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const long long i = base + k;
            const float f = x[i < n ? i : n - 1];
            if (i < n && !pg_is_nan(f) && pg_key(f) <= thres) { flags |= 1u << k; ++cnt; }
        }
        sm[threadIdx.x] = cnt;
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {
            const unsigned a = threadIdx.x >= o ? sm[threadIdx.x - o] : 0u;
            __syncthreads();
            sm[threadIdx.x] += a;
            __syncthreads();
        }
        unsigned r = chunk_base[c] + sm[threadIdx.x] - cnt;                       // positions with score <= threshold before `base`
        __syncthreads();                                                         // `sm` is written again by the next chunk
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const long long i = base + k;
            if (i >= n) break;
            int lo = 0, hi = G - 1;                                              // is i the first position of a group?
            while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (goff[mid] <= i) lo = mid; else hi = mid - 1; }
            if (goff[lo] == i) fstart[lo] = r;
            if (flags & (1u << k)) { sel[r] = (int)i; ++r; }
        }
    }
}

// out[2 + g] = count of group g; out[2 + G + goff[g] + j] = the j-th selected position of group g, relative to the group
__global__ __launch_bounds__(256) void pg_sel_scatter_kernel(const int* __restrict__ sel, const unsigned* __restrict__ fstart,
                                                             const long long* __restrict__ goff, int G, int* __restrict__ out) {
    const long long total = fstart[G];
    const long long step = (long long)gridDim.x * 256;
    for (long long r = (long long)blockIdx.x * 256 + threadIdx.x; r < total; r += step) {
        const long long i = sel[r];
        int lo = 0, hi = G - 1;
        while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (goff[mid] <= i) lo = mid; else hi = mid - 1; }
        out[2 + (long long)G + goff[lo] + (r - fstart[lo])] = (int)(i - goff[lo]);
    }
    for (long long g = (long long)blockIdx.x * 256 + threadIdx.x; g < G; g += step) out[2 + g] = (int)(fstart[g + 1] - fstart[g]);
}

static inline long long pg_align(long long b) { return (b + 255) / 256 * 256; }
static inline long long pg_hist_rows(long long n) {
    const long long nb = (n + 2047) / 2048;
    return nb < 1 ? 1 : nb > PG_HIST_BLOCKS ? PG_HIST_BLOCKS : nb;
}

// device workspace, in bytes: state | histogram rows | chunk counts | chunk bases | selected positions | group starts | group offsets
extern "C" long long dp_select_smallest_workspace(long long n, int groups) {
    if (n < 1 || groups < 1) return 0;
    const long long chunks = (n + PG_CHUNK - 1) / PG_CHUNK;
    return pg_align(16) + pg_align(pg_hist_rows(n) * PG_HIST_ROW * 4) + 2 * pg_align(chunks * 4) + pg_align(n * 4) +
           pg_align(((long long)groups + 1) * 4) + pg_align(((long long)groups + 1) * 8);
}

extern "C" int dp_select_smallest(const float* scores, long long n, const long long* group_off, int groups, long long k, void* work,
                                  long long work_bytes, int* out_dev, int* out_host, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (!scores || !group_off || !work || !out_dev || !out_host || n < 1 || n > INT_MAX || groups < 1 || k < 1 || k > n)
        return (int)hipErrorInvalidValue;
    if (group_off[0] != 0 || group_off[groups] != n || work_bytes < dp_select_smallest_workspace(n, groups))
        return (int)hipErrorInvalidValue;
    for (int g = 0; g < groups; ++g)
        if (group_off[g + 1] <= group_off[g]) return (int)hipErrorInvalidValue;
    const long long chunks = (n + PG_CHUNK - 1) / PG_CHUNK;
    const int rows = (int)pg_hist_rows(n);
    char* p = (char*)work;
    unsigned* state = (unsigned*)p;            p += pg_align(16);
    unsigned* partial = (unsigned*)p;          p += pg_align((long long)rows * PG_HIST_ROW * 4);
    unsigned* chunk_count = (unsigned*)p;      p += pg_align(chunks * 4);
    unsigned* chunk_base = (unsigned*)p;       p += pg_align(chunks * 4);
    int* sel = (int*)p;                        p += pg_align(n * 4);
    unsigned* fstart = (unsigned*)p;           p += pg_align(((long long)groups + 1) * 4);
    long long* goff = (long long*)p;
    const size_t out_bytes = sizeof(int) * (size_t)(2 + groups + n);
    int e = (int)hipMemcpyAsync(goff, group_off, sizeof(long long) * ((size_t)groups + 1), hipMemcpyHostToDevice, st);
    if (e) return e;
    e = (int)hipMemsetAsync(out_dev, 0, out_bytes, st);
    if (e) return e;
    PG_LAUNCH(pg_sel_init_kernel, dim3(1), dim3(64), 0, st, state, (unsigned)k);
    for (int shift = 24; shift >= 0; shift -= 8) {
        PG_LAUNCH(pg_sel_hist_kernel, dim3(rows), dim3(256), 0, st, scores, n, (const unsigned*)state, shift, partial);
        PG_LAUNCH(pg_sel_pick_kernel, dim3(1), dim3(256), 0, st, (const unsigned*)partial, rows, shift, state, out_dev);
    }
    const unsigned cgrid = (unsigned)(chunks < PG_CHUNK_BLOCKS ? chunks : PG_CHUNK_BLOCKS);
    PG_LAUNCH(pg_sel_count_kernel, dim3(cgrid), dim3(256), 0, st, scores, n, (const unsigned*)state, chunks, chunk_count);
    PG_LAUNCH(pg_sel_scan_kernel, dim3(1), dim3(256), 0, st, (const unsigned*)chunk_count, chunks, chunk_base, state);
    PG_LAUNCH(pg_sel_compact_kernel, dim3(cgrid), dim3(256), 0, st, scores, n, chunks, (const unsigned*)chunk_base,
              (const long long*)goff, groups, (const unsigned*)state, sel, fstart);
    const long long sb = (n + 255) / 256;
    PG_LAUNCH(pg_sel_scatter_kernel, dim3((unsigned)(sb < 4096 ? sb : 4096)), dim3(256), 0, st, (const int*)sel, (const unsigned*)fstart,
              (const long long*)goff, groups, out_dev);
    e = DP_LAUNCH_CHECK();
    if (e) return e;
    e = (int)hipMemcpyAsync(out_host, out_dev, out_bytes, hipMemcpyDeviceToHost, st);
    if (e) return e;
    e = (int)hipStreamSynchronize(st);
    if (e) return e;
    return out_host[1] != 0 ? (int)hipErrorInvalidValue : 0;                     // a NaN has no rank: the call is refused
}
