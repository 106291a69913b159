// Reductions behind the evaluation job's Inception Score, KID and precision / recall (metrics.py: knn_radii2, inside_manifold,
// kernel_inception_distance, inception_score).  The N x N products come from dp_nt_gemm in blocks (ops.bmm_nt: G = X . Y^T); the
// kernels here turn a Gram block into the quantity wanted without ever holding more than that block:
//   em_row_norms2_kernel     |x_i|^2 per row, in double
//   em_knn_merge_kernel<K>   the K smallest squared distances per row, merged over column blocks
//   em_inside_ball_kernel    hit_i |= any_j (d2_ij <= r2_j)
//   em_poly_part_kernel / em_poly_final_kernel     sum (gamma g + c0)^degree and its diagonal, in double, two stages; g itself the
//                            double sum of fp32 partial Gram slabs
//   em_isc_rows_kernel       log-sum-exp and sum_c p (l - lse) per row of the logits, in double
//   em_isc_colmeans_kernel   q_c = mean_i exp(l_ic - lse_i) over a row range, in double
// d2_ij = max(xn_i + yn_j - 2 G_ij, 0) is formed in double from double norms and rounded to fp32 once: the only fp32 error
// in it is the Gram element's.  No atomics anywhere; every sum has a fixed order, so two calls give the same bits.
#include "dp_common.h"
#include <math.h>

// The launch macro of this file: the body of the library's own (dp_common.h) -- the ring store, the count, the launch -- under a
// name of its own, so that the launch sites of this file are tabled by this file's test module
// (tests/test_eval_metrics_gpu.py: BRANCHES / LAUNCH_SITES / CASES).
#define EM_LAUNCH(k, ...) do { dp_launch_names[dp_launches++ & (DP_LAUNCH_RING - 1)] = #k; hipLaunchKernelGGL(k, __VA_ARGS__); } while (0)

#define EM_ROWS_PER_BLOCK 4          // 256 threads: one wavefront per row
#define EM_MAX_BLOCKS 65536

__device__ __forceinline__ double em_wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

__device__ __forceinline__ float em_wave_min(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
    return v;
}

// Sum over the 256 threads of a block in a fixed order; `sm` holds >= 4 doubles.  Every thread gets the result.
__device__ __forceinline__ double em_block_sum_d(double v, double* sm) {
    v = em_wave_sum_d(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    return (sm[0] + sm[1]) + (sm[2] + sm[3]);
}

__device__ __forceinline__ float em_dist2(double xn, double yn, float g) { return (float)fmax(xn + yn - 2.0 * (double)g, 0.0); }

// Elements in front of the first 16-byte aligned one of a row (at most `cols`).
__device__ __forceinline__ long long em_head(const float* g, long long cols) {
    const long long h = (long long)(((16u - (unsigned)((uintptr_t)g & 15u)) & 15u) >> 2);
    return h < cols ? h : cols;
}

// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void em_row_norms2_kernel(const float* __restrict__ x, long long n, int d, long long ld,
                                                            double* __restrict__ out) {
    const int lane = threadIdx.x & 63;
    for (long long row = (long long)blockIdx.x * EM_ROWS_PER_BLOCK + (threadIdx.x >> 6); row < n;
         row += (long long)gridDim.x * EM_ROWS_PER_BLOCK) {
        const float* p = x + row * ld;
        double s = 0.0;
        for (int i = lane; i < d; i += 64) { const double v = (double)p[i]; s += v * v; }
        s = em_wave_sum_d(s);
        if (lane == 0) out[row] = s;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// One wavefront per row.  Every lane keeps the K smallest values it has seen, ascending, in K registers (an unrolled
// compare-swap chain: no indexed register array, no scratch); then K rounds of a wave minimum over the lanes' heads, in each of
// which the lowest lane holding the minimum drops its head.
template <int K>
__device__ __forceinline__ void em_insert(float (&b)[K], float v) {
#pragma unroll
    for (int i = 0; i < K; ++i) {
        const float lo = fminf(b[i], v), hi = fmaxf(b[i], v);
        b[i] = lo;
        v = hi;
    }
}

template <int K>
__global__ __launch_bounds__(256) void em_knn_merge_kernel(const float* __restrict__ G, long long rows, long long cols, long long ldg,
                                                           const double* __restrict__ xn, const double* __restrict__ yn, int first,
                                                           float* __restrict__ best) {
    const int lane = threadIdx.x & 63;
    for (long long row = (long long)blockIdx.x * EM_ROWS_PER_BLOCK + (threadIdx.x >> 6); row < rows;
         row += (long long)gridDim.x * EM_ROWS_PER_BLOCK) {
        const float* g = G + row * ldg;
        const double x2 = xn[row];
        float b[K];
#pragma unroll
        for (int i = 0; i < K; ++i) b[i] = INFINITY;
        if (!first && lane < K) em_insert<K>(b, best[row * K + lane]);
        const long long head = em_head(g, cols);
        const long long nvec = (cols - head) >> 2;
        if (lane < head) em_insert<K>(b, em_dist2(x2, yn[lane], g[lane]));
        const f32x4* gv = reinterpret_cast<const f32x4*>(g + head);
        for (long long v = lane; v < nvec; v += 64) {
            const f32x4 q = gv[v];
            const double* y = yn + head + 4 * v;
            em_insert<K>(b, em_dist2(x2, y[0], q.x));
            em_insert<K>(b, em_dist2(x2, y[1], q.y));
            em_insert<K>(b, em_dist2(x2, y[2], q.z));
            em_insert<K>(b, em_dist2(x2, y[3], q.w));
        }
        const long long t = head + 4 * nvec + lane;
        if (t < cols) em_insert<K>(b, em_dist2(x2, yn[t], g[t]));
#pragma unroll
        for (int r = 0; r < K; ++r) {
            const float m = em_wave_min(b[0]);
            const unsigned long long owners = __ballot(b[0] == m);
            if (lane == (int)__builtin_ctzll(owners | (1ull << 63))) {
#pragma unroll
                for (int i = 0; i + 1 < K; ++i) b[i] = b[i + 1];
                b[K - 1] = INFINITY;
            }
            if (lane == 0) best[row * K + r] = m;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// One wavefront per row; a row that is already inside a ball is skipped, and the row's loop ends at the first 64-lane step in
// which some lane found one (the flag is the same whichever lane finds it).
__global__ __launch_bounds__(256) void em_inside_ball_kernel(const float* __restrict__ G, long long rows, long long cols, long long ldg,
                                                             const double* __restrict__ xn, const double* __restrict__ yn,
                                                             const float* __restrict__ r2, int* __restrict__ hit) {
    const int lane = threadIdx.x & 63;
    for (long long row = (long long)blockIdx.x * EM_ROWS_PER_BLOCK + (threadIdx.x >> 6); row < rows;
         row += (long long)gridDim.x * EM_ROWS_PER_BLOCK) {
        if (hit[row]) continue;
        const float* g = G + row * ldg;
        const double x2 = xn[row];
        const long long head = em_head(g, cols);
        const long long nvec = (cols - head) >> 2;
        bool in = false;
        if (lane < head) in = em_dist2(x2, yn[lane], g[lane]) <= r2[lane];
        const long long t = head + 4 * nvec + lane;
        if (t < cols) in = in || em_dist2(x2, yn[t], g[t]) <= r2[t];
        bool any = __ballot(in) != 0ull;
        const f32x4* gv = reinterpret_cast<const f32x4*>(g + head);
        // four 16-byte loads per lane in flight per step (index clamped instead of a load under an `if`: the loads are issued
        // together), one ballot per step
        for (long long v0 = 0; v0 < nvec && !any; v0 += 4 * 64) {
            f32x4 q[4];
            long long vi[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const long long v = v0 + u * 64 + lane;
                vi[u] = v < nvec ? v : nvec - 1;
                q[u] = gv[vi[u]];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const double* y = yn + head + 4 * vi[u];
                const float* r = r2 + head + 4 * vi[u];
                const double y0 = y[0], y1 = y[1], y2 = y[2], y3 = y[3];
                const float r0 = r[0], r1 = r[1], r2v = r[2], r3 = r[3];
                // `|`, not `||`: a short-circuit would put each later load behind a branch on the earlier comparison
                in = in | (em_dist2(x2, y0, q[u].x) <= r0) | (em_dist2(x2, y1, q[u].y) <= r1) | (em_dist2(x2, y2, q[u].z) <= r2v) |
                     (em_dist2(x2, y3, q[u].w) <= r3);
            }
            any = __ballot(in) != 0ull;
        }
        if (lane == 0 && any) hit[row] = 1;
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// The Gram element is the double sum of `slabs` fp32 partial products G[s][row][col] (slab stride `slab` floats), in slab order: the
// caller splits the feature dimension, because dp_nt_gemm's element is one k-ordered fp32 fma chain whose rounding error grows with
// its length (for the all-positive pool3 features, linearly in the partial sum) and the cube triples it.
// Stage 1: block b sums rows b, b + gridDim.x, ... of (gamma g + c0)^degree in double (thread-strided over the row, then the block's
// fixed-order sum) -> part[b], and the elements with row == column -> part[gridDim.x + b].  Stage 2: one block adds the partials.
__global__ __launch_bounds__(256) void em_poly_part_kernel(const float* __restrict__ G, int slabs, long long slab, long long rows,
                                                           long long cols, long long ldg, double gamma, double coef0, int degree,
                                                           double* __restrict__ part) {
    __shared__ double sm[4];
    double s = 0.0, dg = 0.0;
    for (long long row = blockIdx.x; row < rows; row += gridDim.x) {
        const float* g = G + row * ldg;
        for (long long j = threadIdx.x; j < cols; j += 256) {
            double e = (double)g[j];
            for (int z = 1; z < slabs; ++z) e += (double)g[z * slab + j];
            const double v = gamma * e + coef0;
            double p = v;
            for (int q = 1; q < degree; ++q) p *= v;
            s += p;
            if (j == row) dg += p;
        }
    }
    s = em_block_sum_d(s, sm);
    dg = em_block_sum_d(dg, sm);
    if (threadIdx.x == 0) { part[blockIdx.x] = s; part[gridDim.x + blockIdx.x] = dg; }
}

__global__ __launch_bounds__(256) void em_poly_final_kernel(const double* __restrict__ part, int nblocks, double* __restrict__ out) {
    __shared__ double sm[4];
    double s = 0.0, dg = 0.0;
    for (int i = threadIdx.x; i < nblocks; i += 256) { s += part[i]; dg += part[nblocks + i]; }
    s = em_block_sum_d(s, sm);
    dg = em_block_sum_d(dg, sm);
    if (threadIdx.x == 0) { out[0] = s; out[1] = dg; }
}

// ---------------------------------------------------------------------------------------------------------------------
// One wavefront per row of the logits: m = max, s = sum exp(l - m), t = sum exp(l - m) (l - m), all in double;
// lse = m + log s and h = sum_c p_c (l_c - lse) = t / s - log s.
__global__ __launch_bounds__(256) void em_isc_rows_kernel(const float* __restrict__ logits, long long n, int c, long long ld,
                                                          double* __restrict__ lse, double* __restrict__ h) {
    const int lane = threadIdx.x & 63;
    for (long long row = (long long)blockIdx.x * EM_ROWS_PER_BLOCK + (threadIdx.x >> 6); row < n;
         row += (long long)gridDim.x * EM_ROWS_PER_BLOCK) {
        const float* p = logits + row * ld;
        float mx = -INFINITY;
        for (int i = lane; i < c; i += 64) mx = fmaxf(mx, p[i]);
        const double m = (double)dp_wave_max(mx);
        double s = 0.0, t = 0.0;
        for (int i = lane; i < c; i += 64) {
            const double z = (double)p[i] - m, e = exp(z);
            s += e;
            t += e * z;
        }
        s = em_wave_sum_d(s);
        t = em_wave_sum_d(t);
        if (lane == 0) {
            const double ls = log(s);
            lse[row] = m + ls;
            h[row] = t / s - ls;
        }
    }
}

// q[c] = mean over rows [lo, hi) of exp(l_rc - lse_r).  A block owns 32 columns; its 8 row lanes each add rows lo + ry, lo + ry + 8, ...
// in order, and the 8 sums are added in a fixed tree.
__global__ __launch_bounds__(256) void em_isc_colmeans_kernel(const float* __restrict__ logits, long long ld, const double* __restrict__ lse,
                                                              long long lo, long long hi, int c, double* __restrict__ q) {
    __shared__ double sm[8][33];
    const int cx = threadIdx.x & 31, ry = threadIdx.x >> 5;
    const int col = blockIdx.x * 32 + cx;
    double s = 0.0;
    if (col < c)
        for (long long r = lo + ry; r < hi; r += 8) s += exp((double)logits[r * ld + col] - lse[r]);
    sm[ry][cx] = s;
    __syncthreads();
    if (ry == 0 && col < c) {
        const double a = (sm[0][cx] + sm[1][cx]) + (sm[2][cx] + sm[3][cx]), b = (sm[4][cx] + sm[5][cx]) + (sm[6][cx] + sm[7][cx]);
        q[col] = (a + b) / (double)(hi - lo);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
static inline unsigned em_row_grid(long long rows) {
    const long long nb = (rows + EM_ROWS_PER_BLOCK - 1) / EM_ROWS_PER_BLOCK;
    return (unsigned)(nb > EM_MAX_BLOCKS ? EM_MAX_BLOCKS : nb);
}

extern "C" int dp_em_row_norms2(const float* x, long long n, int d, long long ld, double* out, void* stream) {
    if (n <= 0) return 0;
    if (d < 0 || ld < d) return (int)hipErrorInvalidValue;
    EM_LAUNCH(em_row_norms2_kernel, dim3(em_row_grid(n)), dim3(256), 0, (hipStream_t)stream, x, n, d, ld, out);
    return DP_LAUNCH_CHECK();
}

#define EM_KNN_CASE(K) case K: EM_LAUNCH(em_knn_merge_kernel<K>, dim3(em_row_grid(rows)), dim3(256), 0, (hipStream_t)stream, G, rows, cols, ldg, xn, yn, first, best); break;
extern "C" int dp_em_knn_merge(const float* G, long long rows, long long cols, long long ldg, const double* xn, const double* yn, int k,
                               int first, float* best, void* stream) {
    if (k < 1 || k > DP_EM_MAX_K) return (int)hipErrorNotSupported;
    if (cols < 0 || ldg < cols) return (int)hipErrorInvalidValue;
    if (rows <= 0) return 0;
    switch (k) {
        EM_KNN_CASE(1) EM_KNN_CASE(2) EM_KNN_CASE(3) EM_KNN_CASE(4) EM_KNN_CASE(5) EM_KNN_CASE(6) EM_KNN_CASE(7) EM_KNN_CASE(8) EM_KNN_CASE(9)
    }
    return DP_LAUNCH_CHECK();
}

extern "C" int dp_em_inside_ball(const float* G, long long rows, long long cols, long long ldg, const double* xn, const double* yn,
                                 const float* r2, int* hit, void* stream) {
    if (cols < 0 || ldg < cols) return (int)hipErrorInvalidValue;
    if (rows <= 0) return 0;
    EM_LAUNCH(em_inside_ball_kernel, dim3(em_row_grid(rows)), dim3(256), 0, (hipStream_t)stream, G, rows, cols, ldg, xn, yn, r2, hit);
    return DP_LAUNCH_CHECK();
}

extern "C" int dp_em_poly_sums(const float* G, int slabs, long long slab_stride, long long rows, long long cols, long long ldg,
                               double gamma, double coef0, int degree, double* part, int nblocks, double* out, void* stream) {
    if (rows <= 0 || cols < 0 || ldg < cols || degree < 1 || nblocks < 1 || nblocks > EM_MAX_BLOCKS || slabs < 1 ||
        (slabs > 1 && slab_stride < (rows - 1) * ldg + cols))
        return (int)hipErrorInvalidValue;
    EM_LAUNCH(em_poly_part_kernel, dim3(nblocks), dim3(256), 0, (hipStream_t)stream, G, slabs, slab_stride, rows, cols, ldg, gamma, coef0,
              degree, part);
    EM_LAUNCH(em_poly_final_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, (const double*)part, nblocks, out);
    return DP_LAUNCH_CHECK();
}

extern "C" int dp_em_isc_rows(const float* logits, long long n, int c, long long ld, double* lse, double* h, void* stream) {
    if (n <= 0) return 0;
    if (c < 1 || ld < c) return (int)hipErrorInvalidValue;
    EM_LAUNCH(em_isc_rows_kernel, dim3(em_row_grid(n)), dim3(256), 0, (hipStream_t)stream, logits, n, c, ld, lse, h);
    return DP_LAUNCH_CHECK();
}

extern "C" int dp_em_isc_colmeans(const float* logits, long long ld, const double* lse, long long lo, long long hi, int c, double* q,
                                  void* stream) {
    if (c < 1 || ld < c || lo < 0 || hi <= lo) return (int)hipErrorInvalidValue;
    EM_LAUNCH(em_isc_colmeans_kernel, dim3((c + 31) / 32), dim3(256), 0, (hipStream_t)stream, logits, ld, lse, lo, hi, c, q);
    return DP_LAUNCH_CHECK();
}
