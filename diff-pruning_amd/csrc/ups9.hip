// Upsample2D's convolution, y = conv3x3(nearest_up2(x), w, pad 1), in 9 multiplies per low-resolution pixel and channel pair.
//
// The four-class sub-pixel form (dp_ups_weff + four 2x2 convolutions, csrc/elementwise.hip) spends 16.  In one dimension
//     y[2i] = w0 x[i-1] + (w1 + w2) x[i],   y[2i+1] = (w0 + w1) x[i] + w2 x[i+1]
// needs only the three products m = g (.) v with g = (w0, w0 + w1 + w2, w2) and v = (x[i-1] - x[i], x[i], x[i+1] - x[i]):
// y[2i] = m0 + m1, y[2i+1] = m1 + m2.  In two dimensions U = G w G^T (3x3 per (co, ci), integer combinations, dp_ups9_u) with
// G = [1 0 0; 1 1 1; 0 0 1], and nine products per pixel.
//
// This file holds the INPUT GRADIENT of that form (the forward and the weight gradient keep the class launches):
//     dx[n][ci][i][j] = sum_co sum_{a,b} U[co][ci][a][b] T[n][co][a][b][i][j],   T = R p R^T,
// p = the 4x4 patch of the HIGH-resolution dy at rows 2i-1 .. 2i+2 / columns 2j-1 .. 2j+2 (zero outside the image) and
// R = [0 -1 0 1; 0 1 1 0; 1 0 -1 0] (T0 = p3 - p1, T1 = p1 + p2, T2 = p0 - p2 along each axis): one implicit GEMM with nine taps
// whose B operand is a signed sum of patch values.  dy is read as it is: no de-interleave pass in front of it.
//
// Mapping: a 256-thread workgroup owns BM = 128 input channels x BN low-resolution pixels (pixels are numbered n * H * W + i * W + j,
// so a block may span image boundaries) and walks the output channels KC at a time.  Per K tile every thread gathers the 4x4
// patch(es) of its (pixel, channel) into registers -- raw buffer loads whose out-of-image elements are out-of-range offsets, i.e.
// zeros -- while the matrix cores work on the previous tile, then transforms them (21 adds) and writes the nine T values to
// LDS as Ts[tap * KC + k][pixel]; U's packed rows (dp_pack_weight mode 1 of U: [8 - tap][co][ld]) go to As[tap * KC + k][m].  The
// inner loop is the plain v_mfma_f32_32x32x2_f32 loop of csrc/gemm.hip over 9 * KC k-steps.  fp32 everywhere, no atomics, one
// workgroup per output tile, every loop bounded by its arguments: the same bits from run to run.
#include "dp_common.h"

#define U9_RSRC_FLAGS 0x00020000
#define U9_OOB 0x80000000u

__device__ __forceinline__ __amdgpu_buffer_rsrc_t u9_rsrc(const float* base, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, (int)bytes, U9_RSRC_FLAGS);
}
// (the empty asm keeps hipcc from turning load(select(valid, off, OOB)) into predicated loads behind exec branches: csrc/gemm.hip)
__device__ __forceinline__ float u9_bload(__amdgpu_buffer_rsrc_t r, unsigned byte_off) {
    asm volatile("" : "+v"(byte_off));
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, (int)byte_off, 0, 0));
}
__device__ __forceinline__ f32x4 u9_bload4(__amdgpu_buffer_rsrc_t r, unsigned byte_off) {
    asm volatile("" : "+v"(byte_off));
    return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(r, (int)byte_off, 0, 0));
}

// WM x WN wavefronts of TM x TN 32x32 MFMA tiles each; OCC = workgroups per CU the register budget is cut for.
template <int BM, int BN, int KC, int WM, int WN, int OCC>
__global__ __launch_bounds__(256, OCC) void ups9_dgrad_kernel(const dp_ups9_params p) {
    constexpr int TM = BM / (32 * WM), TN = BN / (32 * WN);
    constexpr int KT = 9 * KC;                      // k-steps of one K tile
    constexpr int PT = BN * KC / 256;               // patches per thread and K tile
    constexpr int KSTEP = 256 / BN;                 // channel distance between a thread's patches
    constexpr int MCH = BM / 4;                     // 16-byte chunks per A row
    constexpr int ACH = KT * MCH;                   // ... per A tile
    constexpr int NA = (ACH + 255) / 256;
    static_assert(WM * WN == 4 && TM >= 1 && TN >= 1 && PT >= 1 && (BN * KC) % 256 == 0 && KT % 2 == 0 && BN <= 256, "tile");
    __shared__ __attribute__((aligned(16))) float As[KT * BM];
    __shared__ __attribute__((aligned(16))) float Ts[KT * BN];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 31, lk = lane >> 5;
    const int wm0 = (wave / WN) * (TM * 32), wn0 = (wave % WN) * (TN * 32);
    const int H = p.H, W = p.W, HW = H * W, W2 = 2 * W, HW4 = 4 * HW;
    const int K = p.K, M = p.M;
    const int NPIX = p.N * HW;
    // row tiles of one pixel block back to back on one XCD (they gather the same patches)
    const int MT = (M + BM - 1) / BM;
    const int PTILES = (NPIX + BN - 1) / BN;
    int mt, ptile;
    {
        const int b = blockIdx.x;
        if (!(PTILES & 7)) {
            const int xcd = b & 7, slot = b >> 3;
            mt = slot % MT;
            ptile = (slot / MT) * 8 + xcd;
        } else {
            mt = b % MT;
            ptile = b / MT;
        }
    }
    const int m0 = mt * BM, px0 = ptile * BN;

    // ---- this thread's patch: pixel tid % BN, channels tid / BN + KSTEP * j of every K tile
    const int ppix = tid % BN, pk0 = tid / BN;
    int pbase;                                       // float offset of patch element (0, 0) of channel 0 (may be negative: never used then)
    bool pvalid, top, bot, left, right;
    {
        const int pixel = px0 + ppix;
        pvalid = pixel < NPIX;
        const int n = pixel / HW, rem = pixel - n * HW;
        const int i = rem / W, j = rem - i * W;
        pbase = (int)(n * p.dy_img_stride) + (2 * i - 1) * W2 + (2 * j - 1);
        top = i > 0, bot = i < H - 1, left = j > 0, right = j < W - 1;
    }
    // ---- A chunks: e = tid + 256 j of [kk = tap * KC + k][m / 4] (offsets are recomputed per tile: a handful of shifts against 2 NA registers)
    const __amdgpu_buffer_rsrc_t rA = u9_rsrc(p.U, p.u_bytes);
    const __amdgpu_buffer_rsrc_t rB = u9_rsrc(p.dy, p.dy_bytes);

    float pr[PT][16];
    f32x4 ar[NA];
    auto load_tile = [&](int k0) {
#pragma unroll
        for (int j = 0; j < NA; ++j) {
            const int e = tid + 256 * j;
            const int kk = e / MCH, m = m0 + 4 * (e % MCH);
            const int tap = kk / KC, k = k0 + kk % KC;
            const bool v = e < ACH && m < p.ldu && k < K;
            ar[j] = u9_bload4(rA, v ? (unsigned)((((8 - tap) * K + k) * p.ldu + m) * 4) : U9_OOB);
        }
#pragma unroll
        for (int q = 0; q < PT; ++q) {
            const int k = k0 + pk0 + KSTEP * q;
            const bool ok = pvalid && k < K;
            const int off0 = pbase + k * HW4;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool rok = ok && (r == 0 ? top : r == 3 ? bot : true);
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const bool v = rok && (c == 0 ? left : c == 3 ? right : true);
                    pr[q][4 * r + c] = u9_bload(rB, v ? (unsigned)((off0 + r * W2 + c) * 4) : U9_OOB);
                }
            }
        }
    };
    auto store_tile = [&]() {
#pragma unroll
        for (int j = 0; j < NA; ++j)
            if (NA * 256 == ACH || tid + 256 * j < ACH) *(f32x4*)&As[(tid + 256 * j) * 4] = ar[j];
#pragma unroll
        for (int q = 0; q < PT; ++q) {
            const float* d = pr[q];
            float t[3][4];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                t[0][c] = d[12 + c] - d[4 + c];
                t[1][c] = d[4 + c] + d[8 + c];
                t[2][c] = d[c] - d[8 + c];
            }
            const int kc = pk0 + KSTEP * q;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                Ts[((3 * a + 0) * KC + kc) * BN + ppix] = t[a][3] - t[a][1];
                Ts[((3 * a + 1) * KC + kc) * BN + ppix] = t[a][1] + t[a][2];
                Ts[((3 * a + 2) * KC + kc) * BN + ppix] = t[a][0] - t[a][2];
            }
        }
    };

    f32x16 acc[TM][TN];
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int tn = 0; tn < TN; ++tn)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[tm][tn][r] = 0.f;

    const int nIter = (K + KC - 1) / KC;
    load_tile(0);
    for (int it = 0; it < nIter; ++it) {
        __syncthreads();                             // the MFMAs of the previous tile have read their operands
        store_tile();
        __syncthreads();
        if (it + 1 < nIter) load_tile((it + 1) * KC);        // in flight during the MFMAs below
        // fragment reads one k-step ahead of the MFMAs that consume them (mfma_tile of csrc/gemm.hip)
        float a[2][TM], b[2][TN];
        auto frag = [&](int ks, float (&fa)[TM], float (&fb)[TN]) {
            const int kk = ks * 2 + lk;
#pragma unroll
            for (int tm = 0; tm < TM; ++tm) fa[tm] = As[kk * BM + wm0 + tm * 32 + li];
#pragma unroll
            for (int tn = 0; tn < TN; ++tn) fb[tn] = Ts[kk * BN + wn0 + tn * 32 + li];
        };
        frag(0, a[0], b[0]);
#pragma unroll
        for (int ks = 0; ks < KT / 2; ++ks) {
            const int cur = ks & 1;
            if (ks + 1 < KT / 2) frag(ks + 1, a[cur ^ 1], b[cur ^ 1]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int tm = 0; tm < TM; ++tm)
#pragma unroll
                for (int tn = 0; tn < TN; ++tn)
                    acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[cur][tm], b[cur][tn], acc[tm][tn], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
    }

    // ---- epilogue.  C/D map of a 32x32 tile: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) {
        const int pixel = px0 + wn0 + tn * 32 + li;
        if (pixel >= NPIX) continue;
        const int n = pixel / HW, rem = pixel - n * HW;
        float* o = p.dx + (long long)n * p.dx_img_stride + rem;
#pragma unroll
        for (int tm = 0; tm < TM; ++tm)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = m0 + wm0 + tm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk;
                if (row < M) {
                    float* q = o + (long long)row * HW;
                    *q = p.accumulate ? *q + acc[tm][tn][r] : acc[tm][tn][r];
                }
            }
    }
}

// Tiles (dp_ups9_params.tile): 0 = 128 x 32 pixels (8 channels per K tile), 1 = 128 x 64 (4), 2 = 128 x 128 (4).
static const int u9_bn[3] = {32, 64, 128};

extern "C" int dp_ups9_dgrad_supported(const dp_ups9_params* pp) {
    const dp_ups9_params& p = *pp;
    if (!p.U || !p.dy || !p.dx || ((uintptr_t)p.U & 15)) return 0;
    if (p.N < 1 || p.M < 1 || p.K < 1 || p.H < 1 || p.W < 1 || p.tile < 0 || p.tile > 2) return 0;
    if (p.ldu < p.M || (p.ldu & 3)) return 0;
    const long long HW = (long long)p.H * p.W;
    const long long npix = HW * p.N;
    if (npix >= (1ll << 29)) return 0;                                             // pixel numbers and block counts are ints
    if (9ll * p.K * p.ldu * 4 != (long long)p.u_bytes || p.u_bytes >= 0x80000000u) return 0;      // U is exactly [9][K][ldu]
    if (p.dy_img_stride < 4 * HW * p.K || p.dx_img_stride < HW * p.M) return 0;     // images do not overlap
    const long long dy_need = ((p.N - 1) * p.dy_img_stride + 4 * HW * p.K) * 4;
    if ((long long)p.dy_bytes < dy_need || p.dy_bytes >= 0x80000000u) return 0;   // 32-bit byte offsets, bit 31 = out of range
    const long long blocks = ((npix + u9_bn[p.tile] - 1) / u9_bn[p.tile]) * ((p.M + 127) / 128);
    if (blocks >= (1ll << 31)) return 0;
    return 1;
}

extern "C" int dp_ups9_dgrad(const dp_ups9_params* pp, void* stream) {
    if (!dp_ups9_dgrad_supported(pp)) return (int)hipErrorInvalidValue;
    const dp_ups9_params& p = *pp;
    const long long npix = (long long)p.N * p.H * p.W;
    const int bn = u9_bn[p.tile];
    const dim3 grid((unsigned)(((npix + bn - 1) / bn) * ((p.M + 127) / 128)));
    hipStream_t st = (hipStream_t)stream;
    if (p.tile == 0)      DP_LAUNCH((ups9_dgrad_kernel<128, 32, 8, 4, 1, 2>), grid, dim3(256), 0, st, p);
    else if (p.tile == 1) DP_LAUNCH((ups9_dgrad_kernel<128, 64, 4, 2, 2, 3>), grid, dim3(256), 0, st, p);
    else                  DP_LAUNCH((ups9_dgrad_kernel<128, 128, 4, 2, 2, 2>), grid, dim3(256), 0, st, p);
    return DP_LAUNCH_CHECK();
}

// U[m][a][b] = (G w[m] G^T)[a][b] for the M = Cout * Cin 3x3 kernels of w: rows (w0, (w0 + w1) + w2, w2), then the same on columns.
__global__ __launch_bounds__(256) void ups9_u_kernel(const float* __restrict__ w, long long M, float* __restrict__ u) {
    for (long long m = (long long)blockIdx.x * 256 + threadIdx.x; m < M; m += (long long)gridDim.x * 256) {
        float g[3][3], t[3][3];
#pragma unroll
        for (int i = 0; i < 9; ++i) g[i / 3][i % 3] = w[m * 9 + i];
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            t[0][c] = g[0][c];
            t[1][c] = (g[0][c] + g[1][c]) + g[2][c];
            t[2][c] = g[2][c];
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            u[m * 9 + 3 * a + 0] = t[a][0];
            u[m * 9 + 3 * a + 1] = (t[a][0] + t[a][1]) + t[a][2];
            u[m * 9 + 3 * a + 2] = t[a][2];
        }
    }
}

extern "C" int dp_ups9_u(const float* w, long long M, float* u, void* stream) {
    if (M <= 0) return 0;
    long long nb = (M + 255) / 256;
    if (nb > 4096) nb = 4096;
    DP_LAUNCH(ups9_u_kernel, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, w, M, u);
    return DP_LAUNCH_CHECK();
}
