// Upsample2D's convolution, y = conv3x3(nearest_up2(x), w, pad 1), in 9 multiplies per low-resolution pixel and channel pair.
//
// The four-class sub-pixel form (dp_ups_weff + four 2x2 convolutions, csrc/elementwise.hip) spends 16.  In one dimension
//     y[2i] = w0 x[i-1] + (w1 + w2) x[i],   y[2i+1] = (w0 + w1) x[i] + w2 x[i+1]
// needs only the three products m = g (.) v with g = (w0, w0 + w1 + w2, w2) and v = (x[i-1] - x[i], x[i], x[i+1] - x[i]):
// y[2i] = m0 + m1, y[2i+1] = m1 + m2.  In two dimensions U = G w G^T (3x3 per (co, ci), integer combinations, dp_ups9_u) with
// G = [1 0 0; 1 1 1; 0 0 1], and nine products per pixel.
//
// This file holds the INPUT GRADIENT and the FORWARD pass of that form (ups9_fwd_kernel, further down); the weight gradient is
// csrc/ups9_wgrad.hip.  The input gradient:
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

typedef float f32x2 __attribute__((ext_vector_type(2)));

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

// ---- forward: y[n][co][2i+ph][2j+pw] = (A^T M A)[ph][pw] (+ bias[co]), M[a][b] = sum_ci U[co][ci][a][b] V[n][ci][a][b][i][j] ----------------
// V = the 3x3 low-resolution patch of x round (i, j), zero outside the image, after (p0 - p1, p1, p2 - p1) along each axis.  Nine
// implicit GEMMs that share nothing but the patch: a 256-thread workgroup owns BM output channels x BN pixels as four 32x32 tiles, one
// per wavefront, and every wavefront keeps all nine accumulators of its tile (144 registers), so that the A^T M A epilogue stays in
// registers and y goes straight to its high-resolution positions, the two pw neighbours as one 8-byte store: no q[4, ...] staging
// buffer, no interleave pass.  U: dp_pack_weight mode 0 of U ([tap][ci][ld]) -> As[tap * KC + k][m]; V -> Vs[tap * KC + k][pixel].
template <int BM, int BN, int KC, int OCC>
__global__ __launch_bounds__(256, OCC) void ups9_fwd_kernel(const dp_ups9_fwd_params p) {
    constexpr int WN = BN / 32;                     // wavefronts along the pixels
    constexpr int KT = 9 * KC;
    constexpr int PT = BN * KC / 256;               // patches per thread and K tile
    constexpr int KSTEP = 256 / BN;
    constexpr int MCH = BM / 4;
    constexpr int ACH = KT * MCH;
    constexpr int NA = (ACH + 255) / 256;
    constexpr int NS = 9 * KC / 2;                  // MFMA steps of one K tile
    static_assert((BM / 32) * WN == 4 && PT >= 1 && BN * KC % 256 == 0 && KC % 2 == 0 && BM % 32 == 0 && BN % 32 == 0, "tile");
    __shared__ __attribute__((aligned(16))) float As[KT * BM];
    __shared__ __attribute__((aligned(16))) float Vs[KT * BN];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 31, lk = lane >> 5;
    const int wm0 = (wave / WN) * 32, wn0 = (wave % WN) * 32;
    const int H = p.H, W = p.W, HW = H * W;
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

    // ---- this thread's patch: pixel tid % BN, channels tid / BN + KSTEP * q of every K tile
    const int ppix = tid % BN, pk0 = tid / BN;
    int pbase;                                       // float offset of patch element (0, 0) of channel 0 (may be negative: never used then)
    bool pvalid, top, bot, left, right;
    {
        const int pixel = px0 + ppix;
        pvalid = pixel < NPIX;
        const int n = pixel / HW, rem = pixel - n * HW;
        const int i = rem / W, j = rem - i * W;
        pbase = (int)(n * p.x_img_stride) + (i - 1) * W + (j - 1);
        top = i > 0, bot = i < H - 1, left = j > 0, right = j < W - 1;
    }
    const __amdgpu_buffer_rsrc_t rA = u9_rsrc(p.U, p.u_bytes);
    const __amdgpu_buffer_rsrc_t rB = u9_rsrc(p.x, p.x_bytes);

    float pr[PT][9];
    f32x4 ar[NA];
    auto load_tile = [&](int k0) {
#pragma unroll
        for (int j = 0; j < NA; ++j) {
            const int e = tid + 256 * j;
            const int kk = e / MCH, m = m0 + 4 * (e % MCH);
            const int tap = kk / KC, k = k0 + kk % KC;
            const bool v = e < ACH && m < p.ldu && k < K;
            ar[j] = u9_bload4(rA, v ? (unsigned)(((tap * K + k) * p.ldu + m) * 4) : U9_OOB);
        }
#pragma unroll
        for (int q = 0; q < PT; ++q) {
            const int k = k0 + pk0 + KSTEP * q;
            const bool ok = pvalid && k < K;
            const int off0 = pbase + k * HW;
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const bool rok = ok && (r == 0 ? top : r == 2 ? bot : true);
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const bool v = rok && (c == 0 ? left : c == 2 ? right : true);
                    pr[q][3 * r + c] = u9_bload(rB, v ? (unsigned)((off0 + r * W + c) * 4) : U9_OOB);
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
            float t[3][3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                t[0][c] = d[c] - d[3 + c];
                t[1][c] = d[3 + c];
                t[2][c] = d[6 + c] - d[3 + c];
            }
            const int kc = pk0 + KSTEP * q;
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                Vs[((3 * a + 0) * KC + kc) * BN + ppix] = t[a][0] - t[a][1];
                Vs[((3 * a + 1) * KC + kc) * BN + ppix] = t[a][1];
                Vs[((3 * a + 2) * KC + kc) * BN + ppix] = t[a][2] - t[a][1];
            }
        }
    };

    f32x16 acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    const int nIter = (K + KC - 1) / KC;
    load_tile(0);
    for (int it = 0; it < nIter; ++it) {
        __syncthreads();                             // the MFMAs of the previous tile have read their operands
        store_tile();
        __syncthreads();
        if (it + 1 < nIter) load_tile((it + 1) * KC);        // in flight during the MFMAs below
        // step s = (k pair s / 9, tap s % 9); fragment reads two steps ahead of the MFMA that consumes them
        float a[3], b[3];
        auto frag = [&](int s, float& fa, float& fb) {
            const int kk = (s % 9) * KC + (s / 9) * 2 + lk;
            fa = As[kk * BM + wm0 + li];
            fb = Vs[kk * BN + wn0 + li];
        };
        frag(0, a[0], b[0]);
        frag(1, a[1], b[1]);
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            if (s + 2 < NS) frag(s + 2, a[(s + 2) % 3], b[(s + 2) % 3]);
            __builtin_amdgcn_sched_barrier(0);
            acc[s % 9] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s % 3], b[s % 3], acc[s % 9], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
    }

    // ---- epilogue.  C/D map of a 32x32 tile: column = lane & 31, row = (r & 3) + 8 (r >> 2) + 4 (lane >> 5)
    const int pixel = px0 + wn0 + li;
    if (pixel >= NPIX) return;
    const int n = pixel / HW, rem = pixel - n * HW;
    const int i = rem / W, j = rem - i * W;
    float* o = p.y + (long long)n * p.y_img_stride + (long long)(2 * i) * (2 * W) + 2 * j;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int row = m0 + wm0 + (r & 3) + 8 * (r >> 2) + 4 * lk;
        if (row < M) {
            const float bv = p.bias ? p.bias[row] : 0.f;
            const float c0 = acc[0][r] + acc[3][r], c1 = acc[1][r] + acc[4][r], c2 = acc[2][r] + acc[5][r];      // rows a = 0, 1
            const float d0 = acc[3][r] + acc[6][r], d1 = acc[4][r] + acc[7][r], d2 = acc[5][r] + acc[8][r];      // rows a = 1, 2
            float* q = o + (long long)row * (4 * HW);
            f32x2 y0, y1;
            y0[0] = (c0 + c1) + bv, y0[1] = (c1 + c2) + bv;
            y1[0] = (d0 + d1) + bv, y1[1] = (d1 + d2) + bv;
            *(f32x2*)q = y0;
            *(f32x2*)(q + 2 * W) = y1;
        }
    }
}

// One tile: 64 output channels x 64 pixels, 8 input channels per K tile.  [measured, profiles/ups9_fwd_gate.txt: a 128 x 32 tile (4 channels
// per K tile, 8 would spill) was slower on every row, by 25 % at the pruned widths, which pad 180 rows to 256 instead of 192.]
#define U9F_BM 64
#define U9F_BN 64

// What dp_ups9_fwd takes (ops.ups9_fwd_shape_ok restates it argument by argument); everything else is hipErrorInvalidValue, nothing launched.
static bool u9f_ok(const dp_ups9_fwd_params& p) {
    if (!p.U || !p.x || !p.y || ((uintptr_t)p.U & 15) || ((uintptr_t)p.y & 7) || ((uintptr_t)p.bias & 3)) return false;
    if (p.N < 1 || p.M < 1 || p.K < 1 || p.H < 1 || p.W < 1) return false;
    if (p.ldu < p.M || (p.ldu & 3)) return false;
    const long long HW = (long long)p.H * p.W;
    const long long npix = HW * p.N;
    if (npix >= (1ll << 29)) return false;                                             // pixel numbers and block counts are ints
    if (9ll * p.K * p.ldu * 4 != (long long)p.u_bytes || p.u_bytes >= 0x80000000u) return false;      // U is exactly [9][K][ldu]
    if (p.x_img_stride < HW * p.K || p.y_img_stride < 4 * HW * p.M || (p.y_img_stride & 1)) return false;      // no overlap; 8-byte stores
    const long long x_need = ((p.N - 1) * p.x_img_stride + HW * p.K) * 4;
    if ((long long)p.x_bytes < x_need || p.x_bytes >= 0x80000000u) return false;      // 32-bit byte offsets, bit 31 = out of range
    const long long blocks = ((npix + U9F_BN - 1) / U9F_BN) * ((p.M + U9F_BM - 1) / U9F_BM);
    if (blocks >= (1ll << 31)) return false;
    return true;
}

extern "C" int dp_ups9_fwd(const dp_ups9_fwd_params* pp, void* stream) {
    const dp_ups9_fwd_params& p = *pp;
    if (!u9f_ok(p)) return (int)hipErrorInvalidValue;
    const long long npix = (long long)p.N * p.H * p.W;
    const dim3 grid((unsigned)(((npix + U9F_BN - 1) / U9F_BN) * ((p.M + U9F_BM - 1) / U9F_BM)));
    static_assert(U9F_BM == 64 && U9F_BN == 64, "the launch below names its tile");
    DP_LAUNCH((ups9_fwd_kernel<64, 64, 8, 2>), grid, dim3(256), 0, (hipStream_t)stream, p);
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
