// The WEIGHT GRADIENT of Upsample2D's convolution, y = conv3x3(nearest_up2(x), w, pad 1), in 9 multiplies per low-resolution pixel and
// channel pair: the third member of the family of csrc/ups9.hip (U = G w G^T, G = [1 0 0; 1 1 1; 0 0 1]).
//     dU[co][ci][a][b] = sum_{n,i,j} dM[n][co][a][b][i][j] V[n][ci][a][b][i][j],      dw = G^T dU G
//     dM = A D A^T of the 2x2 block D of the HIGH-resolution dy at rows 2i, 2i+1 / columns 2j, 2j+1, A = [1 0; 1 1; 0 1]:
//          d00, d00 + d01, d01;  d00 + d10, (d00 + d01) + (d10 + d11), d01 + d11;  d10, d10 + d11, d11
//     V  = B^T d B of the 3x3 low-resolution neighbourhood d of x round (i, j), zero outside the image BEFORE the differences
//          ((p0 - p1, p1, p2 - p1) along each axis): the operand ups9_fwd_kernel forms.
// The four class launches it replaces (2x2 taps each, csrc/gemm.hip) spend 16 products, need a de-interleaved copy of dy, four split-K
// reductions and the dp_ups_wfold launch; here dy and x are read where they lie and two launches do everything:
//   dp_ups9_wgrad         nine NT GEMMs over the pixels that share their gathers.  A 256-thread workgroup owns 64 output channels x 64
//                         input channels as four 32x32 tiles, one per wavefront, and every wavefront keeps the nine accumulators of its
//                         tile (144 registers, two workgroups per CU).  K tiles of 16 low-resolution pixels, numbered n * H * W + i * W + j
//                         over all images (a tile may span an image boundary); per K tile every thread gathers four (pixel, co) blocks of
//                         dy -- two 8-byte raw buffer loads each -- and four (pixel, ci) neighbourhoods of x -- nine 4-byte loads each,
//                         out-of-image elements as out-of-range offsets, i.e. zeros -- while the matrix cores work on the previous tile,
//                         then transforms them in registers and writes Ds[tap * 16 + pixel][co] / Vs[tap * 16 + pixel][ci] (row pitch 66
//                         floats: the 32 lanes of a store group hit 32 banks).  72 v_mfma_f32_32x32x2_f32 per wavefront and K tile.
//                         Split-K: workgroup (tile, split) takes the K tiles [split * tiles_per_split, ...) and writes its partial to
//                         ws[split][9][Co][ld].  fp32 throughout, no atomics, one workgroup per output tile and split.
//   dp_ups9_wgrad_reduce  one thread per (co, ci): adds the splits in ascending order, folds dw = G^T dU G and writes (accumulates
//                         into) gw[Co][Ci][3][3].
// Every loop is bounded by the arguments and every sum has one fixed order: the same bits from run to run.
#include "dp_common.h"

// The launch macro of this file: the body of the library's own (dp_common.h) under a name of its own, so that the launch sites of
// this file are tabled by this file's test module (tests/test_ups9_wgrad_cpu.py), as stage.hip, magnitude.hip and unipc.hip do.
#define U9W_LAUNCH(k, ...) do { dp_launch_names[dp_launches++ & (DP_LAUNCH_RING - 1)] = #k; hipLaunchKernelGGL(k, __VA_ARGS__); } while (0)

typedef float f32x2 __attribute__((ext_vector_type(2)));

#define U9W_RSRC_FLAGS 0x00020000
#define U9W_OOB 0x80000000u
#define U9W_BM 64                 // output channels per workgroup
#define U9W_BN 64                 // input channels per workgroup
#define U9W_KP 16                 // low-resolution pixels per K tile
#define U9W_LD 66                 // LDS row pitch (floats)

__device__ __forceinline__ __amdgpu_buffer_rsrc_t u9w_rsrc(const float* base, unsigned bytes) {
    return __builtin_amdgcn_make_buffer_rsrc((void*)base, 0, (int)bytes, U9W_RSRC_FLAGS);
}
// (the empty asm keeps hipcc from turning load(select(valid, off, OOB)) into predicated loads behind exec branches: csrc/gemm.hip)
__device__ __forceinline__ float u9w_bload(__amdgpu_buffer_rsrc_t r, unsigned byte_off) {
    asm volatile("" : "+v"(byte_off));
    return __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(r, (int)byte_off, 0, 0));
}
__device__ __forceinline__ f32x2 u9w_bload2(__amdgpu_buffer_rsrc_t r, unsigned byte_off) {
    asm volatile("" : "+v"(byte_off));
    return __builtin_bit_cast(f32x2, __builtin_amdgcn_raw_buffer_load_b64(r, (int)byte_off, 0, 0));
}

__global__ __launch_bounds__(256, 2) void ups9_wgrad_kernel(const dp_ups9_wgrad_params p) {
    constexpr int BM = U9W_BM, BN = U9W_BN, KP = U9W_KP, LD = U9W_LD;
    constexpr int PT = BM * KP / 256;               // (pixel, channel) gathers per thread, operand and K tile
    constexpr int NS = 9 * KP / 2;                  // MFMA steps of one K tile
    static_assert(BM == 64 && BN == 64 && KP == 16 && PT == 4 && LD >= BM && LD >= BN, "tile");
    __shared__ __attribute__((aligned(16))) float Ds[9 * KP * LD];
    __shared__ __attribute__((aligned(16))) float Vs[9 * KP * LD];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int li = lane & 31, lk = lane >> 5;
    const int wm0 = (wave >> 1) * 32, wn0 = (wave & 1) * 32;
    const int H = p.H, W = p.W, HW = H * W, W2 = 2 * W, HW4 = 4 * HW;
    const int Co = p.Co, Ci = p.Ci;
    const int NPIX = p.N * HW;
    const int NKT = (NPIX + KP - 1) / KP;
    // the output tiles of one split back to back on one XCD (they gather the same pixels)
    const int CT = (Ci + BN - 1) / BN;
    const int TILES = ((Co + BM - 1) / BM) * CT;
    int tile, split;
    {
        const int b = blockIdx.x;
        if (!(p.splits & 7)) {
            const int xcd = b & 7, slot = b >> 3;
            tile = slot % TILES;
            split = (slot / TILES) * 8 + xcd;
        } else {
            tile = b % TILES;
            split = b / TILES;
        }
    }
    const int m0 = (tile / CT) * BM, c0 = (tile % CT) * BN;
    const int kt0 = split * p.tiles_per_split;
    const int kt1 = kt0 + p.tiles_per_split < NKT ? kt0 + p.tiles_per_split : NKT;

    // ---- this thread's gathers: pixel tid % 16 of the K tile, channels 4 * wave + (lane / 16) + 16 q of the workgroup's 64
    const int ppix = tid & 15, pch = 4 * wave + ((lane >> 4) & 3);
    const __amdgpu_buffer_rsrc_t rD = u9w_rsrc(p.dy, p.dy_bytes);
    const __amdgpu_buffer_rsrc_t rX = u9w_rsrc(p.x, p.x_bytes);

    f32x2 dr[PT][2];
    float xr[PT][9];
    auto load_tile = [&](int kt) {
        const int pixel = kt * KP + ppix;
        const bool pvalid = pixel < NPIX;
        const int n = pixel / HW, rem = pixel - n * HW;
        const int i = rem / W, j = rem - i * W;
        // float offsets; only used when pvalid (then below 2^29: the extents are below 2 GiB)
        const int dbase = (int)(n * p.dy_img_stride) + (2 * i) * W2 + 2 * j;
        const int xbase = (int)(n * p.x_img_stride) + (i - 1) * W + (j - 1);
        const bool top = i > 0, bot = i < H - 1, left = j > 0, right = j < W - 1;
#pragma unroll
        for (int q = 0; q < PT; ++q) {
            const int co = m0 + pch + 16 * q;
            const bool ok = pvalid && co < Co;
            const int off = dbase + co * HW4;
            dr[q][0] = u9w_bload2(rD, ok ? (unsigned)(off * 4) : U9W_OOB);
            dr[q][1] = u9w_bload2(rD, ok ? (unsigned)((off + W2) * 4) : U9W_OOB);
        }
#pragma unroll
        for (int q = 0; q < PT; ++q) {
            const int ci = c0 + pch + 16 * q;
            const bool ok = pvalid && ci < Ci;
            const int off0 = xbase + ci * HW;
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                const bool rok = ok && (r == 0 ? top : r == 2 ? bot : true);
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const bool v = rok && (c == 0 ? left : c == 2 ? right : true);
                    xr[q][3 * r + c] = u9w_bload(rX, v ? (unsigned)((off0 + r * W + c) * 4) : U9W_OOB);
                }
            }
        }
    };
    auto store_tile = [&]() {
#pragma unroll
        for (int q = 0; q < PT; ++q) {
            const float d00 = dr[q][0][0], d01 = dr[q][0][1], d10 = dr[q][1][0], d11 = dr[q][1][1];
            const float r0 = d00 + d01, r2 = d10 + d11;
            float* o = &Ds[ppix * LD + pch + 16 * q];
            o[0 * KP * LD] = d00;
            o[1 * KP * LD] = r0;
            o[2 * KP * LD] = d01;
            o[3 * KP * LD] = d00 + d10;
            o[4 * KP * LD] = r0 + r2;
            o[5 * KP * LD] = d01 + d11;
            o[6 * KP * LD] = d10;
            o[7 * KP * LD] = r2;
            o[8 * KP * LD] = d11;
        }
#pragma unroll
        for (int q = 0; q < PT; ++q) {
            const float* d = xr[q];
            float t[3][3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                t[0][c] = d[c] - d[3 + c];
                t[1][c] = d[3 + c];
                t[2][c] = d[6 + c] - d[3 + c];
            }
            float* o = &Vs[ppix * LD + pch + 16 * q];
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                o[(3 * a + 0) * KP * LD] = t[a][0] - t[a][1];
                o[(3 * a + 1) * KP * LD] = t[a][1];
                o[(3 * a + 2) * KP * LD] = t[a][2] - t[a][1];
            }
        }
    };

    f32x16 acc[9];
#pragma unroll
    for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) acc[t][r] = 0.f;

    if (kt0 < kt1) load_tile(kt0);
    for (int kt = kt0; kt < kt1; ++kt) {
        __syncthreads();                             // the MFMAs of the previous tile have read their operands
        store_tile();
        __syncthreads();
        if (kt + 1 < kt1) load_tile(kt + 1);         // in flight during the MFMAs below
        // step s = (pixel pair s / 9, tap s % 9); fragment reads two steps ahead of the MFMA that consumes them
        float a[3], b[3];
        auto frag = [&](int s, float& fa, float& fb) {
            const int kk = (s % 9) * KP + (s / 9) * 2 + lk;
            fa = Ds[kk * LD + wm0 + li];
            fb = Vs[kk * LD + wn0 + li];
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
    const int col = c0 + wn0 + li;
    if (col >= Ci) return;
#pragma unroll
    for (int t = 0; t < 9; ++t) {
        float* o = p.ws + ((long long)split * 9 + t) * Co * (long long)p.ld + col;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = m0 + wm0 + (r & 3) + 8 * (r >> 2) + 4 * lk;
            if (row < Co) o[(long long)row * p.ld] = acc[t][r];
        }
    }
}

// dU = sum of the splits in ascending order; dw = G^T dU G: rows (u0 + u1, u1, u1 + u2), then the same on columns.
__global__ __launch_bounds__(256) void ups9_wgrad_reduce_kernel(const float* __restrict__ ws, int splits, int Co, int Ci, int ld,
                                                                float* __restrict__ gw, int accumulate) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= Co * Ci) return;
    const int co = idx / Ci, ci = idx - co * Ci;
    const long long tap_stride = (long long)Co * ld, split_stride = 9 * tap_stride;
    const float* s = ws + (long long)co * ld + ci;
    float u[3][3];
#pragma unroll
    for (int t = 0; t < 9; ++t) u[t / 3][t % 3] = s[t * tap_stride];
    for (int z = 1; z < splits; ++z) {
        s += split_stride;
#pragma unroll
        for (int t = 0; t < 9; ++t) u[t / 3][t % 3] += s[t * tap_stride];
    }
    float g[3][3];
#pragma unroll
    for (int b = 0; b < 3; ++b) {
        g[0][b] = u[0][b] + u[1][b];
        g[1][b] = u[1][b];
        g[2][b] = u[1][b] + u[2][b];
    }
    float* o = gw + (long long)idx * 9;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const float v0 = g[r][0] + g[r][1], v1 = g[r][1], v2 = g[r][1] + g[r][2];
        o[3 * r + 0] = accumulate ? o[3 * r + 0] + v0 : v0;
        o[3 * r + 1] = accumulate ? o[3 * r + 1] + v1 : v1;
        o[3 * r + 2] = accumulate ? o[3 * r + 2] + v2 : v2;
    }
}

// The native shape predicate: what the two launchers take (ops.ups9_wgrad_shape_ok restates it argument by argument); everything else is
// hipErrorInvalidValue, nothing launched.  Like u9f_ok of csrc/ups9.hip it is applied by the launchers themselves and not exported.
static int dp_ups9_wgrad_supported(const dp_ups9_wgrad_params* pp) {
    if (!pp) return 0;
    const dp_ups9_wgrad_params& p = *pp;
    if (!p.dy || !p.x || !p.ws || !p.gw) return 0;
    if (((uintptr_t)p.dy & 7) || ((uintptr_t)p.x & 3) || ((uintptr_t)p.ws & 3) || ((uintptr_t)p.gw & 3)) return 0;      // 8-byte loads from dy
    if (p.N < 1 || p.Co < 1 || p.Ci < 1 || p.H < 1 || p.W < 1 || p.splits < 1 || p.tiles_per_split < 1) return 0;
    if (p.ld < p.Ci || p.ws_floats < (long long)p.splits * 9 * p.Co * p.ld) return 0;                       // ws holds [splits][9][Co][ld]
    const long long HW = (long long)p.H * p.W;
    const long long npix = HW * p.N;
    if (npix >= (1ll << 29)) return 0;                                             // pixel numbers and block counts are ints
    if (p.dy_img_stride < 4 * HW * p.Co || (p.dy_img_stride & 1) || p.x_img_stride < HW * p.Ci) return 0;      // no overlap; 8-byte loads
    const long long dy_need = ((p.N - 1) * p.dy_img_stride + 4 * HW * p.Co) * 4;
    const long long x_need = ((p.N - 1) * p.x_img_stride + HW * p.Ci) * 4;
    if ((long long)p.dy_bytes < dy_need || p.dy_bytes >= 0x80000000u) return 0;   // 32-bit byte offsets, bit 31 = out of range
    if ((long long)p.x_bytes < x_need || p.x_bytes >= 0x80000000u) return 0;
    const long long nkt = (npix + U9W_KP - 1) / U9W_KP;
    if ((long long)p.splits * p.tiles_per_split < nkt || (long long)(p.splits - 1) * p.tiles_per_split >= nkt) return 0;   // every split has work
    const long long tiles = (long long)((p.Co + U9W_BM - 1) / U9W_BM) * ((p.Ci + U9W_BN - 1) / U9W_BN);
    if (tiles * p.splits >= (1ll << 31) || (long long)p.Co * p.Ci >= (1ll << 31)) return 0;
    return 1;
}

extern "C" int dp_ups9_wgrad(const dp_ups9_wgrad_params* pp, void* stream) {
    if (!dp_ups9_wgrad_supported(pp)) return (int)hipErrorInvalidValue;
    const dp_ups9_wgrad_params& p = *pp;
    const long long tiles = (long long)((p.Co + U9W_BM - 1) / U9W_BM) * ((p.Ci + U9W_BN - 1) / U9W_BN);
    U9W_LAUNCH(ups9_wgrad_kernel, dim3((unsigned)(tiles * p.splits)), dim3(256), 0, (hipStream_t)stream, p);
    return DP_LAUNCH_CHECK();
}

extern "C" int dp_ups9_wgrad_reduce(const dp_ups9_wgrad_params* pp, void* stream) {
    if (!dp_ups9_wgrad_supported(pp)) return (int)hipErrorInvalidValue;
    const dp_ups9_wgrad_params& p = *pp;
    const unsigned nb = (unsigned)(((long long)p.Co * p.Ci + 255) / 256);
    U9W_LAUNCH(ups9_wgrad_reduce_kernel, dim3(nb), dim3(256), 0, (hipStream_t)stream, (const float*)p.ws, p.splits, p.Co, p.Ci, p.ld, p.gw,
               p.accumulate);
    return DP_LAUNCH_CHECK();
}
