// Nearest-codebook vector quantizer of the VQ autoencoder (diffusers VectorQuantizer.forward, vae.py:332-364, legacy=True,
// remap=None), forward only.
//
// One thread per latent pixel p = (n, h, w); the codebook is streamed through LDS in chunks of VQ_CHUNK codes that the block's
// 256 pixels share (every lane reads the same LDS address: a broadcast).  The distance is the direct form sum_d (z_d - e_d)^2 --
// not |z|^2 + |e|^2 - 2 z.e, which cancels digits -- and codes are visited in increasing k with a strict `<`, so among equal
// fp32 distances the lowest k wins (torch.argmin).  z_q = z + (e - z), the two fp32 roundings of `z + (z_q - z).detach()`.
// The loss (1 + beta) * mean((e_idx - z)^2) is a per-block fp64 partial of the minimum distances plus a one-block reduction:
// no float atomics, the same bits on every run.
#include <hip/hip_runtime.h>
#include "dp_common.h"
#include "dp_hip.h"

#define VQ_THREADS 256
#define VQ_CHUNK 512
#define VQ_DMAX 16

template <int D>
__global__ __launch_bounds__(VQ_THREADS) void vq_quantize_kernel(const float* __restrict__ z, long long z_bs, int HW, long long P,
                                                                 const float* __restrict__ E, int K, float* __restrict__ zq,
                                                                 long long zq_bs, long long* __restrict__ idx,
                                                                 double* __restrict__ partial) {
    __shared__ float cb[VQ_CHUNK * D];
    __shared__ double red[VQ_THREADS / DP_WAVE];
    const long long p = (long long)blockIdx.x * VQ_THREADS + threadIdx.x;
    const bool live = p < P;
    long long n = 0;
    int hw = 0;
    float zv[D];
    if (live) {
        n = p / HW;
        hw = (int)(p - n * HW);
        const float* zp = z + n * z_bs + hw;
#pragma unroll
        for (int d = 0; d < D; ++d) zv[d] = zp[(long long)d * HW];
    } else {
#pragma unroll
        for (int d = 0; d < D; ++d) zv[d] = 0.f;
    }
    float best = INFINITY;
    int bi = 0;
    for (int k0 = 0; k0 < K; k0 += VQ_CHUNK) {
        const int kc = min(VQ_CHUNK, K - k0);
        __syncthreads();                                   // the previous chunk is no longer read
        for (int i = threadIdx.x; i < kc * D; i += VQ_THREADS) cb[i] = E[(long long)k0 * D + i];
        __syncthreads();
        for (int k = 0; k < kc; ++k) {
            float acc = 0.f;
#pragma unroll
            for (int d = 0; d < D; ++d) {
                const float t = __fsub_rn(zv[d], cb[k * D + d]);
                acc = __fmaf_rn(t, t, acc);
            }
            if (acc < best) {                              // strict: the first (lowest) k of equal distances is kept
                best = acc;
                bi = k0 + k;
            }
        }
    }
    double mine = 0.0;
    if (live) {
        const float* e = E + (long long)bi * D;
        float* o = zq + n * zq_bs + hw;
        double s = 0.0;
#pragma unroll
        for (int d = 0; d < D; ++d) {
            const float ed = e[d];
            o[(long long)d * HW] = __fadd_rn(zv[d], __fsub_rn(ed, zv[d]));
            const double t = (double)ed - (double)zv[d];
            s += t * t;
        }
        mine = s;
        if (idx) idx[p] = bi;
    }
    if (partial) {
        for (int off = DP_WAVE / 2; off > 0; off >>= 1) mine += __shfl_xor(mine, off, DP_WAVE);
        if ((threadIdx.x & (DP_WAVE - 1)) == 0) red[threadIdx.x / DP_WAVE] = mine;
        __syncthreads();
        if (threadIdx.x == 0) {
            double s = 0.0;
            for (int w = 0; w < VQ_THREADS / DP_WAVE; ++w) s += red[w];
            partial[blockIdx.x] = s;
        }
    }
}

extern "C" int dp_vq_blocks(long long P) { return (int)((P + VQ_THREADS - 1) / VQ_THREADS); }

extern "C" int dp_vq_quantize(const float* z, long long z_bs, int D, int HW, long long P, const float* E, int K, float* zq,
                              long long zq_bs, long long* idx, double* partial, void* stream) {
    if (D < 1 || D > VQ_DMAX) return (int)hipErrorNotSupported;
    if (K < 1 || HW < 1 || P < 0 || !z || !E || !zq) return (int)hipErrorInvalidValue;
    if (P == 0) return 0;
    const long long blocks = (P + VQ_THREADS - 1) / VQ_THREADS;
    if (blocks > 0x7fffffffLL) return (int)hipErrorInvalidValue;
    hipStream_t s = (hipStream_t)stream;
    switch (D) {
#define VQ_CASE(DD)                                                                                                          \
    case DD:                                                                                                                 \
        DP_LAUNCH(vq_quantize_kernel<DD>, dim3((unsigned)blocks), dim3(VQ_THREADS), 0, s, z, z_bs, HW, P, E, K, zq, zq_bs, idx, \
                  partial);                                                                                                  \
        break;
        VQ_CASE(1) VQ_CASE(2) VQ_CASE(3) VQ_CASE(4) VQ_CASE(5) VQ_CASE(6) VQ_CASE(7) VQ_CASE(8)
        VQ_CASE(9) VQ_CASE(10) VQ_CASE(11) VQ_CASE(12) VQ_CASE(13) VQ_CASE(14) VQ_CASE(15) VQ_CASE(16)
#undef VQ_CASE
    }
    return DP_LAUNCH_CHECK();
}

// loss[0] = (float)(scale * sum of the nblocks partials), summed in a fixed order (one block, strided per thread, then the tree)
__global__ __launch_bounds__(256) void vq_loss_kernel(const double* __restrict__ partial, int n, double scale,
                                                      float* __restrict__ loss) {
    __shared__ double red[256];
    double s = 0.0;
    for (int i = threadIdx.x; i < n; i += 256) s += partial[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if (threadIdx.x < off) red[threadIdx.x] += red[threadIdx.x + off];
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = (float)(red[0] * scale);
}

extern "C" int dp_vq_loss(const double* partial, int nblocks, double scale, float* loss, void* stream) {
    if (nblocks <= 0 || !partial || !loss) return (int)hipErrorInvalidValue;
    DP_LAUNCH(vq_loss_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partial, nblocks, scale, loss);
    return DP_LAUNCH_CHECK();
}
