// The elementwise kernels of the KL autoencoder (diffusers/models/autoencoder_kl.py, vae.py:384-428):
//   dp_gaussian_posterior  DiagonalGaussianDistribution in ONE pass over the moments: the clamped log-variance, std, var, the
//                          reparameterised sample scale * (mean + std * noise) and the per-image KL to the unit Gaussian, whichever
//                          of them the caller asks for.  The reference runs a chunk, a clamp, two exps with a multiply, and per
//                          sample / kl call three and six more elementwise launches plus a reduction.
//   dp_tile_blend          one tile of tiled_encode / tiled_decode: blend_v with the tile above, blend_h with the tile to the left
//                          (2 * blend_extent slice assignments of three launches each in the reference), the crop to row_limit and
//                          the tile's place in the two torch.cat, in one launch.
//
// Rounding: every fp32 operation is rounded separately (clang fp contract(off): hipcc would otherwise fuse a * b + c into one
// v_fma_f32), in the reference's order.  exp is the device library's expf (range reduction in extended precision), not v_exp_f32 on
// a pre-multiplied argument: at |lv| of 20 .. 30 the rounding of lv * log2(e) alone costs 2^-24 * 43 relative.  The blend weights
// k / e and 1 - k / e are formed in double and rounded once, as the reference's Python scalars reach an fp32 tensor.
//
// KL: every lane adds its elements' terms in double in the order it meets them, a block combines its 256 lanes by a fixed tree and
// stores one partial; a second launch adds an image's partials in a fixed order.  No atomics: the same call gives the same bits.
// The grid depends on N, chw and on whether the 16-byte path is taken, not on which outputs are asked for.
//
// Plain vector loads and stores, 64-bit element indices.
#include "dp_common.h"
#include "dp_headtail_plan.h"                  // dp_bytes_overlap

// The launch macro of this file: the body of the library's own (dp_common.h) under a name of its own, so that the launch sites of
// this file are tabled by this file's test module (tests/test_vae_gpu.py), as unipc.hip, dpm_solver.hip and stage.hip do.
#define VAE_LAUNCH(k, ...) do { dp_launch_names[dp_launches++ & (DP_LAUNCH_RING - 1)] = #k; hipLaunchKernelGGL(k, __VA_ARGS__); } while (0)

struct post_want { bool lv, sd, vr, z, kl; };

__device__ __forceinline__ void post_one(float mean, float raw, float nz, float scale, const post_want& w, float& lv, float& sd,
                                         float& vr, float& zz, double& acc) {
#pragma clang fp contract(off)
    lv = raw < -30.f ? -30.f : (raw > 20.f ? 20.f : raw);             // a NaN fails both tests and stays, as torch.clamp leaves it
    sd = (w.sd || w.z) ? expf(0.5f * lv) : 0.f;                         // 0.5 * lv is exact
    vr = (w.vr || w.kl) ? expf(lv) : 0.f;
    zz = 0.f;
    if (w.z) {
        const float p = sd * nz;
        const float s = mean + p;
        zz = scale == 1.f ? s : scale * s;
    }
    if (w.kl) {
        const double m2 = (double)mean * (double)mean;                  // exact
        acc += ((m2 + (double)vr) - 1.0) - (double)lv;
    }
}

// The sum of the block's 256 accumulators, in a fixed tree; valid in lane 0.
__device__ __forceinline__ double post_block_sum(double acc, double* red) {
    red[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    const double r = red[0];
    __syncthreads();
    return r;
}

// grid (blocks per image, images); both dimensions stride.  VEC: chw % 4 == 0, m_stride % 4 == 0, every pointer 16-byte aligned.
// noise and z may be one buffer: no __restrict__ on them.  ws[n * gridDim.x + blockIdx.x]: the block's partial KL sum of image n.
template <bool VEC>
__global__ __launch_bounds__(256) void gaussian_posterior_kernel(const float* __restrict__ m, long long m_stride, int N, long long chw,
                                                                 const float* noise, float scale, float* __restrict__ logvar,
                                                                 float* __restrict__ stdo, float* __restrict__ var, float* z,
                                                                 double* __restrict__ ws) {
    __shared__ double red[256];
    const post_want w = {logvar != nullptr, stdo != nullptr, var != nullptr, z != nullptr, ws != nullptr};
    const long long tid = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long stride = (long long)gridDim.x * 256;
    for (int n = blockIdx.y; n < N; n += gridDim.y) {
        const float* mean = m + (long long)n * m_stride;
        const float* raw = mean + chw;
        const long long o = (long long)n * chw;
        double acc = 0.0;
        if (VEC) {
            const long long n4 = chw / 4;
            for (long long i = tid; i < n4; i += stride) {
                const long long at = 4 * i;
                const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
                const float4 mv = (w.z || w.kl) ? *reinterpret_cast<const float4*>(mean + at) : zero;
                const float4 rv = *reinterpret_cast<const float4*>(raw + at);
                const float4 nv = w.z ? *reinterpret_cast<const float4*>(noise + o + at) : zero;
                float4 lv, sd, vr, zz;
                post_one(mv.x, rv.x, nv.x, scale, w, lv.x, sd.x, vr.x, zz.x, acc);
                post_one(mv.y, rv.y, nv.y, scale, w, lv.y, sd.y, vr.y, zz.y, acc);
                post_one(mv.z, rv.z, nv.z, scale, w, lv.z, sd.z, vr.z, zz.z, acc);
                post_one(mv.w, rv.w, nv.w, scale, w, lv.w, sd.w, vr.w, zz.w, acc);
                if (w.lv) *reinterpret_cast<float4*>(logvar + o + at) = lv;
                if (w.sd) *reinterpret_cast<float4*>(stdo + o + at) = sd;
                if (w.vr) *reinterpret_cast<float4*>(var + o + at) = vr;
                if (w.z) *reinterpret_cast<float4*>(z + o + at) = zz;             // after the load of this lane's noise
            }
        } else {
            for (long long i = tid; i < chw; i += stride) {
                const float ms = (w.z || w.kl) ? mean[i] : 0.f;
                const float ns = w.z ? noise[o + i] : 0.f;
                float lv, sd, vr, zz;
                post_one(ms, raw[i], ns, scale, w, lv, sd, vr, zz, acc);
                if (w.lv) logvar[o + i] = lv;
                if (w.sd) stdo[o + i] = sd;
                if (w.vr) var[o + i] = vr;
                if (w.z) z[o + i] = zz;
            }
        }
        if (w.kl) {                                                              // uniform over the block
            const double s = post_block_sum(acc, red);
            if (threadIdx.x == 0) ws[(long long)n * gridDim.x + blockIdx.x] = s;
        }
    }
}

// kl[n] = (float)(0.5 * sum of image n's `per` partials): lane t adds partials t, t + 256, ... in that order, then the fixed tree.
__global__ __launch_bounds__(256) void gaussian_kl_combine_kernel(const double* __restrict__ ws, int per, int N, float* __restrict__ kl) {
    __shared__ double red[256];
    for (int n = blockIdx.x; n < N; n += gridDim.x) {
        double acc = 0.0;
        for (int i = threadIdx.x; i < per; i += 256) acc += ws[(long long)n * per + i];
        const double s = post_block_sum(acc, red);
        if (threadIdx.x == 0) kl[n] = (float)(0.5 * s);
    }
}

// grid (blocks per plane, planes); both dimensions stride.  b is read and written by the lane that owns the element only.
__global__ __launch_bounds__(256) void tile_blend_kernel(float* b, int planes, int Hb, int Wb, const float* __restrict__ a, int Ha, int ev,
                                                         const float* __restrict__ l, int Wl, int eh, float* __restrict__ out, int Hout,
                                                         int Wout, int oy, int ox, int row_limit) {
#pragma clang fp contract(off)
    const int hw = Hb * Wb;
    for (int p = blockIdx.y; p < planes; p += gridDim.y) {
        float* bp = b + (long long)p * hw;
        const float* ap = a ? a + (long long)p * Ha * Wb : nullptr;
        const float* lp = l ? l + (long long)p * Hb * Wl : nullptr;
        float* op = out ? out + (long long)p * Hout * Wout : nullptr;
        for (int i = blockIdx.x * 256 + threadIdx.x; i < hw; i += gridDim.x * 256) {
            const int y = i / Wb, x = i - y * Wb;
            float v = bp[i];
            if (ap && y < ev) {
                const double r = (double)y / (double)ev;
                const float w1 = (float)r, w0 = (float)(1.0 - r);
                const float t0 = ap[(long long)(Ha - ev + y) * Wb + x] * w0;
                const float t1 = v * w1;
                v = t0 + t1;
            }
            if (lp && x < eh) {
                const double r = (double)x / (double)eh;
                const float w1 = (float)r, w0 = (float)(1.0 - r);
                const float t0 = lp[(long long)y * Wl + (Wl - eh + x)] * w0;
                const float t1 = v * w1;
                v = t0 + t1;
            }
            if (ap || lp) bp[i] = v;
            if (op && y < row_limit && x < row_limit) op[(long long)(oy + y) * Wout + (ox + x)] = v;
        }
    }
}

static inline int post_blocks_per_image(int N, long long work) {
    const int ny = N < DP_VAE_MAX_BLOCKS ? N : DP_VAE_MAX_BLOCKS;
    const long long cap = DP_VAE_MAX_BLOCKS / ny > 1 ? DP_VAE_MAX_BLOCKS / ny : 1;
    const long long nb = (work + 255) / 256;
    return (int)(nb > cap ? cap : nb < 1 ? 1 : nb);
}

extern "C" long long dp_gaussian_posterior_ws(int N, long long chw) {
    if (N <= 0 || chw <= 0) return 0;
    return (long long)N * post_blocks_per_image(N, chw);            // the 4-byte path's count: the 16-byte path needs no more
}

extern "C" int dp_gaussian_posterior(const float* moments, long long m_stride, int N, long long chw, const float* noise, float scale,
                                     float* logvar, float* std, float* var, float* z, float* kl, double* kl_ws, void* stream) {
    if (N <= 0 || chw <= 0) return 0;
    if (!moments || (N > 1 && m_stride < 2 * chw) || (z && !noise) || (kl && !kl_ws)) return (int)hipErrorInvalidValue;
    if (!z) noise = nullptr;                                          // not read without a sample
    if (!kl) kl_ws = nullptr;
    const unsigned long long plane = 4ull * (unsigned long long)N * (unsigned long long)chw;
    const unsigned long long m_bytes = 4ull * ((unsigned long long)(N - 1) * (unsigned long long)(N > 1 ? m_stride : 0) + 2ull * chw);
    const void* outs[6] = {logvar, std, var, z, kl, kl_ws};
    const unsigned long long out_bytes[6] = {plane, plane, plane, plane, 4ull * N, 8ull * (unsigned long long)dp_gaussian_posterior_ws(N, chw)};
    for (int o = 0; o < 6; o++) {
        if (!outs[o]) continue;
        for (int p = o + 1; p < 6; p++)
            if (dp_bytes_overlap(outs[o], out_bytes[o], outs[p], out_bytes[p])) return (int)hipErrorInvalidValue;
        if (dp_bytes_overlap(outs[o], out_bytes[o], moments, m_bytes)) return (int)hipErrorInvalidValue;
        if (dp_bytes_overlap(outs[o], out_bytes[o], noise, plane) && !(o == 3 && (const void*)z == (const void*)noise)) return (int)hipErrorInvalidValue;
    }
    bool vec = chw % 4 == 0 && (N == 1 || m_stride % 4 == 0) && ((uintptr_t)moments & 15) == 0 && ((uintptr_t)noise & 15) == 0;
    for (int o = 0; o < 4; o++) vec = vec && ((uintptr_t)outs[o] & 15) == 0;
    const int bpi = post_blocks_per_image(N, vec ? chw / 4 : chw);
    const dim3 grid((unsigned)bpi, (unsigned)(N < DP_VAE_MAX_BLOCKS ? N : DP_VAE_MAX_BLOCKS));
    const hipStream_t st = (hipStream_t)stream;
    if (vec) VAE_LAUNCH((gaussian_posterior_kernel<true>), grid, dim3(256), 0, st, moments, m_stride, N, chw, noise, scale, logvar, std, var, z, kl_ws);
    else VAE_LAUNCH((gaussian_posterior_kernel<false>), grid, dim3(256), 0, st, moments, m_stride, N, chw, noise, scale, logvar, std, var, z, kl_ws);
    if (kl) VAE_LAUNCH(gaussian_kl_combine_kernel, dim3((unsigned)(N < DP_VAE_MAX_BLOCKS ? N : DP_VAE_MAX_BLOCKS)), dim3(256), 0, st, kl_ws, bpi, N, kl);
    return DP_LAUNCH_CHECK();
}

extern "C" int dp_tile_blend(float* b, int planes, int Hb, int Wb, const float* a, int Ha, int ev, const float* l, int Wl, int eh,
                             float* out, int Hout, int Wout, int oy, int ox, int row_limit, void* stream) {
    if (planes <= 0 || Hb <= 0 || Wb <= 0) return 0;
    if (!b || (long long)Hb * Wb >= (1ll << 29)) return (int)hipErrorInvalidValue;
    if (a && (Ha <= 0 || ev < 1 || ev > Ha || ev > Hb)) return (int)hipErrorInvalidValue;
    if (l && (Wl <= 0 || eh < 1 || eh > Wl || eh > Wb)) return (int)hipErrorInvalidValue;
    if (!a) { Ha = 0; ev = 0; }
    if (!l) { Wl = 0; eh = 0; }
    const int ch = Hb < row_limit ? Hb : row_limit, cw = Wb < row_limit ? Wb : row_limit;     // the crop
    if (out && (row_limit < 1 || oy < 0 || ox < 0 || Hout <= 0 || Wout <= 0 || (long long)oy + ch > Hout || (long long)ox + cw > Wout))
        return (int)hipErrorInvalidValue;
    const unsigned long long P = (unsigned long long)planes;
    const unsigned long long nb = 4ull * P * Hb * Wb, na = 4ull * P * Ha * Wb, nl = 4ull * P * Hb * Wl, no = out ? 4ull * P * Hout * Wout : 0;
    if (dp_bytes_overlap(b, nb, a, na) || dp_bytes_overlap(b, nb, l, nl) || dp_bytes_overlap(b, nb, out, no) || dp_bytes_overlap(out, no, a, na) ||
        dp_bytes_overlap(out, no, l, nl))
        return (int)hipErrorInvalidValue;
    if (!a && !l && !out) return 0;                                   // nothing to blend and nowhere to put it
    const long long hw = (long long)Hb * Wb;
    long long gx = (hw + 255) / 256;
    if (gx > 1024) gx = 1024;
    long long gy = DP_VAE_MAX_BLOCKS * 2 / gx;
    if (gy > planes) gy = planes;
    if (gy < 1) gy = 1;
    VAE_LAUNCH(tile_blend_kernel, dim3((unsigned)gx, (unsigned)gy), dim3(256), 0, (hipStream_t)stream, b, planes, Hb, Wb, a, Ha, ev, l, Wl, eh,
               out, Hout, Wout, oy, ox, row_limit);
    return DP_LAUNCH_CHECK();
}
