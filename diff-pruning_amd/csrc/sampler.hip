// The two elementwise kernels of the ddpm_exp sampler (ddpm_exp/functions/denoising.py, ddpm_exp/runners/diffusion.py:390-537):
//   dp_denoise_step  one update of generalized_steps (mode 0, denoising.py:23-29) or ddpm_steps (mode 1, denoising.py:53-65) in
//                    ONE pass: the next state and, when asked for, the x0 prediction the reference appends to x0_preds.  The
//                    reference runs about a dozen elementwise launches per step.
//   dp_image_to_u8   inverse_data_transform (datasets/__init__.py:177-186, shipped configs) + the byte conversion of
//                    torchvision.utils.save_image, fp32 NCHW -> uint8 NHWC: the FID job moves one byte per value to the host.
// Both are memory bound and small beside the UNet forward of a sampling step (about 12 MB at CIFAR batch 256): one pass and
// 16-byte accesses, nothing more.
//
// Rounding: every operation of the reference's expressions is rounded separately (clang fp contract(off): hipcc would otherwise
// fuse a * b + c into one v_fma_f32), the division is a true IEEE division, and the scalars arrive from the host, which computes
// them with 0-d fp32 torch ops in the reference's order (ddpm_exp_sampler.py) -- the way dp_ddpm_step takes its coefficients.
// dp_ddim_step / dp_ddpm_step (elementwise.hip) share no device code with this file and are unchanged.
#include "dp_common.h"
#include "dp_headtail_plan.h"

struct DenoiseCoef {
    float p0, p1, p2, p3, p4, p5;
};

// mode 0:  x0 = (x - e * s1) / s2;              next = s3 * x0 + c1 * z + c2 * e        (p0..p4 = s1, s2, s3, c1, c2)
// mode 1:  x0 = clamp(r1 * x - r2 * e, -1, 1);  next = (k0 * x0 + kx * x) / d + sig * z  (p0..p5 = r1, r2, k0, kx, d, sig)
// HAS_Z false: the noise term is absent (eta = 0, where c1 is exactly 0, and the t = 0 mask of ddpm_steps).
template <int MODE>
__device__ __forceinline__ float denoise_one(float x, float e, float z, bool has_z, const DenoiseCoef& c, float& x0) {
#pragma clang fp contract(off)
    if (MODE == 0) {
        const float es = e * c.p0;
        x0 = (x - es) / c.p1;
        float v = c.p2 * x0;
        if (has_z) {
            const float nz = c.p3 * z;
            v = v + nz;
        }
        const float ce = c.p4 * e;
        return v + ce;
    } else {
        const float a = c.p0 * x;
        const float b = c.p1 * e;
        x0 = fminf(fmaxf(a - b, -1.0f), 1.0f);
        const float m0 = c.p2 * x0;
        const float m1 = c.p3 * x;
        float v = (m0 + m1) / c.p4;
        if (has_z) {
            const float nz = c.p5 * z;
            v = v + nz;
        }
        return v;
    }
}

// The head / body / tail loop of dp_headtail.h (dp_ht_for), written out: this kernel pre-offsets its bases (x + head) where dp_ht_for's
// callers index x + at, and the dp_ht_for form of it timed slower than this one beyond the run-to-run spread in 2 of 6 comparisons
// (profiles/headtail_refactor.md), so the loop stays as it was.  `next` may be `x` itself (no __restrict__ on the two): an element is
// read and written by the same lane, in that order.  x0_out aliases nothing.
template <int MODE>
__global__ __launch_bounds__(256) void denoise_step_kernel(const float* x, const float* __restrict__ e, const float* __restrict__ z,
                                                           DenoiseCoef c, float* next, float* __restrict__ x0_out, long long n,
                                                           long long head) {
    const long long tid = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long stride = (long long)gridDim.x * 256;
    const long long n4 = (n - head) / 4;
    const bool has_z = z != nullptr;
    const float4* x4 = reinterpret_cast<const float4*>(x + head);
    const float4* e4 = reinterpret_cast<const float4*>(e + head);
    const float4* z4 = reinterpret_cast<const float4*>(has_z ? z + head : nullptr);
    float4* o4 = reinterpret_cast<float4*>(next + head);
    float4* p4 = reinterpret_cast<float4*>(x0_out ? x0_out + head : nullptr);
    for (long long i = tid; i < n4; i += stride) {
        const float4 xv = x4[i];
        const float4 ev = e4[i];
        const float4 zv = has_z ? z4[i] : make_float4(0.f, 0.f, 0.f, 0.f);
        float4 ov, pv;
        ov.x = denoise_one<MODE>(xv.x, ev.x, zv.x, has_z, c, pv.x);
        ov.y = denoise_one<MODE>(xv.y, ev.y, zv.y, has_z, c, pv.y);
        ov.z = denoise_one<MODE>(xv.z, ev.z, zv.z, has_z, c, pv.z);
        ov.w = denoise_one<MODE>(xv.w, ev.w, zv.w, has_z, c, pv.w);
        o4[i] = ov;
        if (x0_out) p4[i] = pv;
    }
    const long long ns = n - 4 * n4;                  // the scalar head and tail (everything when head == n)
    for (long long j = tid; j < ns; j += stride) {
        const long long i = j < head ? j : 4 * n4 + j;
        float p;
        const float v = denoise_one<MODE>(x[i], e[i], has_z ? z[i] : 0.f, has_z, c, p);
        next[i] = v;
        if (x0_out) x0_out[i] = p;
    }
}

extern "C" int dp_denoise_step(const float* x, const float* eps, const float* z, int mode, float p0, float p1, float p2, float p3,
                               float p4, float p5, float* next, float* x0_out, long long n, void* stream) {
    if (n <= 0) return 0;
    if (!x || !eps || !next || (mode != 0 && mode != 1)) return (int)hipErrorInvalidValue;
    const void* ptrs[5] = {x, eps, next, z, x0_out};
    const long long head = dp_ht_head(n, ptrs, 5);
    const unsigned grid = dp_ht_blocks(n, head, DP_DENOISE_MAX_BLOCKS);
    const DenoiseCoef c{p0, p1, p2, p3, p4, p5};
    if (mode == 0)
        DP_LAUNCH(denoise_step_kernel<0>, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, eps, z, c, next, x0_out, n, head);
    else
        DP_LAUNCH(denoise_step_kernel<1>, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, eps, z, c, next, x0_out, n, head);
    return DP_LAUNCH_CHECK();
}

// ---------------------------------------------------------------------------------------------
// fp32 [N][C][H][W] (image stride x_img_stride floats) -> uint8 [N][H][W][C], the inverse of dp_u8_to_float:
//   v = rescaled ? clamp((x + 1) / 2, 0, 1) : clamp(x, 0, 1)           inverse_data_transform, datasets/__init__.py:177-186
//   byte = (unsigned char) clamp(v * 255 + 0.5, 0, 255)                 save_image: mul(255).add_(0.5).clamp_(0, 255).to(uint8)
// The multiply and the add are rounded separately, so the byte equals the torch fp32 expression bit for bit.
// torchvision is absent from the build machine AND from the reference tree: save_image's formula above is recalled, not read,
// and parity with torchvision itself is unpinned.  A NaN input gives byte 0 (fmaxf drops it); torch leaves that cast undefined.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned image_byte(float x, int rescaled) {
#pragma clang fp contract(off)
    if (rescaled) {
        const float s = x + 1.0f;
        x = s / 2.0f;
    }
    const float v = fminf(fmaxf(x, 0.0f), 1.0f);
    const float m = v * 255.0f;
    const float r = m + 0.5f;
    return (unsigned)fminf(fmaxf(r, 0.0f), 255.0f);
}

// VEC: one lane per 4 consecutive pixels of one image: C 16-byte loads, C 4-byte stores (C <= 4, HW % 4 == 0, aligned).
// else: one lane per output byte.
template <bool VEC>
__global__ __launch_bounds__(256) void image_to_u8_kernel(const float* __restrict__ x, long long x_img_stride, int N, int C,
                                                          long long HW, int rescaled, unsigned char* __restrict__ out) {
    const long long tid = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long stride = (long long)gridDim.x * 256;
    if (VEC) {
        const long long q = HW / 4;
        const long long total = (long long)N * q;
        for (long long i = tid; i < total; i += stride) {
            const long long n = i / q;
            const long long hw = (i - n * q) * 4;
            unsigned b[16];
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                if (c < C) {
                    const float4 v = *reinterpret_cast<const float4*>(x + n * x_img_stride + (long long)c * HW + hw);
                    b[0 * 4 + c] = image_byte(v.x, rescaled);
                    b[1 * 4 + c] = image_byte(v.y, rescaled);
                    b[2 * 4 + c] = image_byte(v.z, rescaled);
                    b[3 * 4 + c] = image_byte(v.w, rescaled);
                }
            }
            // the 4 * C bytes of pixels hw .. hw + 3 in pixel-major order, packed into C little-endian words
            unsigned* o = reinterpret_cast<unsigned*>(out + (n * HW + hw) * C);
            unsigned word = 0;
            int k = 0;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    if (c < C) {
                        word |= b[p * 4 + c] << (8 * (k & 3));
                        if ((++k & 3) == 0) {
                            o[(k >> 2) - 1] = word;
                            word = 0;
                        }
                    }
                }
            }
        }
    } else {
        const long long per = (long long)C * HW;
        const long long total = (long long)N * per;
        for (long long i = tid; i < total; i += stride) {
            const long long n = i / per;
            const long long r = i - n * per;
            const long long hw = r / C;
            const int c = (int)(r - hw * C);
            out[i] = (unsigned char)image_byte(x[n * x_img_stride + (long long)c * HW + hw], rescaled);
        }
    }
}

extern "C" int dp_image_to_u8(const float* x, long long x_img_stride, int N, int C, int H, int W, int rescaled,
                              unsigned char* out, void* stream) {
    const long long HW = (long long)H * W;
    const long long total = (long long)N * C * HW;
    if (total <= 0) return 0;
    if (!x || !out || x_img_stride < (long long)C * HW) return (int)hipErrorInvalidValue;
    const bool vec = C <= 4 && HW % 4 == 0 && x_img_stride % 4 == 0 && ((uintptr_t)x & 15) == 0 && ((uintptr_t)out & 3) == 0;
    const long long work = vec ? (long long)N * (HW / 4) : total;
    const long long nb = (work + 255) / 256;
    const unsigned grid = (unsigned)(nb > DP_DENOISE_MAX_BLOCKS ? DP_DENOISE_MAX_BLOCKS : nb < 1 ? 1 : nb);
    if (vec)
        DP_LAUNCH(image_to_u8_kernel<true>, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, x_img_stride, N, C, HW, rescaled, out);
    else
        DP_LAUNCH(image_to_u8_kernel<false>, dim3(grid), dim3(256), 0, (hipStream_t)stream, x, x_img_stride, N, C, HW, rescaled, out);
    return DP_LAUNCH_CHECK();
}
