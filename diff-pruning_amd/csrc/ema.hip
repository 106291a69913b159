// LitEma's update on its own (ldm/modules/ema.py:40-44): s -= one_minus_decay * (s - p) over flat fp32 buffers, for the batches of
// a gradient-accumulation window that end without an optimizer step (ddpm.py:366-368 runs the EMA at the end of EVERY batch).
// The expression is the EMA half of dp_adamw_ema (optim.hip adamw_one), rounded after every operation, so a shadow kept by
// this kernel and one kept by the fused update agree bit for bit.  8 B read + 4 B written per element: 16-byte accesses per
// lane when both pointers are 16-byte aligned, 4-byte accesses for the n % 4 tail and for unaligned views.
#include "dp_common.h"

__device__ __forceinline__ float ema_one(float s, float p, float omd) {
#pragma clang fp contract(off)      // LitEma rounds the difference, the product and the subtraction separately
    return s - omd * (s - p);
}

template <bool VEC>
__global__ __launch_bounds__(256) void ema_update_kernel(float* __restrict__ s, const float* __restrict__ p, long long n, float omd) {
    const long long tid = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long stride = (long long)gridDim.x * 256;
    const long long n4 = VEC ? n / 4 : 0;
    if (VEC) {
        float4* s4 = reinterpret_cast<float4*>(s);
        const float4* p4 = reinterpret_cast<const float4*>(p);
        for (long long i = tid; i < n4; i += stride) {
            float4 si = s4[i];
            const float4 pi = p4[i];
            si.x = ema_one(si.x, pi.x, omd);
            si.y = ema_one(si.y, pi.y, omd);
            si.z = ema_one(si.z, pi.z, omd);
            si.w = ema_one(si.w, pi.w, omd);
            s4[i] = si;
        }
    }
    for (long long i = 4 * n4 + tid; i < n; i += stride)         // the scalar tail (everything when !VEC)
        s[i] = ema_one(s[i], p[i], omd);
}

extern "C" int dp_ema_update(float* s, const float* p, long long n, float one_minus_decay, void* stream) {
    if (n <= 0) return 0;
    if (!s || !p) return (int)hipErrorInvalidValue;
    const bool vec = ((((uintptr_t)s) | ((uintptr_t)p)) & 15) == 0 && n >= 4;
    long long nb = ((vec ? n / 4 : n) + 255) / 256;
    if (nb > 4096) nb = 4096;                            // the cap of dp_adamw_ema: 16 blocks of 256 per CU, grid-stride beyond
    if (nb < 1) nb = 1;
    if (vec)
        DP_LAUNCH(ema_update_kernel<true>, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, s, p, n, one_minus_decay);
    else
        DP_LAUNCH(ema_update_kernel<false>, dim3((unsigned)nb), dim3(256), 0, (hipStream_t)stream, s, p, n, one_minus_decay);
    return DP_LAUNCH_CHECK();
}
