// LitEma's update on its own (ldm/modules/ema.py:40-44): s -= one_minus_decay * (s - p) over flat fp32 buffers, for the batches of
// a gradient-accumulation window that end without an optimizer step (ddpm.py:366-368 runs the EMA at the end of EVERY batch).
// The expression (dp_lit_ema) and the alignment and grid rule (dp_flat_grid) are the ones dp_adamw_ema uses (optim.hip
// adamw_one); both live in dp_common.h, so a shadow kept by this kernel and one kept by the fused update agree bit for bit
// (tests/test_train_state_gpu.py pins it).  The float4 / tail loop is kept per kernel: sharing it through a functor changed the
// address arithmetic hipcc generates.  8 B read + 4 B written per element: 16-byte accesses per lane when both pointers are
// 16-byte aligned, 4-byte accesses for the n % 4 tail and for unaligned views.
#include "dp_common.h"

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
            si.x = dp_lit_ema(si.x, pi.x, omd);
            si.y = dp_lit_ema(si.y, pi.y, omd);
            si.z = dp_lit_ema(si.z, pi.z, omd);
            si.w = dp_lit_ema(si.w, pi.w, omd);
            s4[i] = si;
        }
    }
    for (long long i = 4 * n4 + tid; i < n; i += stride)         // the scalar tail (everything when !VEC)
        s[i] = dp_lit_ema(s[i], p[i], omd);
}

extern "C" int dp_ema_update(float* s, const float* p, long long n, float one_minus_decay, void* stream) {
    if (n <= 0) return 0;
    if (!s || !p) return (int)hipErrorInvalidValue;
    bool vec;
    const unsigned nb = dp_flat_grid((uintptr_t)s | (uintptr_t)p, n, &vec);
    if (vec)
        DP_LAUNCH(ema_update_kernel<true>, dim3(nb), dim3(256), 0, (hipStream_t)stream, s, p, n, one_minus_decay);
    else
        DP_LAUNCH(ema_update_kernel<false>, dim3(nb), dim3(256), 0, (hipStream_t)stream, s, p, n, one_minus_decay);
    return DP_LAUNCH_CHECK();
}
