// The stage study's snapshot kernel (ddpm_exp/prune_ssim.py: one prune per stage s from the gradients of timesteps 0 .. s - 1).
//   dp_fold_sum   out[i] = ((srcs[0][i] + srcs[1][i]) + srcs[2][i]) + srcs[3][i], k = 1 .. 4 sources, plain fp32 adds in exactly
//                 that order -- the sum HipSweepStep.finish() forms with its chain of `main += pipeline` launches -- written to a
//                 buffer of its own: no source is written, so a sweep that is snapshotted goes on bit for bit as one that is not.
// The k source pointers travel BY VALUE in the kernel arguments (FoldSrcs): no device-side pointer table, no staging copy, nothing
// to keep alive, so the launch can be enqueued between two sweep timesteps (and would be safe under stream capture).
// Alignment and grid rule: dp_flat_grid (dp_common.h), as dp_ema_update / dp_adamw_ema: 16-byte accesses per lane when `out` and
// every source are 16-byte aligned and n >= 4, 4-byte accesses for the n % 4 tail and for unaligned views; at most 4096 blocks,
// grid-stride beyond.  4 k B read + 4 B written per element, one pass.
#include "dp_common.h"

// The launch macro of this file: the body of the library's own (dp_common.h) under a name of its own, so that the launch sites of
// this file are tabled by this file's test module (tests/test_stage_study_gpu.py), as evalmetrics.hip and prune_global.hip do.
#define ST_LAUNCH(k, ...) do { dp_launch_names[dp_launches++ & (DP_LAUNCH_RING - 1)] = #k; hipLaunchKernelGGL(k, __VA_ARGS__); } while (0)

#define ST_MAX_SRCS 4
struct FoldSrcs { const float* p[ST_MAX_SRCS]; };

template <int K, bool VEC>
__global__ __launch_bounds__(256) void fold_sum_kernel(float* __restrict__ out, FoldSrcs s, long long n) {
    const long long tid = (long long)blockIdx.x * 256 + threadIdx.x;
    const long long stride = (long long)gridDim.x * 256;
    const long long n4 = VEC ? n / 4 : 0;
    if (VEC) {
        float4* o4 = reinterpret_cast<float4*>(out);
        for (long long i = tid; i < n4; i += stride) {
            float4 v[K];
#pragma unroll
            for (int j = 0; j < K; ++j) v[j] = reinterpret_cast<const float4*>(s.p[j])[i];       // K independent loads in flight
            float4 a = v[0];
#pragma unroll
            for (int j = 1; j < K; ++j) { a.x = a.x + v[j].x; a.y = a.y + v[j].y; a.z = a.z + v[j].z; a.w = a.w + v[j].w; }
            o4[i] = a;
        }
    }
    for (long long i = 4 * n4 + tid; i < n; i += stride) {        // the scalar tail (everything when !VEC)
        float a = s.p[0][i];
#pragma unroll
        for (int j = 1; j < K; ++j) a = a + s.p[j][i];
        out[i] = a;
    }
}

extern "C" int dp_fold_sum(float* out, const float* const* srcs, int k, long long n, void* stream) {
    if (n <= 0) return 0;
    if (!out || !srcs || k < 1 || k > ST_MAX_SRCS) return (int)hipErrorInvalidValue;
    FoldSrcs s{};
    uintptr_t bits = (uintptr_t)out;
    const uintptr_t o0 = (uintptr_t)out, o1 = o0 + 4ull * (unsigned long long)n;
    for (int j = 0; j < k; ++j) {
        if (!srcs[j]) return (int)hipErrorInvalidValue;
        const uintptr_t s0 = (uintptr_t)srcs[j], s1 = s0 + 4ull * (unsigned long long)n;
        if (o0 < s1 && s0 < o1) return (int)hipErrorInvalidValue;             // `out` overlaps a source: the sources are read-only
        s.p[j] = srcs[j];
        bits |= s0;
    }
    bool vec;
    const unsigned nb = dp_flat_grid(bits, n, &vec);
    const hipStream_t st = (hipStream_t)stream;
    // one site per instantiation: the launch ring keeps the stringised kernel expression of the site that launched
    switch (2 * k + (vec ? 1 : 0)) {
        case 2: ST_LAUNCH((fold_sum_kernel<1, false>), dim3(nb), dim3(256), 0, st, out, s, n); break;
        case 3: ST_LAUNCH((fold_sum_kernel<1, true>), dim3(nb), dim3(256), 0, st, out, s, n); break;
        case 4: ST_LAUNCH((fold_sum_kernel<2, false>), dim3(nb), dim3(256), 0, st, out, s, n); break;
        case 5: ST_LAUNCH((fold_sum_kernel<2, true>), dim3(nb), dim3(256), 0, st, out, s, n); break;
        case 6: ST_LAUNCH((fold_sum_kernel<3, false>), dim3(nb), dim3(256), 0, st, out, s, n); break;
        case 7: ST_LAUNCH((fold_sum_kernel<3, true>), dim3(nb), dim3(256), 0, st, out, s, n); break;
        case 8: ST_LAUNCH((fold_sum_kernel<4, false>), dim3(nb), dim3(256), 0, st, out, s, n); break;
        default: ST_LAUNCH((fold_sum_kernel<4, true>), dim3(nb), dim3(256), 0, st, out, s, n); break;
    }
    return DP_LAUNCH_CHECK();
}
