// The device loop of the head / body / tail step kernels (ldm_sampler.hip, dpm_solver.hip, unipc.hip, threshold.hip; sampler.hip
// writes the same loop out); the host rule that chooses `head` and the grid is dp_headtail_plan.h.  A new elementwise step kernel
// starts from these two.
#pragma once
#include "dp_common.h"
#include "dp_headtail_plan.h"

// Elements [0, head) and [head + 4 n4, n) take 4-byte accesses, the n4 = (n - head) / 4 groups between them 16-byte ones: vec(at) for
// the group at elements at .. at + 3, at = head + 4 i, then one(i) for each scalar element, both strided over the lanes (tid, stride).
// The launcher chooses head so that every pointer + head is 16-byte aligned, or head = n (all scalar).  A callback loads everything
// it reads before it stores anything: the aliases the kernels permit (an output that is one of the inputs) rest on that.
template <typename V, typename O>
__device__ __forceinline__ void dp_ht_for(long long n, long long head, long long tid, long long stride, V&& vec, O&& one) {
    const long long n4 = (n - head) / 4;
    for (long long i = tid; i < n4; i += stride) vec(head + 4 * i);
    const long long ns = n - 4 * n4;                  // the scalar head and tail (everything when head == n)
    for (long long j = tid; j < ns; j += stride) one(j < head ? j : 4 * n4 + j);
}

// p[at .. at + 3] / p[i], or zeros without touching p when the kernel does not read it
__device__ __forceinline__ float4 dp_ld4(const float* p, long long at, bool use) {
    return use ? *reinterpret_cast<const float4*>(p + at) : make_float4(0.f, 0.f, 0.f, 0.f);
}

__device__ __forceinline__ float dp_ld1(const float* p, long long i, bool use) { return use ? p[i] : 0.f; }

__device__ __forceinline__ void dp_st4(float* p, long long at, const float4& v) { *reinterpret_cast<float4*>(p + at) = v; }
