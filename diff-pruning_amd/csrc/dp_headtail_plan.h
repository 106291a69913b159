// The host rule of the head / body / tail step kernels (dp_headtail.h; stated once in include/dp_hip.h, "the head / body / tail
// access rule").  Integer arithmetic on pointer VALUES: nothing is dereferenced, no HIP header is needed, and a plain host compiler
// builds it (tests/test_headtail_plan_cpu.py).  Not the all-or-nothing VEC rule of ema.hip, optim.hip and stage.hip: that one is
// dp_flat_grid (dp_common.h).
#pragma once
#include <stdint.h>

// [a, a + la) and [b, b + lb) share a byte (the same buffer included).  A null pointer and an empty range share none.
static inline bool dp_bytes_overlap(const void* a, unsigned long long la, const void* b, unsigned long long lb) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a && b && la && lb && a0 < b0 + lb && b0 < a0 + la;
}

// The scalar head of n fp32 elements: 0 .. 3 elements (at most n) when every non-null pointer shares one 4-byte-aligned phase
// modulo 16, so that pointer + head is 16-byte aligned for all of them; otherwise n: everything is scalar.
static inline long long dp_ht_head(long long n, const void* const* ptrs, int count) {
    uintptr_t a = 16;
    for (int i = 0; i < count; ++i) {
        if (!ptrs[i]) continue;
        const uintptr_t v = (uintptr_t)ptrs[i] & 15;
        if (a == 16) a = v;
        if (v != a || (v & 3) != 0) return n;
    }
    const long long head = a == 16 ? 0 : (long long)(((16 - a) & 15) / 4);
    return head > n ? n : head;
}

// Lanes wanted: one per float4 group or one per scalar element, whichever loop is longer.
static inline long long dp_ht_work(long long n, long long head) {
    const long long n4 = (n - head) / 4;
    return n4 > n - 4 * n4 ? n4 : n - 4 * n4;
}

// Blocks of 256 lanes for that, in [1, cap].
static inline unsigned dp_ht_blocks(long long n, long long head, long long cap) {
    const long long nb = (dp_ht_work(n, head) + 255) / 256;
    return (unsigned)(nb > cap ? cap : nb < 1 ? 1 : nb);
}
