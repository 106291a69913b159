// Prints dp_ht_head / dp_ht_blocks / dp_bytes_overlap (csrc/dp_headtail_plan.h) for a fixed case list; tests/test_headtail_plan_cpu.py
// builds this with the host compiler, runs it and compares every line with a Python restatement of the rule.  The pointers are made
// up from integers: the functions under test are arithmetic on pointer values and dereference nothing.
//   H <n> <p0,p1,...> <head> <blocks at cap 1> <blocks at cap 4096>
//   O <a> <la> <b> <lb> <0|1>
#include <stdio.h>

#include "dp_headtail_plan.h"

static const void* ptr(unsigned long long v) { return (const void*)(uintptr_t)v; }

static void head_case(long long n, const unsigned long long* vals, int count) {
    const void* ptrs[8];
    printf("H %lld ", n);
    for (int i = 0; i < count; ++i) {
        ptrs[i] = ptr(vals[i]);
        printf("%s%llu", i ? "," : "", vals[i]);
    }
    const long long head = dp_ht_head(n, ptrs, count);
    printf(" %lld %u %u\n", head, dp_ht_blocks(n, head, 1), dp_ht_blocks(n, head, 4096));
}

static void overlap_case(unsigned long long a, unsigned long long la, unsigned long long b, unsigned long long lb) {
    printf("O %llu %llu %llu %llu %d\n", a, la, b, lb, dp_bytes_overlap(ptr(a), la, ptr(b), lb) ? 1 : 0);
}

int main() {
    const long long ns[8] = {1, 2, 3, 4, 5, 77, 1003, 4ll * 4096 * 256 + 4099};
    const unsigned long long base = 0x7f0000001000ull;           // 16-byte aligned
    for (int k = 0; k < 8; ++k) {
        const long long n = ns[k];
        for (unsigned long long phase = 0; phase < 16; ++phase) {
            const unsigned long long one = base + phase;
            head_case(n, &one, 1);
        }
        for (int count = 2; count <= 6; ++count) {
            for (unsigned long long phase = 0; phase < 16; phase += 4) {
                unsigned long long v[6];
                for (int i = 0; i < count; ++i) v[i] = base + 0x10000ull * i + phase;
                head_case(n, v, count);                              // all of one phase
                for (int odd = 0; odd < count; odd += count - 1) {   // the first or the last differs: by 4 bytes, by 2 bytes
                    v[odd] += 4;
                    head_case(n, v, count);
                    v[odd] -= 2;
                    head_case(n, v, count);
                    v[odd] -= 2;
                }
                for (int null_at = 0; null_at < count; null_at += (count > 2 ? count / 2 : 1)) {    // front, middle, end
                    const unsigned long long keep = v[null_at];
                    v[null_at] = 0;
                    head_case(n, v, count);
                    v[null_at] = keep;
                }
                const unsigned long long keep = v[count - 1];
                v[count - 1] = 0;
                head_case(n, v, count);
                v[count - 1] = keep;
            }
            const unsigned long long nulls[6] = {0, 0, 0, 0, 0, 0};
            head_case(n, nulls, count);
        }
    }
    overlap_case(1000, 100, 2000, 100);      // disjoint
    overlap_case(2000, 100, 1000, 100);
    overlap_case(1000, 100, 1100, 100);      // touching
    overlap_case(1100, 100, 1000, 100);
    overlap_case(1000, 101, 1100, 100);      // one shared byte
    overlap_case(1100, 100, 1000, 101);
    overlap_case(1000, 100, 1000, 100);      // identical
    overlap_case(1000, 400, 1100, 4);        // one inside the other
    overlap_case(0, 100, 1000, 100);         // one null pointer
    overlap_case(1000, 100, 0, 100);
    overlap_case(0, 100, 0, 100);            // both null
    overlap_case(1000, 400, 1100, 0);        // an empty range shares no byte
    overlap_case(1100, 0, 1000, 400);
    return 0;
}
