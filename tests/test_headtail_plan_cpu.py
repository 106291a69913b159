"""The host rule of the head / body / tail step kernels (csrc/dp_headtail_plan.h: dp_ht_head, dp_ht_blocks, dp_bytes_overlap) against a
Python restatement, on the host (`-m "not gpu"`).  The GPU tests of those kernels pin their results bit for bit at every alignment but
cannot see which access width ran: a head rule that wrongly returned n (all scalar) would pass every one of them.  This test pins it.
tests/headtail_plan_main.cpp is built with the host compiler and UndefinedBehaviorSanitizer and run as a child process."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))


def head(n, ptrs):
    """0 .. 3 scalar elements (at most n) when every non-null pointer shares one 4-byte-aligned phase modulo 16, else n."""
    phases = {p % 16 for p in ptrs if p}
    if not phases:
        return 0
    if len(phases) > 1 or next(iter(phases)) % 4:
        return n
    return min(n, (16 - next(iter(phases))) % 16 // 4)


def blocks(n, head_, cap):
    """ceil(max(n4, n - 4 n4) / 256) in [1, cap], n4 = (n - head) // 4 float4 groups."""
    n4 = (n - head_) // 4
    return min(cap, max(1, -(-max(n4, n - 4 * n4) // 256)))


def overlap(a, la, b, lb):
    return bool(a and b and set(range(a, a + la)) & set(range(b, b + lb)))


def test_plan_header_matches_the_rule(tmp_path):
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++') or '/opt/rocm/llvm/bin/clang++'
    exe = str(tmp_path / 'headtail_plan')
    subprocess.run([cxx, '-std=c++17', '-O1', '-Wall', '-Werror', '-fsanitize=undefined', '-fno-sanitize-recover=all',
                    '-I' + os.path.join(ROOT, 'diff-pruning_amd', 'csrc'), os.path.join(HERE, 'headtail_plan_main.cpp'), '-o', exe],
                   check=True)
    out = subprocess.run([exe], check=True, stdout=subprocess.PIPE, universal_newlines=True).stdout.split('\n')
    lines = [ln.split() for ln in out if ln]
    heads = [ln for ln in lines if ln[0] == 'H']
    overlaps = [ln for ln in lines if ln[0] == 'O']
    assert len(heads) + len(overlaps) == len(lines)
    seen_n, seen_counts, widths = set(), set(), set()
    for _, n, ptrs, got_head, got_b1, got_b4096 in heads:
        n, ptrs = int(n), [int(p) for p in ptrs.split(',')]
        h = head(n, ptrs)
        assert (int(got_head), int(got_b1), int(got_b4096)) == (h, blocks(n, h, 1), blocks(n, h, 4096)), (n, ptrs)
        seen_n.add(n)
        seen_counts.add(len(ptrs))
        widths.add(h == n)
    # the case list the program is meant to walk: every n, 1 .. 6 pointers, every phase of one pointer, launches of both widths
    assert seen_n == {1, 2, 3, 4, 5, 77, 1003, 4 * 4096 * 256 + 4099} and seen_counts == {1, 2, 3, 4, 5, 6} and widths == {True, False}
    assert {p[0] % 16 for _, _, ps, *_ in heads for p in [[int(v) for v in ps.split(',')]] if len(p) == 1} == set(range(16))
    assert any(all(int(v) == 0 for v in ps.split(',')) for _, _, ps, *_ in heads)
    assert any(int(b) == 4096 for *_, b in heads) and any(int(b) == 1 for *_, b in heads)
    answers = set()
    for _, a, la, b, lb, got in overlaps:
        a, la, b, lb = int(a), int(la), int(b), int(lb)
        assert int(got) == overlap(a, la, b, lb), (a, la, b, lb)
        answers.add(int(got))
    assert len(overlaps) >= 11 and answers == {0, 1}
