#!/usr/bin/env python3
"""The evaluation metrics beside FID (diff-pruning_amd/metrics.py: precision_recall, kernel_inception_distance, inception_score) at
the size the LDM numbers are read at: seeded 50 000 x 2048 features against 50 000 x 2048 and 50 000 x 1008 logits, one MI355X.
Appends one JSON line per figure to --out (default profiles/eval_metrics_bench.jsonl).
  wall            median of --repeats runs of each of the three functions (host clock around work that ends on the host: each returns
                  Python floats), after one warm run, and the peak reserved device memory of a run
  gemm_share      the same four blocked passes of precision_recall with the products alone (ops.bmm_nt), as a share of its wall time
  row_reduction   em_knn_merge_kernel<4> and em_inside_ball_kernel on one full G block (4096 x 50 000): device events around --iters
                  back-to-back launches; bytes/s of the G block read, as a share of the 6.3 TB/s achievable HBM rate.  The inside
                  kernel is timed on negative squared radii (no row ever ends early: every element is read)
  reference       the reference's own procedure on the same device and features: torch.cdist in 10 000-row batches, kthvalue for the
                  radii, (d <= r).any for the flags
    python tools/bench_eval_metrics.py [--n 50000] [--repeats 3] [--iters 20]"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
HBM = 6.3e12


def wall(fn, repeats):
    fn()                                                      # code objects, allocator
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_reserved()
    runs = []
    for _ in range(repeats):
        t0 = time.time()
        r = fn()
        torch.cuda.synchronize()
        runs.append(time.time() - t0)
    return statistics.median(runs), runs, torch.cuda.max_memory_reserved() - base, r


def events_ms(fn, iters):
    for _ in range(3):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def reference_prc(f1, f2, k=3, batch=10000):
    def radii(f):
        out = []
        for lo in range(0, f.shape[0], batch):
            out.append(torch.cdist(f[lo:lo + batch], f).kthvalue(k + 1, dim=1).values)
        return torch.cat(out)

    def inside(b, a, r):
        out = []
        for lo in range(0, b.shape[0], batch):
            out.append((torch.cdist(b[lo:lo + batch], a) <= r[None, :]).any(1))
        return torch.cat(out)
    p = inside(f1, f2, radii(f2)).float().mean().item()
    r = inside(f2, f1, radii(f1)).float().mean().item()
    return {'precision': p, 'recall': r}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--n', type=int, default=50000)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'eval_metrics_bench.jsonl'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_eval_metrics needs an MI355X: there is no CPU path to time')
    M = importlib.import_module('diff-pruning_amd.metrics')
    dev = torch.device('cuda')
    n, d, c = args.n, 2048, 1008
    g = torch.Generator(device=dev).manual_seed(2020)
    # pool3-like rows: non-negative (ReLU + average pool), a shared mean, the second set a little narrower and shifted
    f1 = torch.randn(n, d, generator=g, device=dev).abs_()
    f2 = torch.randn(n, d, generator=g, device=dev).abs_().mul_(0.9).add_(0.05)
    logits = torch.randn(n, c, generator=g, device=dev).mul_(3.0)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def emit(**kw):
        kw.update(tool='bench_eval_metrics', n=n, d=d, repeats=args.repeats)
        print(json.dumps(kw), flush=True)
        with open(args.out, 'a') as f:                        # as it goes: a later figure that fails keeps the earlier ones
            f.write(json.dumps(kw) + '\n')

    def figure(name, fn):
        med, runs, peak, r = wall(fn, args.repeats)
        emit(figure='wall', function=name, seconds=round(med, 4), runs_seconds=[round(t, 4) for t in runs], peak_reserved_mib=round(peak / 2 ** 20, 1),
             result={k: round(v, 6) for k, v in r.items()})
        return med

    t_prc = figure('precision_recall', lambda: M.precision_recall(f1, f2, 3))
    figure('kernel_inception_distance', lambda: M.kernel_inception_distance(f1, f2))
    figure('inception_score', lambda: M.inception_score(logits))

    def gemm_only():
        for x, y in ((f2, f2), (f1, f2), (f1, f1), (f2, f1)):
            for _ in M._gram_blocks(x, y, 4096, 65536):
                pass
        return {}
    t_gemm, runs, _, _ = wall(gemm_only, args.repeats)
    emit(figure='gemm_share', seconds=round(t_gemm, 4), runs_seconds=[round(t, 4) for t in runs], share_of_precision_recall=round(t_gemm / t_prc, 4),
         tflops=round(4 * 2.0 * n * n * d / t_gemm / 1e12, 2))

    rows = min(4096, n)
    G = M.ops.bmm_nt(f1[:rows].unsqueeze(0), f2.unsqueeze(0))[0]
    xn, yn = M.row_norms2(f1[:rows]), M.row_norms2(f2)
    best = torch.empty((rows, 4), dtype=torch.float32, device=dev)
    hit = torch.zeros(rows, dtype=torch.int32, device=dev)
    never = torch.full((n,), -1.0, dtype=torch.float32, device=dev)
    nbytes = 4.0 * rows * n
    for name, fn in (('em_knn_merge_kernel<4>', lambda: M.knn_merge(G, xn, yn, best, True)),
                     ('em_inside_ball_kernel', lambda: M.inside_ball(G, xn, yn, never, hit))):
        ms = events_ms(fn, args.iters)
        emit(figure='row_reduction', kernel=name, block=[rows, n], ms=round(ms, 4), g_bytes_per_s=round(nbytes / ms * 1e3, 0),
             share_of_6p3_tbps=round(nbytes / ms * 1e3 / HBM, 4), iters=args.iters)
    assert int(hit.sum()) == 0
    del G

    med, runs, peak, r = wall(lambda: reference_prc(f1, f2), args.repeats)
    emit(figure='reference', procedure='torch.cdist in 10000-row batches + kthvalue / any', seconds=round(med, 4),
         runs_seconds=[round(t, 4) for t in runs], peak_reserved_mib=round(peak / 2 ** 20, 1), result={k: round(v, 6) for k, v in r.items()})


if __name__ == '__main__':
    main()
