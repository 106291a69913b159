#!/usr/bin/env python3
"""Dynamic thresholding (diff-pruning_amd/diffusion.py, csrc/threshold.hip) on one MI355X, seeded weights.
Appends one JSON line per figure to --out (default profiles/threshold_bench.jsonl).  Nothing here is bounded: these are reports.
  pipeline_step   ms per step of a --steps-step DDIMPipeline on the CIFAR UNet at B = --batch with thresholding
                  (sample_max_value 2.0), beside the clipped pipeline from the same run: wall clock around a pipeline call that ends
                  in a device synchronise (the read-back of the images), after one warm call; median of --repeats.
  quantile, step, fused   dp_x0_abs_quantile, dp_x0_step (thresholded, from a given table) and the fused dp_x0_threshold_step alone
                  at [256, 3, 32, 32] and [16, 3, 256, 256] (an epsilon model, DDIM update): device events around --calls
                  back-to-back calls, median of --repeats, in microseconds per call, beside the reference's eager
                  `_threshold_sample` (torch.quantile: a sort of every image) plus its step expressions on the same device and
                  buffers.  Algorithmic bytes (quantile: 8 per element and pass over x and m -- one pass on the LDS route, five on
                  the multi-block one, which recomputes x0 from x and m in every pass instead of writing the keys once; step: 8
                  read, 8 written with x0_out; fused: 16 read, 8 written) over the time as a share of the 6.3 TB/s achievable HBM rate.
  routes          both quantile routes at a row length both accept (3 x 64 x 64).
    python tools/bench_threshold.py [--batch 256] [--repeats 3] [--calls 100] [--steps 100]"""
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
HBM_ACHIEVABLE = 6.3e12                                   # bytes / s
SA, SB = 0.8, 0.6
COEF = dict(sa=SA, sb=SB, c0=0.9, c1=0.3, cz=0.0, ratio=0.995, max_value=2.0)


def pkg(sub):
    return importlib.import_module('diff-pruning_amd.' + sub)


def wall(fn, repeats):
    fn()                                                      # warm: code objects, packed weights, the capture path
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        t0 = time.time()
        fn()
        torch.cuda.synchronize()
        out.append(time.time() - t0)
    return statistics.median(out), out


def device_us(fn, calls, repeats):
    """Microseconds per call: device events around `calls` back-to-back calls, median of `repeats` after one warm round."""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        out.append(1000.0 * a.elapsed_time(b) / calls)
    return statistics.median(out), out


def eager_threshold_step(x, m):
    """The reference's expressions for one thresholded DDIM step of an epsilon model (scalars as Python floats)."""
    x0 = (x - SB * m) / SA
    B = x0.shape[0]
    flat = x0.reshape(B, -1)
    s = torch.quantile(flat.abs(), COEF['ratio'], dim=1)
    s = torch.clamp(s, min=1, max=COEF['max_value']).unsqueeze(1)
    x0 = (torch.clamp(flat, -s, s) / s).reshape(x0.shape)
    return COEF['c0'] * x0 + COEF['c1'] * m, x0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--calls', type=int, default=100)
    ap.add_argument('--steps', type=int, default=100)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'threshold_bench.jsonl'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_threshold needs an MI355X: there is no CPU path to time')
    ops, syn, unet, diffusion = pkg('ops'), pkg('synthetic'), pkg('unet'), pkg('diffusion')
    dev = torch.device('cuda')
    lines = []

    def emit(**kw):
        kw.update(tool='bench_threshold', repeats=args.repeats)
        lines.append(kw)
        print(json.dumps(kw), flush=True)

    def r2(v):
        return [round(t, 2) for t in v]

    def share(nbytes, us):
        return round(nbytes / (us * 1e-6) / HBM_ACHIEVABLE, 3)

    E, TH, DDIM = ops.X0_PRED_EPSILON, ops.X0_TREAT_THRESHOLD, ops.X0_MODE_DDIM
    for shape in ((256, 3, 32, 32), (16, 3, 256, 256), (64, 3, 64, 64)):
        B, n = shape[0], shape[1] * shape[2] * shape[3]
        N = B * n
        gen = torch.Generator(device=dev).manual_seed(1)
        x, m = (torch.randn(shape, device=dev, generator=gen) for _ in range(2))
        out, x0 = torch.empty_like(x), torch.empty_like(x)
        routes = [ops.X0_ROUTE_MULTI] + ([ops.X0_ROUTE_LDS] if n <= ops.THRESHOLD_LDS_MAX else [])
        if shape[2] == 64:                                                       # both routes at a row length both accept
            res = {}
            for route in routes:
                res[route] = device_us(lambda: ops.x0_abs_quantile(x, m, E, SA, SB, 0.995, 2.0, route=route), args.calls, args.repeats)
            emit(figure='routes', shape=list(shape), row=n, lds_us_per_call=round(res[ops.X0_ROUTE_LDS][0], 2),
                 lds_runs=r2(res[ops.X0_ROUTE_LDS][1]), multi_block_us_per_call=round(res[ops.X0_ROUTE_MULTI][0], 2),
                 multi_block_runs=r2(res[ops.X0_ROUTE_MULTI][1]), multi_block_x0='recomputed from x and m in each of 5 passes')
            continue
        route = routes[-1]
        passes = 1 if route == ops.X0_ROUTE_LDS else 5
        q, qr = device_us(lambda: ops.x0_abs_quantile(x, m, E, SA, SB, 0.995, 2.0, route=route), args.calls, args.repeats)
        stats = ops.x0_abs_quantile(x, m, E, SA, SB, 0.995, 2.0, route=route)
        s, sr = device_us(lambda: ops.x0_step(x, m, DDIM, E, TH, COEF, stats=stats, out=out, x0_out=x0), args.calls, args.repeats)
        f, fr = device_us(lambda: ops.x0_step(x, m, DDIM, E, TH, COEF, out=out, x0_out=x0), args.calls, args.repeats)
        e, er = device_us(lambda: eager_threshold_step(x, m), max(5, args.calls // 10), args.repeats)
        emit(figure='kernels', shape=list(shape), row=n, route='lds' if route == ops.X0_ROUTE_LDS else 'multi_block',
             quantile_us=round(q, 2), quantile_runs=r2(qr), quantile_bytes=8 * N * passes, quantile_share_of_hbm_6p3=share(8 * N * passes, q),
             step_us=round(s, 2), step_runs=r2(sr), step_bytes=16 * N, step_share_of_hbm_6p3=share(16 * N, s),
             thresholded_step_us=round(f, 2), thresholded_step_runs=r2(fr), thresholded_step_launches=1 if passes == 1 else 12,
             thresholded_step_bytes=(16 if passes == 1 else 8 * passes + 8) * N + 8 * N,
             thresholded_step_share_of_hbm_6p3=share((16 if passes == 1 else 8 * passes + 8) * N + 8 * N, f),
             eager_torch_us=round(e, 2), eager_torch_runs=r2(er), eager_over_thresholded_step=round(e / f, 2))
        del x, m, out, x0
        torch.cuda.empty_cache()

    # ---- the pipelines
    model = unet.UNet2DModel(**syn.CIFAR_CFG)
    syn.det_init_(model, 0)
    model = model.to(dev).eval()
    B, n = args.batch, args.steps
    thr = diffusion.DDIMPipeline(model, diffusion.DDIMScheduler(thresholding=True, sample_max_value=2.0))
    clip = diffusion.DDIMPipeline(model, diffusion.DDIMScheduler())

    def run(pipe):
        return lambda: pipe(batch_size=B, generator=torch.Generator().manual_seed(0), num_inference_steps=n, output_type='numpy')
    tmed, truns = wall(run(thr), args.repeats)
    cmed, cruns = wall(run(clip), args.repeats)
    emit(figure='pipeline_step', config='CIFAR_CFG', batch=B, steps=n, thresholded_ms_per_step=round(1000 * tmed / n, 3),
         thresholded_runs_ms_per_step=[round(1000 * r / n, 3) for r in truns], clipped_ms_per_step=round(1000 * cmed / n, 3),
         clipped_runs_ms_per_step=[round(1000 * r / n, 3) for r in cruns], thresholded_over_clipped=round(tmed / cmed, 4))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'a') as f:
        for kw in lines:
            f.write(json.dumps(kw) + '\n')


if __name__ == '__main__':
    main()
