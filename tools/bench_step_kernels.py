#!/usr/bin/env python3
"""Kernel-only timing of the elementwise step launchers of sampler.hip, ldm_sampler.hip and threshold.hip, for comparing two builds
of the library: one library per process (DP_HIP_LIB), the processes alternated by the caller.  Device events around `calls`
back-to-back calls, median of `repeats` after warm calls: the method of tools/bench_threshold.py's `kernels` figure and
tools/bench_ldm_sampler.py's `kernel` figure, at their shapes (the pipeline sizes) and at a size whose traffic is past the 256 MB
last-level cache (HBM).  Appends one JSON line per call and shape to <out.jsonl>.  Nothing here is bounded: these are reports.
    DP_HIP_LIB=<lib> python tools/bench_step_kernels.py <label> <run> <out.jsonl>"""
import importlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ops = importlib.import_module('diff-pruning_amd.ops')
L = importlib.import_module('diff-pruning_amd._lib')
label, run, out_path = sys.argv[1], int(sys.argv[2]), sys.argv[3]
dev = torch.device('cuda')
CALLS, REPEATS = 100, 7


def device_us(fn):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(REPEATS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(CALLS):
            fn()
        b.record()
        b.synchronize()
        out.append(1000.0 * a.elapsed_time(b) / CALLS)
    return statistics.median(out), out


lines = []


def emit(kernel, shape, med, runs):
    kw = dict(tool='bench_step_kernels', lib=label, run=run, lib_file=os.path.basename(L.LIB_PATH), kernel=kernel, shape=list(shape), calls=CALLS,
              repeats=REPEATS, median_us=round(med, 3), runs_us=[round(r, 3) for r in runs])
    lines.append(kw)
    print(json.dumps(kw), flush=True)


def rnd(shape, seed):
    return torch.randn(shape, device=dev, generator=torch.Generator(device=dev).manual_seed(seed))


# ---- sampler.hip: denoise_step_kernel<0> (generalized, eta 0: no z) and <1> (ddpm_noisy: z), with and without x0_out
for shape in ((256, 3, 32, 32), (512, 3, 256, 256)):
    x, e, z = rnd(shape, 1), rnd(shape, 2), rnd(shape, 3)
    out, x0 = torch.empty_like(x), torch.empty_like(x)
    emit('denoise_step_kernel<0>', shape, *device_us(lambda: ops.denoise_step(x, e, 0, (0.6, 0.8, 0.9, 0.0, 0.3), out=out)))
    emit('denoise_step_kernel<0> x0_out', shape, *device_us(lambda: ops.denoise_step(x, e, 0, (0.6, 0.8, 0.9, 0.0, 0.3), out=out, x0_out=x0)))
    emit('denoise_step_kernel<1> z', shape, *device_us(lambda: ops.denoise_step(x, e, 1, (1.2, 0.7, 0.4, 0.5, 0.9, 0.1), z=z, out=out)))
    del x, e, z, out, x0
    torch.cuda.empty_cache()

# ---- ldm_sampler.hip: cfg_denoise_step_kernel<0, true> (guided DDIM) and <3, true> (PLMS, three history buffers)
for shape in ((50, 3, 64, 64), (2048, 3, 64, 64)):
    x, e = rnd(shape, 4), rnd((2 * shape[0],) + shape[1:], 5)
    hist = [rnd(shape, 6 + i) for i in range(3)]
    out, x0, eg = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    coef = (0.6, 0.8, 0.85, 0.5, 0.0)
    emit('cfg_denoise_step_kernel<0, true>', shape, *device_us(lambda: ops.cfg_denoise_step(x, e, coef, scale=3.0, out=out)))
    emit('cfg_denoise_step_kernel<0, true> x0_out', shape, *device_us(lambda: ops.cfg_denoise_step(x, e, coef, scale=3.0, out=out, x0_out=x0)))
    emit('cfg_denoise_step_kernel<3, true> x0_out eg_out', shape,
         *device_us(lambda: ops.cfg_denoise_step(x, e, coef, scale=3.0, order=3, hist=hist, out=out, x0_out=x0, eg_out=eg)))
    del x, e, hist, out, x0, eg
    torch.cuda.empty_cache()

# ---- threshold.hip: the calls of tools/bench_threshold.py's `kernels` figure, plus one shape past the cache
E, TH, DDIM = ops.X0_PRED_EPSILON, ops.X0_TREAT_THRESHOLD, ops.X0_MODE_DDIM
COEF = dict(sa=0.8, sb=0.6, c0=0.9, c1=0.3, cz=0.0, ratio=0.995, max_value=2.0)
for shape in ((256, 3, 32, 32), (16, 3, 256, 256), (256, 3, 256, 256)):
    n = shape[1] * shape[2] * shape[3]
    x, m = rnd(shape, 9), rnd(shape, 10)
    out, x0 = torch.empty_like(x), torch.empty_like(x)
    route = ops.X0_ROUTE_LDS if n <= ops.THRESHOLD_LDS_MAX else ops.X0_ROUTE_MULTI
    name = 'lds' if route == ops.X0_ROUTE_LDS else 'multi_block'
    emit('dp_x0_abs_quantile ' + name, shape, *device_us(lambda: ops.x0_abs_quantile(x, m, E, 0.8, 0.6, 0.995, 2.0, route=route)))
    stats = ops.x0_abs_quantile(x, m, E, 0.8, 0.6, 0.995, 2.0, route=route)
    emit('th_step_kernel', shape, *device_us(lambda: ops.x0_step(x, m, DDIM, E, TH, COEF, stats=stats, out=out, x0_out=x0)))
    if route == ops.X0_ROUTE_LDS:
        emit('th_lds_kernel<true>', shape, *device_us(lambda: ops.x0_step(x, m, DDIM, E, TH, COEF, out=out, x0_out=x0)))
    del x, m, out, x0
    torch.cuda.empty_cache()

os.makedirs(os.path.dirname(os.path.abspath(out_path)), exist_ok=True)
with open(out_path, 'a') as f:
    for kw in lines:
        f.write(json.dumps(kw) + '\n')
