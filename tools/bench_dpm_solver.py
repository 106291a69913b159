#!/usr/bin/env python3
"""DPMSolverMultistepScheduler (diff-pruning_amd/diffusion.py, csrc/dpm_solver.hip) at the CIFAR config, seeded weights, one MI355X.
Appends one JSON line per figure to --out (default profiles/dpm_solver_bench.jsonl).  Nothing here is bounded: these are reports.
  pipeline_step   ms per step of DDPMPipeline with the 20-step solver (dpmsolver++, order 2) at B = --batch, beside DDIMPipeline's
                  20 steps from the same run: wall clock around a pipeline call that ends in a device synchronise (the read-back of
                  the images), after one warm call; median of --repeats.  Both are one UNet forward plus one small launch per step.
  kernel          dp_dpm_solver_step alone, per order: device events around --calls back-to-back launches (so a launch that is
                  shorter than the host's enqueue measures the enqueue), median of --repeats, in microseconds per call -- at the
                  pipeline's own size (B x 3 x 32 x 32, cache resident) and at --big elements, where the 4 (order + 3) algorithmic
                  bytes per element (x, e, order - 1 history buffers read; x', m0 written) come from and go to HBM: that time over
                  the bytes is given as a share of the 6.3 TB/s achievable HBM rate.  Beside each: the reference's eager torch
                  expression for the same step on the same device and buffers (about a dozen launches).
    python tools/bench_dpm_solver.py [--batch 256] [--repeats 3] [--calls 200] [--big 67108864]"""
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


def eager_step(x, e, m1, m2, c, order, data_pred):
    """The reference's expression for one step (its scalars are 0-d CPU tensors, which torch hands to each elementwise kernel as
    a scalar argument: Python floats do the same)."""
    m0 = (x - c['sigma_s'] * e) / c['alpha_s'] if data_pred else e
    if order == 1:
        return c['kx'] * x - c['k0'] * m0, m0
    if order == 2:
        D1 = c['ir0'] * (m0 - m1)
        return c['kx'] * x - c['k0'] * m0 - c['k1'] * D1, m0
    D10, D11 = c['ir0'] * (m0 - m1), c['ir1'] * (m1 - m2)
    D1 = D10 + c['q'] * (D10 - D11)
    D2 = c['iq'] * (D10 - D11)
    return c['kx'] * x - c['k0'] * m0 - c['k1'] * D1 - c['k2'] * D2, m0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--big', type=int, default=1 << 26)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'dpm_solver_bench.jsonl'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_dpm_solver needs an MI355X: there is no CPU path to time')
    ops, syn, unet, diffusion = pkg('ops'), pkg('synthetic'), pkg('unet'), pkg('diffusion')
    dev = torch.device('cuda')
    B = args.batch
    lines = []

    def emit(**kw):
        kw.update(tool='bench_dpm_solver', config='CIFAR_CFG', batch=B, repeats=args.repeats)
        lines.append(kw)
        print(json.dumps(kw), flush=True)

    # ---- the kernel alone, beside the eager expression
    sched = diffusion.DPMSolverMultistepScheduler(solver_order=3)
    sched.set_timesteps(args.steps)
    ts = sched._ts
    for label, n, calls in (('pipeline_size', B * 3 * 32 * 32, args.calls), ('hbm_size', args.big, max(10, args.calls // 10))):
        gen = torch.Generator(device=dev).manual_seed(1)
        x, e, m1, m2 = (torch.randn(n, device=dev, generator=gen) for _ in range(4))
        out, ring = torch.empty_like(x), torch.empty_like(x)
        for order in (1, 2, 3):
            c = sched.step_coefs(order, ts[7], ts[8], ts[6], ts[5])
            med, runs = device_us(lambda: ops.dpm_solver_step(x, e, c, order=order, data_pred=True, m1=m1, m2=m2, out=out, m0_out=ring),
                                  calls, args.repeats)
            emed, eruns = device_us(lambda: eager_step(x, e, m1, m2, c, order, True), calls, args.repeats)
            nbytes = 4 * (order + 3) * n
            emit(figure='kernel', size=label, elements=n, order=order, calls=calls, us_per_call=round(med, 2),
                 runs_us_per_call=[round(r, 2) for r in runs], algorithmic_bytes=nbytes, tb_per_s=round(nbytes / med / 1e6, 3),
                 share_of_hbm_6p3=round(nbytes / (med * 1e-6) / HBM_ACHIEVABLE, 3), eager_torch_us_per_call=round(emed, 2),
                 eager_torch_runs_us_per_call=[round(r, 2) for r in eruns], eager_over_kernel=round(emed / med, 2))
        del x, e, m1, m2, out, ring
        torch.cuda.empty_cache()

    # ---- the pipelines
    model = unet.UNet2DModel(**syn.CIFAR_CFG)
    syn.det_init_(model, 0)
    model = model.to(dev).eval()
    n = args.steps
    solver = diffusion.DDPMPipeline(model, diffusion.DPMSolverMultistepScheduler(solver_order=2))
    ddim = diffusion.DDIMPipeline(model, diffusion.DDIMScheduler())
    smed, sruns = wall(lambda: solver(batch_size=B, generator=torch.Generator().manual_seed(0), num_inference_steps=n, output_type='numpy'), args.repeats)
    dmed, druns = wall(lambda: ddim(batch_size=B, generator=torch.Generator().manual_seed(0), num_inference_steps=n, output_type='numpy'), args.repeats)
    assert solver.scheduler.num_inference_steps == n
    emit(figure='pipeline_step', steps=n, solver_ms_per_step=round(1000 * smed / n, 3), solver_runs_ms_per_step=[round(1000 * r / n, 3) for r in sruns],
         ddim_pipeline_ms_per_step=round(1000 * dmed / n, 3), ddim_pipeline_runs_ms_per_step=[round(1000 * r / n, 3) for r in druns])
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'a') as f:
        for kw in lines:
            f.write(json.dumps(kw) + '\n')


if __name__ == '__main__':
    main()
