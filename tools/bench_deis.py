#!/usr/bin/env python3
"""DEISMultistepScheduler and DPMSolverSinglestepScheduler (diff-pruning_amd/diffusion.py, csrc/deis.hip) at the CIFAR config, seeded
weights, one MI355X.  Appends one JSON line per figure to --out (default profiles/deis_bench.jsonl).  Nothing here is bounded: these
are reports.
  kernel          each step form of dp_deis_step / dp_dpm_single_step alone (epsilon model; singlestep under dpmsolver++): device
                  events around --calls back-to-back launches (so a launch that is shorter than the host's enqueue measures the
                  enqueue), median of --repeats, in microseconds per call -- at the pipeline's own size (B x 3 x 32 x 32, cache
                  resident) and at --big elements, where the kernel's own bytes per element (every buffer it reads, x' and m0
                  written) come from and go to HBM: that time over the bytes is given as a share of the 6.3 TB/s achievable HBM
                  rate.  Beside each: an eager torch restatement of the reference's expression for the same step on the same device
                  and buffers, with its count of elementwise launches (`eager_ops`, counted in the reference source: the singlestep
                  third-order update forms D1_0, D1_1, D1 and D2 whichever solver type is set).
  thresholded     the thresholded second-order DEIS step ([B, 3 x 32 x 32] rows: the exact quantile's launch and the step's) beside
                  the reference's sort-based _threshold_sample and update in eager torch.
  loop            ms per model evaluation of DDPMPipeline with each class at 10 and 20 steps, beside DPMSolverMultistepScheduler in
                  the same run: wall clock around a pipeline call that ends in a device synchronise (the read-back of the images),
                  after one warm call; median of --repeats.
    python tools/bench_deis.py [--batch 256] [--repeats 3] [--calls 200] [--big 67108864]"""
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


def eager_threshold(x0, ratio, max_value):
    """The reference's _threshold_sample on [B, n] rows: torch.quantile sorts every row."""
    s = torch.quantile(x0.abs(), ratio, dim=1)
    s = torch.clamp(s, min=1, max=max_value).unsqueeze(1)
    return torch.clamp(x0, -s, s) / s


def eager_deis(x, m, m1, m2, c, order, thr=None):
    """The reference's expression for one DEIS step, epsilon model (its scalars are 0-d CPU tensors, which torch hands to each
    elementwise kernel as a scalar argument: Python floats do the same)."""
    x0 = (x - c['sb'] * m) / c['sa']
    if thr:
        x0 = eager_threshold(x0, *thr)
    m0 = (x - c['sa'] * x0) / c['sb']
    if order == 1:
        return c['kx'] * x - c['k0'] * m0, m0
    if order == 2:
        return c['at'] * (x / c['as0'] + c['c1'] * m0 + c['c2'] * m1), m0
    return c['at'] * (x / c['as0'] + c['c1'] * m0 + c['c2'] * m1 + c['c3'] * m2), m0


DEIS_EAGER_OPS = {1: 9, 2: 12, 3: 14}                         # convert there and back (6) + the update


def eager_single(x, xs, m, m1, m2, c, order, heun):
    """The reference's expression for one singlestep step, epsilon model under dpmsolver++ (k1 is passed negated where the
    reference adds the term; the count of launches is the same)."""
    m0 = (x - c['sb'] * m) / c['sa']
    if order == 1:
        return c['kx'] * x - c['k0'] * m0, m0
    if order == 2:
        D1 = c['ir0'] * (m0 - m1)
        return c['kx'] * xs - c['k0'] * m1 - c['k1'] * D1, m0
    r0, r1 = 1.0 / c['ir0'], 1.0 / c['ir1']
    D1_0, D1_1 = c['ir1'] * (m1 - m2), c['ir0'] * (m0 - m2)
    D1 = (r0 * D1_0 - r1 * D1_1) / (r0 - r1)
    D2 = 2.0 * (D1_1 - D1_0) / (r0 - r1)
    if not heun:
        return c['kx'] * xs - c['k0'] * m2 - c['k1'] * D1_1, m0
    return c['kx'] * xs - c['k0'] * m2 - c['k1'] * D1 - c['k2'] * D2, m0


SINGLE_EAGER_OPS = {(1, False): 6, (2, False): 10, (3, False): 19, (3, True): 21}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--big', type=int, default=1 << 26)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'deis_bench.jsonl'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_deis needs an MI355X: there is no CPU path to time')
    ops, syn, unet, diffusion = pkg('ops'), pkg('synthetic'), pkg('unet'), pkg('diffusion')
    dev = torch.device('cuda')
    B = args.batch
    lines = []

    def emit(**kw):
        kw.update(tool='bench_deis', config='CIFAR_CFG', batch=B, repeats=args.repeats)
        lines.append(kw)
        print(json.dumps(kw), flush=True)

    def kernel_line(figure, label, form, n, calls, nbytes, eager_ops, med, runs, emed, eruns, **more):
        emit(figure=figure, size=label, form=form, elements=n, calls=calls, us_per_call=round(med, 2),
             runs_us_per_call=[round(r, 2) for r in runs], kernel_bytes=nbytes, tb_per_s=round(nbytes / med / 1e6, 3),
             share_of_hbm_6p3=round(nbytes / (med * 1e-6) / HBM_ACHIEVABLE, 3), eager_ops=eager_ops, eager_torch_us_per_call=round(emed, 2),
             eager_torch_runs_us_per_call=[round(r, 2) for r in eruns], eager_over_kernel=round(emed / med, 2), **more)

    # ---- the kernels alone, beside the eager expressions
    deis = diffusion.DEISMultistepScheduler(solver_order=3)
    deis.set_timesteps(20)
    ts = deis._ts
    singles = {h: diffusion.DPMSolverSinglestepScheduler(solver_order=3, solver_type='heun' if h else 'midpoint') for h in (False, True)}
    row = 3 * 32 * 32
    for label, n, calls in (('pipeline_size', B * row, args.calls), ('hbm_size', args.big, max(10, args.calls // 10))):
        gen = torch.Generator(device=dev).manual_seed(1)
        x, xs, m, m1, m2 = (torch.randn(n, device=dev, generator=gen) for _ in range(5))
        out, ring = torch.empty_like(x), torch.empty_like(x)
        for order in (1, 2, 3):
            c = deis.step_coefs(order, ts[7], ts[8], ts[6], ts[5])
            med, runs = device_us(lambda: ops.deis_step(x, m, c, order=order, m1=m1, m2=m2, out=out, m0_out=ring), calls, args.repeats)
            emed, eruns = device_us(lambda: eager_deis(x, m, m1, m2, c, order), calls, args.repeats)
            kernel_line('kernel', label, 'deis_o%d' % order, n, calls, 4 * (order + 3) * n, DEIS_EAGER_OPS[order], med, runs, emed, eruns)
        for order, heun in ((1, False), (2, False), (3, False), (3, True)):
            c = singles[heun].step_coefs(order, ts[7], ts[8], ts[6], ts[5])
            med, runs = device_us(lambda: ops.dpm_single_step(x, m, c, order=order, heun=heun, xs=xs, m1=m1, m2=m2, out=out, m0_out=ring),
                                  calls, args.repeats)
            emed, eruns = device_us(lambda: eager_single(x, xs, m, m1, m2, c, order, heun), calls, args.repeats)
            reads = 2 if order == 1 else order + 2                  # x, m | x, xs, m and the history
            kernel_line('kernel', label, 'single_o%d_%s' % (order, 'heun' if heun else 'midpoint'), n, calls, 4 * (reads + 2) * n,
                        SINGLE_EAGER_OPS[(order, heun)], med, runs, emed, eruns)
        if label != 'pipeline_size':                                 # the thresholded step on rows: at the pipeline's size alone
            del x, xs, m, m1, m2, out, ring
            torch.cuda.empty_cache()
            continue
        rows = B
        shape = (rows, n // rows)
        c = deis.step_coefs(2, ts[7], ts[8], ts[6], ts[5])
        x2, m2d, h1, o2, r2 = (t.reshape(shape) for t in (x, m, m1, out, ring))

        def fused():
            st = ops.x0_abs_quantile(x2, m2d, ops.X0_PRED_EPSILON, c['sa'], c['sb'], 0.995, 2.0)
            return ops.deis_step(x2, m2d, c, order=2, m1=h1, stats=st, out=o2, m0_out=r2)
        tcalls = max(5, calls // 20)
        med, runs = device_us(fused, tcalls, args.repeats)
        emed, eruns = device_us(lambda: eager_deis(x2, m2d, h1, None, c, 2, thr=(0.995, 2.0)), tcalls, args.repeats)
        kernel_line('thresholded', label, 'deis_o2_thresholded', n, tcalls, 4 * 5 * n, DEIS_EAGER_OPS[2] + 6, med, runs, emed, eruns,
                    rows=rows, row_length=shape[1], note='kernel_bytes is the step alone; the quantile reads x and m again per pass')
        del x, xs, m, m1, m2, out, ring, x2, m2d, h1, o2, r2
        torch.cuda.empty_cache()

    # ---- the loops
    model = unet.UNet2DModel(**syn.CIFAR_CFG)
    syn.det_init_(model, 0)
    model = model.to(dev).eval()
    classes = (('deis', diffusion.DEISMultistepScheduler), ('dpm_singlestep', diffusion.DPMSolverSinglestepScheduler),
               ('dpm_multistep', diffusion.DPMSolverMultistepScheduler))
    for n in (10, 20):
        res = {}
        for name, cls in classes:
            pipe = diffusion.DDPMPipeline(model, cls(solver_order=2))
            med, runs = wall(lambda: pipe(batch_size=B, generator=torch.Generator().manual_seed(0), num_inference_steps=n, output_type='numpy'),
                             args.repeats)
            assert pipe.scheduler.num_inference_steps == n
            res[name + '_ms_per_evaluation'] = round(1000 * med / n, 3)
            res[name + '_runs_ms_per_evaluation'] = [round(1000 * r / n, 3) for r in runs]
        emit(figure='loop', steps=n, solver_order=2, **res)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'a') as f:
        for kw in lines:
            f.write(json.dumps(kw) + '\n')


if __name__ == '__main__':
    main()
