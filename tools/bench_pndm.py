#!/usr/bin/env python3
"""PNDMScheduler / PNDMPipeline (diff-pruning_amd/diffusion.py, csrc/pndm.hip) at the CIFAR config, seeded weights, one MI355X.
Appends one JSON line per figure to --out (default profiles/pndm_bench.jsonl).  Nothing here is bounded: these are reports.
  pipeline_eval   ms per model evaluation of PNDMPipeline with --steps inference steps (the timestep list is longer: twelve
                  Runge-Kutta calls, then steps - 3 multistep ones) at B = --batch, beside DDIMPipeline's --steps evaluations from the
                  same run: wall clock around a pipeline call that ends in a device synchronise (the read-back of the images), after
                  one warm call; median of --repeats.  Both are one UNet forward plus one small launch per evaluation.
  kernel          dp_pndm_step alone for PRK0, PRK3, PLMS4 and PLMS4 under v-prediction: device events around --calls back-to-back
                  launches (so a launch that is shorter than the host's enqueue measures the enqueue), median of --repeats, in
                  microseconds per call -- at the pipeline's own size (B x 3 x 32 x 32, cache resident) and at --big elements,
                  where the mode's algorithmic bytes per element (PRK0: x, e read, x', acc, hist written, 20; PRK3: x, e, acc read,
                  x' written, 16; PLMS4: x, e, h1 .. h3 read, x', hist written, 28) come from and go to HBM: that time over the bytes
                  is given as a share of the 6.3 TB/s achievable HBM rate.  Beside each: the reference's eager torch expression for
                  the same step on the same device and buffers (about a dozen launches).
    python tools/bench_pndm.py [--batch 256] [--repeats 3] [--calls 200] [--big 67108864]"""
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


def eager_step(mode, v_pred, x, e, acc, h1, h2, h3, c):
    """The reference's expressions for one step (its scalars are 0-d CPU tensors, which torch hands to each elementwise kernel as
    a scalar argument: Python floats do the same).  Returns what the step leaves behind."""
    new_acc = None
    if mode == 'PRK0':
        new_acc = 0 + 1 / 6 * e
        m = e
    elif mode == 'PRK3':
        m = acc + 1 / 6 * e
    else:
        m = (1 / 24) * (55 * e - 59 * h1 + 37 * h2 - 9 * h3)
    if v_pred:
        m = c['sa'] * m + c['sb'] * x
    return c['sc'] * x - c['d'] * m / c['den'], new_acc


# (mode, v_prediction, algorithmic bytes per element)
KERNEL_CASES = (('PRK0', False, 20), ('PRK3', False, 16), ('PLMS4', False, 28), ('PLMS4', True, 28))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--big', type=int, default=1 << 26)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'pndm_bench.jsonl'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_pndm needs an MI355X: there is no CPU path to time')
    ops, syn, unet, diffusion = pkg('ops'), pkg('synthetic'), pkg('unet'), pkg('diffusion')
    dev = torch.device('cuda')
    B = args.batch
    lines = []

    def emit(**kw):
        kw.update(tool='bench_pndm', config='CIFAR_CFG', batch=B, repeats=args.repeats)
        lines.append(kw)
        print(json.dumps(kw), flush=True)

    # ---- the kernel alone, beside the eager expression
    for label, n, calls in (('pipeline_size', B * 3 * 32 * 32, args.calls), ('hbm_size', args.big, max(10, args.calls // 10))):
        gen = torch.Generator(device=dev).manual_seed(1)
        x, e, acc, h1, h2, h3 = (torch.randn(n, device=dev, generator=gen) for _ in range(6))
        out, ring = torch.empty_like(x), torch.empty_like(x)
        for mode, v, per_element in KERNEL_CASES:
            c = diffusion.PNDMScheduler(prediction_type='v_prediction' if v else 'epsilon').step_coefs(500, 480)
            m = getattr(ops, 'PNDM_' + mode)
            med, runs = device_us(lambda: ops.pndm_step(x, e, c, m, v_pred=v, acc=acc, hist=(h1, h2, h3), out=out, hist_out=ring),
                                  calls, args.repeats)
            emed, eruns = device_us(lambda: eager_step(mode, v, x, e, acc, h1, h2, h3, c), calls, args.repeats)
            nbytes = per_element * n
            emit(figure='kernel', size=label, elements=n, mode=mode, v_prediction=v, calls=calls, us_per_call=round(med, 2),
                 runs_us_per_call=[round(r, 2) for r in runs], algorithmic_bytes=nbytes, tb_per_s=round(nbytes / med / 1e6, 3),
                 share_of_hbm_6p3=round(nbytes / (med * 1e-6) / HBM_ACHIEVABLE, 3), eager_torch_us_per_call=round(emed, 2),
                 eager_torch_runs_us_per_call=[round(r, 2) for r in eruns], eager_over_kernel=round(emed / med, 2))
        del x, e, acc, h1, h2, h3, out, ring
        torch.cuda.empty_cache()

    # ---- the pipelines
    model = unet.UNet2DModel(**syn.CIFAR_CFG)
    syn.det_init_(model, 0)
    model = model.to(dev).eval()
    n = args.steps
    pndm = diffusion.PNDMPipeline(model, diffusion.PNDMScheduler())
    ddim = diffusion.DDIMPipeline(model, diffusion.DDIMScheduler())
    pmed, pruns = wall(lambda: pndm(batch_size=B, generator=torch.Generator().manual_seed(0), num_inference_steps=n, output_type='numpy'), args.repeats)
    dmed, druns = wall(lambda: ddim(batch_size=B, generator=torch.Generator().manual_seed(0), num_inference_steps=n, output_type='numpy'), args.repeats)
    evals = len(pndm.scheduler._ts)
    assert pndm.scheduler.num_inference_steps == n and pndm.scheduler.counter == evals
    emit(figure='pipeline_eval', steps=n, pndm_model_evaluations=evals, pndm_ms_per_evaluation=round(1000 * pmed / evals, 3),
         pndm_runs_ms_per_evaluation=[round(1000 * r / evals, 3) for r in pruns], ddim_model_evaluations=n,
         ddim_pipeline_ms_per_evaluation=round(1000 * dmed / n, 3), ddim_pipeline_runs_ms_per_evaluation=[round(1000 * r / n, 3) for r in druns])
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'a') as f:
        for kw in lines:
            f.write(json.dumps(kw) + '\n')


if __name__ == '__main__':
    main()
