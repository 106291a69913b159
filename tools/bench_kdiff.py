#!/usr/bin/env python3
"""LMSDiscreteScheduler and the two KDPM2 schedulers (diff-pruning_amd/diffusion.py, csrc/kdiff.hip) at the CIFAR config, seeded
weights, one MI355X.  Appends one JSON line per figure to --out (default profiles/kdiff_bench.jsonl).  Nothing here is bounded: these
are reports.
  kernel          dp_kdpm2_step (first-order call, second-order call, second-order call with noise; the last under v-prediction
                  too) and dp_lms_step at order 4 (epsilon and v-prediction) and order 1 alone: device events around --calls
                  back-to-back launches (so a launch that is shorter than the host's enqueue measures the enqueue), median of
                  --repeats, in microseconds per call -- at 2^16 .. 2^26 elements in steps of 4 (--sizes).  Beside each: an eager
                  torch restatement of the reference's operation sequence for the same call on the same device and buffers (five to
                  twelve launches), which is the yardstick, and the algorithmic bytes per element of the fused call (KDPM2: x, e
                  [, the saved sample][, the noise] read, x' written: 12 / 16 / 20; LMS: x, e and order - 1 derivatives read, x', the
                  new derivative and x0 written: 20 at order 1, 32 at order 4) over the time as a share of the 6.3 TB/s achievable HBM
                  rate -- meaningful at the sizes that do not fit the caches.
  loop_eval       ms per model evaluation of the canonical loop -- scale_model_input, the captured forward, step -- with
                  LMSDiscreteScheduler and KDPM2DiscreteScheduler beside EulerDiscreteScheduler at --steps inference steps and
                  B = --batch (KDPM2 evaluates the model 2 * steps - 1 times): wall clock around a call that ends in a device
                  synchronise, after one warm call; median of --repeats.  The LMS line also gives the host time of the quadrature
                  of one pass over the table, which the first pass pays and later passes over the same table do not.
    python tools/bench_kdiff.py [--batch 256] [--repeats 3] [--calls 200]"""
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


def eager_x0(v_pred, sample, e, c):
    """(The reference's scalars are 0-d CPU tensors, which torch hands to each elementwise kernel as a scalar argument: Python floats
    do the same.)"""
    if v_pred:
        return e * c['c_out'] + (sample / c['c_den'])
    return sample - c['sig'] * e


def eager_kdpm2(v_pred, x, e, saved, z, c):
    d = (x - eager_x0(v_pred, x, e, c)) / c['sig']
    prev = (x if saved is None else saved) + d * c['dt']
    if z is not None:
        prev = prev + z * c['sigma_up']
    return prev


def eager_lms(v_pred, x, e, history, c):
    x0 = eager_x0(v_pred, x, e, c)
    d = (x - x0) / c['sig']
    return x + sum(c['c%d' % k] * h for k, h in enumerate([d] + history)), d, x0


COEFS = dict(sig=14.6, c_out=-0.9976, c_den=214.16, dt=-3.2, sigma_up=1.7, c0=-3.9, c1=2.4, c2=-1.1, c3=0.21)
KDPM2_COEFS = {k: COEFS[k] for k in ('sig', 'c_out', 'c_den', 'dt', 'sigma_up')}
# (shape, v_prediction, algorithmic bytes per element) and (order, v_prediction, bytes)
KDPM2_CASES = (('FIRST', False, 12), ('SECOND', False, 16), ('SECOND_NOISE', False, 20), ('SECOND_NOISE', True, 20))
LMS_CASES = ((4, False, 32), (4, True, 32), (1, False, 20))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--sizes', type=int, nargs='*', default=[1 << k for k in (16, 18, 20, 22, 24, 26)])
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'kdiff_bench.jsonl'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_kdiff needs an MI355X: there is no CPU path to time')
    ops, syn, unet, diffusion = pkg('ops'), pkg('synthetic'), pkg('unet'), pkg('diffusion')
    dev = torch.device('cuda')
    B = args.batch
    lines = []

    def emit(**kw):
        kw.update(tool='bench_kdiff', config='CIFAR_CFG', batch=B, repeats=args.repeats)
        lines.append(kw)
        print(json.dumps(kw), flush=True)

    def kernel_line(n, calls, name, per_element, fn, eager, **more):
        med, runs = device_us(fn, calls, args.repeats)
        emed, eruns = device_us(eager, calls, args.repeats)
        nbytes = per_element * n
        emit(figure='kernel', elements=n, kernel=name, calls=calls, us_per_call=round(med, 2),
             runs_us_per_call=[round(r, 2) for r in runs], algorithmic_bytes=nbytes, tb_per_s=round(nbytes / med / 1e6, 3),
             share_of_hbm_6p3=round(nbytes / (med * 1e-6) / HBM_ACHIEVABLE, 3), eager_torch_us_per_call=round(emed, 2),
             eager_torch_runs_us_per_call=[round(r, 2) for r in eruns], eager_over_kernel=round(emed / med, 2), **more)

    # ---- the kernels alone, beside the eager expressions
    c = COEFS
    for n in args.sizes:
        calls = args.calls if n <= 1 << 22 else max(10, args.calls // 10)
        gen = torch.Generator(device=dev).manual_seed(1)
        x, e, z, saved, d1, d2, d3 = (torch.randn(n, device=dev, generator=gen) for _ in range(7))
        out, d_out, x0_out = (torch.empty_like(x) for _ in range(3))
        for shape, v, per_element in KDPM2_CASES:
            p = ops.KDIFF_V if v else ops.KDIFF_EPSILON
            xs, noise = (saved if shape != 'FIRST' else None), (z if shape == 'SECOND_NOISE' else None)
            kernel_line(n, calls, 'dp_kdpm2_step', per_element, lambda: ops.kdpm2_step(x, e, KDPM2_COEFS, p, saved=xs, noise=noise, out=out),
                        lambda: eager_kdpm2(v, x, e, xs, noise, c), shape=shape, v_prediction=v)
        for order, v, per_element in LMS_CASES:
            p = ops.KDIFF_V if v else ops.KDIFF_EPSILON
            history = [d1, d2, d3][:order - 1]
            coef = {k: c[k] for k in ops.LMS_COEF[:3 + order]}
            kernel_line(n, calls, 'dp_lms_step', per_element,
                        lambda: ops.lms_step(x, e, coef, order, p, history=history, out=out, d_out=d_out, x0_out=x0_out),
                        lambda: eager_lms(v, x, e, history, c), order=order, v_prediction=v)
        del x, e, z, saved, d1, d2, d3, out, d_out, x0_out
        torch.cuda.empty_cache()

    # ---- the canonical loop beside the Euler loop
    model = unet.UNet2DModel(**syn.CIFAR_CFG)
    syn.det_init_(model, 0)
    model = model.to(dev).eval()
    n = args.steps
    shape = (B, 3, 32, 32)
    kept = {}

    def loop(name):
        s = kept.get(name)
        if s is None:
            s = kept[name] = getattr(diffusion, name)()
            s.set_timesteps(n)
        else:
            s.derivatives = []                                # a second pass over the same table: LMS keeps its coefficients
            s.sample = None
        x = diffusion.randn_tensor(shape, generator=torch.Generator().manual_seed(0), device=dev) * s.init_noise_sigma
        s.is_scale_input_called = True
        fwd = model.sampling_forward(shape, len(s._ts))
        try:
            with torch.no_grad():
                for t in s._ts:
                    x = s.step(fwd(s.scale_model_input(x, t), t), t, x).prev_sample
        finally:
            fwd.close()
        return (x / 2 + 0.5).clamp(0, 1).cpu()
    res = {}
    for name in ('EulerDiscreteScheduler', 'LMSDiscreteScheduler', 'KDPM2DiscreteScheduler'):
        med, runs = wall(lambda: loop(name), args.repeats)
        evals = len(kept[name]._ts)
        res[name] = dict(evaluations=evals, ms_per_evaluation=round(1000 * med / evals, 3), runs_ms_per_evaluation=[round(1000 * r / evals, 3) for r in runs])
    s = diffusion.LMSDiscreteScheduler()
    s.set_timesteps(n)
    t0 = time.time()
    for i in range(n):
        s.lms_coefficients(min(i + 1, 4), i)
    quad_ms = 1000 * (time.time() - t0)
    emit(figure='loop_eval', steps=n, euler=res['EulerDiscreteScheduler'], lms=res['LMSDiscreteScheduler'], kdpm2=res['KDPM2DiscreteScheduler'],
         lms_quadrature_host_ms_per_pass=round(quad_ms, 2), lms_quadrature_host_ms_per_step=round(quad_ms / n, 3))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'a') as f:
        for kw in lines:
            f.write(json.dumps(kw) + '\n')


if __name__ == '__main__':
    main()
