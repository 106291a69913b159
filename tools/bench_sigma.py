#!/usr/bin/env python3
"""The sigma-space schedulers (diff-pruning_amd/diffusion.py, csrc/sigma.hip) at the CIFAR config, seeded weights, one MI355X.
Appends one JSON line per figure to --out (default profiles/sigma_bench.jsonl).  Nothing here is bounded: these are reports.
  kernel          dp_sigma_step for every mode (the Euler step with and without churn, and under v-prediction), dp_sigma_scale and
                  dp_sigma_add_noise alone: device events around --calls back-to-back launches (so a launch that is shorter than the
                  host's enqueue measures the enqueue), median of --repeats, in microseconds per call -- at the loop's own size
                  (B x 3 x 32 x 32, cache resident) and at --big elements, where the mode's algorithmic bytes per element (EULER,
                  HEUN1: x, e read, x' and x0 / d written, 16; with churn, ANCESTRAL: the noise too, 20; HEUN2: x, e, d1, the saved
                  sample read, x' written, 20; scale: 8; add_noise: 12) come from and go to HBM: that time over the bytes is given as
                  a share of the 6.3 TB/s achievable HBM rate.  Beside each: the reference's eager torch expression for the same
                  call on the same device and buffers (three to nine launches), which is the yardstick.
  loop_eval       ms per model evaluation of the canonical loop -- scale_model_input, the captured forward, step -- with
                  EulerDiscreteScheduler at --steps inference steps (48 of 50 timesteps fractional) at B = --batch, with and
                  without the scale_model_input launch (the cost of keeping it a launch of its own), beside DDIMPipeline's --steps
                  evaluations from the same run: wall clock around a call that ends in a device synchronise, after one warm call;
                  median of --repeats.
    python tools/bench_sigma.py [--batch 256] [--repeats 3] [--calls 200] [--big 67108864]"""
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


def eager_step(mode, v_pred, churn, x, e, z, d1, saved, c):
    """The reference's expressions for one call (its scalars are 0-d CPU tensors, which torch hands to each elementwise kernel as
    a scalar argument: Python floats do the same).  Returns what the call leaves behind."""
    sample = x
    if churn:
        sample = sample + (z * c['s_noise']) * c['k']
    if v_pred:
        x0 = e * c['c_out'] + (sample / c['c_den'])
    else:
        x0 = sample - c['sig'] * e
    d = (sample - x0) / c['sig']
    if mode == 'HEUN2':
        d = (d1 + d) / 2
        sample = saved
    prev = sample + d * c['dt']
    if mode == 'ANCESTRAL':
        prev = prev + z * c['sigma_up']
    return prev, (d if mode == 'HEUN1' else x0)


# (mode, v_prediction, churn, algorithmic bytes per element)
KERNEL_CASES = (('EULER', False, False, 16), ('EULER', True, False, 16), ('EULER', False, True, 20), ('ANCESTRAL', False, False, 20),
                ('HEUN1', False, False, 16), ('HEUN2', False, False, 20))
COEFS = dict(s_noise=1.003, k=2.5, sig=14.6, c_out=-0.9976, c_den=214.16, dt=-3.2, sigma_up=1.7)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--big', type=int, default=1 << 26)
    ap.add_argument('--steps', type=int, default=50)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sigma_bench.jsonl'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_sigma needs an MI355X: there is no CPU path to time')
    ops, syn, unet, diffusion = pkg('ops'), pkg('synthetic'), pkg('unet'), pkg('diffusion')
    dev = torch.device('cuda')
    B = args.batch
    lines = []

    def emit(**kw):
        kw.update(tool='bench_sigma', config='CIFAR_CFG', batch=B, repeats=args.repeats)
        lines.append(kw)
        print(json.dumps(kw), flush=True)

    def kernel_line(label, n, calls, name, per_element, fn, eager, **more):
        med, runs = device_us(fn, calls, args.repeats)
        emed, eruns = device_us(eager, calls, args.repeats)
        nbytes = per_element * n
        emit(figure='kernel', size=label, elements=n, kernel=name, calls=calls, us_per_call=round(med, 2),
             runs_us_per_call=[round(r, 2) for r in runs], algorithmic_bytes=nbytes, tb_per_s=round(nbytes / med / 1e6, 3),
             share_of_hbm_6p3=round(nbytes / (med * 1e-6) / HBM_ACHIEVABLE, 3), eager_torch_us_per_call=round(emed, 2),
             eager_torch_runs_us_per_call=[round(r, 2) for r in eruns], eager_over_kernel=round(emed / med, 2), **more)

    # ---- the kernels alone, beside the eager expressions
    c = COEFS
    for label, n, calls in (('loop_size', B * 3 * 32 * 32, args.calls), ('hbm_size', args.big, max(10, args.calls // 10))):
        gen = torch.Generator(device=dev).manual_seed(1)
        x, e, z, d1, saved = (torch.randn(n, device=dev, generator=gen) for _ in range(5))
        out, aux = torch.empty_like(x), torch.empty_like(x)
        for mode, v, churn, per_element in KERNEL_CASES:
            m, p = getattr(ops, 'SIGMA_' + mode), ops.SIGMA_V if v else ops.SIGMA_EPSILON
            noise = z if churn or mode == 'ANCESTRAL' else None
            kernel_line(label, n, calls, 'dp_sigma_step', per_element,
                        lambda: ops.sigma_step(x, e, c, m, p, noise=noise, d1=d1, saved=saved, out=out, aux_out=aux),
                        lambda: eager_step(mode, v, churn, x, e, z, d1, saved, c), mode=mode, v_prediction=v, churn=churn)
        kernel_line(label, n, calls, 'dp_sigma_scale', 8, lambda: ops.sigma_scale(x, 14.63, out=out), lambda: x / 14.63)
        images = B if n % B == 0 else 1
        x2, z2, sig = x.reshape(images, -1), z.reshape(images, -1), torch.rand(images, device=dev, generator=gen) * 20
        kernel_line(label, n, calls, 'dp_sigma_add_noise', 12, lambda: ops.sigma_add_noise(x2, z2, sig, out=out.reshape(images, -1)),
                    lambda: x2 + z2 * sig[:, None], images=images)
        del x, e, z, d1, saved, out, aux, x2, z2
        torch.cuda.empty_cache()

    # ---- the canonical loop beside DDIMPipeline
    model = unet.UNet2DModel(**syn.CIFAR_CFG)
    syn.det_init_(model, 0)
    model = model.to(dev).eval()
    n = args.steps
    shape = (B, 3, 32, 32)

    def loop(scale):
        s = diffusion.EulerDiscreteScheduler()
        x = diffusion.randn_tensor(shape, generator=torch.Generator().manual_seed(0), device=dev) * s.init_noise_sigma
        s.set_timesteps(n)
        s.is_scale_input_called = True
        fwd = model.sampling_forward(shape, len(s._ts))
        try:
            with torch.no_grad():
                for t in s._ts:
                    x = s.step(fwd(s.scale_model_input(x, t) if scale else x, t), t, x).prev_sample
        finally:
            fwd.close()
        return (x / 2 + 0.5).clamp(0, 1).cpu()
    ddim = diffusion.DDIMPipeline(model, diffusion.DDIMScheduler())
    emed, eruns = wall(lambda: loop(True), args.repeats)
    umed, uruns = wall(lambda: loop(False), args.repeats)
    dmed, druns = wall(lambda: ddim(batch_size=B, generator=torch.Generator().manual_seed(0), num_inference_steps=n, output_type='numpy'), args.repeats)
    s = diffusion.EulerDiscreteScheduler()
    s.set_timesteps(n)
    emit(figure='loop_eval', steps=n, fractional_timesteps=sum(t != round(t) for t in s._ts), euler_ms_per_evaluation=round(1000 * emed / n, 3),
         euler_runs_ms_per_evaluation=[round(1000 * r / n, 3) for r in eruns],
         euler_without_scale_launch_ms_per_evaluation=round(1000 * umed / n, 3),
         euler_without_scale_launch_runs_ms_per_evaluation=[round(1000 * r / n, 3) for r in uruns],
         ddim_pipeline_ms_per_evaluation=round(1000 * dmed / n, 3), ddim_pipeline_runs_ms_per_evaluation=[round(1000 * r / n, 3) for r in druns])
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'a') as f:
        for kw in lines:
            f.write(json.dumps(kw) + '\n')


if __name__ == '__main__':
    main()
