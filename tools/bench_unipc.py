#!/usr/bin/env python3
"""UniPCMultistepScheduler (diff-pruning_amd/diffusion.py, csrc/unipc.hip) at the CIFAR config, seeded weights, one MI355X.
Appends one JSON line per figure to --out (default profiles/unipc_bench.jsonl).  Nothing here is bounded: these are reports.
  pipeline_step   ms per step of DDPMPipeline with the 10-step UniPC scheduler (bh2, predict_x0, order 3) at B = --batch, beside
                  DDIMPipeline's 10 steps and the 20-step DPM-Solver pipeline from the same run: wall clock around a pipeline call
                  that ends in a device synchronise (the read-back of the images), after one warm call; median of --repeats.  Each
                  is one UNet forward plus one small launch per step.
  kernel          dp_unipc_step alone for (pc, pp) = (0, 1), (1, 2), (3, 3): device events around --calls back-to-back launches (so
                  a launch that is shorter than the host's enqueue measures the enqueue), median of --repeats, in microseconds per
                  call -- at the pipeline's own size (B x 3 x 32 x 32, cache resident) and at --big elements, where the
                  4 (reads + writes) algorithmic bytes per element (reads: e, x_pred, x_last when pc > 0, max(pc, pp - 1) history
                  buffers; writes: m_new, x_next, x_c when pc > 0) come from and go to HBM: that time over the bytes is given as a
                  share of the 6.3 TB/s achievable HBM rate.  Beside each: the reference's eager torch expression for the same
                  step on the same device and buffers (stack, einsum and all: about forty launches at the third order).
    python tools/bench_unipc.py [--batch 256] [--repeats 3] [--calls 200] [--big 67108864]"""
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


def eager_update(x, m0, older, m_t, cx, c0, cB, rks, rhos):
    """One UniP (m_t None) or UniC update in the reference's eager form: the differences stacked and contracted by einsum."""
    D1s = [(mi - m0) / rk for mi, rk in zip(older, rks)]
    x_t_ = cx * x - c0 * m0
    k = len(D1s)
    res = torch.einsum('k,bkchw->bchw', rhos[:k], torch.stack(D1s, dim=1)) if D1s else 0
    if m_t is None:
        return x_t_ - cB * res
    return x_t_ - cB * (res + rhos[k] * (m_t - m0))


def eager_step(e, x, xl, hist, c, pc, pp, rho_c, rho_p):
    """The reference's expressions for one `step` (its scalars are 0-d CPU tensors, which torch hands to each elementwise kernel
    as a scalar argument: Python floats do the same; the rhos are device vectors, as the reference builds them)."""
    m_new = (x - c['sigma_s'] * e) / c['alpha_s']
    xs = x
    if pc:
        xs = eager_update(xl, hist[0], hist[1:pc], m_new, c['c_cx'], c['c_c0'], c['c_cB'], [c.get('c_rk1'), c.get('c_rk2')], rho_c)
    new = [m_new] + list(hist)
    return eager_update(xs, new[0], new[1:pp], None, c['p_cx'], c['p_c0'], c['p_cB'], [c.get('p_rk1'), c.get('p_rk2')], rho_p), xs, m_new


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--big', type=int, default=1 << 26)
    ap.add_argument('--steps', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'unipc_bench.jsonl'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_unipc needs an MI355X: there is no CPU path to time')
    ops, syn, unet, diffusion = pkg('ops'), pkg('synthetic'), pkg('unet'), pkg('diffusion')
    dev = torch.device('cuda')
    B = args.batch
    lines = []

    def emit(**kw):
        kw.update(tool='bench_unipc', config='CIFAR_CFG', batch=B, repeats=args.repeats)
        lines.append(kw)
        print(json.dumps(kw), flush=True)

    # ---- the kernel alone, beside the eager expression
    sched = diffusion.UniPCMultistepScheduler(solver_order=3)
    sched.set_timesteps(20)
    ts = sched._ts
    for label, shape, calls in (('pipeline_size', (B, 3, 32, 32), args.calls), ('hbm_size', (args.big // 3072, 3, 32, 32), max(20, args.calls // 10))):
        n = shape[0] * shape[1] * shape[2] * shape[3]
        gen = torch.Generator(device=dev).manual_seed(1)
        e, x, xl, m0, m1, m2 = (torch.randn(shape, device=dev, generator=gen) for _ in range(6))
        out, xc, ring = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
        for pc, pp in ((0, 1), (1, 2), (3, 3)):
            c = sched.step_coefs(pc, pp, ts[7], ts[8], [ts[4], ts[5], ts[6]])
            rho_c = torch.tensor([c.get('c_rho1', 0.0), c.get('c_rho2', 0.0)][:max(pc - 1, 0)] + [c.get('c_rho_last', 0.0)], device=dev)
            rho_p = torch.tensor([c.get('p_rho1', 0.0), c.get('p_rho2', 0.0)][:pp - 1] + [0.0], device=dev)
            med, runs = device_us(lambda: ops.unipc_step(e, x, c, pc=pc, pp=pp, predict_x0=True, x_last=xl, hist=[m0, m1, m2], out=out,
                                                         x_c=xc, m_new=ring), calls, args.repeats)
            emed, eruns = device_us(lambda: eager_step(e, x, xl, [m0, m1, m2], c, pc, pp, rho_c, rho_p), calls, args.repeats)
            reads, writes = 2 + (1 if pc else 0) + max(pc, pp - 1), 2 + (1 if pc else 0)
            nbytes = 4 * (reads + writes) * n
            emit(figure='kernel', size=label, elements=n, pc=pc, pp=pp, calls=calls, us_per_call=round(med, 2),
                 runs_us_per_call=[round(r, 2) for r in runs], reads=reads, writes=writes, algorithmic_bytes=nbytes,
                 tb_per_s=round(nbytes / med / 1e6, 3), share_of_hbm_6p3=round(nbytes / (med * 1e-6) / HBM_ACHIEVABLE, 3),
                 eager_torch_us_per_call=round(emed, 2), eager_torch_runs_us_per_call=[round(r, 2) for r in eruns],
                 eager_over_kernel=round(emed / med, 2))
        del e, x, xl, m0, m1, m2, out, xc, ring
        torch.cuda.empty_cache()

    # ---- the pipelines
    model = unet.UNet2DModel(**syn.CIFAR_CFG)
    syn.det_init_(model, 0)
    model = model.to(dev).eval()
    n = args.steps
    unipc = diffusion.DDPMPipeline(model, diffusion.UniPCMultistepScheduler(solver_order=3))
    ddim = diffusion.DDIMPipeline(model, diffusion.DDIMScheduler())
    dpm = diffusion.DDPMPipeline(model, diffusion.DPMSolverMultistepScheduler(solver_order=2))

    def run(pipe, steps):
        return lambda: pipe(batch_size=B, generator=torch.Generator().manual_seed(0), num_inference_steps=steps, output_type='numpy')
    umed, uruns = wall(run(unipc, n), args.repeats)
    dmed, druns = wall(run(ddim, n), args.repeats)
    pmed, pruns = wall(run(dpm, 2 * n), args.repeats)
    assert unipc.scheduler.num_inference_steps == n
    emit(figure='pipeline_step', unipc_steps=n, unipc_ms_per_step=round(1000 * umed / n, 3),
         unipc_runs_ms_per_step=[round(1000 * r / n, 3) for r in uruns], unipc_ms_per_image_batch=round(1000 * umed, 1),
         ddim_steps=n, ddim_pipeline_ms_per_step=round(1000 * dmed / n, 3), ddim_pipeline_runs_ms_per_step=[round(1000 * r / n, 3) for r in druns],
         dpm_steps=2 * n, dpm_solver_ms_per_step=round(1000 * pmed / (2 * n), 3),
         dpm_solver_runs_ms_per_step=[round(1000 * r / (2 * n), 3) for r in pruns], dpm_solver_ms_per_image_batch=round(1000 * pmed, 1))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'a') as f:
        for kw in lines:
            f.write(json.dumps(kw) + '\n')


if __name__ == '__main__':
    main()
