#!/usr/bin/env python3
"""The ddpm_exp sampler (diff-pruning_amd/ddpm_exp_sampler.py) at the CIFAR config, seeded weights, one MI355X.  Appends one JSON
line per figure to --out (default profiles/ddpm_exp_sampler_bench.jsonl); each figure is the median of --repeats runs, wall
clock around work that ends in a device synchronise, after one warm run.
  generalized_step   ms per step of `generalized`, n = 100, eta 0, B = 256 -- and, from the same run, DDIMPipeline's step (both are
                     one UNet forward plus one small launch)
  ddpm_noisy_step    ms per step of `ddpm_noisy`, n = 1000, keep='last'
  sample_fid         images per second of Sampler.sample_fid (n = 100) with PNG writing on and off
    python tools/bench_ddpm_exp_sampler.py [--batch 256] [--repeats 3] [--ddpm-steps 1000]"""
import argparse
import importlib
import json
import os
import shutil
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def pkg(sub):
    return importlib.import_module('diff-pruning_amd.' + sub)


def wall(fn, repeats, warm=None):
    (warm or fn)()                                            # warm: code objects, packed weights, the capture path
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        t0 = time.time()
        fn()
        torch.cuda.synchronize()
        out.append(time.time() - t0)
    return statistics.median(out), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=256)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--ddpm-steps', type=int, default=1000)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ddpm_exp_sampler_bench.jsonl'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_ddpm_exp_sampler needs an MI355X: there is no CPU path to time')
    S, syn, unet, diffusion = pkg('ddpm_exp_sampler'), pkg('synthetic'), pkg('unet'), pkg('diffusion')
    dev = torch.device('cuda')
    model = unet.UNet2DModel(**syn.CIFAR_CFG)
    syn.det_init_(model, 0)
    model = model.to(dev).eval()
    betas = S.linear_betas()
    B = args.batch
    x = torch.from_numpy(syn.det_noise((B, 3, 32, 32), 7)).to(dev)
    lines = []

    def emit(**kw):
        kw.update(tool='bench_ddpm_exp_sampler', config='CIFAR_CFG', batch=B, repeats=args.repeats)
        lines.append(kw)
        print(json.dumps(kw), flush=True)

    gen = S.Sampler(model, betas, (3, 32, 32), timesteps=100, sample_type='generalized', eta=0.0)
    n = len(gen.seq)
    med, runs = wall(lambda: gen.sample_image(x), args.repeats)
    pipe = diffusion.DDIMPipeline(model, diffusion.DDIMScheduler())
    pmed, pruns = wall(lambda: pipe(batch_size=B, generator=torch.Generator().manual_seed(0), num_inference_steps=100,
                                    output_type='numpy'), args.repeats)
    emit(figure='generalized_step', steps=n, ms_per_step=round(1000 * med / n, 3), runs_ms_per_step=[round(1000 * r / n, 3) for r in runs],
         ddim_pipeline_ms_per_step=round(1000 * pmed / 100, 3), ddim_pipeline_runs_ms_per_step=[round(1000 * r / 100, 3) for r in pruns])

    dd = S.Sampler(model, betas, (3, 32, 32), timesteps=args.ddpm_steps, sample_type='ddpm_noisy')
    g = torch.Generator(device=dev).manual_seed(1)
    short = S.Sampler(model, betas, (3, 32, 32), timesteps=10, sample_type='ddpm_noisy')      # the same kernels, 10 steps
    med, runs = wall(lambda: dd.sample_image(x, generator=g), args.repeats, warm=lambda: short.sample_image(x, generator=g))
    emit(figure='ddpm_noisy_step', steps=len(dd.seq), ms_per_step=round(1000 * med / len(dd.seq), 3),
         runs_ms_per_step=[round(1000 * r / len(dd.seq), 3) for r in runs])

    for save in (True, False):
        tmp = tempfile.mkdtemp(prefix='dp_fid_')
        count = [0]

        def job():
            count[0] += 1
            return gen.sample_fid(os.path.join(tmp, str(count[0])), total_n_samples=2 * B, batch_size=B, seed=3, rank=0, world=1, save=save)
        try:
            med, runs = wall(job, args.repeats)
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
        emit(figure='sample_fid', png=save, images=2 * B, steps=n, images_per_s=round(2 * B / med, 1),
             runs_images_per_s=[round(2 * B / r, 1) for r in runs])
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'a') as f:
        for kw in lines:
            f.write(json.dumps(kw) + '\n')


if __name__ == '__main__':
    main()
