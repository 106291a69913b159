#!/usr/bin/env python3
"""The ldm_exp samplers (diff-pruning_amd/ldm_sampler.py) at cin256-v2, seeded weights, one MI355X.  Appends one JSON line per figure
to --out (default profiles/ldm_sampler_bench.jsonl); each figure is the median of --repeats runs, wall clock around work that ends
in a device synchronise, after one short warm run.
  guided_step      ms per guided DDIM step (scale 3.0, eta 0, --steps steps) at every --batch, beside ldm_sweep.ddim_sample_cfg from
                   the same run: one forward of 2 x batch rows dominates both, so the two should agree within the run-to-run spread,
                   which is reported (max - min of the runs over their median)
  kernel           dp_cfg_denoise_step alone against the two launches it replaces (dp_cfg_combine + dp_ddim_step) at [50, 3, 64, 64]:
                   microseconds per call and GB/s of each path's own algorithmic bytes (4 tensors against 6)
  sample_classes   images per second of sample_classes (one class batch of 50, --fid-steps steps, VQ-f4 first stage) with PNG
                   writing on and off
    python tools/bench_ldm_sampler.py [--batch 8 50] [--steps 250] [--fid-steps 20] [--repeats 3]"""
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
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)


def pkg(sub):
    return importlib.import_module('diff-pruning_amd.' + sub)


def wall(fn, repeats, warm):
    warm()                                                    # code objects, packed weights
    torch.cuda.synchronize()
    out = []
    for _ in range(repeats):
        t0 = time.time()
        fn()
        torch.cuda.synchronize()
        out.append(time.time() - t0)
    return statistics.median(out), out


def events_us(fn, iters=200, warm=20):
    for _ in range(warm):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return 1000.0 * a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, nargs='+', default=[8, 50])
    ap.add_argument('--steps', type=int, default=250)
    ap.add_argument('--fid-steps', type=int, default=20)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ldm_sampler_bench.jsonl'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_ldm_sampler needs an MI355X: there is no CPU path to time')
    import vq_ref
    S, syn, ldm, ldm_sweep, ops, vq = (pkg(m) for m in ('ldm_sampler', 'synthetic', 'ldm', 'ldm_sweep', 'ops', 'vq'))
    dev = torch.device('cuda')
    model = ldm.UNetModel(**syn.LDM_CIN256_CFG)
    syn.det_init_(model, 0)
    model = model.to(dev).eval()
    emb = ldm_sweep.ClassEmbedder(syn.LDM_CIN256_CFG['context_dim'], 1001).to(dev)
    sched = ldm_sweep.LdmSchedule()
    smp = S.DDIMSampler(model, sched)
    lines = []

    def emit(**kw):
        kw.update(tool='bench_ldm_sampler', config='LDM_CIN256_CFG', repeats=args.repeats)
        lines.append(kw)
        print(json.dumps(kw), flush=True)

    def spread(runs):
        return round((max(runs) - min(runs)) / statistics.median(runs), 4)

    for B in args.batch:
        x_T = torch.from_numpy(syn.det_noise((B, 3, 64, 64), 7)).to(dev)
        c = emb(torch.tensor(B * [3], device=dev))
        uc = emb(torch.tensor(B * [1000], device=dev))

        def new(steps):
            return smp.sample(steps, B, (3, 64, 64), conditioning=c, x_T=x_T, unconditional_guidance_scale=3.0, unconditional_conditioning=uc)

        def old(steps):
            return ldm_sweep.ddim_sample_cfg(model, sched, x_T, c, uc, S=steps, scale=3.0)
        n = len(S.ddim_timesteps('uniform', args.steps, 1000))
        med, runs = wall(lambda: new(args.steps), args.repeats, lambda: new(4))
        omed, oruns = wall(lambda: old(args.steps), args.repeats, lambda: old(4))
        emit(figure='guided_step', batch=B, steps=n, ms_per_step=round(1000 * med / n, 3), runs_ms_per_step=[round(1000 * r / n, 3) for r in runs],
             spread=spread(runs), ddim_sample_cfg_ms_per_step=round(1000 * omed / n, 3),
             ddim_sample_cfg_runs_ms_per_step=[round(1000 * r / n, 3) for r in oruns], ddim_sample_cfg_spread=spread(oruns))

    B = 50
    n = B * 3 * 64 * 64
    x = torch.from_numpy(syn.det_noise((B, 3, 64, 64), 8)).to(dev)
    e = torch.from_numpy(syn.det_noise((2 * B, 3, 64, 64), 9)).to(dev)
    coef = [float(v) for v in S.sampling_tables(sched.alphas_cumprod, S.ddim_timesteps('uniform', 250, 1000), 0.0)[125]]
    _, a, a_prev, sig = sched.ddim(250)
    out, x0 = torch.empty_like(x), torch.empty_like(x)
    one = events_us(lambda: ops.cfg_denoise_step(x, e, coef, scale=3.0, out=out))
    one_x0 = events_us(lambda: ops.cfg_denoise_step(x, e, coef, scale=3.0, out=out, x0_out=x0))
    two = events_us(lambda: ops.ddim_step(x, ops.cfg_combine(e[:B], e[B:], 3.0), float(a[125]), float(a_prev[125]), float(sig[125]), None,
                                          clip=False, out=out))
    emit(figure='kernel', shape=[B, 3, 64, 64], one_launch_us=round(one, 2), one_launch_gbps=round(4 * 4 * n / one / 1e3, 1),
         one_launch_with_x0_us=round(one_x0, 2), one_launch_with_x0_gbps=round(5 * 4 * n / one_x0 / 1e3, 1),
         two_launches_us=round(two, 2), two_launches_gbps=round(6 * 4 * n / two / 1e3, 1))

    first = vq.VQModel(**syn.VQ_F4_CFG)
    first.load_state_dict(vq_ref.params(syn.VQ_F4_CFG, 7, torch.float32))
    first = first.to(dev).eval()
    for save in (True, False):
        tmp = tempfile.mkdtemp(prefix='dp_ldm_fid_')
        count = [0]

        def job(steps=args.fid_steps):
            count[0] += 1
            return S.sample_classes(smp, emb, first, os.path.join(tmp, str(count[0])), classes=[3], ipc=B, batch_size=B, ddim_steps=steps,
                                    scale=3.0, seed=3, rank=0, world=1, save=save)
        try:
            med, runs = wall(job, args.repeats, lambda: job(2))
        finally:
            shutil.rmtree(tmp, ignore_errors=True)
        emit(figure='sample_classes', png=save, images=B, steps=args.fid_steps, images_per_s=round(B / med, 2),
             runs_images_per_s=[round(B / r, 2) for r in runs], class_batch_limit=S.max_class_batch(model, (3, 64, 64)))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'a') as f:
        for kw in lines:
            f.write(json.dumps(kw) + '\n')


if __name__ == '__main__':
    main()
