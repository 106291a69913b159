#!/usr/bin/env python3
"""The stage study (diff-pruning_amd/stage_study.py, csrc/stage.hip) at the CIFAR config, seeded weights, one MI355X.  Appends one JSON
line per figure to --out (default profiles/stage_study_bench.jsonl); wall clock around work that ends in a device synchronise, after
one warm run; medians of --repeats.
  staged_sweep   the --steps-timestep sweep at batch --batch with a snapshot at every stage (50, 100, ..., --steps) against the same sweep
                 without, in alternating pairs in one run: the difference is the cost of the snapshots, reported beside the unstaged
                 sweep's own run-to-run spread
  fold_sum       dp_fold_sum alone, k = 2, at the CIFAR and the bedroom-256 parameter counts: time and TB/s of its 12 algorithmic
                 bytes per element, beside the copy + axpby spelling (20 bytes per element, two launches) from the same run
  study          stage_study.run: wall time split into sweep, prunes, sampling and SSIM -- and the reference's procedure on the same
                 engine, a fresh taylor_sweep(num_steps=s) per stage: measured with --measure-reference, otherwise EXTRAPOLATED from
                 the unstaged sweep's time per timestep (the line says which)
    python tools/bench_stage_study.py [--batch 128] [--steps 1000] [--images 64] [--sample-steps 100] [--repeats 3]"""
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


def pkg(sub):
    return importlib.import_module('diff-pruning_amd.' + sub)


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.time()
    r = fn()
    torch.cuda.synchronize()
    return time.time() - t0, r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=128)                 # --taylor_batch_size's default
    ap.add_argument('--steps', type=int, default=1000)
    ap.add_argument('--stage-every', type=int, default=50)
    ap.add_argument('--images', type=int, default=64)
    ap.add_argument('--sample-steps', type=int, default=100)
    ap.add_argument('--ratio', type=float, default=0.3)
    ap.add_argument('--repeats', type=int, default=3)
    ap.add_argument('--measure-reference', action='store_true')
    ap.add_argument('--skip', nargs='*', default=[], choices=['staged_sweep', 'fold_sum', 'study'])
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'stage_study_bench.jsonl'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('bench_stage_study needs an MI355X: there is no CPU path to time')
    S, syn, unet, diffusion, sweep, ops = (pkg(m) for m in ('stage_study', 'synthetic', 'unet', 'diffusion', 'sweep', 'ops'))
    dev = torch.device('cuda')
    B = args.batch
    stages = list(range(args.stage_every, args.steps + 1, args.stage_every))
    clean = torch.from_numpy(syn.det_clean((B, 3, 32, 32), 1)).to(dev)
    noise = torch.from_numpy(syn.det_noise((B, 3, 32, 32), 2)).to(dev)
    x_T = torch.from_numpy(syn.det_noise((args.images, 3, 32, 32), 7)).to(dev)
    sched = diffusion.DDPMScheduler()

    def fresh():
        m = unet.UNet2DModel(**syn.CIFAR_CFG)
        syn.det_init_(m, 0)
        return m.to(dev).eval()

    def emit(**kw):
        kw.update(tool='bench_stage_study', config='CIFAR_CFG', batch=B, steps=args.steps, repeats=args.repeats)
        print(json.dumps(kw), flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, 'a') as f:
            f.write(json.dumps(kw) + '\n')

    model = fresh()
    n_params = sum(p.numel() for p in model.parameters())

    def run_sweep(st, steps=None):
        return sweep.taylor_sweep(model, sched, clean, noise, num_steps=steps or args.steps, loss_kind='sum', stages=st)

    per_step_ms = None
    if 'staged_sweep' not in args.skip:
        timed(lambda: run_sweep(None, 20))                             # warm: code objects, packs, the second pipeline
        plain, staged = [], []
        for _ in range(args.repeats):                                  # alternating pairs
            plain.append(timed(lambda: run_sweep(None))[0])
            t, res = timed(lambda: run_sweep(stages))
            staged.append(t)
            del res
        mp, ms = statistics.median(plain), statistics.median(staged)
        per_step_ms = 1000 * mp / args.steps
        emit(figure='staged_sweep', stages=len(stages), snapshot_bytes=4 * n_params * len(stages), unstaged_s=round(mp, 3),
             staged_s=round(ms, 3), runs_unstaged_s=[round(v, 3) for v in plain], runs_staged_s=[round(v, 3) for v in staged],
             snapshots_cost_s=round(ms - mp, 3), unstaged_spread_s=round(max(plain) - min(plain), 3),
             staged_spread_s=round(max(staged) - min(staged), 3), ms_per_timestep=round(per_step_ms, 3))

    if 'fold_sum' not in args.skip:
        bed = unet.UNet2DModel(**syn.BEDROOM_CFG)
        counts = dict(cifar=n_params, bedroom256=sum(p.numel() for p in bed.parameters()))
        del bed
        for name, n in counts.items():
            a, b, out = (torch.randn(n, device=dev) for _ in range(3))

            def fold():
                for _ in range(20):
                    ops.fold_sum(out, [a, b])

            def spelled():
                for _ in range(20):
                    out.copy_(a)
                    ops.axpby(b, 1.0, out, 1.0)
            fold(), spelled()
            tf = statistics.median(timed(fold)[0] for _ in range(args.repeats)) / 20
            ts = statistics.median(timed(spelled)[0] for _ in range(args.repeats)) / 20
            emit(figure='fold_sum', params=name, n=n, k=2, fold_sum_us=round(1e6 * tf, 1), fold_sum_TBps=round(12 * n / tf / 1e12, 3),
                 achievable_TBps=6.3, copy_axpby_us=round(1e6 * ts, 1), copy_axpby_TBps_of_its_20_bytes=round(20 * n / ts / 1e12, 3))
            del a, b, out

    if 'study' not in args.skip:
        sargs = dict(timesteps=args.sample_steps, sample_type='generalized', skip_type='uniform', eta=0.0)

        def study():
            tm = {}
            t, _ = timed(lambda: S.run(model, sched, clean, noise, x_T, [0] + stages, pruning_ratio=args.ratio, loss_kind='sum',
                                       sampler_args=sargs, n_ssim=min(32, args.images), num_steps=args.steps, timings=tm))
            return t, tm
        runs = [study() for _ in range(args.repeats)]
        runs.sort(key=lambda r: r[0])
        t, tm = runs[len(runs) // 2]
        line = dict(figure='study', stages=len(stages) + 1, images=args.images, sample_steps=args.sample_steps, total_s=round(t, 2),
                    runs_total_s=[round(r[0], 2) for r in runs], sweep_s=round(tm['sweep_s'], 2), prunes_s=round(tm['prune_s'], 2),
                    sampling_s=round(tm['sample_s'], 2), ssim_s=round(tm['ssim_s'], 2), timesteps_one_sweep=args.steps,
                    timesteps_fresh_sweep_per_stage=sum(stages))
        if args.measure_reference:
            def per_stage():
                for s in stages:
                    run_sweep(None, s)
            line.update(fresh_sweeps_s=round(timed(per_stage)[0], 2), fresh_sweeps='measured')
        else:
            ms_step = per_step_ms if per_step_ms is not None else 1000 * tm['sweep_s'] / args.steps
            line.update(fresh_sweeps_s=round(sum(stages) * ms_step / 1000, 2),
                        fresh_sweeps='EXTRAPOLATED: %d timesteps x %.3f ms, the measured time per timestep of the %s'
                        % (sum(stages), ms_step, 'unstaged sweep' if per_step_ms is not None else "study's own sweep"))
        emit(**line)


if __name__ == '__main__':
    main()
