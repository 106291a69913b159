#!/usr/bin/env python3
"""Distillation finetune at the C4 shapes: the ratio-0.3 pruned CIFAR UNet (19.85 M parameters) as the student at batch 128 with
dropout 0.1, the unpruned CIFAR UNet (35.7 M) as the frozen teacher.  Milliseconds per step, natively replayed, in one process:
  (a) today's finetune step (no teacher)
  (b) the teacher's forward alone (UNet2DModel.sampling_forward, captured and replayed)
  (c) the KD step, teacher after the student's input on the same stream (DP_KD_OVERLAP=0)
  (d) the KD step, teacher forward on the side stream beside the student's forward (DP_KD_OVERLAP=1)
Each figure is the median over --steps steps of the device-event interval between consecutive steps, after --warmup steps;
--rounds repeats (a)-(d) in turn so that every round sees the same clocks.  Prints one JSON line.
    python tools/bench_kd.py [--steps 20] [--warmup 5] [--rounds 3] [--only abcd]"""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests', 'golden')):
    if p not in sys.path:
        sys.path.insert(0, p)
import golden_common as gc   # noqa: E402


def pkg(sub):
    return importlib.import_module('diff-pruning_amd.' + sub)


def cifar(dev, pruned):
    """bench.py's configs[3] model (seeded CIFAR UNet, two-step Taylor sweep of 16 images, ratio 0.3) or the unpruned one."""
    unet, sweep, diffusion = pkg('unet'), pkg('sweep'), pkg('diffusion')
    m = unet.UNet2DModel(**gc.CIFAR_CFG)
    gc.det_init_(m, 0)
    m = m.to(dev).eval()
    if pruned:
        c = torch.from_numpy(gc.det_clean((16, 3, 32, 32), 1)).to(dev)
        n = torch.from_numpy(gc.det_noise((16, 3, 32, 32), 2)).to(dev)
        sweep.taylor_sweep(m, diffusion.DDPMScheduler(), c, n, num_steps=2, reduce_grads=False)
        sweep.prune_model(m, 0.3)
        for p in m.parameters():
            p.grad = None
    return m


def timed(fn, steps, warmup):
    """Median ms between consecutive device events recorded after each call (the step's span on the device, gaps included)."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    ev[0].record()
    for k in range(steps):
        fn()
        ev[k + 1].record()
    torch.cuda.synchronize()
    return statistics.median(ev[k].elapsed_time(ev[k + 1]) for k in range(steps))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--batch', type=int, default=128)
    ap.add_argument('--only', default='abcd')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_kd needs the GPU'
    dev = torch.device('cuda', 0)
    train, diffusion = pkg('train'), pkg('diffusion')
    B = args.batch
    clean = torch.from_numpy(gc.det_clean((B, 3, 32, 32), 300)).to(dev)
    noise = torch.from_numpy(gc.det_noise((B, 3, 32, 32), 400)).to(dev)
    gen = torch.Generator().manual_seed(0)

    def ts():
        return train.antithetic_timesteps(B, 1000, gen).to(dev, non_blocking=True)

    teacher = train.load_teacher(cifar(dev, False), dev)
    runs = {}
    if 'a' in args.only:
        fa = train.FinetuneEngine(cifar(dev, True), diffusion.DDPMScheduler(), lr=2e-4, dropout=0.1, dropout_seed=1)
        runs['a_plain_step'] = lambda: fa.step(clean, noise, ts())
    if 'b' in args.only:
        fwd = teacher.sampling_forward((B, 3, 32, 32), 1 << 30, replay=True)
        tb = torch.full((B,), 500, dtype=torch.long, device=dev)

        def teacher_only():
            with torch.no_grad():
                fwd(clean, tb)
        runs['b_teacher_forward'] = teacher_only
    engines = {}
    for key, ov in (('c_kd_serial', '0'), ('d_kd_overlap', '1')):
        if key[0] in args.only:
            engines[key] = (train.FinetuneEngine(cifar(dev, True), diffusion.DDPMScheduler(), lr=2e-4, dropout=0.1, dropout_seed=1,
                                                 teacher=teacher), ov)

            def kd_step(ft=engines[key][0], ov=ov):
                os.environ['DP_KD_OVERLAP'] = ov
                return ft.step(clean, noise, ts())
            runs[key] = kd_step
    res = {k: [] for k in runs}
    for _ in range(args.rounds):
        for k, fn in runs.items():
            res[k].append(timed(fn, args.steps, args.warmup))
    out = dict(bench='kd_finetune_c4', batch=B, steps=args.steps, warmup=args.warmup, rounds=args.rounds,
               student_params=19851157, teacher_params=sum(p.numel() for p in teacher.parameters()),
               ms_per_step={k: [round(v, 3) for v in vs] for k, vs in res.items()},
               median_ms={k: round(statistics.median(vs), 3) for k, vs in res.items()})
    for key, (ft, _) in engines.items():
        out.setdefault('replayed', {})[key] = ft._cap is not None and ft._cap['call'].replay is not None
        out.setdefault('replay_info', {})[key] = dict(ft._cap['call'].info) if ft._cap else None
    if all(k in res for k in ('a_plain_step', 'b_teacher_forward', 'c_kd_serial')):
        a, b, c = (statistics.median(res[k]) for k in ('a_plain_step', 'b_teacher_forward', 'c_kd_serial'))
        out['serial_vs_sum'] = round(c / (a + b), 4)                       # done-criterion: <= 1.05
    if 'c_kd_serial' in res and 'd_kd_overlap' in res:
        out['overlap_gain_per_round'] = [round(1 - d / c, 4) for c, d in zip(res['c_kd_serial'], res['d_kd_overlap'])]
    print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
