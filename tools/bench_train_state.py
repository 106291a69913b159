#!/usr/bin/env python3
"""Save and load times of the one-file training state (checkpoint.save_training_state / load_training_state) on one MI355X:
  c4       train.FinetuneEngine on the ratio-0.3 pruned CIFAR-10 UNet (19.85 M parameters), EMA on
  cin256   ldm_train.LdmFinetuneEngine on the cin256-v2 UNet + class embedder (400.9 M parameters), LitEma on
Per leg a child interpreter under its own time limit takes one optimizer step (so the moments are not all zero), then reports
  save_s / load_s    median wall time of `--repeat` saves / loads, device synchronised before and after (a save ends when the file
                     is in place; a load ends when the flat buffers hold the state)
  file_mb            size of the file (weights + m + v + shadow: 16 B per parameter with EMA)
  state_dict_s       engine.state_dict() alone (device-side clones), load_state_dict_s likewise
The parent runs the legs one after the other and stops at the first that does not exit with status 0.  One JSON line per leg.
    python tools/bench_train_state.py [--legs c4,cin256] [--repeat 3] [--dir /dev/shm]"""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tests', 'golden')):
    if p not in sys.path:
        sys.path.insert(0, p)


def pkg(sub):
    return importlib.import_module('diff-pruning_amd.' + sub)


def _timed(fn, repeat):
    import torch
    out = []
    for _ in range(repeat):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return statistics.median(out)


def leg(name, args):
    import torch
    import golden_common as gc
    assert torch.cuda.is_available(), 'bench_train_state needs the GPU'
    dev = torch.device('cuda', 0)
    checkpoint = pkg('checkpoint')
    if name == 'c4':
        train, diffusion, sweep, unet = pkg('train'), pkg('diffusion'), pkg('sweep'), pkg('unet')
        model = unet.UNet2DModel(**gc.CIFAR_CFG)
        gc.det_init_(model, 0)
        model = model.to(dev).eval()
        clean = torch.from_numpy(gc.det_clean((4, 3, 32, 32), 1)).to(dev)
        noise = torch.from_numpy(gc.det_noise((4, 3, 32, 32), 2)).to(dev)
        sweep.taylor_sweep(model, diffusion.DDPMScheduler(), clean, noise, num_steps=8)
        sweep.prune_model(model, 0.3)
        for p in model.parameters():
            p.grad = None
        ft = train.FinetuneEngine(model, diffusion.DDPMScheduler(), dropout=0.1, dropout_seed=1, replay=False)
        B = 16
        ft.step(torch.from_numpy(gc.det_clean((B, 3, 32, 32), 3)).to(dev), torch.from_numpy(gc.det_noise((B, 3, 32, 32), 4)).to(dev),
                train.antithetic_timesteps(B, 1000, torch.Generator().manual_seed(0)))
    else:
        ldm, ldm_sweep, ldm_train = pkg('ldm'), pkg('ldm_sweep'), pkg('ldm_train')
        cfg = gc.LDM_CIN256_CFG
        model = ldm.UNetModel(**cfg)
        gc.det_init_(model, 9)
        model = model.to(dev).eval()
        embedder = ldm_sweep.ClassEmbedder(cfg['context_dim'], 1001).to(dev)
        ft = ldm_train.LdmFinetuneEngine(model, embedder, lr=1.28e-4, use_ema=True)
        B = 2
        ft.step(torch.from_numpy(gc.det_noise((B, 3, 64, 64), 300)).to(dev), torch.tensor([3, 500]),
                noise=torch.from_numpy(gc.det_noise((B, 3, 64, 64), 400)).to(dev), timesteps=torch.tensor([10, 900]))
    torch.cuda.synchronize()
    out = dict(leg=name, params=int(ft.flat_p.numel()), repeat=args.repeat, dir=args.dir)
    with tempfile.TemporaryDirectory(dir=args.dir) as d:
        path = os.path.join(d, 'state.pt')
        out['save_s'] = _timed(lambda: checkpoint.save_training_state(path, ft), args.repeat)
        out['file_mb'] = os.path.getsize(path) / 2 ** 20
        before = ft.flat_p.clone()
        out['load_s'] = _timed(lambda: checkpoint.load_training_state(path, ft), args.repeat)
        assert torch.equal(before, ft.flat_p)
    sd = [None]
    out['state_dict_s'] = _timed(lambda: sd.__setitem__(0, ft.state_dict()), args.repeat)
    out['load_state_dict_s'] = _timed(lambda: ft.load_state_dict(sd[0]), args.repeat)
    print(json.dumps(out, sort_keys=True), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--legs', default='c4,cin256')
    ap.add_argument('--repeat', type=int, default=3)
    ap.add_argument('--dir', default=None, help='directory the file is written to (default: the system temporary directory)')
    ap.add_argument('--leg-timeout', type=int, default=300, help='seconds one leg may take')
    ap.add_argument('--leg', default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.leg is not None:
        return leg(args.leg, args)
    for name in args.legs.split(','):
        cmd = [sys.executable, os.path.abspath(__file__), '--leg', name, '--repeat', str(args.repeat)] + (['--dir', args.dir] if args.dir else [])
        try:
            p = subprocess.run(cmd, timeout=args.leg_timeout, capture_output=True, text=True)
        except subprocess.TimeoutExpired:
            print(json.dumps(dict(leg=name, error='time limit of %d s' % args.leg_timeout)), flush=True)
            return 124                             # nothing more is started on the device
        if p.returncode != 0:
            print(json.dumps(dict(leg=name, error='exit status %d' % p.returncode, tail=p.stderr[-2000:])), flush=True)
            return p.returncode                    # the first failing leg ends the run
        print([ln for ln in p.stdout.splitlines() if ln.startswith('{')][-1], flush=True)
    return 0


if __name__ == '__main__':
    sys.exit(main())
