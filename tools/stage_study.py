#!/usr/bin/env python3
"""ddpm_exp/prune_ssim.py + compute_pruned_ssim_curve.py for all stages in one run (diff-pruning_amd/stage_study.py): one staged Taylor
sweep, then per stage a prune, samples from one fixed x_T written as `{out}/{stage}/{i}.png`, and the SSIM / MSE of the first
--n-ssim images against stage 0's.  The result (stages, losses, relative_loss, per-stage masks, parameters, MACs, SSIM, MSE, and the
stage at which each --thr would stop a Diff-Pruning sweep) is written to `{out}/stage_study.json`.  No plotting.

The model: --model DIR (a Diffusers UNet2DModel directory) or --ckpt FILE, an original-DDPM checkpoint (a `Model` state dict or the
`[state_dict, ...]` list of runners/diffusion.py:207-211) with --config, the ddpm_exp config (.yml or .json) that holds its
`model:` / `data:` / `diffusion:` / `sampling:` blocks.  The sweep's images: one batch of --taylor-batch-size from the config's dataset
under --data-root, or with --use_generated_samples the unpruned model's own samples (prune_test.py:231-236).
    python tools/stage_study.py --ckpt model.ckpt --config cifar10.yml --data-root data --out run/prune_ssim [--stages 0 50 ... 1000]"""
import argparse
import importlib
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def pkg(sub):
    return importlib.import_module('diff-pruning_amd.' + sub)


def read_config(path):
    with open(path) as f:
        if path.endswith('.json'):
            return json.load(f)
        import yaml
        return yaml.safe_load(f)


def importance_of(name):
    P = pkg('pruning')
    table = dict(taylor=P.TaylorImportance, ours=P.TaylorImportance, magnitude=P.MagnitudeImportance, random=P.RandomImportance,
                 abs_taylor=P.AbsTaylorImportance, fisher=P.FisherImportance,
                 first_order_taylor=lambda: P.FullTaylorImportance(order=1), second_order_taylor=lambda: P.FullTaylorImportance(order=2))
    if name not in table:
        raise SystemExit('unknown --pruner %r (known: %s)' % (name, ', '.join(sorted(table))))
    return table[name]()


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument('--model', type=str, default=None)
    ap.add_argument('--ckpt', type=str, default=None)
    ap.add_argument('--config', type=str, default=None)
    ap.add_argument('--data-root', type=str, default='data')
    ap.add_argument('--use_generated_samples', action='store_true')
    ap.add_argument('--taylor-batch-size', type=int, default=128)
    ap.add_argument('--stages', type=int, nargs='+', default=list(range(0, 1001, 50)))
    ap.add_argument('--pruning-ratio', type=float, default=0.3)
    ap.add_argument('--pruner', type=str, default='taylor')
    ap.add_argument('--n-samples', type=int, default=None, help='images sampled per stage (default: sampling.batch_size, else 64)')
    ap.add_argument('--n-ssim', type=int, default=32)
    ap.add_argument('--timesteps', type=int, default=100)
    ap.add_argument('--sample-type', type=str, default='generalized')
    ap.add_argument('--skip-type', type=str, default='uniform')
    ap.add_argument('--eta', type=float, default=0.0)
    ap.add_argument('--thr', type=float, nargs='*', default=[0.05])
    ap.add_argument('--seed', type=int, default=1234)
    ap.add_argument('--out', type=str, required=True)
    args = ap.parse_args(argv)
    if not torch.cuda.is_available():
        raise SystemExit('stage_study needs an MI355X: there is no CPU path')
    if (args.model is None) == (args.ckpt is None):
        raise SystemExit('give --model DIR or --ckpt FILE (with --config)')
    S, train, data, diffusion, E = (pkg(m) for m in ('stage_study', 'train', 'data', 'diffusion', 'ddpm_exp_sampler'))
    dev = torch.device('cuda')
    cfg = read_config(args.config) if args.config else {}
    mc, dc, fc = cfg.get('model', {}), cfg.get('data', {}), cfg.get('diffusion', {})
    if args.ckpt is not None:
        if not mc:
            raise SystemExit('--ckpt needs --config with the checkpoint\'s model: block')
        model = train.load_teacher(args.ckpt, dev, ch=mc['ch'], ch_mult=mc['ch_mult'], num_res_blocks=mc['num_res_blocks'],
                                   attn_resolutions=mc['attn_resolutions'], image_size=dc['image_size'],
                                   in_channels=mc.get('in_channels', 3), out_ch=mc.get('out_ch', 3))
    else:
        model = train.load_teacher(args.model, dev)
    for p in model.parameters():
        p.requires_grad_(True)
    size = int(dc.get('image_size', model.config['sample_size']))
    chans = int(dc.get('channels', model.config['in_channels']))
    rescaled = bool(dc.get('rescaled', True))
    sched = diffusion.DDPMScheduler(num_train_timesteps=int(fc.get('num_diffusion_timesteps', 1000)),
                                    beta_start=float(fc.get('beta_start', 1e-4)), beta_end=float(fc.get('beta_end', 0.02)))
    gen = torch.Generator(device=dev).manual_seed(args.seed)
    n = args.n_samples or int(cfg.get('sampling', {}).get('batch_size', 64))
    x_T = torch.randn(n, chans, size, size, device=dev, generator=gen)
    sargs = dict(timesteps=args.timesteps, sample_type=args.sample_type, skip_type=args.skip_type, eta=args.eta, rescaled=rescaled)
    if args.use_generated_samples:                                   # prune_test.py:231-236: the unpruned model's own samples
        with torch.no_grad():
            x = E.Sampler(model, sched.betas, (chans, size, size), **sargs).sample_image(x_T)
        clean = data.inverse_data_transform(x, rescaled)
        clean = 2.0 * clean - 1.0 if rescaled else clean              # data_transform of the shipped configs
    else:
        if not dc:
            raise SystemExit('the sweep\'s images come from the config\'s data: block (--config), or pass --use_generated_samples')
        ds, kw = data.dataset_from_config(dc, root=args.data_root, train=True)
        clean = next(iter(data.DeviceLoader(ds, args.taylor_batch_size, dev, shuffle=True, seed=args.seed, drop_last=True, **kw)))
    noise = torch.randn(clean.shape, device=dev, generator=gen)
    os.makedirs(args.out, exist_ok=True)
    res = S.run(model, sched, clean, noise, x_T, args.stages, pruning_ratio=args.pruning_ratio, loss_kind='sum',
                importance=importance_of(args.pruner), sampler_args=sargs, out_dir=args.out, n_ssim=args.n_ssim)
    res['steps_for_threshold'] = {str(t): S.steps_for_threshold(res['losses'], t) for t in args.thr}
    res['args'] = vars(args)
    path = os.path.join(args.out, 'stage_study.json')
    with open(path, 'w') as f:
        json.dump(res, f)
    print('stages %s\nssim   %s\nwrote %s' % (res['stages'], ['%.4f' % p['ssim'] for p in res['per_stage']], path))
    return res


if __name__ == '__main__':
    main()
