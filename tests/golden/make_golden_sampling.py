#!/usr/bin/env python3
"""Teacher-forced sampling fixtures of the full-size CIFAR-10 UNet (run in the build container only, on the CPU; imports the
reference's UNet2DModel, DDIMScheduler and DDPMScheduler through make_golden.py's import shim).

On seeded weights the 100-step DDIM chain is chaotic: the reference's own fp32 run leaves its fp64 run after ~10 steps and ends
with almost every uint8 value different.  So the fixtures pin what stays meaningful:
  * per step: the input x_k of the reference's fp64 trajectory (rounded to fp32), the fp64 eps on that x_k and the fp64
    DDIMScheduler.step output on (eps, x_k) -- plus the reference's own fp32 eps error on x_k and the share of x0 at the clip bound;
  * the early chain: the fp64 trajectory at a few states and the reference fp32 chain's gap to it at every state.
Models: 'full' = CIFAR_CFG with det_init_(m, 0); 'pruned' = the same after make_golden.do_c1's sweep and ratio-0.3 prune
(19 851 157 parameters, cifar_c1.json shapes).  x_T = torch.randn from torch.Generator().manual_seed(seed) (the pipeline's
randn_tensor path).  Step 99 has t = 0: prev_t < 0, so the step uses final_alpha_cumprod.  "fp64" is the reference model cast to
double as it stands: its attention blocks upcast the softmax to fp32 (upcast_softmax), which the fp64 oracle restates too.
Stored arrays are fp32; the fp64 sum / abs-sum / sum of squares of every stored eps and step output are kept beside them.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_sampling.py

Writes sampling_cifar.npz (full model + early chain), sampling_cifar_pruned.npz and sampling_cifar_edges.npz (DDIM eta 0.5,
skip_type 'quad', DDPMScheduler fixed_small at t in {999, 500, 1, 0}; teacher-forced on the full model)."""
import copy
import json
import os
import sys
import time
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg                                            # noqa: E402  (reference import shim, model builders)
import golden_common as gc                                          # noqa: E402
from diffusers import DDIMScheduler, DDPMScheduler                  # noqa: E402  (reference)
from diffusers.models.attention_processor import Attention, AttnProcessor      # noqa: E402
import diffusers.schedulers.scheduling_ddpm as ref_ddpm_mod         # noqa: E402

B = 2
N_STEPS = 100
STEPS = [0, 1, 10, 25, 50, 75, 98, 99]        # teacher-forced step indices (into the 100 uniform timesteps)
CHAIN_STATES = [1, 2, 3, 5, 8, 10]            # x_k of the free-running fp64 chain (x_k = input of step k, x_0 = x_T)
MODEL_SEED = 0
XT_SEED = {'full': 7, 'pruned': 8}
ETA, ETA_STEPS, ETA_NOISE_SEEDS = 0.5, [50, 98], [41, 42]
QUAD_STEPS = [0, 1]                           # first two steps of the quad schedule from the full model's x_T
DDPM_T, DDPM_X_FROM, DDPM_NOISE_SEEDS = [999, 500, 1, 0], [None, 50, 98, 99], [43, 44, 45, 46]


def _ddim(skip='uniform'):
    s = DDIMScheduler(num_train_timesteps=1000)
    s.skip_type = skip
    s.set_timesteps(N_STEPS)
    return s


def _x0_clip_share(s, x, eps, t):
    a = s.alphas_cumprod[int(t)].double()
    x0 = (x - (1 - a) ** 0.5 * eps) / a ** 0.5
    return float((x0.abs() > 1.0).double().mean())


def _u8(x):
    return ((x.double() / 2 + 0.5).clamp(0, 1) * 255).round().to(torch.uint8).numpy()


def _sums(a):
    a = a.double()
    return [float(a.sum()), float(a.abs().sum()), float((a * a).sum())]


def _models():
    full = mg.build_ref_unet(gc.CIFAR_CFG, MODEL_SEED)
    pruned = mg.build_ref_unet(gc.CIFAR_CFG, MODEL_SEED)            # make_golden.do_c1, step for step
    sched = DDPMScheduler(num_train_timesteps=1000)
    clean = torch.from_numpy(gc.det_clean((4, 3, 32, 32), 1))
    noise = torch.from_numpy(gc.det_noise((4, 3, 32, 32), 2))
    mg.sweep(pruned, sched, clean, noise, 8)
    mg.prune_run(pruned, 32, 0.3)
    c1 = json.load(open(os.path.join(HERE, 'cifar_c1.json')))
    n = sum(p.numel() for p in pruned.parameters())
    assert n == 19851157 == c1['params_after'], n
    assert {k: list(p.shape) for k, p in pruned.named_parameters()} == c1['shapes_after']
    out = {}
    for name, m in (('full', full), ('pruned', pruned)):
        for mod in m.modules():
            if isinstance(mod, Attention):
                mod.set_processor(AttnProcessor())
        m.zero_grad(set_to_none=True)
        for p in m.parameters():
            p.requires_grad_(False)
        m.eval()
        out[name] = (m, copy.deepcopy(m).double())
    return out


@torch.no_grad()
def _teacher_forced(m32, m64, s, x_in, t):
    """(x rounded to fp32, fp64 eps on it, fp64 step output, reference fp32 eps error, x0 clip share)."""
    x = x_in.float()
    x64 = x.double()
    eps64 = m64(x64, t).sample
    eps32 = m32(x, t).sample
    out64 = s.step(eps64, t, x64, eta=0.0).prev_sample
    return x, eps64, out64, float((eps32.double() - eps64).abs().max()), _x0_clip_share(s, x64, eps64, t)


@torch.no_grad()
def do_model(name, m32, m64, with_chain):
    s = _ddim()
    ts = s.timesteps.clone()
    x_T = torch.randn((B, 3, 32, 32), generator=torch.Generator().manual_seed(XT_SEED[name]))
    from diffusers.utils import randn_tensor
    assert torch.equal(x_T, randn_tensor((B, 3, 32, 32), generator=torch.Generator().manual_seed(XT_SEED[name])))
    t0 = time.time()
    traj64 = [x_T.double()]
    for t in ts:                                                     # the reference's fp64 100-step uniform DDIM trajectory
        traj64.append(s.step(m64(traj64[-1], t).sample, t, traj64[-1], eta=0.0).prev_sample)
    print('%s: fp64 chain %.1fs' % (name, time.time() - t0))
    rec = dict(x=[], eps=[], out=[], e_ref32=[], clip_share=[], eps_sums=[], out_sums=[])
    for k in STEPS:
        x, eps64, out64, e32, share = _teacher_forced(m32, m64, s, traj64[k], ts[k])
        for key, v in (('x', x.numpy()), ('eps', eps64.float().numpy()), ('out', out64.float().numpy()), ('e_ref32', e32),
                       ('clip_share', share), ('eps_sums', _sums(eps64)), ('out_sums', _sums(out64))):
            rec[key].append(v)
        print('  step %2d t=%3d  e_ref32 %.2e  x0 clipped %.3f' % (k, int(ts[k]), e32, share))
    res = dict(model_seed=np.int64(MODEL_SEED), xT_seed=np.int64(XT_SEED[name]), n_steps=np.int64(N_STEPS),
               steps=np.array(STEPS, np.int64), timesteps=ts.numpy()[STEPS].astype(np.int64), x_T=x_T.numpy(),
               params=np.int64(sum(p.numel() for p in m32.parameters())),
               **{k: np.array(v, np.float32 if k in ('x', 'eps', 'out') else np.float64) for k, v in rec.items()})
    if with_chain:
        x32 = x_T.clone()
        gap = [0.0]
        for t in ts:                                                 # the reference's own fp32 chain
            x32 = s.step(m32(x32, t).sample, t, x32, eta=0.0).prev_sample
            gap.append(float((x32.double() - traj64[len(gap)]).abs().max()))
        u64, u32 = _u8(traj64[-1]), _u8(x32)
        res.update(chain_states=np.array(CHAIN_STATES, np.int64),
                   chain_x=np.stack([traj64[k].float().numpy() for k in CHAIN_STATES]),
                   chain_gap_ref32=np.array(gap, np.float64),
                   end_x_fp64=traj64[-1].float().numpy(), end_x_fp32=x32.numpy(), image_u8_fp64=u64, image_u8_fp32=u32,
                   end_abs_ref32=np.float64((x32.double() - traj64[-1]).abs().max()))
        print('  fp32 chain gap at states 1..10:', ['%.1e' % g for g in gap[1:11]], 'end %.2f, uint8 differing %d / %d'
              % (gap[-1], int((u64 != u32).sum()), u64.size))
    return res, traj64


@torch.no_grad()
def do_edges(m32, m64, traj64, x_T):
    res = {}
    s = _ddim()
    ts = s.timesteps
    for j, (k, seed) in enumerate(zip(ETA_STEPS, ETA_NOISE_SEEDS)):   # DDIM eta 0.5, caller-supplied variance noise
        t = ts[k]
        x = traj64[k].float()
        vn = torch.from_numpy(gc.det_noise((B, 3, 32, 32), seed))
        eps64 = m64(x.double(), t).sample
        out64 = s.step(eps64, t, x.double(), eta=ETA, variance_noise=vn.double()).prev_sample
        e32 = float((m32(x, t).sample.double() - eps64).abs().max())
        res.update({'eta:%d:x' % j: x.numpy(), 'eta:%d:eps' % j: eps64.float().numpy(), 'eta:%d:out' % j: out64.float().numpy(),
                    'eta:%d:noise' % j: vn.numpy(), 'eta:%d:t' % j: np.int64(t), 'eta:%d:step' % j: np.int64(k),
                    'eta:%d:noise_seed' % j: np.int64(seed), 'eta:%d:e_ref32' % j: np.float64(e32),
                    'eta:%d:out_sums' % j: np.array(_sums(out64))})
    res['eta'] = np.float64(ETA)
    q = _ddim('quad')
    qs = q.timesteps
    x = x_T.double()
    for k in range(max(QUAD_STEPS) + 1):                             # the quad chain's first steps (prev_t = t - T // n quirk)
        t = qs[k]
        eps64 = m64(x.float().double(), t).sample
        out64 = q.step(eps64, t, x.float().double(), eta=0.0).prev_sample
        if k in QUAD_STEPS:
            j = QUAD_STEPS.index(k)
            e32 = float((m32(x.float(), t).sample.double() - eps64).abs().max())
            res.update({'quad:%d:x' % j: x.float().numpy(), 'quad:%d:eps' % j: eps64.float().numpy(),
                        'quad:%d:out' % j: out64.float().numpy(), 'quad:%d:t' % j: np.int64(t), 'quad:%d:step' % j: np.int64(k),
                        'quad:%d:e_ref32' % j: np.float64(e32), 'quad:%d:out_sums' % j: np.array(_sums(out64))})
        x = out64
    res['quad_timesteps'] = qs.numpy().astype(np.int64)
    d = DDPMScheduler(num_train_timesteps=1000, variance_type='fixed_small')
    d.set_timesteps(1000)
    real = ref_ddpm_mod.randn_tensor
    for j, (t, src, seed) in enumerate(zip(DDPM_T, DDPM_X_FROM, DDPM_NOISE_SEEDS)):
        x = (x_T if src is None else traj64[src]).float()
        vn = torch.from_numpy(gc.det_noise((B, 3, 32, 32), seed))
        drawn = []
        ref_ddpm_mod.randn_tensor = lambda shape, generator=None, device=None, dtype=None: (drawn.append(1), vn.to(dtype))[1]
        try:
            eps64 = m64(x.double(), t).sample
            out64 = d.step(eps64, t, x.double()).prev_sample
        finally:
            ref_ddpm_mod.randn_tensor = real
        assert len(drawn) == (1 if t > 0 else 0), (t, drawn)
        e32 = float((m32(x, t).sample.double() - eps64).abs().max())
        res.update({'ddpm:%d:x' % j: x.numpy(), 'ddpm:%d:eps' % j: eps64.float().numpy(), 'ddpm:%d:out' % j: out64.float().numpy(),
                    'ddpm:%d:noise' % j: vn.numpy(), 'ddpm:%d:t' % j: np.int64(t), 'ddpm:%d:noise_seed' % j: np.int64(seed),
                    'ddpm:%d:e_ref32' % j: np.float64(e32), 'ddpm:%d:out_sums' % j: np.array(_sums(out64))})
    res['n_eta'], res['n_quad'], res['n_ddpm'] = np.int64(len(ETA_STEPS)), np.int64(len(QUAD_STEPS)), np.int64(len(DDPM_T))
    return res


def _savez(name, arrays):
    """np.savez with a fixed member timestamp: regenerating the fixtures gives the same bytes."""
    with zipfile.ZipFile(os.path.join(HERE, name), 'w', zipfile.ZIP_STORED) as z:
        for k in sorted(arrays):
            with z.open(zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0)), 'w', force_zip64=True) as f:
                np.lib.format.write_array(f, np.asanyarray(arrays[k]), allow_pickle=False)


def main():
    t0 = time.time()
    models = _models()
    print('models %.1fs' % (time.time() - t0))
    full, traj = do_model('full', *models['full'], with_chain=True)
    _savez('sampling_cifar.npz', full)
    edges = do_edges(*models['full'], traj, torch.from_numpy(full['x_T']))
    _savez('sampling_cifar_edges.npz', edges)
    pruned, _ = do_model('pruned', *models['pruned'], with_chain=False)
    _savez('sampling_cifar_pruned.npz', pruned)
    for f in ('sampling_cifar.npz', 'sampling_cifar_edges.npz', 'sampling_cifar_pruned.npz'):
        print(f, os.path.getsize(os.path.join(HERE, f)))
    print('done %.1fs' % (time.time() - t0))


if __name__ == '__main__':
    main()
