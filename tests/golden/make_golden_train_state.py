#!/usr/bin/env python3
"""Golden vectors of the training state a stopped finetune continues from (build container only, on the CPU; reads the reference at
generation time, commits data only).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_train_state.py

DDPM: the DDIM code base's own `Model` (tiny width: ch 32, ch_mult [1, 2, 2, 2], 2 res blocks, attention at 8, 16 x 16; its
GroupNorm has 32 groups), `get_optimizer` from configs/cifar10.yml's optim section and `EMAHelper(0.9999)`, driven by the runner's
step (runners/diffusion.py:286-322: antithetic t, noise_estimation_loss, zero_grad, backward, clip_grad_norm_(1.0), step,
ema update) without dropout (torch's dropout RNG is not the engine's Philox).  After step 3 the `states` list of :331-344 is taken
-- [model, optimizer.state_dict(), epoch, step, ema_helper.state_dict()] -- then two further steps run.  In fp32 and in fp64.
Weights come from golden_common.det_param by ORIGINAL name (tests/kd_ref.original_state_dict rebuilds them).

LDM: make_golden_ldm._latent_diffusion() (LatentDiffusion at LDM_TINY_CFG) + the AdamW of configure_optimizers + LitEma as in
make_golden_ldm_finetune.py: the optimizer state after 2 steps, then one further step.  fp32 and fp64 (in fp64 the sinusoidal
embedding keeps its fp32 values, as tests/ldm_finetune_ref does).

Committed: the parameter-name order of each model's parameters(), `step` and `param_groups`, the structure of the states list, losses,
and per tensor (in that order) 96 sampled elements (tests/ldm_finetune_ref.sample_index; of the class embedding the rows 3, 7, 500,
1000) of exp_avg, exp_avg_sq, the shadow (at the save step) and the parameters after the last step -- the fp32 run's values and the
fp64 run's as `fp32 + delta64` -- plus e_ref32, the fp32 run's distance from the fp64 run in the measure the tests use
(max |a - b| over all samples / max |b|).  One .npz per array: train_state_<ddpm|ldm>_<array>.npz."""
import json
import os
import sys
from types import SimpleNamespace as NS

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, '/root/reference/ddpm_exp')
import golden_common as gc                                   # noqa: E402
from ldm_finetune_ref import sample_index                    # noqa: E402

ARCH = dict(ch=32, ch_mult=[1, 2, 2, 2], num_res_blocks=2, attn_resolutions=[8], image_size=16)
SEED, B, CLEAN_SEED, NOISE_SEED, T_SEED = 5, 4, 30, 40, 100
SAVE_AT, FURTHER = 3, 2
LDM_IDS, LDM_SAVE_AT, LDM_FURTHER, LDM_X_SEED, LDM_NOISE_SEED, LDM_LR, LDM_EMA_DECAY = [3, 500, 3, 1000], 2, 1, 80, 90, 1.28e-4, 0.9999


def _samples(names, tensors):
    return np.concatenate([t.detach().reshape(-1).double().numpy()[sample_index(t.numel(), name=n, row=t.shape[-1] if t.dim() else 1)]
                           for n, t in zip(names, tensors)])


def _gap(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


def _jsonable(groups):
    return [{k: (list(v) if isinstance(v, tuple) else v) for k, v in g.items()} for g in groups]


def ddpm(dtype):
    import models.diffusion as MD
    from models.diffusion import Model
    from models.ema import EMAHelper
    from functions import get_optimizer
    config = NS(model=NS(type='simple', in_channels=3, out_ch=3, ch=ARCH['ch'], ch_mult=ARCH['ch_mult'],
                         num_res_blocks=ARCH['num_res_blocks'], attn_resolutions=ARCH['attn_resolutions'], dropout=0.0,
                         resamp_with_conv=True, ema_rate=0.9999, ema=True),
                data=NS(image_size=ARCH['image_size']), diffusion=NS(num_diffusion_timesteps=1000),
                optim=NS(weight_decay=0.0, optimizer='Adam', lr=2e-4, beta1=0.9, amsgrad=False, eps=1e-8, grad_clip=1.0))
    torch.manual_seed(0)
    model = Model(config)
    with torch.no_grad():
        for n, p in model.named_parameters():
            p.copy_(torch.from_numpy(gc.det_param(n, tuple(p.shape), SEED)))
    model = model.to(dtype)
    names = [n for n, _ in model.named_parameters()]
    assert names == list(model.state_dict())
    optimizer = get_optimizer(config, model.parameters())
    ema_helper = EMAHelper(mu=config.model.ema_rate)
    ema_helper.register(model)
    betas = torch.from_numpy(np.linspace(1e-4, 0.02, 1000, dtype=np.float64)).float().to(dtype)      # get_beta_schedule('linear')
    out = dict(names=names, losses=[], timesteps=[])
    real = MD.get_timestep_embedding
    if dtype != torch.float32:                               # the sinusoidal embedding keeps its fp32 values in the fp64 run
        MD.get_timestep_embedding = lambda *a, **k: real(*a, **k).to(dtype)
    try:
        return _ddpm_steps(config, model, optimizer, ema_helper, betas, names, out, dtype)
    finally:
        MD.get_timestep_embedding = real


def _ddpm_steps(config, model, optimizer, ema_helper, betas, names, out, dtype):
    from functions.losses import noise_estimation_loss
    step = 0
    for k in range(SAVE_AT + FURTHER):
        model.train()
        step += 1
        x = torch.from_numpy(gc.det_clean((B, 3, 16, 16), CLEAN_SEED + k)).to(dtype)
        e = torch.from_numpy(gc.det_noise((B, 3, 16, 16), NOISE_SEED + k)).to(dtype)
        t = torch.randint(low=0, high=1000, size=(B // 2 + 1,), generator=torch.Generator().manual_seed(T_SEED + k))
        t = torch.cat([t, 1000 - t - 1], dim=0)[:B]
        loss = noise_estimation_loss(model, x, t, e, betas)
        optimizer.zero_grad()
        loss.backward()
        torch.nn.utils.clip_grad_norm_(model.parameters(), config.optim.grad_clip)
        optimizer.step()
        ema_helper.update(model)
        out['losses'].append(float(loss))
        out['timesteps'].append(t.tolist())
        if step == SAVE_AT:
            states = [model, optimizer.state_dict(), 0, step, ema_helper.state_dict()]
            sd = states[1]
            out.update(states_len=len(states), optimizer_keys=list(sd), state_keys=list(sd['state'][0]),
                       param_groups=_jsonable(sd['param_groups']), steps=[float(sd['state'][i]['step']) for i in range(len(names))],
                       step_dtype=str(sd['state'][0]['step'].dtype), step_dim=sd['state'][0]['step'].dim(),
                       ema_type=type(states[4]).__name__, ema_len=len(states[4]), epoch=states[2], step=states[3],
                       shapes={n: list(p.shape) for n, p in model.named_parameters()},
                       exp_avg=_samples(names, [sd['state'][i]['exp_avg'] for i in range(len(names))]),
                       exp_avg_sq=_samples(names, [sd['state'][i]['exp_avg_sq'] for i in range(len(names))]),
                       shadow=_samples(names, list(states[4])))
    out['params_final'] = _samples(names, [p for p in model.parameters()])
    return out


def unet_modules(ld):
    return list(ld.model.diffusion_model.modules())


def ldm(dtype):
    import make_golden_ldm as M
    from ldm.modules.ema import LitEma
    import ldm.modules.diffusionmodules.openaimodel as OM
    ld, cfg = M._latent_diffusion()
    real = OM.timestep_embedding
    if dtype != torch.float32:
        ld = ld.to(dtype)
        ld.model.diffusion_model.dtype = dtype
        OM.timestep_embedding = lambda *a, **k: real(*a, **k).to(dtype)      # its fp32 values, as tests/ldm_finetune_ref keeps them
        for mod in unet_modules(ld):                         # GroupNorm32 casts its input to fp32: the fp64 run normalises in fp64
            if type(mod).__name__ == 'GroupNorm32':
                mod.forward = (lambda m: lambda x: torch.nn.GroupNorm.forward(m, x))(mod)
    try:
        ld.train()
        ld.learning_rate, ld.use_scheduler = LDM_LR, False
        opt = ld.configure_optimizers()
        assert type(opt).__name__ == 'AdamW'
        ema = LitEma(ld.model, decay=LDM_EMA_DECAY)
        unet, emb = ld.model.diffusion_model, ld.cond_stage_model.embedding.weight
        names = [n for n, _ in unet.named_parameters()] + ['embedding.weight']
        tensors = lambda: [p for _, p in unet.named_parameters()] + [emb]           # noqa: E731
        assert all(a is b for a, b in zip(opt.param_groups[0]['params'], tensors()))      # UNet, then the embedder (ddpm.py:1372-1381)
        H = cfg['image_size']
        shape = (len(LDM_IDS), cfg['in_channels'], H, H)
        x = torch.from_numpy(gc.det_noise(shape, LDM_X_SEED)).to(dtype)
        ids = torch.tensor(LDM_IDS)
        out = dict(names=names, losses=[], timesteps=[])
        for k in range(LDM_SAVE_AT + LDM_FURTHER):
            t = torch.tensor([0, 250, 999, 17 + k])
            noise = torch.from_numpy(gc.det_noise(shape, LDM_NOISE_SEED + k)).to(dtype)
            c = ld.get_learned_conditioning({'class_label': ids})
            loss, _ = ld.p_losses(x, c, t, noise=noise)
            opt.zero_grad()
            loss.backward()
            opt.step()
            ema(ld.model)
            out['losses'].append(float(loss.detach()))
            out['timesteps'].append(t.tolist())
            if k + 1 == LDM_SAVE_AT:
                sd = opt.state_dict()
                shadow = dict(ema.named_buffers())
                ss = [shadow[ema.m_name2s_name['diffusion_model.' + n]] for n in names[:-1]]
                out.update(optimizer_keys=list(sd), state_keys=list(sd['state'][0]), param_groups=_jsonable(sd['param_groups']),
                           steps=[float(sd['state'][i]['step']) for i in range(len(names))], step_dtype=str(sd['state'][0]['step'].dtype),
                           shapes=[list(p.shape) for p in tensors()], num_updates=int(shadow['num_updates']),
                           exp_avg=_samples(names, [sd['state'][i]['exp_avg'] for i in range(len(names))]),
                           exp_avg_sq=_samples(names, [sd['state'][i]['exp_avg_sq'] for i in range(len(names))]),
                           shadow=_samples(names[:-1], ss))
        out['params_final'] = _samples(names, tensors())
        return out
    finally:
        OM.timestep_embedding = real


ARRAYS = ('exp_avg', 'exp_avg_sq', 'shadow', 'params_final')


def main():
    torch.set_num_threads(16)
    meta = {}
    for tag, fn in (('ddpm', ddpm), ('ldm', ldm)):
        r32, r64 = fn(torch.float32), fn(torch.float64)
        assert r32['names'] == r64['names'] and r32['timesteps'] == r64['timesteps']
        m = {k: v for k, v in r32.items() if not isinstance(v, np.ndarray)}
        m['param_names'] = m.pop('names')
        m['losses_fp64'] = r64['losses']
        m['e_ref32'] = {k: _gap(r32[k], r64[k]) for k in ARRAYS}
        m['e_ref32']['loss'] = max(abs(a - b) / abs(b) for a, b in zip(r32['losses'], r64['losses']))
        for k in ARRAYS:
            # one file per array (a committed file stays under 1 MiB): the fp32 run's samples and the fp64 run's as fp32 + delta
            f32 = r32[k].astype(np.float32)
            np.savez_compressed(os.path.join(HERE, 'train_state_%s_%s.npz' % (tag, k)), fp32=f32,
                                delta64=(r64[k] - f32.astype(np.float64)).astype(np.float32))
        meta[tag] = m
        print(tag, 'losses', m['losses'], 'e_ref32', m['e_ref32'], 'tensors', len(m['param_names']))
    meta['ddpm'].update(arch=ARCH, seed=SEED, batch=B, clean_seed=CLEAN_SEED, noise_seed=NOISE_SEED, t_seed=T_SEED, save_at=SAVE_AT,
                        further=FURTHER, ema_rate=0.9999, grad_clip=1.0)
    meta['ldm'].update(class_ids=LDM_IDS, save_at=LDM_SAVE_AT, further=LDM_FURTHER, x_seed=LDM_X_SEED, noise_seed=LDM_NOISE_SEED,
                       lr=LDM_LR, ema_decay=LDM_EMA_DECAY, config=dict(gc.LDM_TINY_CFG))
    with open(os.path.join(HERE, 'train_state.json'), 'w') as f:
        json.dump(meta, f)


if __name__ == '__main__':
    main()
