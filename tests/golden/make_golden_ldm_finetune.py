#!/usr/bin/env python3
"""Golden vectors of the LDM finetune step (build container only, on the CPU; seconds): K = 3 training
steps of the reference's own LatentDiffusion -- get_learned_conditioning, p_losses, the AdamW that configure_optimizers builds
(ldm/models/diffusion/ddpm.py:553-565, 1022-1056, 1372-1381: UNet + class embedder, "Also optimizing conditioner params!") and
LitEma (ldm/modules/ema.py) -- on the object make_golden_ldm._latent_diffusion() builds behind empty stand-ins for Lightning /
taming.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_ldm_finetune.py

Width: dict(LDM_TINY_CFG, model_channels=64), NOT the 32 channels of the other LDM fixtures.  With one channel per GroupNorm group
the biases in front of a GroupNorm have a gradient that is zero in exact arithmetic and rounding noise in fp32, and Adam's
m / sqrt(v) turns that noise into full-size steps: no fp32 run, the reference's included, is then comparable with another.

B = 4, class ids [3, 500, 3, 1000] (a repeated id and the unconditional one), per-image timesteps [0, 250, 999, 17 + k], the same
x_start at every step, noise per step, all from golden_common.det_noise; lr 1.28e-4 (run.sh: 2e-6 x 16 x 4 GPUs).

The model has 44 M parameters and a committed file at most 1 MiB, so the fixture stores of EVERY tensor (UNet parameters in
named_parameters order, then the embedding): sum and abs-sum of its step-1 gradient, of its value after step K and of its LitEma
shadow after step K (json), and the same three quantities at tests/ldm_finetune_ref.sample_index's elements -- the whole tensor up
to 96 elements, else 96 evenly strided ones; of the embedding the rows 3, 7, 500, 1000 (npz, concatenated in that order).  In full: the step-1 gradient rows and the final
rows of the touched embedding ids, the final embedding row 7 (weight decay only), a few named tensors.  Data only."""
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import golden_common as gc                      # noqa: E402
import make_golden_ldm as M                     # noqa: E402  (reference imports + the LatentDiffusion stand-in scaffolding)
from ldm_finetune_ref import FIXTURE_CFG, LR, EMA_DECAY, EMB_ROWS, sample_index      # noqa: E402

IDS, K, X_SEED, NOISE_SEED = [3, 500, 3, 1000], 3, 80, 90
FULL = ('input_blocks.0.0.weight', 'input_blocks.4.1.transformer_blocks.0.attn2.to_v.weight',
        'input_blocks.4.1.transformer_blocks.0.attn2.to_q.weight', 'input_blocks.4.1.transformer_blocks.0.norm2.weight',
        'time_embed.0.bias', 'out.2.weight', 'out.2.bias')


def _stats(t):
    return [float(t.double().sum()), float(t.double().abs().sum())]


def main():
    torch.set_num_threads(16)
    from ldm.modules.ema import LitEma
    saved = gc.LDM_TINY_CFG
    gc.LDM_TINY_CFG = FIXTURE_CFG               # _latent_diffusion() builds whatever golden_common calls the tiny LDM config
    try:
        ld, cfg = M._latent_diffusion()
    finally:
        gc.LDM_TINY_CFG = saved
    assert cfg['model_channels'] == 64
    ld.train()
    ld.learning_rate, ld.use_scheduler = LR, False
    opt = ld.configure_optimizers()
    g = opt.param_groups[0]
    assert type(opt).__name__ == 'AdamW' and (g['lr'], g['betas'], g['eps'], g['weight_decay']) == (LR, (0.9, 0.999), 1e-8, 0.01)
    ema = LitEma(ld.model, decay=EMA_DECAY)
    unet, emb = ld.model.diffusion_model, ld.cond_stage_model.embedding.weight
    names = [n for n, _ in unet.named_parameters()]
    tensors = lambda: [p for _, p in unet.named_parameters()] + [emb]           # noqa: E731
    all_names = names + ['embedding.weight']

    def samples(ts):
        return np.concatenate([t.detach().reshape(-1).numpy()[sample_index(t.numel(), name=n, row=t.shape[-1] if t.dim() else 1)]
                               for n, t in zip(all_names, ts)])
    H = cfg['image_size']
    shape = (len(IDS), cfg['in_channels'], H, H)
    x = torch.from_numpy(gc.det_noise(shape, X_SEED))
    ids = torch.tensor(IDS)
    meta = dict(config=cfg, class_ids=IDS, steps=K, x_seed=X_SEED, noise_seed=NOISE_SEED, lr=LR, ema_decay=EMA_DECAY,
                timesteps=[], losses=[], names=names + ['embedding.weight'],
                shapes=[list(p.shape) for p in tensors()], ema_buffers=len(list(ema.buffers())))
    arrays = {}
    for k in range(K):
        t = torch.tensor([0, 250, 999, 17 + k])
        noise = torch.from_numpy(gc.det_noise(shape, NOISE_SEED + k))
        c = ld.get_learned_conditioning({'class_label': ids})
        loss, _ = ld.p_losses(x, c, t, noise=noise)
        opt.zero_grad()
        loss.backward()
        if k == 0:
            gs = [p.grad if p.grad is not None else torch.zeros_like(p) for p in tensors()]
            meta['grad1_stats'] = [_stats(g_) for g_ in gs]
            meta['grad1_zero'] = [n for n, g_ in zip(meta['names'], gs) if float(g_.abs().max()) == 0.0]
            arrays['grad1_samples'] = samples(gs)
            for n in FULL:
                arrays['grad1:' + n] = dict(unet.named_parameters())[n].grad.numpy().copy()
            arrays['grad1_emb_rows'] = emb.grad[sorted(set(IDS))].numpy().copy()
        opt.step()
        ema(ld.model)
        meta['timesteps'].append(t.tolist())
        meta['losses'].append(float(loss.detach()))
    ps = [p.detach() for p in tensors()]
    meta['final_stats'] = [_stats(p) for p in ps]
    arrays['final_samples'] = samples(ps)
    shadow = dict(ema.named_buffers())
    ss = [shadow[ema.m_name2s_name['diffusion_model.' + n]] for n in names]
    meta['ema_stats'] = [_stats(s) for s in ss]
    meta['ema_decay_after'] = float(shadow['decay'])
    meta['ema_num_updates'] = int(shadow['num_updates'])
    arrays['ema_samples'] = samples(ss)
    P = dict(unet.named_parameters())
    for n in FULL:
        arrays['final:' + n] = P[n].detach().numpy().copy()
        arrays['ema:' + n] = ss[names.index(n)].numpy().copy()
    arrays['final_emb_rows'] = emb.detach()[list(EMB_ROWS)].numpy().copy()
    meta['emb_rows'] = list(EMB_ROWS)
    meta['grad1_emb_row_ids'] = sorted(set(IDS))
    meta['full'] = list(FULL)
    np.savez_compressed(os.path.join(HERE, 'ldm_finetune.npz'), **arrays)
    with open(os.path.join(HERE, 'ldm_finetune.json'), 'w') as f:
        json.dump(meta, f)
    print('ldm finetune ok: losses', meta['losses'], 'zero-gradient tensors', len(meta['grad1_zero']), 'of', len(meta['names']),
          'ema buffers', meta['ema_buffers'])


if __name__ == '__main__':
    main()
