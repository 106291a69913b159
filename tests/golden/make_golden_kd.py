#!/usr/bin/env python3
"""Golden vectors of the distillation finetune step (run in the build container only, on the CPU; imports the reference's
ddpm_exp/models/diffusion.py `Model` and ddpm_exp/functions/losses.py `noise_estimation_kd_loss`).

Teacher: Model(ch=64, ch_mult=[1, 2, 2, 2], num_res_blocks=2, attn_resolutions=[8], image_size=16), eval mode.
Student: the same with ch=32 (a narrower student), train mode, dropout 0 (torch's dropout RNG is not the engine's Philox; the
engine's masks are pinned by tiny_dropout.json).  Weights come from golden_common.det_param by ORIGINAL parameter name, so the
tests rebuild them without the reference and convert them with checkpoint.convert_ddpm_original.

One step as runners/diffusion.py:295-324 runs it with --kd: antithetic t from a seeded generator, linear betas, the KD loss,
backward, clip_grad_norm_(1.0), torch.optim.Adam as functions/__init__.py:4-8 builds it from configs/cifar10.yml, then
EMAHelper(0.9999).update.

Writes kd.npz (S, T, full gradients of three tensors) and kd.json (loss, terms, per-parameter statistics)."""
import json
import os
import sys
from types import SimpleNamespace as NS

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, '/root/reference/ddpm_exp')
import golden_common as gc                     # noqa: E402
from models.diffusion import Model             # noqa: E402
from models.ema import EMAHelper               # noqa: E402
from functions.losses import noise_estimation_kd_loss     # noqa: E402

BASE = dict(ch_mult=[1, 2, 2, 2], num_res_blocks=2, attn_resolutions=[8], image_size=16)
TEACHER = dict(BASE, ch=64)
STUDENT = dict(BASE, ch=32)
T_SEED, S_SEED = 61, 62
B, CLEAN_SEED, NOISE_SEED, T_GEN_SEED = 4, 63, 64, 65
FULL = ('conv_in.weight', 'down.1.attn.0.q.weight', 'conv_out.weight')


def _model(c):
    config = NS(model=NS(type='simple', in_channels=3, out_ch=3, ch=c['ch'], ch_mult=c['ch_mult'],
                         num_res_blocks=c['num_res_blocks'], attn_resolutions=c['attn_resolutions'], dropout=0.0,
                         resamp_with_conv=True),
                data=NS(image_size=c['image_size']), diffusion=NS(num_diffusion_timesteps=1000))
    return Model(config)


def _init(model, seed):
    with torch.no_grad():
        for n, p in model.named_parameters():
            p.copy_(torch.from_numpy(gc.det_param(n, tuple(p.shape), seed)))


def _stats(t):
    return [float(t.double().sum()), float(t.double().abs().sum())]


def main():
    torch.manual_seed(0)
    teacher, student = _model(TEACHER), _model(STUDENT)
    _init(teacher, T_SEED)
    _init(student, S_SEED)
    teacher.eval()
    student.train()
    x0 = torch.from_numpy(gc.det_clean((B, 3, 16, 16), CLEAN_SEED))
    e = torch.from_numpy(gc.det_noise((B, 3, 16, 16), NOISE_SEED))
    gen = torch.Generator().manual_seed(T_GEN_SEED)
    t = torch.randint(low=0, high=1000, size=(B // 2 + 1,), generator=gen)          # runners/diffusion.py:295-299
    t = torch.cat([t, 1000 - t - 1], dim=0)[:B]
    betas = torch.from_numpy(np.linspace(1e-4, 0.02, 1000, dtype=np.float64)).float()   # get_beta_schedule('linear')
    loss = noise_estimation_kd_loss(student, teacher, x0, t, e, betas)
    # the two terms and both outputs, recomputed outside the loss (same inputs, no grad)
    with torch.no_grad():
        a = (1 - betas).cumprod(dim=0).index_select(0, t).view(-1, 1, 1, 1)
        x = x0 * a.sqrt() + e * (1.0 - a).sqrt()
        S = student(x, t.float())
        T = teacher(x, t.float())
        kd = (T - S).square().sum(dim=(1, 2, 3)).mean(dim=0)
        eps = (e - S).square().sum(dim=(1, 2, 3)).mean(dim=0)
    optimizer = torch.optim.Adam(student.parameters(), lr=2e-4, weight_decay=0.0, betas=(0.9, 0.999), amsgrad=False, eps=1e-8)
    ema = EMAHelper(mu=0.9999)
    ema.register(student)
    optimizer.zero_grad()
    loss.backward()
    grad_stats = {n: _stats(p.grad) for n, p in student.named_parameters()}
    full = {n: p.grad.detach().clone() for n, p in student.named_parameters() if n in FULL}
    norm = torch.nn.utils.clip_grad_norm_(student.parameters(), 1.0)
    optimizer.step()
    ema.update(student)
    param_stats = {n: _stats(p.detach()) for n, p in student.named_parameters()}
    ema_stats = {n: _stats(s) for (n, _), s in zip(student.named_parameters(), ema.shadow)}
    np.savez(os.path.join(HERE, 'kd.npz'), S=S.numpy(), T=T.numpy(),
             **{'grad:' + n: g.numpy() for n, g in full.items()})
    json.dump(dict(teacher=TEACHER, student=STUDENT, teacher_seed=T_SEED, student_seed=S_SEED, batch=B, clean_seed=CLEAN_SEED,
                   noise_seed=NOISE_SEED, timesteps=[int(v) for v in t], weights=[0.7, 0.3],
                   loss=float(loss), kd=float(kd), eps=float(eps), grad_norm=float(norm),
                   grad_stats=grad_stats, full_grads=list(FULL), param_stats=param_stats, ema_stats=ema_stats,
                   optim=dict(lr=2e-4, betas=[0.9, 0.999], eps=1e-8, weight_decay=0.0, grad_clip=1.0, ema_rate=0.9999)),
              open(os.path.join(HERE, 'kd.json'), 'w'))
    print('kd ok: loss %.6f (kd %.6f, eps %.6f), grad norm %.4f, teacher %d / student %d parameters'
          % (float(loss), float(kd), float(eps), float(norm), sum(p.numel() for p in teacher.parameters()),
             sum(p.numel() for p in student.parameters())))


if __name__ == '__main__':
    main()
