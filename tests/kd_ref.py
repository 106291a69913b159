"""Restatement of the distillation finetune loss (ddpm_exp/functions/losses.py:17-31) on the oracle's UNet forward, for the
KD tests (test infrastructure only).  Pinned against tests/golden/kd.npz / kd.json, written by the reference itself
(tests/golden/make_golden_kd.py); the full-size GPU test relies on it."""
import contextlib

import numpy as np
import torch

import golden_common as gc
from oracle import diffusion_ref as D
from oracle import unet_ref as U


def reference_acp():
    """alpha-bar as ddpm_exp computes it: get_beta_schedule('linear') in fp64 -> fp32 betas, (1 - b).cumprod in fp32."""
    betas = torch.from_numpy(np.linspace(1e-4, 0.02, 1000, dtype=np.float64)).float()
    return (1 - betas).cumprod(dim=0)


@contextlib.contextmanager
def _embedding_in(dtype):
    """The oracle's sinusoidal embedding is fp32, as the reference computes it; an fp64 restatement takes those values exactly."""
    real = U.timestep_embedding
    if dtype != torch.float32:
        U.timestep_embedding = lambda *a, **k: real(*a, **k).to(dtype)
    try:
        yield
    finally:
        U.timestep_embedding = real


def kd_loss(Ps, cfg_s, Pt, cfg_t, clean, noise, t, weights=(0.7, 0.3), drop=None, acp=None):
    """Returns (loss, kd, eps, S, T) in the dtype of the parameters: S = student(x, t) (with `drop`, a philox_ref.DropSpec),
    T = teacher(x, t) without gradient, loss = w_kd mean_b sum_chw (T - S)^2 + w_eps mean_b sum_chw (e - S)^2."""
    acp = D.alphas_cumprod() if acp is None else acp
    x = D.add_noise(acp, clean, noise, t)
    with _embedding_in(next(iter(Ps.values())).dtype):
        S = U.unet_forward(Ps, cfg_s, x, t, drop)
        with torch.no_grad():
            T = U.unet_forward(Pt, cfg_t, x, t)
    kd = (T - S).square().sum(dim=(1, 2, 3)).mean(dim=0)
    eps = (noise - S).square().sum(dim=(1, 2, 3)).mean(dim=0)
    return weights[0] * kd + weights[1] * eps, kd, eps, S, T


def original_state_dict(ckpt, arch, seed, unet_cls):
    """The original-DDPM `Model` state dict the fixture generator initialised: det_param by ORIGINAL name and shape (the
    names / shapes come from this package's inverse converter, so no reference import is needed)."""
    cfg = ckpt.unet2d_config_from_ddpm_original(arch['ch'], arch['ch_mult'], arch['num_res_blocks'], arch['attn_resolutions'],
                                                arch['image_size'])
    shapes = {k: tuple(v.shape) for k, v in ckpt.convert_to_ddpm_original(unet_cls(**cfg).state_dict()).items()}
    return cfg, {k: torch.from_numpy(gc.det_param(k, s, seed)) for k, s in shapes.items()}
