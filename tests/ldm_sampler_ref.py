"""What the ldm_exp sampler tests share: the case lists, the toy model of the CPU chains (tests/golden/make_golden_ldm_sampler.py
runs the reference's samplers over it too), the fp32 schedule, the fixture readers and the issue's bounds.  No reference code."""
import os

import numpy as np
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
U = 2.0 ** -24                                   # unit roundoff of fp32

TABLES_FILE = 'ldm_sampler_tables.npz'
STEPS_FILE = 'ldm_sampler_steps.npz'
TOY_FILE = 'ldm_sampler_toy.npz'
CHAINS_FILE = 'ldm_sampler_chains.npz'

TABLE_S, TABLE_ETAS, TABLE_DISCR = (20, 50, 250), (0.0, 0.5, 1.0), ('uniform', 'quad')
COLS = ('s1m', 'sqrt_a_t', 'sqrt_a_prev', 'c_dir', 'sigma')

STEP_SHAPE = (2, 3, 16, 16)
# name -> (sampler, S, eta, index, guidance scale (None: unguided), temperature, history length (PLMS))
STEP_CASES = {
    'ddim:eta0': ('ddim', 20, 0.0, 13, 3.0, 1.0, None),
    'ddim:eta0.5:temp0.8': ('ddim', 20, 0.5, 7, 3.0, 0.8, None),
    'ddim:eta1:scale1.5': ('ddim', 50, 1.0, 49, 1.5, 1.0, None),
    'ddim:eta1:unguided': ('ddim', 50, 1.0, 0, None, 1.0, None),
    'ddim:eta0:unguided': ('ddim', 20, 0.0, 19, None, 1.0, None),
    'plms:h0': ('plms', 20, 0.0, 19, 3.0, 1.0, 0),           # two evaluations: orders 0 and 4 of the kernel
    'plms:h1': ('plms', 20, 0.0, 18, 3.0, 1.0, 1),
    'plms:h2': ('plms', 20, 0.0, 17, 3.0, 1.0, 2),
    'plms:h3': ('plms', 20, 0.0, 9, 3.0, 1.0, 3),
    'plms:h3:unguided': ('plms', 20, 0.0, 0, None, 1.0, 3),
}

TOY_SHAPE = (2, 3, 8, 8)
TOY_CTX = 4
# name -> (sampler, discretisation, S, eta, temperature)
TOY_CHAINS = {
    'ddim:uniform:eta0': ('ddim', 'uniform', 20, 0.0, 1.0),
    'ddim:quad:eta0': ('ddim', 'quad', 20, 0.0, 1.0),
    'ddim:uniform:eta0.5': ('ddim', 'uniform', 20, 0.5, 0.8),
    'ddim:quad:eta0.5': ('ddim', 'quad', 20, 0.5, 0.8),
    'ddim:uniform:eta1:S50': ('ddim', 'uniform', 50, 1.0, 1.0),
    'plms:uniform': ('plms', 'uniform', 20, 0.0, 1.0),
}
TOY_SCALE = 3.0
LOG_EVERY = 5

# the chains on LDM_TINY_CFG (B = 2, 16 x 16, the weights and inputs of ldm_sampler.npz): name -> (sampler, eta, temperature)
UNET_CHAINS = {'ddim:eta0': ('ddim', 0.0, 1.0), 'ddim:eta0.5': ('ddim', 0.5, 0.8), 'plms': ('plms', 0.0, 1.0)}
UNET_S, UNET_SCALE, UNET_SEED = 20, 3.0, 9
X_T_SEED, COND_SEED, UNCOND_SEED = 51, 52, 53


def load(name):
    return np.load(os.path.join(GOLD, name))


def table_key(S, eta, discr):
    return '%d:%g:%s' % (S, eta, discr)


def alphas_cumprod32():
    """The fp32 table LatentDiffusion registers at cin256-v2 (linear_start 0.0015, linear_end 0.0195): fp64 cumprod, cast once."""
    betas = torch.linspace(0.0015 ** 0.5, 0.0195 ** 0.5, 1000, dtype=torch.float64) ** 2
    return torch.tensor(np.cumprod(1.0 - betas.numpy(), axis=0), dtype=torch.float32)


class Schedule:
    num_timesteps = 1000

    def __init__(self):
        self.alphas_cumprod = alphas_cumprod32()


def toy_model(x, t, c):
    """A smooth eps(x, t, context) with cross-pixel and cross-channel coupling, in x's dtype.  Only correctly rounded elementwise
    operations (add, multiply, divide, abs) and moves, each its own torch call: the same bits on every host, so that a chain over
    it can be compared with the reference's own run for equality.  t: one integer per row; c: [rows, 1, TOY_CTX]."""
    s = (t.to(x.dtype) / 1000.0).view(-1, 1, 1, 1)
    k = (c.to(x.dtype)[:, 0, 0] * 0.5 + c.to(x.dtype)[:, 0, TOY_CTX - 1] * 0.25).view(-1, 1, 1, 1)
    mix = torch.roll(x, shifts=(1, 1), dims=(1, 3)) * 0.25 + torch.roll(x, shifts=1, dims=2) * 0.125
    u = x * 0.5 + mix + k
    v = torch.roll(x, shifts=2, dims=3) * 0.75 + s * 3.0
    return u / (u.abs() + 1.0) * (s * 0.25 + 0.75) + v / (v.abs() + 1.0) * 0.125


def single_step_bound(e_ref32, y64):
    """The bound of a fixture step: max(4 e_ref32, 4 * 2^-24 * max|y64|), the rule of tests/ddpm_exp_sampler_ref.py."""
    return max(4.0 * float(e_ref32), 4.0 * U * float(np.abs(y64).max()))


def ulp_distance(a, b):
    """Distance in units of the last place between two fp32 arrays of one sign pattern (positive table entries)."""
    ai = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    bi = np.ascontiguousarray(b, np.float32).view(np.int32).astype(np.int64)
    return np.abs(ai - bi)


def step_coef(S_mod, name):
    """The five host scalars of a fixture step, from the package's own tables."""
    _, S, eta, index, _, _, _ = STEP_CASES[name]
    return [float(v) for v in S_mod.sampling_tables(alphas_cumprod32(), S_mod.ddim_timesteps('uniform', S, 1000), eta)[index]]


def run_step(ops, S_mod, g, name, device='cpu'):
    """A fixture step through `ops.cfg_denoise_step` (the kernel, or its CPU stand-in): (next, x0, guided eps or None).  The
    first PLMS step is the two launches PLMSSampler makes of it: order 0 on the first eps, order 4 on the second."""
    kind, S, eta, index, scale, temp, nh = STEP_CASES[name]
    coef = step_coef(S_mod, name)

    def t(k):
        return torch.from_numpy(g[k]).to(device)

    def eps(u, c):
        return torch.cat([t(u), t(c)]) if scale is not None else t(u)
    x, e = t('x'), eps('e_u', 'e_c')
    x0 = torch.empty_like(x)
    if kind == 'ddim':
        z = t(name + ':z') if coef[4] != 0.0 else None
        return ops.cfg_denoise_step(x, e, coef, scale=scale, z=z, temperature=temp, x0_out=x0), x0, None
    eg = torch.empty_like(x)
    if nh == 0:
        x_prev = ops.cfg_denoise_step(x, e, coef, scale=scale, order=0, eg_out=eg)
        nxt = ops.cfg_denoise_step(x, eps('e2_u', 'e2_c'), coef, scale=scale, order=4, hist=[eg], out=x_prev, x0_out=x0)
    else:
        nxt = ops.cfg_denoise_step(x, e, coef, scale=scale, order=nh, hist=[t('h1'), t('h2'), t('h3')][:nh], x0_out=x0, eg_out=eg)
    return nxt, x0, eg
