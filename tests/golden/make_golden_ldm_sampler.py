#!/usr/bin/env python3
"""Fixtures of the ldm_exp samplers (run in the build container only, on the CPU): the reference's own DDIMSampler and PLMSSampler
(ldm/models/diffusion/ddim.py, plms.py), imported through make_golden_ldm.py's shim.  The only override is `register_buffer`,
whose one line forces 'cuda' (make_golden_ldm.py:211-213 does the same); LatentDiffusion is the stand-in of make_golden_ldm.py's
ldm_sampler(): the handful of attributes the samplers read, over the reference's own make_beta_schedule.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_ldm_sampler.py

Noise.  The samplers draw `torch.randn(shape)` from the global generator at every step.  Nothing is patched: the generator is
seeded before a run and the same draws are made again afterwards to record them; a run on fp64 states draws the same fp32 values.

"fp64".  `torch.full((b, 1, 1, 1), table[index])` makes fp32 scalars whatever the state's dtype, so a run of these samplers on
fp64 states and fp64 eps is the fp64 evaluation of every elementwise expression FROM THE SAME fp32 SCALARS -- the reference point
tests/ddpm_exp_sampler_ref.py builds by hand for the other sampler.  The reference UNetModel casts to fp32 inside (GroupNorm32,
`x.type(self.dtype)`), so the fp64 chains run the samplers over oracle/ldm_ref.ldm_unet_forward in fp64 (its fp32 timestep
sinusoid upcast).

Writes (deterministic zip members, every file under 1 MiB):
  ldm_sampler_tables.npz   (a) for S in {20, 50, 250} x eta in {0, 0.5, 1} x {uniform, quad}: ddim_timesteps and the five fp32
                           scalars (s1m, sqrt_a_t, sqrt_a_prev, c_dir, sigma) of every index, read off the sampler's buffers by the
                           expressions of ddim.py:188-198 at b = 2, and a flag per index: 0 when the four fp32 square roots this
                           host's torch took equal the correctly rounded ones
  ldm_sampler_steps.npz    (b) p_sample_ddim and p_sample_plms (history of 0 .. 3) on stored x, eps halves, noise and history, in
                           fp32 and fp64, at indices whose flags are clean
  ldm_sampler_toy.npz      the reference's fp32 chains over the toy model of tests/ldm_sampler_ref.py (the CPU tests demand equality)
  ldm_sampler_chains.npz   (c) chains on LDM_TINY_CFG (B = 2, 16 x 16, the weights and inputs of ldm_sampler.npz), log_every_t = 5:
                           DDIM eta 0, DDIM eta 0.5 at temperature 0.8 with its recorded noise, PLMS; the fp64 states and x0
                           predictions and the reference fp32 chain's gap to them"""
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import make_golden_ldm as mgl                                          # noqa: E402  (reference import shim: sys.path, stubs, UNetModel)
import golden_common as gc                                             # noqa: E402
import ldm_sampler_ref as R                                            # noqa: E402  (case lists, toy model; reference-free)
from ldm.models.diffusion.ddim import DDIMSampler                      # noqa: E402  (reference)
from ldm.models.diffusion.plms import PLMSSampler                      # noqa: E402  (reference)
from ldm.modules.diffusionmodules.util import make_beta_schedule       # noqa: E402  (reference)

NOISE_SEED = 1234


class CpuDDIM(DDIMSampler):
    def register_buffer(self, name, attr):        # the reference moves every buffer to 'cuda' here; no arithmetic
        setattr(self, name, attr)


class CpuPLMS(PLMSSampler):
    def register_buffer(self, name, attr):
        setattr(self, name, attr)


class Host:                                       # what the samplers read from LatentDiffusion
    num_timesteps = 1000
    device = torch.device('cpu')
    parameterization = 'eps'

    def __init__(self, apply_model=None):
        betas = make_beta_schedule('linear', 1000, linear_start=0.0015, linear_end=0.0195, cosine_s=8e-3)
        acp = np.cumprod(1.0 - betas, axis=0)
        self.betas = torch.tensor(betas, dtype=torch.float32)
        self.alphas_cumprod = torch.tensor(acp, dtype=torch.float32)
        self.alphas_cumprod_prev = torch.tensor(np.append(1.0, acp[:-1]), dtype=torch.float32)
        assert torch.equal(self.alphas_cumprod, R.alphas_cumprod32())
        self.apply_model = apply_model


def sqrt_ok(t):
    """True where torch's fp32 sqrt of `t` is the correctly rounded one (fp64 sqrt rounded once more: innocuous for a square root)."""
    return torch.equal(t.sqrt(), t.double().sqrt().float())


def noise_of(seed, n, shape):
    torch.manual_seed(seed)
    return [torch.randn(shape) for _ in range(n)]


def gap(a32, a64):
    return float((a32.double() - a64).abs().max())


# ---------------------------------------------------------------------------------------------- (a)
def do_tables():
    out, flags = {}, {}
    for S in R.TABLE_S:
        for eta in R.TABLE_ETAS:
            for discr in R.TABLE_DISCR:
                s = CpuDDIM(Host())
                s.make_schedule(S, ddim_discretize=discr, ddim_eta=eta, verbose=False)
                n = len(s.ddim_timesteps)
                rows, flag = np.zeros((n, 5), np.float32), np.zeros(n, np.uint8)
                one_minus = 1. - s.ddim_alphas
                for index in range(n):
                    b = 2                                                                   # ddim.py:188-198
                    a_t = torch.full((b, 1, 1, 1), s.ddim_alphas[index])
                    a_prev = torch.full((b, 1, 1, 1), s.ddim_alphas_prev[index])
                    sigma_t = torch.full((b, 1, 1, 1), s.ddim_sigmas[index])
                    sqrt_one_minus_at = torch.full((b, 1, 1, 1), s.ddim_sqrt_one_minus_alphas[index])
                    dir_arg = 1. - a_prev - sigma_t ** 2
                    vals = [sqrt_one_minus_at, a_t.sqrt(), a_prev.sqrt(), dir_arg.sqrt(), sigma_t]
                    assert all(v.dtype == torch.float32 for v in vals)
                    rows[index] = [float(v[0]) for v in vals]
                    s1m_ok = float(sqrt_one_minus_at[0]) == float(one_minus[index].double().sqrt().float())
                    flag[index] = 0 if (s1m_ok and sqrt_ok(a_t) and sqrt_ok(a_prev) and sqrt_ok(dir_arg)) else 1
                key = R.table_key(S, eta, discr)
                out[key + ':timesteps'] = np.asarray(s.ddim_timesteps, np.int64)
                out[key + ':table'] = rows
                out[key + ':flag'] = flag
                flags[key] = flag
                print('  table %-18s n %3d flagged %d %s' % (key, n, int(flag.sum()), list(np.nonzero(flag)[0])))
                assert flag.mean() <= 0.05, key
    return out, flags


# ---------------------------------------------------------------------------------------------- (b)
def do_steps(flags):
    B = R.STEP_SHAPE[0]
    names = ['x', 'e_u', 'e_c', 'h1', 'h2', 'h3', 'e2_u', 'e2_c']
    T = {n: torch.from_numpy(gc.det_noise(R.STEP_SHAPE, 61 + k)) for k, n in enumerate(names)}
    out = {n: t.numpy() for n, t in T.items()}
    cond, uncond = torch.zeros(B, 1, R.TOY_CTX), torch.ones(B, 1, R.TOY_CTX)
    for k, (name, (kind, S, eta, index, scale, temp, nh)) in enumerate(R.STEP_CASES.items()):
        res = {}
        for tag, dt in (('32', torch.float32), ('64', torch.float64)):
            calls = [0]

            def apply_model(x_in, t_in, c_in):
                first = calls[0] == 0
                calls[0] += 1
                eu, ec = (T['e_u'], T['e_c']) if first else (T['e2_u'], T['e2_c'])
                if x_in.shape[0] == 2 * B:
                    assert torch.equal(c_in, torch.cat([uncond, cond])) and torch.equal(t_in[:B], t_in[B:])
                    return torch.cat([eu, ec]).to(dt)
                return eu.to(dt)
            s = (CpuDDIM if kind == 'ddim' else CpuPLMS)(Host(apply_model))
            s.make_schedule(S, ddim_eta=eta, verbose=False)
            assert flags[R.table_key(S, eta, 'uniform')][index] == 0, (name, 'pick an index whose square roots are clean')
            t = torch.full((B,), int(s.ddim_timesteps[index]), dtype=torch.long)
            kw = dict(index=index, temperature=temp, unconditional_guidance_scale=1.0 if scale is None else scale,
                      unconditional_conditioning=None if scale is None else uncond)
            torch.manual_seed(NOISE_SEED + k)
            with torch.no_grad():
                if kind == 'ddim':
                    nxt, x0 = s.p_sample_ddim(T['x'].to(dt), cond, t, **kw)
                    eg = None
                else:
                    old = [T[h].to(dt) for h in ('h3', 'h2', 'h1')][3 - nh:]               # oldest first, as plms.py appends
                    nxt, x0, eg = s.p_sample_plms(T['x'].to(dt), cond, t, old_eps=old, t_next=t, **kw)
            assert calls[0] == (2 if nh == 0 else 1) and nxt.dtype == dt and x0.dtype == dt
            res[tag] = (nxt, x0, eg)
        out[name + ':z'] = noise_of(NOISE_SEED + k, 1, R.STEP_SHAPE)[0].numpy()
        for j, what in enumerate(('next', 'x0')):
            out['%s:%s_32' % (name, what)] = res['32'][j].numpy()
            out['%s:%s_64' % (name, what)] = res['64'][j].numpy()
            out['%s:e_ref32_%s' % (name, what)] = np.float64(gap(res['32'][j], res['64'][j]))
        if res['32'][2] is not None:
            out[name + ':eg32'] = res['32'][2].numpy()
        print('  step %-22s e_ref32 next %.2e x0 %.2e' % (name, out[name + ':e_ref32_next'], out[name + ':e_ref32_x0']))
    return out


# ---------------------------------------------------------------------------------------------- chains
def run_chain(kind, host, discr, S, eta, temp, x_T, cond, uncond, scale, seed):
    s = (CpuDDIM if kind == 'ddim' else CpuPLMS)(host)
    B = x_T.shape[0]
    torch.manual_seed(seed)
    with torch.no_grad():
        if discr == 'uniform':
            out, inter = s.sample(S=S, batch_size=B, shape=list(x_T.shape[1:]), conditioning=cond, eta=eta, temperature=temp,
                                  verbose=False, x_T=x_T, log_every_t=R.LOG_EVERY, unconditional_guidance_scale=scale,
                                  unconditional_conditioning=uncond)
        else:                                 # sample() always builds the uniform schedule: make_schedule + the loop it calls
            s.make_schedule(S, ddim_discretize=discr, ddim_eta=eta, verbose=False)
            loop = s.ddim_sampling if kind == 'ddim' else s.plms_sampling
            out, inter = loop(cond, tuple(x_T.shape), x_T=x_T, temperature=temp, log_every_t=R.LOG_EVERY,
                              unconditional_guidance_scale=scale, unconditional_conditioning=uncond)
    assert torch.equal(out, inter['x_inter'][-1])
    return torch.stack(inter['x_inter']), torch.stack(inter['pred_x0']), len(s.ddim_timesteps)


def do_toy():
    x_T = torch.from_numpy(gc.det_noise(R.TOY_SHAPE, 80))
    cond = torch.from_numpy(gc.det_noise((R.TOY_SHAPE[0], 1, R.TOY_CTX), 81))
    uncond = torch.from_numpy(gc.det_noise((R.TOY_SHAPE[0], 1, R.TOY_CTX), 82))
    out = dict(x_T=x_T.numpy(), cond=cond.numpy(), uncond=uncond.numpy())
    host = Host(R.toy_model)
    for k, (name, (kind, discr, S, eta, temp)) in enumerate(R.TOY_CHAINS.items()):
        xs, x0s, n = run_chain(kind, host, discr, S, eta, temp, x_T, cond, uncond, R.TOY_SCALE, NOISE_SEED + 100 + k)
        out[name + ':x_inter32'], out[name + ':pred_x0_32'] = xs.numpy(), x0s.numpy()
        if eta != 0:
            out[name + ':noise'] = torch.stack(noise_of(NOISE_SEED + 100 + k, n, R.TOY_SHAPE)).numpy()
        assert np.isfinite(out[name + ':x_inter32']).all()
        print('  toy %-24s steps %d logged %d  max|x| %.3f' % (name, n, xs.shape[0], float(xs[-1].abs().max())))
    return out


def do_unet_chains():
    from oracle import ldm_ref
    cfg = gc.LDM_TINY_CFG
    unet = mgl.UNetModel(**cfg).eval()
    gc.det_init_(unet, R.UNET_SEED)
    P64 = {n: torch.from_numpy(gc.det_param(n, s, R.UNET_SEED)).double() for n, s in ldm_ref.ldm_param_shapes(cfg).items()}
    for n, p in unet.named_parameters():
        assert torch.equal(p.detach().double(), P64[n]), n
    B, H = 2, cfg['image_size']
    x_T = torch.from_numpy(gc.det_noise((B, cfg['in_channels'], H, H), R.X_T_SEED))
    cond = torch.from_numpy(gc.det_noise((B, 1, cfg['context_dim']), R.COND_SEED))
    uncond = torch.from_numpy(gc.det_noise((B, 1, cfg['context_dim']), R.UNCOND_SEED))
    host32 = Host(lambda x, t, c: unet(x, t, context=c))
    temb32 = ldm_ref.timestep_embedding              # the oracle forms the sinusoid in fp32 (as the reference does): upcast it

    def unet64(x, t, c):
        ldm_ref.timestep_embedding = lambda *a, **k: temb32(*a, **k).double()
        try:
            return ldm_ref.ldm_unet_forward(P64, cfg, x, t, c)
        finally:
            ldm_ref.timestep_embedding = temb32
    host64 = Host(unet64)
    out = {}
    for k, (name, (kind, eta, temp)) in enumerate(R.UNET_CHAINS.items()):
        seed = NOISE_SEED + 200 + k
        xs32, x0s32, n = run_chain(kind, host32, 'uniform', R.UNET_S, eta, temp, x_T, cond, uncond, R.UNET_SCALE, seed)
        xs64, x0s64, _ = run_chain(kind, host64, 'uniform', R.UNET_S, eta, temp, x_T.double(), cond.double(), uncond.double(),
                                   R.UNET_SCALE, seed)
        assert xs64.dtype == torch.float64 and xs64.shape == xs32.shape
        out[name + ':x_inter64'], out[name + ':pred_x0_64'] = xs64.numpy(), x0s64.numpy()
        out[name + ':gap_x_inter'] = np.array([gap(a, c) for a, c in zip(xs32, xs64)], np.float64)
        out[name + ':gap_pred_x0'] = np.array([gap(a, c) for a, c in zip(x0s32, x0s64)], np.float64)
        if eta != 0:
            out[name + ':noise'] = torch.stack(noise_of(seed, n, tuple(x_T.shape))).numpy()
        print('  unet %-12s gap x %s' % (name, ' '.join('%.1e' % g for g in out[name + ':gap_x_inter'])))
        print('  %-17s gap x0 %s' % ('', ' '.join('%.1e' % g for g in out[name + ':gap_pred_x0'])))
        if name == 'ddim:eta0':                  # the run make_golden_ldm.py's ldm_sampler() recorded
            old = np.load(os.path.join(HERE, 'ldm_sampler.npz'))
            d = float(np.abs(old['x_inter'] - xs32.numpy()).max())
            print('  distance from ldm_sampler.npz (the same run, recorded earlier): %.1e' % d)
            assert d < 1e-4, 'ldm_sampler.npz holds another run'
    return out


def _savez(name, arrays):
    """np.savez with a fixed member timestamp: regenerating the fixtures gives the same bytes."""
    with zipfile.ZipFile(os.path.join(HERE, name), 'w', zipfile.ZIP_STORED) as z:
        for k in sorted(arrays):
            with z.open(zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0)), 'w', force_zip64=True) as f:
                np.lib.format.write_array(f, np.asanyarray(arrays[k]), allow_pickle=False)


def main():
    tables, flags = do_tables()
    _savez(R.TABLES_FILE, tables)
    _savez(R.STEPS_FILE, do_steps(flags))
    _savez(R.TOY_FILE, do_toy())
    _savez(R.CHAINS_FILE, do_unet_chains())
    for f in (R.TABLES_FILE, R.STEPS_FILE, R.TOY_FILE, R.CHAINS_FILE):
        size = os.path.getsize(os.path.join(HERE, f))
        assert size < (1 << 20), (f, size)
        print(f, size)


if __name__ == '__main__':
    main()
