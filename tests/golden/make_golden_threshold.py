#!/usr/bin/env python3
"""Fixtures of the thresholding / x0 / v-prediction steps of DDPMScheduler and DDIMScheduler (run in the build container only, on the
CPU): the reference's own diffusers.schedulers.scheduling_ddpm.DDPMScheduler and scheduling_ddim.DDIMScheduler, imported through
make_golden.py's shim.  Nothing of the reference is copied or edited.  One local wrapper stands between the reference's DDPM module
and this machine while it runs: `randn_tensor` as that module sees it hands back the case's stored noise (single steps: the
reference's DDPM `step` takes no `variance_noise`) or draws in fp32 and casts (the fp64 chains: the same noise as the fp32 chain).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_threshold.py

Writes (deterministic zip members, every file under 1 MiB; the case lists and seeds live in tests/threshold_ref.py):
  threshold_ddpm_steps.npz, threshold_ddim_steps_<model>_eta<eta>.npz
        single steps on [4, 3, 8, 8] inputs: three model types x {no clip, clip, thresholding at sample_max_value 1.0, 1.5, 4.0} x the
        first, a middle and the last timestep of a 10-step table (DDIM: x eta 0 / 0.5 with a supplied variance_noise x
        use_clipped_model_output off / on; DDPM: a supplied variance_noise): prev_sample and pred_original_sample of the reference in
        fp32 and in fp64 and their distances e_ref32.  The seeded inputs of a (scheduler, model type, timestep) group are scaled per
        image (the stored `scale:*`) so that the 0.995 quantile of |x0| is about 0.6, 1.25, 2.5 and 6: s ends clamped at 1, strictly
        between, and at the maximum -- asserted below for every thresholding fixture with sample_max_value > 1.
  threshold_chains.npz   10-step chains of the reference UNet2DModel (TINY_CFG, det_init_ seed 5) with thresholding at
        sample_max_value = 2.0 (R.CHAINS, two per scheduler, one of them a v-prediction chain): the fp64 states and the reference
        fp32 chain's gap to them
  threshold_toy.npz      the same chains over the closed-form R.toy_model at 8 x 8: the reference's fp32 states too"""
import copy
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg                                            # noqa: E402  (reference import shim: sys.path, model builder)
import golden_common as gc                                          # noqa: E402
import threshold_ref as R                                           # noqa: E402  (case lists, stand-ins; reference-free)
from diffusers import DDIMScheduler, DDPMScheduler                  # noqa: E402  (reference)
from diffusers.schedulers import scheduling_ddpm as ref_ddpm        # noqa: E402  (reference)
from diffusers.utils import randn_tensor                            # noqa: E402  (reference)

REAL_RANDN = ref_ddpm.randn_tensor
assert REAL_RANDN is randn_tensor
HAND = {'noise': None}


def handed_randn(shape, generator=None, device=None, dtype=None):
    """randn_tensor as the reference's DDPM module sees it (module docstring)."""
    if HAND['noise'] is not None:
        assert tuple(shape) == tuple(HAND['noise'].shape)
        return HAND['noise'].to(dtype)
    return REAL_RANDN(shape, generator=generator, device=device, dtype=torch.float32).to(dtype)


ref_ddpm.randn_tensor = handed_randn
CLASSES = {'ddpm': DDPMScheduler, 'ddim': DDIMScheduler}


def gap(a32, a64):
    return float((a32.double() - a64).abs().max())


def group_scale(sched, pred, where, s, t):
    """fp32 scale per image: R.TARGETS over the 0.995 quantile of the unscaled inputs' |x0| (fp64)."""
    x, m, _ = R.base_inputs(sched, pred, where)
    a = s.alphas_cumprod[t].double()
    x0 = R.form(R.PRED[pred], x.double(), m.double(), a ** 0.5, (1 - a) ** 0.5)[0]
    q = torch.quantile(x0.reshape(x.shape[0], -1).abs(), 0.995, dim=1)
    return (torch.tensor(R.TARGETS, dtype=torch.float64) / q).float().numpy()


def check_s_spread(key, pred, x, m, s, t, max_value):
    a = s.alphas_cumprod[t]
    st = R.abs_quantile(x, m, R.PRED[pred], float(a ** 0.5), float((1 - a) ** 0.5), 0.995, max_value)[:, 3].numpy()
    assert (st == 1.0).any() and ((st > 1.0) & (st < max_value)).any() and (st == np.float32(max_value)).any(), (key, st)


def one_step(out, key, s, t, x, m, kw32, kw64):
    r32 = s.step(m, t, x, **kw32)
    r64 = s.step(m.double(), t, x.double(), **kw64)
    assert r32.prev_sample.dtype == torch.float32 and r64.prev_sample.dtype == torch.float64 and r64.pred_original_sample.dtype == torch.float64
    for what, a32, a64 in (('prev', r32.prev_sample, r64.prev_sample), ('x0', r32.pred_original_sample, r64.pred_original_sample)):
        assert np.isfinite(a32.numpy()).all() and np.isfinite(a64.numpy()).all(), key
        out['%s:%s32' % (key, what)], out['%s:%s64' % (key, what)] = a32.numpy().copy(), a64.numpy().copy()
        out['%s:e_ref32_%s' % (key, what)] = np.float64(gap(a32, a64))
    out[key + ':t'] = np.int64(t)
    print('  %-58s t %3d  e_ref32 prev %.2e x0 %.2e  max|prev| %.2e max|x0| %.2e' % (
        key, t, out[key + ':e_ref32_prev'], out[key + ':e_ref32_x0'], float(r64.prev_sample.abs().max()), float(r64.pred_original_sample.abs().max())))


def scheduler(sched, pred, treat):
    s = CLASSES[sched](**R.sched_kwargs(pred, treat))
    s.set_timesteps(R.N_STEPS)
    return s


def do_ddpm():
    out = {}
    for case in R.ddpm_cases():
        pred, treat, where = case
        s = scheduler('ddpm', pred, treat)
        t = R.timestep_at(s.timesteps, where)
        sk = R.scale_key('ddpm', pred, where)
        if sk not in out:
            out[sk] = group_scale('ddpm', pred, where, s, t)
        x, m, z = R.scaled_inputs('ddpm', pred, where, out[sk])
        if R.TREATS[treat].get('sample_max_value', 1.0) > 1.0:
            check_s_spread(R.ddpm_key(case), pred, x, m, s, t, R.TREATS[treat]['sample_max_value'])
        HAND['noise'] = z
        try:
            one_step(out, R.ddpm_key(case), s, t, x, m, {}, {})
        finally:
            HAND['noise'] = None
    assert R.timestep_at(s.timesteps, 'last') == 0 and int(s.previous_timestep(0)) < 0
    return {R.ddpm_file(): out}


def do_ddim():
    files = {R.ddim_file(p, e): {} for p in R.PREDS for e in (0.0, 0.5)}
    for case in R.ddim_cases():
        pred, treat, where, eta, ucmo = case
        out = files[R.ddim_file(pred, eta)]
        s = scheduler('ddim', pred, treat)
        t = R.timestep_at(s.timesteps, where)
        sk = R.scale_key('ddim', pred, where)
        if sk not in out:
            out[sk] = group_scale('ddim', pred, where, s, t)
        x, m, z = R.scaled_inputs('ddim', pred, where, out[sk])
        if R.TREATS[treat].get('sample_max_value', 1.0) > 1.0:
            check_s_spread(R.ddim_key(case), pred, x, m, s, t, R.TREATS[treat]['sample_max_value'])
        kw = dict(eta=eta, use_clipped_model_output=ucmo)
        one_step(out, R.ddim_key(case), s, t, x, m, dict(kw, variance_noise=z if eta > 0 else None),
                 dict(kw, variance_noise=z.double() if eta > 0 else None))
    assert R.timestep_at(s.timesteps, 'last') - s.config.num_train_timesteps // s.num_inference_steps < 0
    return files


def chains(model32, model64, shape, store):
    out = {}
    for name, sched, kw, step_kw in R.CHAINS:
        runs = {}
        for tag, model in (('64', model64), ('32', model32)):
            s = CLASSES[sched](**kw)
            s.set_timesteps(R.CHAIN_STEPS)
            gen = torch.Generator().manual_seed(R.CHAIN_SEED)
            x_T = randn_tensor(shape, generator=gen)
            assert x_T.dtype == torch.float32
            xs = [x_T.double() if tag == '64' else x_T]
            extra = dict(step_kw, generator=gen) if sched == 'ddpm' else dict(step_kw)
            with torch.no_grad():
                for t in s.timesteps:
                    xs.append(s.step(model(xs[-1], t), t, xs[-1], **extra).prev_sample)
            runs[tag] = xs
        assert all(v.dtype == torch.float64 for v in runs['64']) and all(v.dtype == torch.float32 for v in runs['32'])
        out.setdefault('x_T', x_T.numpy())
        assert np.array_equal(out['x_T'], x_T.numpy())
        out[name + ':timesteps'] = s.timesteps.numpy().astype(np.int64)
        for tag in store:
            out[name + ':xs' + tag] = np.stack([v.numpy() for v in runs[tag]])
            assert np.isfinite(out[name + ':xs' + tag]).all()
        out[name + ':gap'] = np.array([gap(a, c) for a, c in zip(runs['32'], runs['64'])], np.float64)
        print('  %-10s max|x| %.2e  gap %s' % (name, max(float(v.abs().max()) for v in runs['64']), ' '.join('%.1e' % g for g in out[name + ':gap'][1:])))
    return out


def do_unet_chains():
    m32 = mg.build_ref_unet(gc.TINY_CFG, R.MODEL_SEED)
    for p in m32.parameters():
        p.requires_grad_(False)
    m64 = copy.deepcopy(m32).double()
    ss = gc.TINY_CFG['sample_size']
    return chains(lambda x, t: m32(x, t).sample, lambda x, t: m64(x, t).sample, (R.CHAIN_B, gc.TINY_CFG['in_channels'], ss, ss), ('64',))


def _savez(name, arrays):
    """np.savez with a fixed member timestamp: regenerating the fixtures gives the same bytes."""
    with zipfile.ZipFile(os.path.join(HERE, name), 'w', zipfile.ZIP_STORED) as z:
        for k in sorted(arrays):
            with z.open(zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0)), 'w', force_zip64=True) as f:
                np.lib.format.write_array(f, np.asanyarray(arrays[k]), allow_pickle=False)


def main():
    torch.manual_seed(0)
    files = do_ddpm()
    files.update(do_ddim())
    files[R.TOY_FILE] = chains(R.toy_model, R.toy_model, R.TOY_SHAPE, ('32', '64'))
    files[R.CHAINS_FILE] = do_unet_chains()
    assert sorted(files) == sorted(R.step_files() + [R.TOY_FILE, R.CHAINS_FILE])
    for name, arrays in files.items():
        _savez(name, arrays)
        size = os.path.getsize(os.path.join(HERE, name))
        assert size < (1 << 20), (name, size)
        print(name, size)


if __name__ == '__main__':
    main()
