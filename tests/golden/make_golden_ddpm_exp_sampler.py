#!/usr/bin/env python3
"""Fixtures of the ddpm_exp sampler (run in the build container only, on the CPU): the reference's own
functions.denoising.generalized_steps / ddpm_steps, imported with ddpm_exp on sys.path next to make_golden.py's shim.

Those functions hard-code `.to('cuda')` and draw `torch.randn_like` from the global generator.  They are called inside `on_cpu`,
which maps a 'cuda' argument of Tensor.to to 'cpu' and swaps torch.randn_like for a recorded noise stream (seeded fp32 values
held in fp64, cast to the working dtype: the fp32 and the fp64 run see the same numbers).  runners/diffusion.py does not import
here (tensorboard and torchvision are missing), so its `seq` lines (:498-529) are restated in `seq_of` and pinned by the lists that
running those lines gave: n = 7 uniform has 8 entries 0, 142, ..., 994; n = 100 quad starts 0, 0, 0, 0, 1, 2 and ends at 800.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_ddpm_exp_sampler.py

Writes (deterministic zip members, every file under 1 MiB):
  ddpm_exp_sampler_seq.npz            (a) the seq list, the fp32 compute_alpha at every entry and alpha(-1) for five (T, n, skip_type)
  ddpm_exp_sampler_steps.npz          (b) single steps on seeded [2, 3, 16, 16] inputs x, e, z: the reference called with
                                      seq = [j, i], xs[1] and x0_preds[0] taken, in fp32 and in fp64 (betas upcast to fp64), their
                                      distance e_ref32
  ddpm_exp_sampler_toy.npz            the reference's fp32 and fp64 chains over the smooth toy model of
                                      tests/ddpm_exp_sampler_ref.py at 8 x 8 (the CPU tests run the Python loops over them)
  ddpm_exp_sampler_chain_{uniform,quad}.npz
                                      (c) B = 2, n = 10 chains of the reference UNet2DModel (TINY_CFG, det_init_ seed 5) as
                                      `lambda x, t: unet(x, t).sample`: x_T, the noise stream, the fp64 states and x0 predictions and
                                      the reference fp32 chain's gap to them at every state."""
import contextlib
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
import ddpm_exp_sampler_ref as R                                    # noqa: E402  (case lists, toy model; reference-free)
from functions.denoising import compute_alpha, generalized_steps, ddpm_steps      # noqa: E402  (reference, ddpm_exp)

MODEL_SEED = 5
X_SEED, E_SEED, Z_SEED = 61, 62, 63
CHAIN_XT_SEED, CHAIN_NOISE_SEED0 = 70, 100
TOY_XT_SEED, TOY_NOISE_SEED0 = 80, 200


def betas32():
    """The runner's table: get_beta_schedule('linear') in float64, cast to fp32 (runners/diffusion.py:88-96, shipped configs)."""
    return torch.from_numpy(np.linspace(0.0001, 0.02, 1000, dtype=np.float64)).float()


def seq_of(num_timesteps, timesteps, skip_type):
    if skip_type == 'uniform':
        skip = num_timesteps // timesteps
        return list(range(0, num_timesteps, skip))
    assert skip_type == 'quad'
    seq = np.linspace(0, np.sqrt(num_timesteps * 0.8), timesteps) ** 2
    return [int(s) for s in list(seq)]


@contextlib.contextmanager
def on_cpu(noise):
    """`noise`: list of fp64 tensors, handed out in order by torch.randn_like."""
    real_to, real_randn_like = torch.Tensor.to, torch.randn_like
    drawn = [0]

    def to(self, *a, **k):
        a = tuple('cpu' if (isinstance(v, str) and v.startswith('cuda')) else v for v in a)
        if isinstance(k.get('device'), str) and k['device'].startswith('cuda'):
            k['device'] = 'cpu'
        return real_to(self, *a, **k)

    def randn_like(t, **k):
        z = noise[drawn[0] % len(noise)].to(t.dtype)
        drawn[0] += 1
        assert z.shape == t.shape
        return z
    torch.Tensor.to, torch.randn_like = to, randn_like
    try:
        yield drawn
    finally:
        torch.Tensor.to, torch.randn_like = real_to, real_randn_like


def run(kind, x, seq, model, betas, eta, noise):
    with on_cpu(noise) as drawn:
        if kind == 'generalized':
            xs, x0s = generalized_steps(x, seq, model, betas, eta=eta)
        else:
            xs, x0s = ddpm_steps(x, seq, model, betas)
    assert drawn[0] == len(seq)
    return xs, x0s


def gap(a32, a64):
    return float((a32.double() - a64).abs().max())


def do_seq():
    out = {}
    b = betas32()
    for k, (T, n, skip) in enumerate(R.SEQ_CASES):
        seq = seq_of(T, n, skip)
        out['%d:seq' % k] = np.array(seq, np.int64)
        out['%d:alpha' % k] = compute_alpha(b, torch.tensor(seq).long()).reshape(-1).numpy()
        out['%d:alpha_m1' % k] = compute_alpha(b, torch.tensor([-1]).long()).reshape(-1).numpy()
    s7, q100 = out['2:seq'], out['1:seq']
    assert len(s7) == 8 and list(s7[:2]) == [0, 142] and s7[-1] == 994
    assert list(q100[:6]) == [0, 0, 0, 0, 1, 2] and q100[-1] == 800 and len(q100) == 100
    assert list(out['0:seq']) == list(range(0, 1000, 10))
    assert float(out['0:alpha_m1'][0]) == 1.0
    return out


def do_steps():
    b32 = betas32()
    b64 = b32.double()
    x = torch.from_numpy(gc.det_noise(R.STEP_SHAPE, X_SEED))
    e = torch.from_numpy(gc.det_noise(R.STEP_SHAPE, E_SEED))
    z = torch.from_numpy(gc.det_noise(R.STEP_SHAPE, Z_SEED))
    out = dict(x=x.numpy(), e=e.numpy(), z=z.numpy())

    def one(name, kind, i, j, eta, scale=1.0):
        xs_, es_ = x * scale, e * scale
        res = {}
        for tag, dt, b in (('32', torch.float32, b32), ('64', torch.float64, b64)):
            ee = es_.to(dt)
            xs, x0s = run(kind, xs_.to(dt), [j, i], lambda xx, t: ee, b, eta, [z.double()])
            assert xs[1].dtype == dt and x0s[0].dtype == dt
            res[tag] = (xs[1], x0s[0])
        out[name + ':next64'], out[name + ':x0_64'] = res['64'][0].numpy(), res['64'][1].numpy()
        out[name + ':next32'], out[name + ':x0_32'] = res['32'][0].numpy(), res['32'][1].numpy()
        out[name + ':e_ref32_next'] = np.float64(gap(res['32'][0], res['64'][0]))
        out[name + ':e_ref32_x0'] = np.float64(gap(res['32'][1], res['64'][1]))
        out[name + ':ij'] = np.array([i, j], np.int64)
        out[name + ':eta'], out[name + ':scale'] = np.float64(eta), np.float64(scale)
        assert np.isfinite(out[name + ':next64']).all() and np.isfinite(out[name + ':next32']).all(), name
        print('  %-22s e_ref32 next %.2e x0 %.2e   max|next| %.2e max|x0| %.2e' % (
            name, out[name + ':e_ref32_next'], out[name + ':e_ref32_x0'], np.abs(out[name + ':next64']).max(),
            np.abs(out[name + ':x0_64']).max()))
        return res
    for (i, j) in R.STEP_PAIRS:
        for eta in R.ETAS:
            one('gen:%d:%d:%g' % (i, j, eta), 'generalized', i, j, eta)
        one('ddpm:%d:%d' % (i, j), 'ddpm_noisy', i, j, 0.0)
    i, j = R.CLAMP_PAIR
    name = 'ddpm_clamp:%d:%d' % (i, j)
    res = one(name, 'ddpm_noisy', i, j, 0.0, R.CLAMP_SCALE)
    share = float((res['64'][1].abs() == 1.0).double().mean())
    assert 0.1 <= share <= 0.9, share
    out[name + ':clamp_share'] = np.float64(share)
    print('  clamp share', share)
    assert sorted(R.step_case_names()) == sorted({k.rsplit(':', 1)[0] for k in out if ':' in k})
    return out


def chains(model32, model64, shape, xt_seed, noise_seed0, skip, prefix, out, store64):
    b32 = betas32()
    seq = seq_of(1000, R.CHAIN_N, skip)
    x_T = torch.from_numpy(gc.det_noise(shape, xt_seed))
    noise = [torch.from_numpy(gc.det_noise(shape, noise_seed0 + k)).double() for k in range(len(seq))]
    out[prefix + 'seq'] = np.array(seq, np.int64)
    out[prefix + 'x_T'] = x_T.numpy()
    out[prefix + 'noise'] = np.stack([n.float().numpy() for n in noise])
    for kind, eta in R.CHAIN_KINDS:
        name = prefix + R.chain_name(kind, eta)
        xs64, x0s64 = run(kind, x_T.double(), seq, model64, b32.double(), eta, noise)
        xs32, x0s32 = run(kind, x_T.clone(), seq, model32, b32, eta, noise)
        assert len(xs64) == len(seq) + 1 and len(x0s64) == len(seq)
        dt = np.float64 if store64 else np.float32
        out[name + ':xs64'] = np.stack([t.numpy() for t in xs64]).astype(dt)
        out[name + ':x0s64'] = np.stack([t.numpy() for t in x0s64]).astype(dt)
        if not store64:                                             # the toy chains: the reference's fp32 run itself
            out[name + ':xs32'] = np.stack([t.numpy() for t in xs32])
            out[name + ':x0s32'] = np.stack([t.numpy() for t in x0s32])
        out[name + ':gap_xs'] = np.array([gap(a, c) for a, c in zip(xs32, xs64)], np.float64)
        out[name + ':gap_x0s'] = np.array([gap(a, c) for a, c in zip(x0s32, x0s64)], np.float64)
        print('  %-28s gap xs %s' % (name, ' '.join('%.1e' % g for g in out[name + ':gap_xs'][1:])))
        print('  %-28s gap x0 %s' % ('', ' '.join('%.1e' % g for g in out[name + ':gap_x0s'])))


def do_unet_chains(skip):
    m32 = mg.build_ref_unet(gc.TINY_CFG, MODEL_SEED)
    for p in m32.parameters():
        p.requires_grad_(False)
    m64 = copy.deepcopy(m32).double()
    out = {}
    ss = gc.TINY_CFG['sample_size']
    chains(lambda x, t: m32(x, t).sample, lambda x, t: m64(x, t).sample, (R.CHAIN_B, gc.TINY_CFG['in_channels'], ss, ss),
           CHAIN_XT_SEED, CHAIN_NOISE_SEED0, skip, '', out, True)
    return out


def _savez(name, arrays):
    """np.savez with a fixed member timestamp: regenerating the fixtures gives the same bytes."""
    with zipfile.ZipFile(os.path.join(HERE, name), 'w', zipfile.ZIP_STORED) as z:
        for k in sorted(arrays):
            with z.open(zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0)), 'w', force_zip64=True) as f:
                np.lib.format.write_array(f, np.asanyarray(arrays[k]), allow_pickle=False)


def main():
    torch.manual_seed(0)
    _savez(R.SEQ_FILE, do_seq())
    _savez(R.STEPS_FILE, do_steps())
    toy = {}
    for skip in ('uniform', 'quad'):
        chains(R.toy_model, R.toy_model, R.TOY_SHAPE, TOY_XT_SEED, TOY_NOISE_SEED0, skip, '%s:' % skip, toy, False)
    _savez(R.TOY_FILE, toy)
    for skip in ('uniform', 'quad'):
        _savez(R.CHAIN_FILES[skip], do_unet_chains(skip))
    for f in [R.SEQ_FILE, R.STEPS_FILE, R.TOY_FILE] + list(R.CHAIN_FILES.values()):
        size = os.path.getsize(os.path.join(HERE, f))
        assert size < (1 << 20), (f, size)
        print(f, size)


if __name__ == '__main__':
    main()
