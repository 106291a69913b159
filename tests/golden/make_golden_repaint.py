#!/usr/bin/env python3
"""Fixtures of RePaintScheduler / RePaintPipeline (run in the build container only, on the CPU): the reference's own
diffusers.schedulers.scheduling_repaint.RePaintScheduler and diffusers.pipelines.repaint.pipeline_repaint, imported through
make_golden.py's shim.

Local wrappers stand between the reference and this machine while its scheduler runs; nothing of the reference is copied or edited.
  * `rounded_pow` (the idea of make_golden_pndm.py): torch's fp32 sqrt on the CPU comes from the host's vector math library: within
    an ulp, not correctly rounded on every host.  While the reference scheduler runs -- and only then: the UNet of the chains does
    not run under it -- a 0-d fp32 tensor raised to 0.5 is evaluated in fp64 and rounded to fp32 once (diffusion._rounded_once does
    the same), and so is torch.sigmoid of the `sigmoid` beta table.  It also lists the 0-d fp32 scalars that meet the data.
  * `fp32_draws`: the reference draws its noise in the data's dtype, and an fp64 draw is not the fp32 draw cast up.  The fp64 runs
    must see the fp32 run's noise, so the two modules' `randn_tensor` draws in fp32 and casts.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_repaint.py

Writes (deterministic zip members, every file under 1 MiB; the case lists and seeds live in tests/repaint_ref.py):
  repaint_tables.npz       (a) the timestep table of every R.TABLE_CASES entry
  repaint_steps.npz        (b) per R.STEP_CASES entry one call of the reference's `step` in fp32 and in fp64 (the same fp32 inputs and
                           noise cast up, the scheduler's own fp32 scalars): prev_sample and pred_original_sample in both precisions,
                           their distances e_ref32 and the six scalars as the reference formed them; per R.UNDO_CASES entry `undo_step`
                           in both precisions with the (a_i, b_i); (d) the two preprocessors' outputs for R.pre_inputs()
  repaint_toy.npz          (c) free-running calls of the reference pipeline's own loop over the closed-form R.toy_model at 8 x 8: the
                           reference's fp32 states themselves (the CPU test asks for the same bits) and the returned images
  repaint_chain_<name>.npz (c) the same over the reference UNet2DModel (TINY_CFG, det_init_ seed 5): the fp64 states and the
                           reference fp32 chain's gap to them at every state"""
import contextlib
import copy
import os
import sys
import zipfile
from types import SimpleNamespace

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg                                            # noqa: E402  (reference import shim: sys.path, model builder)
import golden_common as gc                                          # noqa: E402
import repaint_ref as R                                             # noqa: E402  (case lists, toy model; reference-free)
from diffusers import RePaintScheduler                              # noqa: E402  (reference)
from diffusers.schedulers import scheduling_repaint as ref_sched    # noqa: E402  (reference)
from diffusers.pipelines.repaint import pipeline_repaint as ref_pipe  # noqa: E402  (reference)

COEF = ('sa', 'sb', 'sap', 's1', 'cd', 'sd')


@contextlib.contextmanager
def rounded_pow(seen=None):
    """`seen`: a list that takes, in order, every 0-d fp32 tensor that multiplies or divides a tensor with dimensions while the
    context is open -- the scalars of `step` and `undo_step` as the reference itself formed them."""
    real = torch.Tensor.__pow__, torch.Tensor.__mul__, torch.Tensor.__truediv__, torch.sigmoid

    def scalar_meets_data(a, b):
        return isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor) and a.dim() == 0 and a.dtype == torch.float32 and b.dim() > 0

    def pow_(self, other):
        if isinstance(other, float) and other == 0.5 and self.dim() == 0 and self.dtype == torch.float32:
            return torch.sqrt(self.double()).float()
        return real[0](self, other)

    def mul_(self, other):
        if seen is not None and scalar_meets_data(self, other):
            seen.append(('mul', float(self)))
        return real[1](self, other)

    def div_(self, other):
        if seen is not None and scalar_meets_data(other, self):
            seen.append(('div', float(other)))
        return real[2](self, other)

    def sigmoid_(t):
        return real[3](t.double()).float() if t.dtype == torch.float32 else real[3](t)
    torch.Tensor.__pow__, torch.Tensor.__mul__, torch.Tensor.__truediv__, torch.sigmoid = pow_, mul_, div_, sigmoid_
    try:
        yield
    finally:
        torch.Tensor.__pow__, torch.Tensor.__mul__, torch.Tensor.__truediv__, torch.sigmoid = real


@contextlib.contextmanager
def fp32_draws():
    real = ref_sched.randn_tensor, ref_pipe.randn_tensor

    def draw(shape, generator=None, device=None, dtype=None, **kw):
        return real[0](shape, generator=generator, device=device, dtype=torch.float32, **kw).to(dtype or torch.float32)
    ref_sched.randn_tensor = ref_pipe.randn_tensor = draw
    try:
        yield
    finally:
        ref_sched.randn_tensor, ref_pipe.randn_tensor = real


def ref_scheduler(n, jump=(10, 10), **kw):
    with rounded_pow():
        s = RePaintScheduler(**kw)
        s.set_timesteps(n, *jump)
    return s


def gap(a32, a64):
    return float((a32.double() - a64).abs().max())


def coefs_of(seen, add_noise):
    """(sa, sb, sap, s1, cd, sd) as fp32 from what one `step` showed: sb *, / sa, [sd *,] cd *, sap *, sap *, s1 *.  Where the noise is
    not added the reference forms std_dev_t but does not use it: it is 0 there (eta = 0, or the variance of t = 0), stored as 0."""
    kinds, vals = [k for k, _ in seen], [v for _, v in seen]
    assert kinds == ['mul', 'div'] + ['mul'] * (5 if add_noise else 4), seen
    sb, sa = vals[0], vals[1]
    sd = vals[2] if add_noise else 0.0
    cd, sap, sap2, s1 = vals[-4:]
    assert sap == sap2
    return np.array([sa, sb, sap, s1, cd, sd], np.float32)


def do_tables(out):
    for case in R.TABLE_CASES:
        s = ref_scheduler(case[0], case[1:])
        ts = s.timesteps.numpy()
        assert ts.dtype == np.int64
        out[R.table_name(case)] = ts
        print('  %-22s %5d entries  %s ... %s' % (R.table_name(case), len(ts), ts[:5].tolist(), ts[-3:].tolist()))
        assert len(ts) == R.TABLE_LENGTHS.get(case, len(ts)), (case, len(ts))
    assert out[R.table_name((2000, 10, 10))].tolist() == out[R.table_name((1000, 10, 10))].tolist()
    assert out[R.table_name((1, 1, 1))].tolist() == [0]


def do_steps(out):
    for k, (name, kw, n, eta, t, form) in enumerate(R.STEP_CASES):
        x, e, o, m = R.step_inputs(k, form)
        res = {}
        for tag, dt in (('32', torch.float32), ('64', torch.float64)):
            s = ref_scheduler(n, **kw)
            s.eta = eta                                                  # as the pipeline sets it
            seen = []
            with rounded_pow(seen), fp32_draws():
                r = s.step(e.to(dt), torch.tensor(t), x.to(dt), o.to(dt), m.to(dt), generator=R.noise_generator(k))
            assert r.prev_sample.dtype == dt and r.pred_original_sample.dtype == dt and r.prev_sample.shape == R.STEP_SHAPE
            res[tag] = (r.prev_sample, r.pred_original_sample, coefs_of(seen, t > 0 and eta > 0))
        (p32, q32, c32), (p64, q64, c64) = res['32'], res['64']
        assert c32.tobytes() == c64.tobytes()                            # the fp64 run forms the same fp32 scalars
        key = 'step:' + name
        assert key + ':prev32' not in out
        out[key + ':prev32'], out[key + ':prev64'] = p32.numpy(), p64.numpy()
        out[key + ':x0_32'], out[key + ':x0_64'] = q32.numpy(), q64.numpy()
        out[key + ':e_ref32'], out[key + ':e_ref32_x0'] = np.float64(gap(p32, p64)), np.float64(gap(q32, q64))
        out[key + ':coefs'] = c32
        assert all(np.isfinite(out[key + ':' + v]).all() for v in ('prev32', 'prev64', 'x0_32', 'x0_64', 'coefs')), key
        print('  %-34s e_ref32 %.2e  x0 %.2e   max|prev| %.2e  coefs %s' % (key, out[key + ':e_ref32'], out[key + ':e_ref32_x0'],
                                                                          np.abs(out[key + ':prev64']).max(), c32.tolist()))


def do_undo(out):
    for k, case in enumerate(R.UNDO_CASES):
        n_inf, t = case
        x = R.undo_input(k)
        res = {}
        for tag, dt in (('32', torch.float32), ('64', torch.float64)):
            s = ref_scheduler(n_inf)
            seen = []
            with rounded_pow(seen), fp32_draws():
                y = s.undo_step(x.to(dt), torch.tensor(t), generator=R.noise_generator(1000 + k))
            assert y.dtype == dt and [kind for kind, _ in seen] == ['mul'] * (2 * R.UNDO_N[k])
            res[tag] = (y, np.array([v for _, v in seen], np.float32).reshape(-1, 2))
        (y32, c32), (y64, c64) = res['32'], res['64']
        assert c32.tobytes() == c64.tobytes() and len(c32) == 1000 // n_inf == R.UNDO_N[k]
        key = R.undo_name(case)
        out[key + ':out32'], out[key + ':out64'], out[key + ':e_ref32'], out[key + ':coefs'] = y32.numpy(), y64.numpy(), np.float64(gap(y32, y64)), c32
        print('  %-20s n %3d  e_ref32 %.2e' % (key, len(c32), out[key + ':e_ref32']))


def do_preprocessors(out):
    image, mask = R.pre_inputs()
    a, b = ref_pipe._preprocess_image(image), ref_pipe._preprocess_mask(mask)
    assert a.dtype == torch.float32 and tuple(a.shape) == (1, 3, 40, 32) and b.dtype == torch.float32 and tuple(b.shape) == (1, 64, 64)
    out['pre:image'], out['pre:mask'] = a.numpy(), b.numpy()
    assert set(np.unique(out['pre:mask']).tolist()) == {0.0, 1.0}


class _Net:
    """What the reference pipeline's loop asks of its `unet`: a call that returns `.sample`, and a dtype."""

    def __init__(self, fn, dtype):
        self.fn, self.dtype = fn, dtype

    def __call__(self, sample, t):
        return SimpleNamespace(sample=self.fn(sample, t))


def run_pipeline(fn, dtype, shape, steps, eta):
    """The reference pipeline's own __call__ (its loop, its draws, its post-processing) on a stand-in for `self`; the scheduler's two
    methods run under rounded_pow and report every state."""
    n, jl, js = steps
    sched = ref_scheduler(n)                                             # the call sets the timesteps anew
    states = []
    real_set, real_step, real_undo = sched.set_timesteps, sched.step, sched.undo_step

    def set_timesteps(*a, **k):
        with rounded_pow():
            return real_set(*a, **k)

    def step(*a, **k):
        if not states:
            states.append(a[2])                                          # x_T: the sample of the first call
        with rounded_pow():
            r = real_step(*a, **k)
        states.append(r.prev_sample)
        return r

    def undo(*a, **k):
        with rounded_pow():
            r = real_undo(*a, **k)
        states.append(r)
        return r
    sched.set_timesteps, sched.step, sched.undo_step = set_timesteps, step, undo
    me = SimpleNamespace(unet=_Net(fn, dtype), scheduler=sched, device=torch.device('cpu'), progress_bar=lambda it: it)
    image, mask = R.chain_inputs(shape)
    with fp32_draws():
        images = ref_pipe.RePaintPipeline.__call__(me, image=image, mask_image=mask, num_inference_steps=n, eta=eta, jump_length=jl,
                                                   jump_n_sample=js, generator=torch.Generator().manual_seed(R.CHAIN_SEED),
                                                   output_type='numpy').images
    assert all(v.dtype == dtype for v in states) and len(states) == len(sched.timesteps) + 1
    return sched.timesteps.numpy(), states, images


def chains(model32, model64, shape, store):
    """store: '64' (the fp64 states, for the GPU test's bound) or '32' (the reference's fp32 states, for the CPU test's bit equality).
    Returns {chain name: arrays}."""
    res = {}
    for name, steps, eta in R.CHAINS:
        ts, xs32, im32 = run_pipeline(model32, torch.float32, shape, steps, eta)
        ts64, xs64, _ = run_pipeline(model64, torch.float64, shape, steps, eta)
        assert ts.tolist() == ts64.tolist() and len(ts) == R.TABLE_LENGTHS[steps]
        out = res[name] = {}
        out[name + ':timesteps'] = ts
        out[name + ':xs' + store] = np.stack([v.numpy() for v in (xs64 if store == '64' else xs32)])
        out[name + ':gap'] = np.array([gap(a, c) for a, c in zip(xs32, xs64)], np.float64)
        if store == '32':
            out[name + ':images'] = np.asarray(im32)
        assert np.isfinite(out[name + ':xs' + store]).all() and out[name + ':gap'][0] == 0.0          # the same x_T
        print('  %-12s %d states  max|x| %.2e  gap %s' % (name, len(xs32), float(xs64[-1].abs().max()),
                                                        ' '.join('%.1e' % g for g in out[name + ':gap'][1:])))
    return res


def _savez(name, arrays):
    """np.savez with a fixed member timestamp: regenerating the fixtures gives the same bytes."""
    with zipfile.ZipFile(os.path.join(HERE, name), 'w', zipfile.ZIP_STORED) as z:
        for k in sorted(arrays):
            with z.open(zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0)), 'w', force_zip64=True) as f:
                np.lib.format.write_array(f, np.asanyarray(arrays[k]), allow_pickle=False)


def main():
    torch.manual_seed(0)
    written = []
    tables = {}
    do_tables(tables)
    _savez(R.TABLES_FILE, tables)
    steps = {}
    do_steps(steps)
    do_undo(steps)
    do_preprocessors(steps)
    _savez(R.STEPS_FILE, steps)
    toy = {}
    for part in chains(R.toy_model, R.toy_model, R.TOY_SHAPE, '32').values():
        toy.update(part)
    _savez(R.TOY_FILE, toy)
    written += [R.TABLES_FILE, R.STEPS_FILE, R.TOY_FILE]
    m32 = mg.build_ref_unet(gc.TINY_CFG, R.MODEL_SEED)
    for p in m32.parameters():
        p.requires_grad_(False)
    m64 = copy.deepcopy(m32).double()
    ss = gc.TINY_CFG['sample_size']
    for name, part in chains(lambda x, t: m32(x, t).sample, lambda x, t: m64(x, t).sample,
                             (R.CHAIN_B, gc.TINY_CFG['in_channels'], ss, ss), '64').items():
        _savez(R.CHAIN_FILE % name, part)
        written.append(R.CHAIN_FILE % name)
    for f in written:
        size = os.path.getsize(os.path.join(HERE, f))
        assert size < (1 << 20), (f, size)
        print(f, size)


if __name__ == '__main__':
    main()
