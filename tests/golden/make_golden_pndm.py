#!/usr/bin/env python3
"""Fixtures of PNDMScheduler (run in the build container only, on the CPU): the reference's own
diffusers.schedulers.scheduling_pndm.PNDMScheduler, imported through make_golden.py's shim.

One local wrapper stands between the reference and this machine while its scheduler runs; nothing of the reference is copied or
edited.  torch's fp32 sqrt on the CPU comes from the host's vector math library: within an ulp, not correctly rounded on every host.
The reference takes its square roots as `tensor ** 0.5`, a tensor method, which a module-level view of torch cannot reach; so while
the reference scheduler runs -- and only then: the UNet of the chains does not run under it -- `rounded_pow` wraps
torch.Tensor.__pow__ so that a 0-d fp32 tensor raised to 0.5 is evaluated in fp64 and rounded to fp32 once
(diffusion._rounded_once does the same).  The fp64 square root is correctly rounded, and rounding it to fp32 gives the correctly
rounded fp32 square root (53 >= 2 x 24 + 2): the reference's arithmetic on a host whose library rounds sqrt correctly.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_pndm.py

Writes (deterministic zip members, every file under 1 MiB; the case lists and seeds live in tests/pndm_ref.py):
  pndm_steps.npz    (a) the timestep table of every R.TABLE_CASES entry with its prk / plms split, or the fact that the reference raised;
                    (b) per R.STEP_RUNS setting a teacher-forced run of the reference's `step` in fp32 and in fp64 over the whole
                    timestep list (call k is handed the seeded x_k, e_k of R.step_inputs; the fp64 run sees the same fp32 values cast
                    up, and the scheduler's own fp32 scalars): the mode each call took, and for the listed calls prev_sample in both
                    precisions with their distance e_ref32 and the fp32 scalars of _get_prev_sample as the reference formed them
  pndm_chains.npz   (c) free-running chains of the reference UNet2DModel (TINY_CFG, det_init_ seed 5) for R.CHAINS from one
                    randn_tensor x_T: the timesteps, the fp64 states and the reference fp32 chain's gap to them at every state
  pndm_toy.npz      the same chains over the closed-form R.toy_model at 8 x 8: the reference's fp32 states themselves (the CPU test
                    asks for the same bits) and their gap to the fp64 chain"""
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
import pndm_ref as R                                                # noqa: E402  (case lists, toy model; reference-free)
from diffusers import PNDMScheduler                                 # noqa: E402  (reference)
from diffusers.utils import randn_tensor                            # noqa: E402  (reference)


@contextlib.contextmanager
def rounded_pow(seen=None):
    """`seen`: a list that takes, in order, every 0-d fp32 tensor that multiplies or divides a tensor with dimensions while the
    context is open -- the scalars of _get_prev_sample as the reference itself formed them: [sa, sb,] sc, d, then den."""
    real = torch.Tensor.__pow__, torch.Tensor.__mul__, torch.Tensor.__truediv__

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
    torch.Tensor.__pow__, torch.Tensor.__mul__, torch.Tensor.__truediv__ = pow_, mul_, div_
    try:
        yield
    finally:
        torch.Tensor.__pow__, torch.Tensor.__mul__, torch.Tensor.__truediv__ = real


def ref_scheduler(n, **kw):
    with rounded_pow():
        s = PNDMScheduler(**kw)
        s.set_timesteps(n)
    return s


def ref_step(s, e, t, x, seen=None):
    with rounded_pow(seen):
        return s.step(e, t, x).prev_sample


def coefs_of(seen, v_pred):
    """(sa, sb, sc, d, den) as fp32 from what one call's rounded_pow saw; sa = sb = 0 for an epsilon model, which forms neither."""
    kinds, vals = [k for k, _ in seen], [v for _, v in seen]
    assert kinds == ['mul'] * (4 if v_pred else 2) + ['div'], seen
    return np.array(([] if v_pred else [0.0, 0.0]) + vals, np.float32)


def watch(s):
    """Log the mode of each `step` (from the reference's own state before the call) and the scalars _get_prev_sample is handed."""
    modes, scalars = [], []
    real_prk, real_plms, real_prev = s.step_prk, s.step_plms, s._get_prev_sample

    def prk(*a, **k):
        modes.append(s.counter % 4)
        return real_prk(*a, **k)

    def plms(*a, **k):
        c, have = s.counter, len(s.ets)
        modes.append(5 if c == 1 else 4 if c == 0 and have == 0 else 4 + min(have, 3) + 1)
        return real_plms(*a, **k)

    def prev(sample, timestep, prev_timestep, model_output):
        scalars.append((int(timestep), int(prev_timestep)))
        return real_prev(sample, timestep, prev_timestep, model_output)
    s.step_prk, s.step_plms, s._get_prev_sample = prk, plms, prev
    return modes, scalars


def gap(a32, a64):
    return float((a32.double() - a64).abs().max())


def do_tables(out):
    for case in R.TABLE_CASES:
        skip, off, n = case
        name = R.table_name(case)
        try:
            s = ref_scheduler(n, **R.table_kwargs(case))
        except ValueError as err:
            assert 'broadcast' in str(err) and not skip and n < 4, (case, err)
            out[name], out[name + ':raises'] = np.zeros(0, np.int64), np.int64(1)
            print('  %-22s the reference raises ValueError (%s)' % (name, str(err)[:60]))
            continue
        ts = s.timesteps.numpy()
        assert ts.dtype == np.int64 and len(ts) == len(s.prk_timesteps) + len(s.plms_timesteps)
        out[name], out[name + ':raises'], out[name + ':n_prk'] = ts, np.int64(0), np.int64(len(s.prk_timesteps))
        print('  %-22s %4d calls  %s ... %s' % (name, len(ts), ts[:6].tolist(), ts[-3:].tolist()))
    assert out[R.table_name((False, 0, 5))].tolist()[:6] == [800, 700, 700, 600, 600, 500] and len(out[R.table_name((False, 0, 5))]) == 14
    assert out[R.table_name((True, 0, 2))].tolist() == [500, 0, 0] and out[R.table_name((True, 0, 1))].tolist() == [0]


def do_steps(out):
    for run in R.STEP_RUNS:
        sname, kw, n, at = run
        name = R.run_name(run)
        res, modes, scal = {}, {}, {}
        for tag, dt in (('32', torch.float32), ('64', torch.float64)):
            s = ref_scheduler(n, **kw)
            modes[tag], scal[tag] = watch(s)
            ts = s.timesteps
            assert len(ts) == R.n_calls(kw, n)
            res[tag] = []
            for k in range(len(ts)):
                x, e = (v.to(dt) for v in R.step_inputs(k))
                seen = []
                prev = ref_step(s, e, ts[k], x, seen)
                assert prev.dtype == dt
                res[tag].append((prev, coefs_of(seen, kw.get('prediction_type') == 'v_prediction')))
        assert modes['32'] == modes['64'] == [R.mode_of_call(kw, k) for k in range(len(ts))], (name, modes)
        assert scal['32'] == scal['64']
        out[name + ':modes'] = np.array(modes['32'], np.int64)
        out[name + ':timesteps'] = ts.numpy()
        out[name + ':t_pairs'] = np.array(scal['32'], np.int64)         # (timestep, prev_timestep) as _get_prev_sample saw them
        for k in at:
            (p32, c32), (p64, c64) = res['32'][k], res['64'][k]
            assert c32.tobytes() == c64.tobytes()                       # the fp64 run forms the same fp32 scalars
            key = '%s@%d' % (name, k)
            out[key + ':prev32'], out[key + ':prev64'] = p32.numpy(), p64.numpy()
            out[key + ':e_ref32'] = np.float64(gap(p32, p64))
            out[key + ':coefs'] = c32                                   # (sa, sb, sc, d, den) as the reference formed them
            assert np.isfinite(out[key + ':prev64']).all() and np.isfinite(out[key + ':prev32']).all(), key
            print('  %-34s %-8s e_ref32 %.2e   max|prev| %.2e' % (key, R.MODES[modes['32'][k]], out[key + ':e_ref32'],
                                                                 np.abs(out[key + ':prev64']).max()))
    assert sorted(R.step_case_ids()) == sorted({k.rsplit(':', 1)[0] for k in out if '@' in k})
    # the stored calls hit all nine modes under both prediction types
    seen = {(R.MODES[int(out[R.run_name(r) + ':modes'][k])], r[1].get('prediction_type') == 'v_prediction') for r in R.STEP_RUNS for k in r[3]}
    assert seen == {(m, v) for m in R.MODES for v in (False, True)} == R.stored_coverage(), sorted(seen)


def chains(model32, model64, shape, out, store):
    """store: '64' (the fp64 states, for the GPU test's bound) or '32' (the reference's fp32 states, for the CPU test's bit equality)."""
    x_T = randn_tensor(shape, generator=torch.Generator().manual_seed(R.CHAIN_SEED))
    assert x_T.dtype == torch.float32
    out['x_T'] = x_T.numpy()
    for name, kw, n in R.CHAINS:
        runs = {}
        for tag, model, x in (('64', model64, x_T.double()), ('32', model32, x_T.clone())):
            s = ref_scheduler(n, **kw)
            xs = [x]
            with torch.no_grad():
                for t in s.timesteps:
                    eps = model(xs[-1], t)                                  # not under rounded_pow
                    xs.append(ref_step(s, eps, t, xs[-1]))
            runs[tag] = xs
        assert len(s.timesteps) == R.n_calls(kw, n)
        assert all(v.dtype == torch.float64 for v in runs['64']) and all(v.dtype == torch.float32 for v in runs['32'])
        out[name + ':timesteps'] = s.timesteps.numpy()
        out[name + ':xs' + store] = np.stack([v.numpy() for v in runs[store]])
        out[name + ':gap'] = np.array([gap(a, c) for a, c in zip(runs['32'], runs['64'])], np.float64)
        assert np.isfinite(out[name + ':xs' + store]).all()
        print('  %-10s max|x| %.2e  gap %s' % (name, float(runs['64'][-1].abs().max()), ' '.join('%.1e' % g for g in out[name + ':gap'][1:])))


def do_unet_chains():
    m32 = mg.build_ref_unet(gc.TINY_CFG, R.MODEL_SEED)
    for p in m32.parameters():
        p.requires_grad_(False)
    m64 = copy.deepcopy(m32).double()
    out = {}
    ss = gc.TINY_CFG['sample_size']
    chains(lambda x, t: m32(x, t).sample, lambda x, t: m64(x, t).sample, (R.CHAIN_B, gc.TINY_CFG['in_channels'], ss, ss), out, '64')
    return out


def _savez(name, arrays):
    """np.savez with a fixed member timestamp: regenerating the fixtures gives the same bytes."""
    with zipfile.ZipFile(os.path.join(HERE, name), 'w', zipfile.ZIP_STORED) as z:
        for k in sorted(arrays):
            with z.open(zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0)), 'w', force_zip64=True) as f:
                np.lib.format.write_array(f, np.asanyarray(arrays[k]), allow_pickle=False)


def main():
    torch.manual_seed(0)
    steps = {}
    do_tables(steps)
    do_steps(steps)
    _savez(R.STEPS_FILE, steps)
    toy = {}
    chains(R.toy_model, R.toy_model, R.TOY_SHAPE, toy, '32')
    _savez(R.TOY_FILE, toy)
    _savez(R.CHAINS_FILE, do_unet_chains())
    for f in (R.STEPS_FILE, R.TOY_FILE, R.CHAINS_FILE):
        size = os.path.getsize(os.path.join(HERE, f))
        assert size < (1 << 20), (f, size)
        print(f, size)


if __name__ == '__main__':
    main()
