#!/usr/bin/env python3
"""Fixtures of DPMSolverMultistepScheduler (run in the build container only, on the CPU): the reference's own
diffusers.schedulers.scheduling_dpmsolver_multistep.DPMSolverMultistepScheduler, imported through make_golden.py's shim.

Two local wrappers stand between the reference and this machine while it runs; nothing of the reference is copied or edited.

(1) torch's fp32 sqrt / log / exp on the CPU come from the host's vector math library: within an ulp, not correctly rounded, and
not the same on every host (two x86 hosts of different vendors with the same torch build disagree on 5 of the 1000 alpha_t entries and on
single exp values).  The solver differences lambda values that lie close together, so one such bit moves a third-order update by
ten times its fp32 rounding error: fixtures written with the host's functions would hold on hosts of one kind only.  `RoundedOnceTorch`
hands the reference's scheduler module a view of torch whose sqrt / log / exp of an fp32 tensor are evaluated in fp64 and rounded to
fp32 once (diffusion._rounded_once does the same): the reference's arithmetic with correctly rounded elementary functions, which is
what it computes on a host whose library rounds them correctly.  The UNet of the chains does not see the view.

(2) With a current numpy the reference's set_timesteps fails inside np.linspace ("step must be greater than zero"): it passes the 0-d
tensor `clipped_idx` in the stop value.  `int_linspace` below turns tensor arguments of np.linspace into ints while the reference
runs.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_dpm_solver.py

Writes (deterministic zip members, every file under 1 MiB; the case lists and seeds live in tests/dpm_solver_ref.py):
  dpm_solver_steps.npz    (a) the timestep table of every R.TABLE_CASES entry, and the reference's alpha_t / sigma_t / lambda_t tables
                          for the two beta schedules in use;
                          (b) per R.STEP_RUNS setting a teacher-forced run of the reference's `step` in fp32 and in fp64 (step k is
                          handed the seeded x_k, e_k of R.step_inputs; the fp64 run sees the same fp32 values cast up, and the
                          scheduler's own fp32 scalars): the order each step took, and for the listed steps prev_sample and the
                          converted model output in both precisions with their distance e_ref32
  dpm_solver_chains.npz   (c) free-running chains of the reference UNet2DModel (TINY_CFG, det_init_ seed 5) for R.CHAINS from one
                          randn_tensor x_T: the timesteps, the fp64 states and the reference fp32 chain's gap to them at every state
  dpm_solver_toy.npz      the same chains over the closed-form R.toy_model at 8 x 8: the reference's fp32 states themselves (the CPU
                          test asks for the same bits) and their gap to the fp64 chain"""
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
import dpm_solver_ref as R                                          # noqa: E402  (case lists, toy model; reference-free)
from diffusers import DPMSolverMultistepScheduler                   # noqa: E402  (reference)
from diffusers.schedulers import scheduling_dpmsolver_multistep as ref_module     # noqa: E402  (reference)
from diffusers.utils import randn_tensor                            # noqa: E402  (reference)


class RoundedOnceTorch:
    """torch, as the reference's scheduler module sees it: sqrt / log / exp of an fp32 tensor evaluated in fp64 and rounded once."""

    def __init__(self, real):
        self._real = real

    def __getattr__(self, name):
        return getattr(self._real, name)

    def _once(self, fn, t):
        return fn(t.double()).float() if t.dtype == torch.float32 else fn(t)

    def sqrt(self, t):
        return self._once(self._real.sqrt, t)

    def log(self, t):
        return self._once(self._real.log, t)

    def exp(self, t):
        return self._once(self._real.exp, t)


assert ref_module.torch is torch
ref_module.torch = RoundedOnceTorch(torch)


@contextlib.contextmanager
def int_linspace():
    real = np.linspace

    def linspace(*a, **k):
        a = tuple(int(v) if isinstance(v, torch.Tensor) else v for v in a)
        k = {n: (int(v) if isinstance(v, torch.Tensor) else v) for n, v in k.items()}
        return real(*a, **k)
    np.linspace = linspace
    try:
        yield
    finally:
        np.linspace = real


def ref_scheduler(n, **kw):
    s = DPMSolverMultistepScheduler(**kw)
    with int_linspace():
        s.set_timesteps(n)
    return s


def watch_orders(s):
    """Log which of the reference's three update methods each `step` calls."""
    seen = []
    for order, name in ((1, 'dpm_solver_first_order_update'), (2, 'multistep_dpm_solver_second_order_update'),
                        (3, 'multistep_dpm_solver_third_order_update')):
        def wrapped(*a, _f=getattr(s, name), _o=order, **k):
            seen.append(_o)
            return _f(*a, **k)
        setattr(s, name, wrapped)
    return seen


def gap(a32, a64):
    return float((a32.double() - a64).abs().max())


def do_tables(out):
    for case in R.TABLE_CASES:
        _, _, _, n = case
        s = ref_scheduler(n, **R.table_kwargs(case))
        ts = s.timesteps.numpy()
        assert ts.dtype == np.int64 and len(ts) == s.num_inference_steps <= n and len(set(ts.tolist())) == len(ts)
        out[R.table_name(case)] = ts
        print('  %-40s %4d steps  %s ... %s' % (R.table_name(case), len(ts), ts[:3].tolist(), ts[-2:].tolist()))
    for sched in ('linear', 'squaredcos_cap_v2'):                                   # the reference's own fp32 tables
        s = DPMSolverMultistepScheduler(beta_schedule=sched)
        for n in ('alpha_t', 'sigma_t', 'lambda_t'):
            out['tables:%s:%s' % (sched, n)] = getattr(s, n).numpy()
            assert out['tables:%s:%s' % (sched, n)].dtype == np.float32
    plain = out[R.table_name(('linear', None, False, 20))]
    clipped = out[R.table_name(R.CLIPPED)]
    assert clipped[0] < 999 and plain[0] == 999, (clipped[0], plain[0])            # the finite lambda_min_clipped does clip
    assert len(out[R.table_name(('linear', None, False, 1000))]) < 1000             # duplicates were removed


def do_steps(out):
    for run in R.STEP_RUNS:
        algo, stype, so, n, at = run
        name = R.run_name(run)
        res, orders = {}, {}
        for tag, dt in (('32', torch.float32), ('64', torch.float64)):
            s = ref_scheduler(n, algorithm_type=algo, solver_type=stype, solver_order=so)
            orders[tag] = watch_orders(s)
            ts = s.timesteps
            assert len(ts) == n
            res[tag] = []
            for k in range(n):
                x, e = (v.to(dt) for v in R.step_inputs(k))
                prev = s.step(e, ts[k], x).prev_sample
                assert prev.dtype == dt and s.model_outputs[-1].dtype == dt
                res[tag].append((prev, s.model_outputs[-1].clone()))
        assert orders['32'] == orders['64'] == (R.ORDERS_10 if n == 10 else R.ORDERS_20)[so], (name, orders)
        out[name + ':orders'] = np.array(orders['32'], np.int64)
        out[name + ':timesteps'] = ts.numpy()
        for k in at:
            (p32, m32), (p64, m64) = res['32'][k], res['64'][k]
            key = '%s@%d' % (name, k)
            out[key + ':prev32'], out[key + ':m0_32'] = p32.numpy(), m32.numpy()
            out[key + ':prev64'], out[key + ':m0_64'] = p64.numpy(), m64.numpy()
            out[key + ':e_ref32_prev'], out[key + ':e_ref32_m0'] = np.float64(gap(p32, p64)), np.float64(gap(m32, m64))
            assert np.isfinite(out[key + ':prev64']).all() and np.isfinite(out[key + ':prev32']).all(), key
            print('  %-36s order %d  e_ref32 prev %.2e m0 %.2e   max|prev| %.2e max|m0| %.2e' % (
                key, orders['32'][k], out[key + ':e_ref32_prev'], out[key + ':e_ref32_m0'], np.abs(out[key + ':prev64']).max(),
                np.abs(out[key + ':m0_64']).max()))
    assert sorted(R.step_case_ids()) == sorted({k.rsplit(':', 1)[0] for k in out if '@' in k})


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
                    xs.append(s.step(model(xs[-1], t), t, xs[-1]).prev_sample)
            runs[tag] = xs
        assert len(s.timesteps) == n and all(v.dtype == torch.float64 for v in runs['64']) and all(v.dtype == torch.float32 for v in runs['32'])
        out[name + ':timesteps'] = s.timesteps.numpy()
        out[name + ':xs' + store] = np.stack([v.numpy() for v in runs[store]])
        out[name + ':gap'] = np.array([gap(a, c) for a, c in zip(runs['32'], runs['64'])], np.float64)
        assert np.isfinite(out[name + ':xs' + store]).all()
        print('  %-18s max|x| %.2e  gap %s' % (name, float(runs['64'][-1].abs().max()), ' '.join('%.1e' % g for g in out[name + ':gap'][1:])))


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
