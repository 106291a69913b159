#!/usr/bin/env python3
"""Fixtures of DEISMultistepScheduler and DPMSolverSinglestepScheduler (run in the build container only, on the CPU): the reference's own
diffusers.schedulers.scheduling_deis_multistep.DEISMultistepScheduler and scheduling_dpmsolver_singlestep.DPMSolverSinglestepScheduler,
imported through make_golden.py's shim.  Nothing of the reference is copied or edited.

The two wrappers of make_golden_dpm_solver.py stand between the reference and this machine while it runs, for the reasons given
there: `RoundedOnceTorch` (the scheduler modules' view of torch: sqrt / log / exp of an fp32 tensor evaluated in fp64 and rounded
once) and `int_linspace`.  One more is needed here: the log-rho coefficients of DEIS call NUMPY's log on 0-d fp32 torch tensors,
which returns an fp32 tensor computed by numpy's own fp32 log -- within an ulp, not correctly rounded, not the same on every host.
`RoundedOnceNumpy` hands the DEIS module a view of numpy whose log of an fp32 tensor is evaluated in fp64 and rounded to fp32 once,
the policy of diffusion._rounded_once, which forms the coefficients the same way.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_deis.py

Writes (deterministic zip members, every file under 1 MiB; the case lists and seeds live in tests/deis_ref.py):
  deis_steps.npz, dpm_single_steps.npz   (one per class)
                      (a) the timestep table of every R.TABLE_CASES entry of both classes; singlestep's `orders` and the order each
                      step actually took for every R.ORDER_CASES entry;
                      (b) per R.STEP_RUNS setting a teacher-forced run of the reference's `step` in fp32 and in fp64 (step k is
                      handed the seeded x_k, e_k of R.step_inputs -- in a thresholded run scaled per image so that the quantile of
                      |x0| falls below 1, inside (1, 2) and above sample_max_value = 2 within the batch, which is asserted here; the
                      fp64 run sees the same fp32 values cast up, and the scheduler's own fp32 scalars): the order each step took,
                      and for the listed steps prev_sample and the converted model output in both precisions with their distance
                      e_ref32
  deis_chains_*.npz   (c) free-running chains of the reference UNet2DModel (TINY_CFG, det_init_ seed 5) for R.CHAINS from one
                      randn_tensor x_T: the timesteps, the fp64 states and the reference fp32 chain's gap to them at every state
  deis_toy.npz        (d) the same chains over the closed-form R.toy_model at 8 x 8: the reference's fp32 states themselves (the CPU
                      test asks for the same bits) and their gap to the fp64 chain"""
import copy
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg                                            # noqa: E402  (reference import shim: sys.path, model builder)
import golden_common as gc                                          # noqa: E402
import make_golden_dpm_solver as gd                                 # noqa: E402  (RoundedOnceTorch, int_linspace, _savez, gap)
import deis_ref as R                                                # noqa: E402  (case lists; reference-free)
import threshold_ref as TR                                          # noqa: E402  (PRED; reference-free)
from diffusers.schedulers import scheduling_deis_multistep as ref_deis            # noqa: E402  (reference)
from diffusers.schedulers import scheduling_dpmsolver_singlestep as ref_single    # noqa: E402  (reference)
from diffusers.utils import randn_tensor                            # noqa: E402  (reference)


class RoundedOnceNumpy:
    """numpy, as the reference's DEIS module sees it: log of an fp32 torch tensor evaluated in fp64 and rounded once."""

    def __init__(self, real):
        self._real = real

    def __getattr__(self, name):
        return getattr(self._real, name)

    def log(self, t):
        if isinstance(t, torch.Tensor) and t.dtype == torch.float32:
            return torch.log(t.double()).float()
        return self._real.log(t)


assert ref_deis.torch is torch and ref_single.torch is torch and ref_deis.np is np
ref_deis.torch = ref_single.torch = gd.RoundedOnceTorch(torch)
ref_deis.np = RoundedOnceNumpy(np)
REF = {'deis': ref_deis.DEISMultistepScheduler, 'single': ref_single.DPMSolverSinglestepScheduler}
UPDATES = {'deis': ('deis_first_order_update', 'multistep_deis_second_order_update', 'multistep_deis_third_order_update'),
           'single': ('dpm_solver_first_order_update', 'singlestep_dpm_solver_second_order_update',
                      'singlestep_dpm_solver_third_order_update')}


def ref_scheduler(cls, n, **kw):
    s = REF[cls](**kw)
    with gd.int_linspace():
        s.set_timesteps(n)
    return s


def watch_orders(cls, s):
    """Log which of the reference's three update methods each `step` calls."""
    seen = []
    for order, name in enumerate(UPDATES[cls], 1):
        def wrapped(*a, _f=getattr(s, name), _o=order, **k):
            seen.append(_o)
            return _f(*a, **k)
        setattr(s, name, wrapped)
    return seen


def do_tables(out):
    for cls, cases in R.TABLE_CASES.items():
        for case in cases:
            s = ref_scheduler(cls, case[2], **R.table_kwargs(case))
            ts = s.timesteps.numpy()
            assert ts.dtype == np.int64 and len(ts) == case[2] and len(set(ts.tolist())) == len(ts), (cls, case)
            out[R.table_name(cls, case)] = ts
    assert out[R.table_name('single', R.CLIPPED)][0] < 999 == out[R.table_name('single', ('squaredcos_cap_v2', None, 20))][0]
    tiny = torch.zeros(1, 1, 2, 2)
    for case in R.ORDER_CASES:
        so, lof, n = case
        s = ref_scheduler('single', n, solver_order=so, lower_order_final=lof)
        seen = watch_orders('single', s)
        for t in s.timesteps:
            s.step(tiny, t, tiny)
        out[R.orders_name(case) + ':orders'] = np.array(s.orders, np.int64)
        out[R.orders_name(case) + ':taken'] = np.array(seen, np.int64)
        print('  %-16s orders %s taken %s' % (R.orders_name(case), s.orders, seen))
    odd = (3, True, 9)
    assert out[R.orders_name(odd) + ':orders'][-1] == 1 and out[R.orders_name(odd) + ':taken'][-1] == 3       # the reference's oddity


def x0_of(run, s, k, x, e):
    """The x0 the reference thresholds at step k, restated for choosing the scales only (fp64)."""
    pred = run[1].get('prediction_type', 'epsilon')
    t = int(s.timesteps[k])
    sa, sb = s.alpha_t[t].double(), s.sigma_t[t].double()
    x, e = x.double(), e.double()
    return {'epsilon': (x - sb * e) / sa, 'sample': e, 'v_prediction': sa * x - sb * e}[pred]


def quantiles(x0, ratio):
    return torch.quantile(x0.abs().reshape(x0.shape[0], -1), ratio, dim=1)


def do_steps(out):
    reached = set()
    for run in R.STEP_RUNS:
        cls, kw, n, at = run
        name = R.run_name(run)
        thr = R.run_thresholds(run)
        last = max(at)
        scales = None
        if thr:                                                                     # per step and image: the quantile lands on its target
            s = ref_scheduler(cls, n, **kw)
            scales = np.zeros((last + 1, R.STEP_SHAPE[0]), np.float32)
            for k in range(last + 1):
                q = quantiles(x0_of(run, s, k, *R.base_inputs(k)), s.config.dynamic_thresholding_ratio)
                scales[k] = (torch.tensor(R.TARGETS, dtype=torch.float64) / q).float().numpy()
                x, e = R.step_inputs(k, scales[k])
                got = quantiles(x0_of(run, s, k, x, e), s.config.dynamic_thresholding_ratio).tolist()
                assert got[0] < 1.0 < got[1] < R.MAX_VALUE < got[2], (name, k, got)
            out[name + ':scale'] = scales
        res, orders = {}, {}
        for tag, dt in (('32', torch.float32), ('64', torch.float64)):
            s = ref_scheduler(cls, n, **kw)
            orders[tag] = watch_orders(cls, s)
            ts = s.timesteps
            assert len(ts) == n
            res[tag] = []
            for k in range(last + 1):
                x, e = (v.to(dt) for v in R.step_inputs(k, None if scales is None else scales[k]))
                prev = s.step(e, ts[k], x).prev_sample
                assert prev.dtype == dt and s.model_outputs[-1].dtype == dt
                res[tag].append((prev, s.model_outputs[-1].clone()))
        assert orders['32'] == orders['64'], (name, orders)
        out[name + ':orders'] = np.array(orders['32'], np.int64)
        out[name + ':timesteps'] = ts.numpy()
        for k in at:
            (p32, m32), (p64, m64) = res['32'][k], res['64'][k]
            key = '%s@%d' % (name, k)
            out[key + ':prev32'], out[key + ':m0_32'] = p32.numpy(), m32.numpy()
            out[key + ':prev64'], out[key + ':m0_64'] = p64.numpy(), m64.numpy()
            out[key + ':e_ref32_prev'], out[key + ':e_ref32_m0'] = np.float64(gd.gap(p32, p64)), np.float64(gd.gap(m32, m64))
            assert np.isfinite(out[key + ':prev64']).all() and np.isfinite(out[key + ':prev32']).all(), key
            pred = TR.PRED[kw.get('prediction_type', 'epsilon')]
            reached.add((R.run_site(run, orders['32'][k]), pred, kw.get('algorithm_type', 'dpmsolver++') if cls == 'single' else 'deis', thr))
            print('  %-100s order %d  e_ref32 prev %.2e m0 %.2e   max|prev| %.2e max|m0| %.2e' % (
                key, orders['32'][k], out[key + ':e_ref32_prev'], out[key + ':e_ref32_m0'], np.abs(out[key + ':prev64']).max(),
                np.abs(out[key + ':m0_64']).max()))
    assert sorted(R.step_case_ids()) == sorted({k.rsplit(':', 1)[0] for k in out if '@' in k})
    # together the stored steps reach every launch site of both kernels, with every model type, algorithm and treatment
    for pred in range(3):
        for thr in (False, True):
            assert {(R.deis_site(o), pred, 'deis', thr) for o in (1, 2, 3)} <= reached, (pred, thr)
            for site in (R.single_site(1, False), R.single_site(2, False), R.single_site(3, False), R.single_site(3, True)):
                assert (site, pred, 'dpmsolver++', thr) in reached, (site, pred, thr)
                assert thr or (site, pred, 'dpmsolver', False) in reached, (site, pred)


def chains(models, shape, out, store, which):
    """store: '64' (the fp64 states, for the GPU test's bound) or '32' (the reference's fp32 states, for the CPU test's bit equality).
    models: (fp32 model, fp64 model); which: the file index of the chains to run, None for all."""
    x_T = randn_tensor(shape, generator=torch.Generator().manual_seed(R.CHAIN_SEED))
    assert x_T.dtype == torch.float32
    out['x_T'] = x_T.numpy()
    for name, cls, kw, n, f in R.CHAINS:
        if which is not None and f != which:
            continue
        runs = {}
        for tag, model, x in (('64', models[1], x_T.double()), ('32', models[0], x_T.clone())):
            s = ref_scheduler(cls, n, **kw)
            xs = [x]
            with torch.no_grad():
                for t in s.timesteps:
                    xs.append(s.step(model(xs[-1], t), t, xs[-1]).prev_sample)
            runs[tag] = xs
        assert len(s.timesteps) == n and all(v.dtype == torch.float64 for v in runs['64']) and all(v.dtype == torch.float32 for v in runs['32'])
        out[name + ':timesteps'] = s.timesteps.numpy()
        out[name + ':xs' + store] = np.stack([v.numpy() for v in runs[store]])
        out[name + ':gap'] = np.array([gd.gap(a, c) for a, c in zip(runs['32'], runs['64'])], np.float64)
        assert np.isfinite(out[name + ':xs' + store]).all()
        print('  %-26s max|x| %.2e  gap %s' % (name, float(runs['64'][-1].abs().max()), ' '.join('%.1e' % g for g in out[name + ':gap'][1:])))


def main():
    torch.manual_seed(0)
    steps = {}
    do_tables(steps)
    do_steps(steps)
    for cls, f in R.STEPS_FILES.items():
        gd._savez(f, {k: v for k, v in steps.items() if k.split(':')[1] == cls or (cls == 'single' and k.startswith('orders:'))})
    toy = {}
    chains((R.toy_model, R.toy_model), R.TOY_SHAPE, toy, '32', None)
    gd._savez(R.TOY_FILE, toy)
    m32 = mg.build_ref_unet(gc.TINY_CFG, R.MODEL_SEED)
    for p in m32.parameters():
        p.requires_grad_(False)
    m64 = copy.deepcopy(m32).double()
    ss = gc.TINY_CFG['sample_size']
    for i, f in enumerate(R.CHAINS_FILES):
        out = {}
        chains((lambda x, t: m32(x, t).sample, lambda x, t: m64(x, t).sample), (R.CHAIN_B, gc.TINY_CFG['in_channels'], ss, ss), out, '64', i)
        gd._savez(f, out)
    for f in tuple(R.STEPS_FILES.values()) + (R.TOY_FILE,) + R.CHAINS_FILES:
        size = os.path.getsize(os.path.join(HERE, f))
        assert size < (1 << 20), (f, size)
        print(f, size)


if __name__ == '__main__':
    main()
