#!/usr/bin/env python3
"""Fixtures of UniPCMultistepScheduler (run in the build container only, on the CPU): the reference's own
diffusers.schedulers.scheduling_unipc_multistep.UniPCMultistepScheduler, imported through make_golden.py's shim.

Local wrappers stand between the reference's scheduler module and this machine while it runs; nothing of the reference is copied
or edited.  `RoundedOnceTorch` hands that module a view of torch in which
(1) sqrt / log / expm1 of an fp32 tensor are evaluated in fp64 and rounded to fp32 once (diffusion._rounded_once does the same;
    the reasoning is in make_golden_dpm_solver.py: torch's fp32 CPU functions differ in the last bit between hosts, and the solver
    differences lambda values that lie close together);
(2) linalg.solve of an fp32 system is solved in fp64 and rounded once, for the same reason;
(3) in the fp64 runs only (`einsum_casts`), einsum casts its fp32 coefficient vector to the operand's dtype: without it the
    reference raises "expected scalar type Double but found Float" on an fp64 sample, its rhos being fp32.
The UNet of the chains does not see the view.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_unipc.py

Writes (deterministic zip members, every file under 1 MiB; the case lists and seeds live in tests/unipc_ref.py):
  unipc_steps.npz    (a) the timestep table of every R.TABLE_CASES entry, and the reference's alpha_t / sigma_t / lambda_t tables for
                     R.SCHEDULES;
                     (b) per R.STEP_RUNS setting a teacher-forced fp32 run of the reference's `step` (step k is handed the seeded
                     x_k, e_k of R.step_inputs): the (corrector order, predictor order) of every step, and for the listed steps the
                     state entering (history, timestep_list, last_sample, lower_order_nums, this_order, t) and leaving it
                     (prev_sample, last_sample, the converted output, this_order) in fp32, the same step from the same entering
                     state in fp64, and their distances e_ref32
  unipc_chains.npz   (c) free-running chains of the reference UNet2DModel (TINY_CFG, det_init_ seed 5) for R.CHAINS from one
                     randn_tensor x_T: the timesteps, the fp64 states and the reference fp32 chain's gap to them at every state
  unipc_toy.npz      the same chains over the closed-form R.toy_model at 8 x 8: the reference's fp32 states themselves, the fp64
                     states and the gap"""
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
import unipc_ref as R                                               # noqa: E402  (case lists, toy model; reference-free)
from diffusers import UniPCMultistepScheduler                       # noqa: E402  (reference)
from diffusers.schedulers import scheduling_unipc_multistep as ref_module         # noqa: E402  (reference)
from diffusers.utils import randn_tensor                            # noqa: E402  (reference)


class _Linalg:
    def __init__(self, real):
        self._real = real

    def __getattr__(self, name):
        return getattr(self._real, name)

    def solve(self, A, b):
        if A.dtype == torch.float32:
            return self._real.solve(A.double(), b.double()).float()
        return self._real.solve(A, b)


class RoundedOnceTorch:
    """torch, as the reference's scheduler module sees it (module docstring)."""
    einsum_casts = False

    def __init__(self, real):
        self._real = real
        self.linalg = _Linalg(real.linalg)

    def __getattr__(self, name):
        return getattr(self._real, name)

    def _once(self, fn, t):
        return fn(t.double()).float() if t.dtype == torch.float32 else fn(t)

    def sqrt(self, t):
        return self._once(self._real.sqrt, t)

    def log(self, t):
        return self._once(self._real.log, t)

    def expm1(self, t):
        return self._once(self._real.expm1, t)

    def einsum(self, eq, coef, operand):
        if self.einsum_casts:
            coef = coef.to(operand.dtype)
        return self._real.einsum(eq, coef, operand)


assert ref_module.torch is torch
VIEW = RoundedOnceTorch(torch)
ref_module.torch = VIEW


def ref_scheduler(n, **kw):
    s = UniPCMultistepScheduler(**kw)
    s.set_timesteps(n)
    return s


def watch(s):
    """Log (corrector order or 0, predictor order) of each `step` from the reference's own two update methods."""
    seen = []

    def c(*a, _f=s.multistep_uni_c_bh_update, **k):
        seen.append(['c', k['order']])
        return _f(*a, **k)

    def p(*a, _f=s.multistep_uni_p_bh_update, **k):
        seen.append(['p', k['order']])
        return _f(*a, **k)
    s.multistep_uni_c_bh_update, s.multistep_uni_p_bh_update = c, p
    return seen


def pairs(seen):
    out, pc = [], 0
    for kind, order in seen:
        if kind == 'c':
            pc = order
        else:
            out.append((pc, order))
            pc = 0
    return out


def gap(a32, a64):
    return float((a32.double() - a64).abs().max())


def do_tables(out):
    for case in R.TABLE_CASES:
        sched, n = case
        s = ref_scheduler(n, beta_schedule=sched)
        ts = s.timesteps.numpy()
        assert ts.dtype == np.int64 and len(ts) == s.num_inference_steps <= n and len(set(ts.tolist())) == len(ts)
        out[R.table_name(case)] = ts
        print('  %-32s %4d steps  %s ... %s' % (R.table_name(case), len(ts), ts[:3].tolist(), ts[-2:].tolist()))
    for sched in R.SCHEDULES:                                                       # the reference's own fp32 tables
        s = UniPCMultistepScheduler(beta_schedule=sched)
        for n in ('alpha_t', 'sigma_t', 'lambda_t'):
            out['tables:%s:%s' % (sched, n)] = getattr(s, n).numpy()
            assert out['tables:%s:%s' % (sched, n)].dtype == np.float32
    assert len(out[R.table_name(('linear', 1000))]) < 1000                          # duplicates were removed


def to64(s):
    """A copy of the fp32 scheduler whose tensors of state are cast up: the same entering state, stepped in fp64."""
    d = copy.copy(s)
    d.model_outputs = [None if m is None else m.double() for m in s.model_outputs]
    d.timestep_list = list(s.timestep_list)
    d.last_sample = None if s.last_sample is None else s.last_sample.double()
    for name in ('multistep_uni_c_bh_update', 'multistep_uni_p_bh_update'):      # the watcher's wrappers are bound to `s`
        d.__dict__.pop(name, None)
    return d


def do_steps(out):
    seen_pairs = set()
    for run in R.STEP_RUNS:
        st, x0, so, lof, dc, sched, n, at = run
        name = R.run_name(run)
        s = ref_scheduler(n, **R.run_kwargs(run))
        assert s.config.solver_type == st
        seen = watch(s)
        ts = s.timesteps
        assert len(ts) == n
        for k in range(n):
            x, e = R.step_inputs(k)
            key = '%s@%d' % (name, k)
            if k in at:
                hist = [m for m in s.model_outputs if m is not None]
                out[key + ':in_n_hist'] = np.int64(len(hist))
                out[key + ':in_hist'] = np.stack([m.numpy() for m in hist]) if hist else np.zeros((0,) + R.STEP_SHAPE, np.float32)
                out[key + ':in_timestep_list'] = np.array([-1 if v is None else int(v) for v in s.timestep_list], np.int64)
                out[key + ':in_has_last'] = np.int64(s.last_sample is not None)
                out[key + ':in_last_sample'] = (s.last_sample if s.last_sample is not None else torch.zeros(R.STEP_SHAPE)).numpy().copy()
                out[key + ':in_lower_order_nums'] = np.int64(s.lower_order_nums)
                out[key + ':in_this_order'] = np.int64(getattr(s, 'this_order', 0) or 0)
                out[key + ':t'] = np.int64(int(ts[k]))
                d = to64(s)
                VIEW.einsum_casts = True
                try:
                    p64 = d.step(e.double(), ts[k], x.double()).prev_sample
                finally:
                    VIEW.einsum_casts = False
                assert p64.dtype == torch.float64 and d.last_sample.dtype == torch.float64
            prev = s.step(e, ts[k], x).prev_sample
            assert prev.dtype == torch.float32
            if k in at:
                pc, pp = pairs(seen)[k]
                seen_pairs.add((pc, pp))
                assert d.this_order == s.this_order == pp and d.lower_order_nums == s.lower_order_nums
                res = dict(prev=(prev, p64), last=(s.last_sample, d.last_sample), m=(s.model_outputs[-1], d.model_outputs[-1]))
                for what, (a32, a64) in res.items():
                    out['%s:%s32' % (key, what)], out['%s:%s64' % (key, what)] = a32.numpy().copy(), a64.numpy().copy()
                    out['%s:e_ref32_%s' % (key, what)] = np.float64(gap(a32, a64))
                    assert np.isfinite(a64.numpy()).all() and np.isfinite(a32.numpy()).all(), key
                out[key + ':pc'], out[key + ':pp'] = np.int64(pc), np.int64(pp)
                print('  %-52s (%d, %d)  e_ref32 prev %.2e last %.2e m %.2e   max|prev| %.2e' % (
                    key, pc, pp, out[key + ':e_ref32_prev'], out[key + ':e_ref32_last'], out[key + ':e_ref32_m'], float(p64.abs().max())))
        got = pairs(seen)
        assert got == R.decisions(so, n, lof, dc), (name, got)
        out[name + ':decisions'] = np.array(got, np.int64)
        out[name + ':timesteps'] = ts.numpy()
    assert sorted(R.step_case_ids()) == sorted({k.split(':in_hist')[0] for k in out if k.endswith(':in_hist')})
    # between them the listed steps reach every (pc, pp) that `step` can produce
    assert seen_pairs == R.reachable_pairs(), (sorted(seen_pairs), sorted(R.reachable_pairs()))
    print('  pairs reached:', sorted(seen_pairs))


def chains(model32, model64, shape, out, store):
    """store: which states to keep: '64' (for the bounds) and / or '32' (the reference's fp32 states, for the CPU test's bit equality)."""
    x_T = randn_tensor(shape, generator=torch.Generator().manual_seed(R.CHAIN_SEED))
    assert x_T.dtype == torch.float32
    out['x_T'] = x_T.numpy()
    for name, kw, n in R.CHAINS:
        runs, decided = {}, {}
        for tag, model, x in (('64', model64, x_T.double()), ('32', model32, x_T.clone())):
            s = ref_scheduler(n, **kw)
            seen = watch(s)
            xs = [x]
            VIEW.einsum_casts = tag == '64'
            try:
                with torch.no_grad():
                    for t in s.timesteps:
                        xs.append(s.step(model(xs[-1], t), t, xs[-1]).prev_sample)
            finally:
                VIEW.einsum_casts = False
            runs[tag], decided[tag] = xs, pairs(seen)
        assert len(s.timesteps) == n and all(v.dtype == torch.float64 for v in runs['64']) and all(v.dtype == torch.float32 for v in runs['32'])
        assert decided['32'] == decided['64'] == R.decisions(kw['solver_order'], n, kw.get('lower_order_final', True), kw.get('disable_corrector', ()))
        assert R.CHAIN_LOW[name] == all(max(p) <= 2 for p in decided['32'])
        out[name + ':timesteps'] = s.timesteps.numpy()
        out[name + ':decisions'] = np.array(decided['32'], np.int64)
        for tag in store:
            out[name + ':xs' + tag] = np.stack([v.numpy() for v in runs[tag]])
            assert np.isfinite(out[name + ':xs' + tag]).all()
        out[name + ':gap'] = np.array([gap(a, c) for a, c in zip(runs['32'], runs['64'])], np.float64)
        print('  %-18s max|x| %.2e  gap %s' % (name, max(float(v.abs().max()) for v in runs['64']), ' '.join('%.1e' % g for g in out[name + ':gap'][1:])))


def do_unet_chains():
    m32 = mg.build_ref_unet(gc.TINY_CFG, R.MODEL_SEED)
    for p in m32.parameters():
        p.requires_grad_(False)
    m64 = copy.deepcopy(m32).double()
    out = {}
    ss = gc.TINY_CFG['sample_size']
    chains(lambda x, t: m32(x, t).sample, lambda x, t: m64(x, t).sample, (R.CHAIN_B, gc.TINY_CFG['in_channels'], ss, ss), out, ('64',))
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
    chains(R.toy_model, R.toy_model, R.TOY_SHAPE, toy, ('32', '64'))
    _savez(R.TOY_FILE, toy)
    _savez(R.CHAINS_FILE, do_unet_chains())
    for f in (R.STEPS_FILE, R.TOY_FILE, R.CHAINS_FILE):
        size = os.path.getsize(os.path.join(HERE, f))
        assert size < (1 << 20), (f, size)
        print(f, size)


if __name__ == '__main__':
    main()
