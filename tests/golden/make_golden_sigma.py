#!/usr/bin/env python3
"""Fixtures of the sigma-space schedulers (run in the build container only, on the CPU): the reference's own EulerDiscreteScheduler,
EulerAncestralDiscreteScheduler and HeunDiscreteScheduler, imported through make_golden.py's shim.

While a reference scheduler runs -- and only then: the UNet of the chains does not run under it -- the `rounded_pow` wrapper of
make_golden_pndm.py is open (a 0-d fp32 tensor raised to 0.5 is evaluated in fp64 and rounded once), and around it `rounded_tables`,
which does the same for what the reference's table code takes from the host's vector math libraries: `tensor ** 0.5` of a whole fp32
table, `tensor.exp()` of the log_linear ramp and `np.log` of an fp32 array.  The reference's arithmetic on a host whose libraries
round these correctly, and the same bits on every host; diffusion._rounded_once does the same.  So that this patch cannot hide a real
table difference, do_tables builds every table once more with `rounded_pow` alone, stores how many entries differ and by how much
(`unpatched:*` in sigma_tables.npz) and asserts the counts of the build host (UNPATCHED_DIFFERING): last bits only.  `recording` lists, in order, every
0-d fp32 tensor that multiplies or divides a tensor with dimensions: the host scalars of a step as the reference itself formed them.
Nothing of the reference is copied or edited.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_sigma.py

Writes (deterministic zip members, every file under 1 MiB; the case lists and seeds live in tests/sigma_ref.py):
  sigma_tables.npz  (a) timesteps (float64), sigmas (fp32) and init_noise_sigma of every R.TABLE_CASES entry
  sigma_steps.npz   (b) per R.STEP_RUNS setting a teacher-forced run of the reference's `step` in fp32 and in fp64 over the whole
                    timestep list (call k is handed the seeded x_k, e_k of R.step_inputs; the fp64 run sees the same fp32 values and
                    the same fp32 noise cast up, and the scheduler's own fp32 scalars): for the listed calls prev_sample and
                    pred_original_sample in both precisions, their distances e_ref32 and the scalars (R.COEF_NAMES);
                    (e) add_noise and scale_model_input cases
  sigma_chains.npz  (c) free-running chains of the reference UNet2DModel (TINY_CFG, det_init_ seed 5) for R.CHAINS from one
                    randn_tensor x_T: the timesteps, the fp64 states and the reference fp32 chain's gap to them at every state
  sigma_toy.npz     (d) the same chains over the closed-form R.toy_model at 8 x 8: the reference's fp32 states themselves and the
                    generator's state after the chain"""
import contextlib
import copy
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg                                            # noqa: E402  (reference import shim: sys.path, model builder)
import golden_common as gc                                          # noqa: E402
import sigma_ref as R                                               # noqa: E402  (case lists, toy model; reference-free)
from make_golden_pndm import rounded_pow, gap, _savez               # noqa: E402
import diffusers                                                    # noqa: E402  (reference)
from diffusers.utils import randn_tensor                            # noqa: E402  (reference)

UNPATCHED_DIFFERING = (102, 1745)                                 # (sigmas, timesteps) that rounded_tables moves on the build host
MODULES = {'euler': 'scheduling_euler_discrete', 'ancestral': 'scheduling_euler_ancestral_discrete', 'heun': 'scheduling_heun_discrete'}


def ref_class(cls):
    return getattr(diffusers, R.CLASSES[cls])


@contextlib.contextmanager
def rounded_tables():
    real_pow, real_exp, real_log = torch.Tensor.__pow__, torch.Tensor.exp, np.log

    def pow_(self, other):
        if isinstance(other, float) and other == 0.5 and self.dim() > 0 and self.dtype == torch.float32:
            return torch.sqrt(self.double()).float()
        return real_pow(self, other)

    def exp_(self):
        return real_exp(self.double()).float() if self.dtype == torch.float32 else real_exp(self)

    def log_(a, *args, **kw):
        if not args and not kw and getattr(a, 'dtype', None) == np.float32:
            return real_log(np.asarray(a, np.float64)).astype(np.float32)
        return real_log(a, *args, **kw)
    torch.Tensor.__pow__, torch.Tensor.exp, np.log = pow_, exp_, log_
    try:
        yield
    finally:
        torch.Tensor.__pow__, torch.Tensor.exp, np.log = real_pow, real_exp, real_log


@contextlib.contextmanager
def recording(seen):
    real_mul, real_div = torch.Tensor.__mul__, torch.Tensor.__truediv__

    def scalar(a, b):
        return isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor) and a.dim() == 0 and a.dtype == torch.float32 and b.dim() > 0

    def mul_(self, other):
        if scalar(self, other) or scalar(other, self):
            seen.append(('mul', float(self if self.dim() == 0 else other)))
        return real_mul(self, other)

    def div_(self, other):
        if scalar(other, self):
            seen.append(('div', float(other)))
        return real_div(self, other)
    torch.Tensor.__mul__, torch.Tensor.__truediv__ = mul_, div_
    try:
        yield
    finally:
        torch.Tensor.__mul__, torch.Tensor.__truediv__ = real_mul, real_div


@contextlib.contextmanager
def reference(seen=None):
    with rounded_tables(), rounded_pow(), recording([] if seen is None else seen):
        yield


@contextlib.contextmanager
def fp32_noise(cls):
    """The fp64 runs draw the fp32 runs' noise: the reference's own randn_tensor in fp32, cast up."""
    if cls == 'heun':                                                # draws nothing
        yield
        return
    mod = importlib.import_module('diffusers.schedulers.' + MODULES[cls])
    real = mod.randn_tensor

    def draw(shape, generator=None, device=None, dtype=None, **kw):
        return real(shape, generator=generator, device=device, dtype=torch.float32, **kw).to(dtype)
    mod.randn_tensor = draw
    try:
        yield
    finally:
        mod.randn_tensor = real


def unpatched_scheduler(cls, n, **kw):
    """The reference with `rounded_pow` alone: its table code on this host's own vector sqrt / exp and numpy's fp32 log."""
    with rounded_pow():
        s = ref_class(cls)(**kw)
        s.set_timesteps(n)
    return s


def ulps(a, b):
    """Per entry of two fp32 arrays of one sign: how many representable values apart."""
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def ref_scheduler(cls, n=None, **kw):
    with reference():
        s = ref_class(cls)(**kw)
        if n is not None:
            s.set_timesteps(n)
    s.is_scale_input_called = True                                   # (no warning from the teacher-forced runs)
    return s


def coefs_of(seen, cls, kw, skw, churn):
    """The scalars of one call by name (R.COEF_NAMES) from what `recording` saw, in the order the reference's expressions use them."""
    pt = kw.get('prediction_type', 'epsilon')
    want = ([('mul', 'k')] if churn else []) + {'epsilon': [('mul', 'sig'), ('div', 'sig')], 'v_prediction': [('mul', 'c_out'), ('div', 'c_den'), ('div', 'sig')],
                                                'sample': [('div', 'sig')]}[pt] + [('mul', 'dt')] + ([('mul', 'sigma_up')] if cls == 'ancestral' else [])
    assert [k for k, _ in seen] == [k for k, _ in want], (seen, want)
    c = dict.fromkeys(R.COEF_NAMES, 0.0)
    for (_, v), (_, name) in zip(seen, want):
        assert c[name] in (0.0, v), (name, seen)                     # sig appears twice for an epsilon model: the same scalar
        c[name] = v
    if churn:
        c['s_noise'] = float(np.float32(skw['s_noise']))
    return np.array([c[n] for n in R.COEF_NAMES], np.float32)


def do_tables(out):
    # what `rounded_tables` changes on this host: entries of the tables that differ from the reference without it
    entries = differing = worst_ulp = moved = 0
    worst_t = 0.0
    for case in R.TABLE_CASES:
        cls, _, _, n = case
        s = ref_scheduler(cls, n, **R.table_kwargs(case))
        name = R.table_name(case)
        ts, sig = s.timesteps.numpy(), s.sigmas.numpy()
        assert ts.dtype == np.float64 and sig.dtype == np.float32 and (len(ts), len(sig)) == R.table_lengths(case), (case, len(ts), len(sig))
        assert np.isfinite(ts).all() and np.isfinite(sig).all() and sig[-1] == 0.0
        out[name + ':timesteps'], out[name + ':sigmas'] = ts, sig
        out[name + ':init_noise_sigma'] = np.float32(float(s.init_noise_sigma))
        u = unpatched_scheduler(cls, n, **R.table_kwargs(case))
        uts, usig = u.timesteps.numpy(), u.sigmas.numpy()
        assert uts.shape == ts.shape and usig.shape == sig.shape and float(u.init_noise_sigma) > 0
        d = ulps(sig, usig)
        entries, differing, worst_ulp = entries + d.size, differing + int((d != 0).sum()), max(worst_ulp, int(d.max()))
        moved, worst_t = moved + int((uts != ts).sum()), max(worst_t, float(np.abs(uts - ts).max()))
        frac = int((ts != np.round(ts)).sum())
        print('  %-48s %4d timesteps (%4d fractional)  sigma %.4g .. %.4g  init %.6g' % (name, len(ts), frac, sig[0], sig[-2], float(s.init_noise_sigma)))
    print('  against the reference without rounded_tables on this host: %d of %d sigmas differ, by at most %d ulp; %d timesteps differ, '
          'by at most %.3g' % (differing, entries, worst_ulp, moved, worst_t))
    out['unpatched:sigmas'] = np.array([entries, differing, worst_ulp], np.int64)
    out['unpatched:timesteps'] = np.array([moved], np.int64)
    out['unpatched:timesteps_worst'] = np.float64(worst_t)
    # the patch replaces a last-bit rounding of the host's libraries and nothing else: a table that differed for another reason would
    # be further off than this, in more places than these
    assert worst_ulp <= 1 and worst_t <= 1e-3 and (differing, moved) == UNPATCHED_DIFFERING, (differing, worst_ulp, moved, worst_t)
    assert int((out[R.table_name(('euler', 'linear', 'plain', 50)) + ':timesteps'] % 1 != 0).sum()) == 48
    assert int((out[R.table_name(('euler', 'linear', 'karras', 10)) + ':timesteps'] % 1 != 0).sum()) == 8


def do_steps(out):
    for run in R.STEP_RUNS:
        sname, cls, kw, skw, n, at = run
        name = R.run_name(run)
        res = {}
        for tag, dt in (('32', torch.float32), ('64', torch.float64)):
            s = ref_scheduler(cls, n, **kw)
            ts = s.timesteps
            assert len(ts) == R.n_calls(cls, n)
            gen = torch.Generator().manual_seed(R.GEN_SEED)
            extra = dict(skw, generator=gen) if cls != 'heun' else {}
            res[tag] = []
            for k in range(len(ts)):
                x, e = (v.to(dt) for v in R.step_inputs(k))
                seen = []
                with reference(seen), fp32_noise(cls):
                    o = s.step(e, ts[k], x, **extra)
                churn = cls == 'euler' and len(seen) == products_without_churn(kw) + 1         # one product more: eps * k
                assert o.prev_sample.dtype == dt
                res[tag].append((o.prev_sample, getattr(o, 'pred_original_sample', None), coefs_of(seen, cls, kw, skw, churn), churn))
        out[name + ':timesteps'] = ts.numpy()
        out[name + ':churn'] = np.array([r[3] for r in res['32']], np.int64)
        for k in at:
            (p32, q32, c32, ch32), (p64, q64, c64, ch64) = res['32'][k], res['64'][k]
            assert c32.tobytes() == c64.tobytes() and ch32 == ch64      # the fp64 run forms the same fp32 scalars
            key = '%s@%d' % (name, k)
            out[key + ':prev32'], out[key + ':prev64'] = p32.numpy(), p64.numpy()
            out[key + ':e_ref32'] = np.float64(gap(p32, p64))
            if q32 is not None:
                out[key + ':x0_32'], out[key + ':x0_64'] = q32.numpy(), q64.numpy()
                out[key + ':e_ref32_x0'] = np.float64(gap(q32, q64))
            out[key + ':coefs'] = c32
            assert np.isfinite(out[key + ':prev64']).all() and np.isfinite(out[key + ':prev32']).all(), key
            print('  %-30s %-9s churn %d  e_ref32 %.2e   max|prev| %.2e' % (key, R.MODES[R.mode_of_call(cls, k)], ch32, out[key + ':e_ref32'],
                                                                          np.abs(out[key + ':prev64']).max()))
    assert sorted(R.step_case_ids()) == sorted({k.rsplit(':', 1)[0] for k in out if '@' in k})
    assert R.stored_coverage() == set(R.INSTANCES), sorted(set(R.INSTANCES) - R.stored_coverage())
    churned = {r[0] for r in R.STEP_RUNS if any(out['%s:churn' % R.run_name(r)][k] for k in r[5])}
    assert churned == {'euler_churn', 'euler_v_churn'}, churned


def products_without_churn(kw):
    """How many scalar-times-tensor products and quotients an Euler step without churn forms (the conversion, / sigma_hat, * dt)."""
    return {'epsilon': 3, 'v_prediction': 4, 'sample': 2}[kw.get('prediction_type', 'epsilon')]


def do_cases(out):
    x, z = (torch.from_numpy(gc.det_noise(R.STEP_SHAPE, 900 + i)) for i in range(2))
    for i, (cls, kw, idx) in enumerate(R.NOISE_CASES):
        s = ref_scheduler(cls, 10, **kw)
        with reference():
            y = s.add_noise(x, z, s.timesteps[idx])
        out['noise:%d:out' % i], out['noise:%d:sigmas' % i] = y.numpy(), s.sigmas[idx].numpy()
    for i, (cls, kw, idx) in enumerate(R.SCALE_CASES):
        s = ref_scheduler(cls, 7, **kw)
        with reference():
            y = s.scale_model_input(x * R.X_SCALE, s.timesteps[idx])
        out['scale:%d:out' % i] = y.numpy()


def chains(model32, model64, shape, out, store):
    """store: '64' (the fp64 states, for the GPU test's bound) or '32' (the reference's fp32 states, for the CPU test's bit equality)."""
    x_T = randn_tensor(shape, generator=torch.Generator().manual_seed(R.CHAIN_SEED))
    assert x_T.dtype == torch.float32
    out['x_T'] = x_T.numpy()
    for name, cls, kw, n, with_gen in R.CHAINS:
        runs = {}
        for tag, model, x in (('64', model64, x_T.double()), ('32', model32, x_T.clone())):
            s = ref_scheduler(cls, **kw)
            x = x * s.init_noise_sigma                                   # pipeline_latent_diffusion_uncond.py: before set_timesteps
            with reference():
                s.set_timesteps(n)
            gen = torch.Generator().manual_seed(R.NOISE_SEED) if with_gen else None
            extra = dict(generator=gen) if cls != 'heun' else {}
            xs = [x]
            with torch.no_grad():
                for t in s.timesteps:
                    with reference():
                        xin = s.scale_model_input(xs[-1], t)
                    eps = model(xin, t)                                  # not under the wrappers
                    with reference(), fp32_noise(cls):
                        xs.append(s.step(eps, t, xs[-1], **extra).prev_sample)
            runs[tag] = xs
        assert len(s.timesteps) == R.n_calls(cls, n)
        assert all(v.dtype == torch.float64 for v in runs['64']) and all(v.dtype == torch.float32 for v in runs['32'])
        out[name + ':timesteps'] = s.timesteps.numpy()
        out[name + ':xs' + store] = np.stack([v.numpy() for v in runs[store]])
        out[name + ':gap'] = np.array([gap(a, c) for a, c in zip(runs['32'], runs['64'])], np.float64)
        if with_gen:
            out[name + ':gen_state'] = gen.get_state().numpy()           # of the fp32 run, the last one
        assert np.isfinite(out[name + ':xs' + store]).all()
        print('  %-16s max|x_0| %.2e  gap %s' % (name, float(runs['64'][-1].abs().max()), ' '.join('%.1e' % g for g in out[name + ':gap'][1:])))


def do_unet_chains():
    m32 = mg.build_ref_unet(gc.TINY_CFG, R.MODEL_SEED)
    for p in m32.parameters():
        p.requires_grad_(False)
    m64 = copy.deepcopy(m32).double()
    out = {}
    ss = gc.TINY_CFG['sample_size']
    chains(lambda x, t: m32(x, t).sample, lambda x, t: m64(x, t).sample, (R.CHAIN_B, gc.TINY_CFG['in_channels'], ss, ss), out, '64')
    return out


def main():
    torch.manual_seed(0)
    tables, steps, toy = {}, {}, {}
    do_tables(tables)
    _savez(R.TABLES_FILE, tables)
    do_steps(steps)
    do_cases(steps)
    _savez(R.STEPS_FILE, steps)
    chains(R.toy_model, R.toy_model, R.TOY_SHAPE, toy, '32')
    _savez(R.TOY_FILE, toy)
    _savez(R.CHAINS_FILE, do_unet_chains())
    for f in (R.TABLES_FILE, R.STEPS_FILE, R.TOY_FILE, R.CHAINS_FILE):
        size = os.path.getsize(os.path.join(HERE, f))
        assert size < (1 << 20), (f, size)
        print(f, size)


if __name__ == '__main__':
    main()
