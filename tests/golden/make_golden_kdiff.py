#!/usr/bin/env python3
"""Fixtures of LMSDiscreteScheduler, KDPM2DiscreteScheduler and KDPM2AncestralDiscreteScheduler (run in the build container only, on
the CPU): the reference's own three classes, imported through make_golden.py's shim.

While a reference scheduler runs -- and only then: the UNet of the chains does not run under it -- the `reference()` context of
make_golden_sigma.py is open (imported, not edited: `rounded_pow`, `rounded_tables`, `recording`), and around it `rounded_log`, which
does for `tensor.log()` of an fp32 tensor what `rounded_tables` does for `tensor.exp()`: evaluated in fp64 and rounded once.  The two
KDPM2 classes take the log of their sigma tables in fp32 torch, which the Euler and Heun classes do not.  The reference's arithmetic
on a host whose libraries round these correctly, and the same bits on every host; diffusion._rounded_once does the same.  So that this
patch cannot hide a real table difference, do_tables builds every table once more with `rounded_pow` alone, stores how many entries
differ and by how much (`unpatched:*` in kdiff_tables.npz) and asserts the counts of the build host (UNPATCHED_DIFFERING): last bits
of the sigmas, a few of the tables derived from them (up to 263 in sigmas_up at n = 1000, which differences neighbouring sigmas), and
timesteps that move by what one such bit is worth (at most 1.2e-4).  Nothing of the reference is copied or edited.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_kdiff.py

Writes (deterministic zip members, every file under 1 MiB; the case lists and seeds live in tests/kdiff_ref.py):
  kdiff_tables.npz       (a) timesteps (float64), sigmas, sigmas_interpol, sigmas_up / sigmas_down (fp32, NaN entries as they are)
                         and init_noise_sigma of every R.TABLE_CASES entry; the multistep coefficients of every index and order
                         1 .. 4 at n in R.LMS_COEF_NS as `get_lms_coefficient` returned them, rounded to fp32 once
  kdiff_steps_lms.npz, kdiff_steps_kdpm2.npz
                         (b) per R.STEP_RUNS setting a teacher-forced run of the reference's `step` in fp32 and in fp64 over the whole
                         timestep list (call k is handed the seeded x_k, e_k of R.step_inputs; the fp64 run sees the same fp32 values,
                         the same fp32 noise cast up, the scheduler's own fp32 scalars and the multistep coefficients rounded to
                         fp32): for the listed calls prev_sample (LMS: and pred_original_sample) in both precisions, their distances
                         e_ref32 and the scalars (R.KDPM2_COEF / R.LMS_COEF); (e) add_noise and scale_model_input cases in both states
  kdiff_chains.npz       (c) free-running chains of the reference UNet2DModel (TINY_CFG, det_init_ seed 5) for R.CHAINS from one
                         randn_tensor x_T: the timesteps, the fp64 states and the reference fp32 chain's gap to them at every state
  kdiff_toy.npz          (d) the same chains over the closed-form R.toy_model at 8 x 8: the reference's fp32 states themselves and the
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
import kdiff_ref as R                                               # noqa: E402  (case lists; reference-free)
from make_golden_pndm import rounded_pow, gap, _savez               # noqa: E402
from make_golden_sigma import reference as sigma_reference, ulps    # noqa: E402
import diffusers                                                    # noqa: E402  (reference)
from diffusers.utils import randn_tensor                            # noqa: E402  (reference)

# entries of (sigmas, sigmas_down, sigmas_interpol, sigmas_up, timesteps) that the table patches move on the build host
UNPATCHED_DIFFERING = (85, 110, 204, 104, 953)
ANCESTRAL_MODULE = 'diffusers.schedulers.scheduling_k_dpm_2_ancestral_discrete'


def ref_class(cls):
    return getattr(diffusers, R.CLASSES[cls])


@contextlib.contextmanager
def rounded_log():
    real = torch.Tensor.log

    def log_(self):
        return real(self.double()).float() if self.dtype == torch.float32 else real(self)
    torch.Tensor.log = log_
    try:
        yield
    finally:
        torch.Tensor.log = real


@contextlib.contextmanager
def reference(seen=None):
    with rounded_log(), sigma_reference(seen):
        yield


@contextlib.contextmanager
def fp32_noise(cls):
    """The fp64 runs draw the fp32 runs' noise: the reference's own randn_tensor in fp32, cast up."""
    if cls != 'kdpm2a':                                              # the others draw nothing
        yield
        return
    mod = importlib.import_module(ANCESTRAL_MODULE)
    real = mod.randn_tensor

    def draw(shape, generator=None, device=None, dtype=None, **kw):
        return real(shape, generator=generator, device=device, dtype=torch.float32, **kw).to(dtype)
    mod.randn_tensor = draw
    try:
        yield
    finally:
        mod.randn_tensor = real


@contextlib.contextmanager
def fp32_coefficients(s, seen):
    """The multistep coefficients of an LMS scheduler rounded to fp32 once -- what torch makes of a Python float that multiplies an
    fp32 tensor, so the fp32 run is unchanged and the fp64 run uses the same values -- and listed in `seen` in the order of the call."""
    if not hasattr(s, 'get_lms_coefficient'):
        yield
        return
    real = s.get_lms_coefficient

    def rounded(order, t, current_order):
        v = float(np.float32(real(order, t, current_order)))
        seen.append((order, current_order, v))
        return v
    s.get_lms_coefficient = rounded
    try:
        yield
    finally:
        del s.get_lms_coefficient


def ref_scheduler(cls, n=None, **kw):
    with reference():
        s = ref_class(cls)(**kw)
        if n is not None:
            s.set_timesteps(n)
    s.is_scale_input_called = True                                   # (no warning from the teacher-forced runs)
    return s


def unpatched_scheduler(cls, n, **kw):
    """The reference with `rounded_pow` alone: its table code on this host's own vector sqrt / log / exp and numpy's fp32 log."""
    with rounded_pow():
        s = ref_class(cls)(**kw)
        s.set_timesteps(n)
    return s


def tables_of(s, cls):
    return dict(sigmas=s.sigmas.numpy(), **{k: getattr(s, k).numpy() for k in R.EXTRA_TABLES[cls]})


def do_tables(out):
    stats = {k: [0, 0, 0] for k in ('sigmas', 'sigmas_interpol', 'sigmas_up', 'sigmas_down')}      # entries, differing, worst ulp
    moved, worst_t = 0, 0.0
    for case in R.TABLE_CASES:
        cls, _, _, n = case
        s = ref_scheduler(cls, n, **R.table_kwargs(case))
        name = R.table_name(case)
        ts, tabs = s.timesteps.numpy(), tables_of(s, cls)
        assert ts.dtype == np.float64 and (len(ts), len(tabs['sigmas'])) == R.table_lengths(case), (case, len(ts), len(tabs['sigmas']))
        assert np.isfinite(tabs['sigmas']).all() and tabs['sigmas'][-1] == 0.0
        # the ancestral class on the cosine schedule: sigmas_down[0] rounds to 0, its log is -inf and the interpolated time NaN
        assert np.isfinite(ts).all() or case[:2] == ('kdpm2a', 'squaredcos_cap_v2'), case
        out[name + ':timesteps'] = ts
        out[name + ':init_noise_sigma'] = np.float32(float(s.init_noise_sigma))
        u = unpatched_scheduler(cls, n, **R.table_kwargs(case))
        uts, utabs = u.timesteps.numpy(), tables_of(u, cls)
        assert uts.shape == ts.shape and float(u.init_noise_sigma) > 0
        for k, v in tabs.items():
            assert v.dtype == np.float32 and v.shape == tabs['sigmas'].shape and utabs[k].shape == v.shape
            out[name + ':' + k] = v
            nan = np.isnan(v)
            assert np.array_equal(nan, np.isnan(utabs[k])), (case, k)          # the patch moves no NaN
            d = ulps(v[~nan], utabs[k][~nan])
            stats[k] = [stats[k][0] + d.size, stats[k][1] + int((d != 0).sum()), max(stats[k][2], int(d.max()))]
            # `sigmas` is one patched sqrt away from exact arithmetic: one ulp at most.  The others difference close values derived
            # from it (sigmas_up: sigmas^2 - sigmas_next^2; sigmas_down: sigmas_next^2 - sigmas_up^2; the ancestral sigmas_interpol:
            # from sigmas_down), so one last bit of a sigma is worth many of theirs: stored, and the counts asserted below
            assert k != 'sigmas' or (d <= 1).all(), (case, k, d.max())
        tnan = np.isnan(ts)
        assert np.array_equal(tnan, np.isnan(uts)), case
        moved, worst_t = moved + int((uts[~tnan] != ts[~tnan]).sum()), max(worst_t, float(np.abs(uts[~tnan] - ts[~tnan]).max()))
        frac = int((ts != np.round(ts)).sum())
        nans = {k: int(np.isnan(v).sum()) for k, v in dict(tabs, timesteps=ts).items() if np.isnan(v).any()}
        print('  %-44s %4d timesteps (%4d fractional)  sigma %.4g .. %.4g  init %.6g  NaN %s' % (
            name, len(ts), frac, tabs['sigmas'][0], tabs['sigmas'][tabs['sigmas'] > 0][-1], float(s.init_noise_sigma), nans or '-'))
    print('  against the reference without the table patches on this host: %d timesteps differ, by at most %.3g; table entries '
          '(of, differing, by at most ulp): %s' % (moved, worst_t, stats))
    for k, v in stats.items():
        out['unpatched:' + k] = np.array(v, np.int64)
    out['unpatched:timesteps'] = np.array([moved], np.int64)
    out['unpatched:timesteps_worst'] = np.float64(worst_t)
    # the patches replace last-bit roundings of the host's libraries and nothing else: a table that differed for another reason would
    # be further off than this, in more places than these
    differing = tuple(stats[k][1] for k in sorted(stats)) + (moved,)
    assert stats['sigmas'][2] <= 1 and worst_t <= 1e-3, (stats, moved, worst_t)
    assert differing == UNPATCHED_DIFFERING, differing
    # the table facts the classes are held to
    k5 = R.table_name(('kdpm2', 'linear', 'plain', 5))
    assert np.isnan(out[k5 + ':sigmas_interpol'][0]) and np.isfinite(out[k5 + ':sigmas_interpol'][1:]).all()
    a5 = out[R.table_name(('kdpm2a', 'linear', 'plain', 5)) + ':timesteps']
    assert a5[0] == 999.0 and a5[2] == 749.25 and 0 < a5[1] - a5[2] < 1e-3, a5
    for cls in ('kdpm2', 'kdpm2a'):
        assert out[R.table_name((cls, 'linear', 'plain', 1)) + ':timesteps'].tolist() == [0.0]
    # the multistep coefficients
    for n in R.LMS_COEF_NS:
        s = ref_scheduler('lms', n)
        for t in range(n):
            for order in range(1, min(t + 1, 4) + 1):
                with reference():
                    got = [s.get_lms_coefficient(order, t, k) for k in range(order)]
                assert all(type(v) is float for v in got)
                out[R.lms_coef_name(n, t, order)] = np.array(got, np.float64).astype(np.float32)
    c = out[R.lms_coef_name(10, 5, 4)]
    print('  lms coefficients at n = 10, index 5, order 4: %s' % ' '.join('%.9g' % v for v in c))


def coefs_of(seen, lms_seen, cls, kw, second):
    """The scalars of one call by name from what `recording` saw, in the order the reference's expressions use them."""
    pt = kw.get('prediction_type', 'epsilon')
    want = {'epsilon': [('mul', 'sig'), ('div', 'sig')], 'v_prediction': [('mul', 'c_out'), ('div', 'c_den'), ('div', 'sig')],
            'sample': [('div', 'sig')]}[pt]
    names = R.LMS_COEF if cls == 'lms' else R.KDPM2_COEF
    if cls != 'lms':
        want = want + [('mul', 'dt')] + ([('mul', 'sigma_up')] if cls == 'kdpm2a' and second else [])
    assert [k for k, _ in seen] == [k for k, _ in want], (seen, want)
    c = dict.fromkeys(names, 0.0)
    for (_, v), (_, name) in zip(seen, want):
        assert c[name] in (0.0, v), (name, seen)                     # sig appears twice for an epsilon model: the same scalar
        c[name] = v
    if cls == 'lms':
        assert [k for _, k, _ in lms_seen] == list(range(len(lms_seen))) and len({o for o, _, _ in lms_seen}) == 1
        for order, k, v in lms_seen:
            c['c%d' % k] = v
    return np.array([c[n] for n in names], np.float32)


def do_steps(outs):
    for run in R.STEP_RUNS:
        sname, cls, kw, skw, n, at = run
        out = outs[R.steps_file(cls)]
        name = R.run_name(run)
        res = {}
        for tag, dt in (('32', torch.float32), ('64', torch.float64)):
            s = ref_scheduler(cls, n, **kw)
            ts = s.timesteps
            assert len(ts) == R.n_calls(cls, n)
            extra = dict(skw, generator=torch.Generator().manual_seed(R.GEN_SEED)) if cls == 'kdpm2a' else dict(skw)
            res[tag] = []
            for k in range(len(ts)):
                x, e = (v.to(dt) for v in R.step_inputs(k))
                seen, lms_seen = [], []
                second = cls != 'lms' and not s.state_in_first_order
                assert cls == 'lms' or second == (k % 2 == 1)
                with reference(seen), fp32_noise(cls), fp32_coefficients(s, lms_seen):
                    o = s.step(e, ts[k], x, **extra)
                assert o.prev_sample.dtype == dt
                if cls == 'lms':
                    assert len(lms_seen) == R.instance_of_call(cls, kw, skw, k)[1] and len(s.derivatives) == min(k + 1, skw.get('order', 4))
                res[tag].append((o.prev_sample, getattr(o, 'pred_original_sample', None), coefs_of(seen, lms_seen, cls, kw, second)))
            assert cls == 'lms' or not s.state_in_first_order          # left with `sample` set after the last call
        out[name + ':timesteps'] = ts.numpy()
        for k in at:
            (p32, q32, c32), (p64, q64, c64) = res['32'][k], res['64'][k]
            assert c32.tobytes() == c64.tobytes()                    # the fp64 run forms the same fp32 scalars
            key = '%s@%d' % (name, k)
            out[key + ':prev32'], out[key + ':prev64'] = p32.numpy(), p64.numpy()
            out[key + ':e_ref32'] = np.float64(gap(p32, p64))
            if q32 is not None:
                out[key + ':x0_32'], out[key + ':x0_64'] = q32.numpy(), q64.numpy()
                out[key + ':e_ref32_x0'] = np.float64(gap(q32, q64))
            out[key + ':coefs'] = c32
            assert np.isfinite(out[key + ':prev64']).all() and np.isfinite(out[key + ':prev32']).all(), key
            print('  %-32s %-44s e_ref32 %.2e   max|prev| %.2e' % (key, R.branch(R.instance_of_call(cls, kw, skw, k)), out[key + ':e_ref32'],
                                                                   np.abs(out[key + ':prev64']).max()))
    stored = {k.rsplit(':', 1)[0] for o in outs.values() for k in o if '@' in k}
    assert sorted(R.step_case_ids()) == sorted(stored)
    assert R.stored_coverage() == set(R.INSTANCES), sorted(set(R.INSTANCES) - R.stored_coverage())


def in_state(s, first):
    s.sample = None if first else torch.zeros(1)
    return s


def do_cases(out):
    x, z = (torch.from_numpy(gc.det_noise(R.STEP_SHAPE, 900 + i)) for i in range(2))
    for i, (cls, kw, idx, first) in enumerate(R.NOISE_CASES):
        s = in_state(ref_scheduler(cls, 10, **kw), first)
        with reference():
            y = s.add_noise(x, z, s.timesteps[idx])
        out['noise:%d:out' % i] = y.numpy()
    for i, (cls, kw, idx, first) in enumerate(R.SCALE_CASES):
        s = in_state(ref_scheduler(cls, 7, **kw), first)
        with reference():
            y = s.scale_model_input(x * R.X_SCALE, s.timesteps[idx])
        out['scale:%d:out' % i] = y.numpy()
        assert np.isfinite(out['scale:%d:out' % i]).all()


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
            extra = dict(generator=gen) if with_gen else {}
            xs = [x]
            with torch.no_grad():
                for t in s.timesteps:
                    with reference():
                        xin = s.scale_model_input(xs[-1], t)
                    eps = model(xin, t)                                  # not under the wrappers
                    with reference(), fp32_noise(cls), fp32_coefficients(s, []):
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
    tables, toy = {}, {}
    steps = {f: {} for f in R.STEPS_FILES.values()}
    do_tables(tables)
    _savez(R.TABLES_FILE, tables)
    do_steps(steps)
    do_cases(steps[R.STEPS_FILES['kdpm2']])
    for f, arrays in steps.items():
        _savez(f, arrays)
    chains(R.toy_model, R.toy_model, R.TOY_SHAPE, toy, '32')
    _savez(R.TOY_FILE, toy)
    _savez(R.CHAINS_FILE, do_unet_chains())
    for f in (R.TABLES_FILE, R.TOY_FILE, R.CHAINS_FILE) + tuple(R.STEPS_FILES.values()):
        size = os.path.getsize(os.path.join(HERE, f))
        assert size < (1 << 20), (f, size)
        print(f, size)


if __name__ == '__main__':
    main()
