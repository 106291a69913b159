"""Dynamic thresholding and x0 / v-prediction in DDPMScheduler and DDIMScheduler on the host (`-m "not gpu"`): the stand-in's
quantile (tests/threshold_ref.py: torch.sort and one exactly rounded fma) against torch.quantile bit for bit; the two schedulers
over the CPU stand-ins of the three new ops (tests/mock_ops_threshold.py) against every fixture step that
tests/golden/make_golden_threshold.py recorded from the reference's own schedulers -- bit for bit against the reference's fp32
result -- and the toy-model chains; the config keys, from_config between the classes, the directory round trip of a thresholding
pipeline; the untouched default path; and the launch-site table of csrc/threshold.hip."""
import ctypes
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

import golden_common as gc
import threshold_ref as R
from helpers import pkg

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture()
def mocked(monkeypatch):
    import mock_ops_threshold as mock
    monkeypatch.setattr(pkg('diffusion'), 'ops', mock)
    del mock.calls[:]
    return mock


# ------------------------------------------------------------------------------------------------ the stand-in's quantile
def _special_rows(n):
    """Rows with ties, zeros of both signs, denormals, an infinity, a NaN (the last row)."""
    gen = torch.Generator().manual_seed(n)
    v = torch.randn(6, n, generator=gen)
    v[0] = torch.round(v[0] * 2) / 2
    v[1] = torch.where(torch.rand(n, generator=gen) < 0.7, torch.zeros(()), v[1]) * torch.where(torch.rand(n, generator=gen) < 0.5, -1.0, 1.0)
    v[2] = v[2] * 1e-41
    v[3, n // 2] = float('inf')
    v[5, n // 3] = float('nan')
    return v


@pytest.mark.parametrize('n', [1, 2, 5, 48, 3072, 12288])
def test_stand_in_quantile_equals_torch_quantile_bit_for_bit(n):
    v = _special_rows(n)
    assert n < 48 or (bool((v[1] == 0).any()) and bool(((v[2] != 0) & (v[2].abs() < 1.17e-38)).any()))
    for ratio in (0.0, 0.3, 0.5, 0.995, 1.0):
        for rows in (v, v[:1], v[:3] * 3.0):
            st = R.abs_quantile(None, rows, R.SAMPLE, 1.0, 0.0, ratio, 2.0)
            want = torch.quantile(rows.abs(), ratio, dim=1)
            assert R.same_bits(st[:, 2], want), (n, ratio, st[:, 2], want)
            assert R.same_bits(st[:, 3], torch.clamp(want, min=1, max=2.0))
            srt = torch.sort(rows.abs(), dim=1).values
            lo, hi, w = R.quantile_rank(ratio, n)
            assert R.same_bits(st[:, 0], srt[:, lo]) and R.same_bits(st[:, 1], srt[:, hi]) and 0 <= w < 1 and hi - lo in (0, 1)
            assert pkg('ops').quantile_rank(ratio, n) == (lo, hi, float(w))
    if n >= 3:
        assert bool(torch.isnan(R.abs_quantile(None, v, R.SAMPLE, 1.0, 0.0, 0.5, 2.0)[5, 2:]).all())
    x, m = torch.randn(3, n, generator=torch.Generator().manual_seed(1)), v[:3] * 0.5
    for pred in (R.EPSILON, R.V):                                                 # through the other two model types
        x0 = R.form(pred, x, m, torch.tensor(0.8), torch.tensor(0.6))[0]
        assert R.same_bits(R.abs_quantile(x, m, pred, 0.8, 0.6, 0.995, 9.0)[:, 2], torch.quantile(x0.abs(), 0.995, dim=1))


def test_fma32_is_rounded_once():
    r = np.random.default_rng(3)
    a, b, c = (r.standard_normal(20000).astype(np.float32) for _ in range(3))
    c = (c * np.float32(1e-3)).astype(np.float32)
    from fractions import Fraction
    got = R.fma32(a, b, c)
    for i in range(0, 20000, 7):
        exact = Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i]))
        lo = np.float32(float(exact))
        cands = [np.nextafter(lo, np.float32(-np.inf)), lo, np.nextafter(lo, np.float32(np.inf))]
        best = min(cands, key=lambda v: (abs(Fraction(float(v)) - exact), int(v.view(np.int32)) & 1))
        assert got[i] == best, (i, got[i], best)
    assert np.isnan(R.fma32(np.float32(np.inf), np.float32(1), np.float32(-np.inf)))                  # inf - inf, as the hardware's


# ------------------------------------------------------------------------------------------------ the fixtures
def test_fixtures_cover_what_they_must():
    assert len(R.ddpm_cases()) == 3 * 5 * 3 and len(R.ddim_cases()) == 3 * 5 * 3 * 4
    for f in R.step_files() + [R.CHAINS_FILE, R.TOY_FILE]:
        assert os.path.getsize(os.path.join(HERE, 'golden', f)) <= 1 << 20, f
    g = R.load(R.ddpm_file())
    for case in R.ddpm_cases():
        k = R.ddpm_key(case)
        assert g[k + ':prev64'].dtype == np.float64 and g[k + ':x032'].shape == R.STEP_SHAPE and g[k + ':x032'].dtype == np.float32
    assert {int(g[R.ddpm_key((p, 'none', 'last')) + ':t']) for p in R.PREDS} == {0}
    for p in R.PREDS:
        for e in (0.0, 0.5):
            g = R.load(R.ddim_file(p, e))
            for case in R.ddim_cases():
                if case[0] == p and case[3] == e:
                    assert g[R.ddim_key(case) + ':prev32'].shape == R.STEP_SHAPE and g[R.ddim_key(case) + ':e_ref32_x0'] >= 0
            # per fixture with sample_max_value > 1: s clamped at 1, strictly between, at the maximum
            for where in R.WHERE:
                t = int(g[R.ddim_key((p, 'thr1.5', where, e, False)) + ':t'])
                s = pkg('diffusion').DDIMScheduler()
                a = s.alphas_cumprod[t]
                x, m, _ = R.scaled_inputs('ddim', p, where, g[R.scale_key('ddim', p, where)])
                for mv in (1.5, 4.0):
                    st = R.abs_quantile(x, m, R.PRED[p], float(a ** 0.5), float((1 - a) ** 0.5), 0.995, mv)[:, 3].numpy()
                    assert (st == 1).any() and ((st > 1) & (st < mv)).any() and (st == np.float32(mv)).any(), (p, where, mv, st)
    ch = R.load(R.CHAINS_FILE)
    assert sorted(c[1] for c in R.CHAINS) == ['ddim', 'ddim', 'ddpm', 'ddpm']
    assert sum(c[2].get('prediction_type') == 'v_prediction' for c in R.CHAINS) == 2
    for name, _, kw, _ in R.CHAINS:
        assert kw['thresholding'] and kw['sample_max_value'] == 2.0
        assert ch[name + ':xs64'].dtype == np.float64 and ch[name + ':xs64'].shape[0] == R.CHAIN_STEPS + 1 == len(ch[name + ':gap'])


def _all_steps():
    import test_threshold_gpu as T
    return T._step_cases()


@pytest.mark.parametrize('group', _all_steps(), ids=lambda g: g[1][:-4])
def test_every_fixture_step_equals_the_references_fp32_bits(group, mocked):
    """Over the stand-ins, from the fixture's inputs: prev_sample and pred_original_sample equal the reference's fp32 result bit
    for bit, every step of every file.  The default path (an epsilon model, no thresholding, no use_clipped_model_output) goes to
    the old op, which the stand-in module only records: its arguments are compared, not its output."""
    import test_threshold_gpu as T
    diffusion = pkg('diffusion')
    sched, fname, cases = group
    g = R.load(fname)
    new = 0
    for case in cases:
        del mocked.calls[:]
        key, prev, x0 = T.run_fixture_step(diffusion, sched, case, g, None)
        default = case[0] == 'epsilon' and not case[1].startswith('thr') and (sched == 'ddpm' or not case[4])
        assert len(mocked.calls) == 1 and (mocked.calls[0][0] == ('%s_step' % sched if default else 'x0_step')), (key, mocked.calls)
        if default:
            assert x0 is None
            continue
        new += 1
        assert np.array_equal(prev.numpy(), g[key + ':prev32']), key
        assert np.array_equal(x0.numpy(), g[key + ':x032']), key
        _, mode, pred, treat, reclip, has_z = mocked.calls[0]
        assert mode == (R.DDPM if sched == 'ddpm' else R.DDIM) and pred == R.PRED[case[0]]
        assert treat == (R.THRESHOLD if case[1].startswith('thr') else R.CLIP if case[1] == 'clip' else R.NONE)
        assert reclip == (sched == 'ddim' and case[4]) and has_z == (int(g[key + ':t']) > 0 if sched == 'ddpm' else case[3] > 0)
    assert new >= len(cases) * 2 // 3


@pytest.mark.parametrize('chain', R.CHAINS, ids=lambda c: c[0])
def test_toy_chains_equal_the_references_fp32_chains(chain, mocked):
    name, which, kw, step_kw = chain
    diffusion = pkg('diffusion')
    g = R.load(R.TOY_FILE)
    s = (diffusion.DDIMScheduler if which == 'ddim' else diffusion.DDPMScheduler)(**kw)
    s.set_timesteps(R.CHAIN_STEPS)
    assert s.timesteps.tolist() == g[name + ':timesteps'].tolist()
    gen = torch.Generator().manual_seed(R.CHAIN_SEED)
    x = diffusion.randn_tensor(R.TOY_SHAPE, generator=gen)
    assert np.array_equal(x.numpy(), g['x_T'])
    extra = dict(step_kw, generator=gen) if which == 'ddpm' else dict(step_kw)
    for k, t in enumerate(s.timesteps.tolist()):
        out = s.step(R.toy_model(x, t), t, x, **extra)
        x = out.prev_sample
        assert out.pred_original_sample is not None and float(out.pred_original_sample.abs().max()) <= 1.0
        assert np.array_equal(x.numpy(), g[name + ':xs32'][k + 1]), (name, k)
    assert len(mocked.calls) == R.CHAIN_STEPS and all(c[0] == 'x0_step' for c in mocked.calls)


# ------------------------------------------------------------------------------------------------ configs, directories, the default path
NEW_KEYS = ('thresholding', 'dynamic_thresholding_ratio', 'sample_max_value')


def test_config_keys_and_from_config_between_the_classes():
    diffusion = pkg('diffusion')
    for cls in (diffusion.DDPMScheduler, diffusion.DDIMScheduler):
        params = [p for p in inspect.signature(cls.__init__).parameters if p != 'self']
        assert set(params) == set(cls._CONFIG_KEYS) == set(vars(cls().config)) and params[-3:] == list(NEW_KEYS)
        s = cls()
        assert s.config.thresholding is False and s.config.dynamic_thresholding_ratio == 0.995 and s.config.sample_max_value == 1.0
        a = cls(thresholding=True, dynamic_thresholding_ratio=0.9, sample_max_value=3.0, prediction_type='v_prediction')
        assert vars(cls.from_config(a.config).config) == vars(a.config)
        assert vars(cls.from_config(dict(vars(a.config), solver_order=3)).config) == vars(a.config)     # foreign keys are dropped
        for other in (diffusion.DDPMScheduler, diffusion.DDIMScheduler):
            b = other.from_config(a.config)
            assert all(getattr(b.config, k) == getattr(a.config, k) for k in NEW_KEYS + ('prediction_type',))
    # the reference's ValueError for anything else
    with pytest.raises(ValueError, match='prediction_type'):
        diffusion.DDIMScheduler(prediction_type='noise')
    s = diffusion.DDPMScheduler(prediction_type='noise')
    with pytest.raises(ValueError, match='prediction_type'):
        s.step(torch.zeros(1, 3, 4, 4), 5, torch.zeros(1, 3, 4, 4))
    # the two multistep solvers keep their refusals, from their constructors, also when a config hands them the keys
    a = diffusion.DDIMScheduler(thresholding=True)
    for solver in (diffusion.DPMSolverMultistepScheduler, diffusion.UniPCMultistepScheduler):
        with pytest.raises(NotImplementedError, match='thresholding'):
            solver.from_config(a.config)
    # what was refused stays refused
    s = diffusion.DDPMScheduler(variance_type='learned_range', prediction_type='sample', thresholding=True)
    s.set_timesteps(10)
    with pytest.raises(NotImplementedError):
        s.step(torch.zeros(1, 6, 4, 4), 900, torch.zeros(1, 3, 4, 4))
    with pytest.raises(NotImplementedError):
        s.step(torch.zeros(1, 3, 4, 4), 900, torch.zeros(1, 3, 4, 4))


def test_ddim_pipeline_keeps_the_keys_when_it_recreates_its_scheduler():
    diffusion = pkg('diffusion')
    unet = pkg('unet').UNet2DModel(**gc.TINY_CFG)
    src = diffusion.DDPMScheduler(thresholding=True, dynamic_thresholding_ratio=0.97, sample_max_value=2.5, prediction_type='sample')
    pipe = diffusion.DDIMPipeline(unet, src)
    assert type(pipe.scheduler) is diffusion.DDIMScheduler
    assert all(getattr(pipe.scheduler.config, k) == getattr(src.config, k) for k in NEW_KEYS + ('prediction_type',))


@pytest.mark.parametrize('which', ['ddim', 'ddpm'])
def test_thresholding_pipeline_directory_round_trip(which, tmp_path):
    diffusion, checkpoint = pkg('diffusion'), pkg('checkpoint')
    unet = pkg('unet').UNet2DModel(**gc.TINY_CFG)
    gc.det_init_(unet, 5)
    kw = dict(thresholding=True, dynamic_thresholding_ratio=0.98, sample_max_value=2.0, prediction_type='v_prediction')
    if which == 'ddim':
        pipe = diffusion.DDIMPipeline(unet, diffusion.DDIMScheduler(**kw))
    else:
        pipe = diffusion.DDPMPipeline(unet, diffusion.DDPMScheduler(**kw))
    d = str(tmp_path / 'pipe')
    pipe.save_pretrained(d)
    with open(os.path.join(d, 'scheduler', 'scheduler_config.json')) as f:
        stored = json.load(f)
    assert stored['thresholding'] is True and stored['dynamic_thresholding_ratio'] == 0.98 and stored['sample_max_value'] == 2.0
    assert {k: v for k, v in stored.items() if not k.startswith('_')} == vars(pipe.scheduler.config)
    back = type(pipe).from_pretrained(d)
    assert type(back.scheduler) is type(pipe.scheduler) and vars(back.scheduler.config) == vars(pipe.scheduler.config)
    alone = type(pipe.scheduler).from_pretrained(d, subfolder='scheduler')
    assert vars(alone.config) == vars(pipe.scheduler.config)
    # the solver classes still raise, from their constructors; trained_betas stays refused by the loader
    with pytest.raises(NotImplementedError, match='prediction_type'):
        diffusion.UniPCMultistepScheduler.from_pretrained(d, subfolder='scheduler')
    stored['prediction_type'] = 'epsilon'
    with open(os.path.join(d, 'scheduler', 'scheduler_config.json'), 'w') as f:
        json.dump(stored, f)
    with pytest.raises(NotImplementedError, match='thresholding'):
        diffusion.UniPCMultistepScheduler.from_pretrained(d, subfolder='scheduler')
    with pytest.raises(NotImplementedError, match='thresholding'):
        diffusion.DPMSolverMultistepScheduler.from_pretrained(d, subfolder='scheduler')
    stored['trained_betas'] = [0.1, 0.2]
    with open(os.path.join(d, 'scheduler', 'scheduler_config.json'), 'w') as f:
        json.dump(stored, f)
    with pytest.raises(NotImplementedError, match='trained_betas'):
        type(pipe.scheduler).from_pretrained(d, subfolder='scheduler')
    # the reference's own configs under tests/golden hold the three keys and load
    for name in sorted(os.listdir(os.path.join(HERE, 'golden'))):
        p = os.path.join(HERE, 'golden', name, 'scheduler', 'scheduler_config.json')
        if os.path.exists(p):
            with open(p) as f:
                cfg = json.load(f)
            assert all(k in cfg for k in NEW_KEYS), name
            cls = getattr(diffusion, cfg['_class_name'])
            assert cls.from_pretrained(os.path.join(HERE, 'golden', name), subfolder='scheduler').config.thresholding is False
    del checkpoint


def test_default_path_still_calls_the_old_ops_with_todays_arguments(mocked):
    diffusion = pkg('diffusion')
    x, e, z = (torch.from_numpy(gc.det_noise((2, 3, 4, 4), s)) for s in (1, 2, 3))
    s = diffusion.DDIMScheduler()
    s.set_timesteps(10)
    out = s.step(e, 444, x, eta=0.5, variance_noise=z)
    assert out.pred_original_sample is None and len(mocked.calls) == 1
    name, kw = mocked.calls[0]
    a_t, a_prev = s.alphas_cumprod[444], s.alphas_cumprod[344]
    assert name == 'ddim_step' and kw['a_t'] == float(a_t) and kw['a_prev'] == float(a_prev) and kw['vnoise'] is z
    assert kw['std'] == float(0.5 * s._get_variance(444, 344) ** 0.5) and kw['clip'] is True and kw['clip_range'] == 1.0 and kw['out'] is None
    del mocked.calls[:]
    s.step(e, 444, x)
    assert mocked.calls[0][1]['std'] == 0.0 and mocked.calls[0][1]['vnoise'] is None
    d = diffusion.DDPMScheduler()
    d.set_timesteps(10)
    del mocked.calls[:]
    out = d.step(e, 500, x, variance_noise=z)
    assert out.pred_original_sample is None and len(mocked.calls) == 1
    name, kw = mocked.calls[0]
    a_t, a_prev = d.alphas_cumprod[500], d.alphas_cumprod[400]
    assert name == 'ddpm_step' and kw['sqrt_a_t'] == float(a_t ** 0.5) and kw['sqrt_b_t'] == float((1 - a_t) ** 0.5)
    assert kw['c_x0'] == float((a_prev ** 0.5 * (1 - a_t / a_prev)) / (1 - a_t)) and kw['vnoise'] is z and kw['clip'] is True
    assert kw['sigma'] == float(d._get_variance(500) ** 0.5) and kw['clip_range'] == 1.0
    # ... and each of the three options leaves it
    for sched, kw in ((diffusion.DDIMScheduler(thresholding=True), {}), (diffusion.DDIMScheduler(prediction_type='sample'), {}),
                      (diffusion.DDIMScheduler(), dict(use_clipped_model_output=True)), (diffusion.DDPMScheduler(thresholding=True), {}),
                      (diffusion.DDPMScheduler(prediction_type='v_prediction'), {})):
        sched.set_timesteps(10)
        del mocked.calls[:]
        out = sched.step(e, 500 if isinstance(sched, diffusion.DDPMScheduler) else 444, x, **kw)
        assert [c[0] for c in mocked.calls] == ['x0_step'] and out.pred_original_sample is not None
    # the scheduler's own _threshold_sample for a caller's tensor
    got = diffusion.DDPMScheduler(thresholding=True, sample_max_value=2.0)._threshold_sample(x * 3)
    B = x.shape[0]
    sq = torch.clamp(torch.quantile((x * 3).reshape(B, -1).abs(), 0.995, dim=1), min=1, max=2.0).reshape(B, 1, 1, 1)
    assert torch.equal(got, torch.clamp(x * 3, -sq, sq) / sq)


# ------------------------------------------------------------------------------------------------ the launch-site table
def test_every_launch_site_of_threshold_hip_is_in_its_branch_table():
    """csrc/threshold.hip launches through TH_LAUNCH, a macro of its own with the body of the library's launch macro, and its sites
    are tabled in tests/test_threshold_gpu.py: a new site changes the count, a new kernel is in no table, an entry without a case
    fails -- before a GPU is needed.  The file is in both build lists, and its entry points are declared and bound."""
    import test_threshold_gpu as T
    import mock_ops_threshold as mock
    L, ops = pkg('_lib'), pkg('ops')
    csrc = os.path.join(ROOT, 'diff-pruning_amd', 'csrc')
    assert list(T.LAUNCH_SITES) == ['threshold.hip']
    src = open(os.path.join(csrc, 'threshold.hip')).read()
    body = src.replace('#define TH_LAUNCH(', '')
    sites = re.findall(r'\bTH_LAUNCH\((\(th_lds_kernel<(?:true|false)>\)|th_[a-z]+_kernel),', body)
    assert len(sites) == T.LAUNCH_SITES['threshold.hip'] == body.count('TH_LAUNCH(') == 8, sites
    assert 'DP_' + 'LAUNCH(' not in src
    assert re.search(r'#define TH_LAUNCH\(k, \.\.\.\).*dp_launch_names\[dp_launches\+\+ & \(DP_LAUNCH_RING - 1\)\] = #k;.*'
                     r'hipLaunchKernelGGL\(k, __VA_ARGS__\)', src)
    assert sorted(sites) == sorted(T.BRANCHES) and len(set(T.BRANCHES)) == len(T.BRANCHES)
    assert all(e in T.CASES and hasattr(T, T.CASES[e]) for e in T.BRANCHES)
    assert set(T.MULTI) | {T.LDS_QUANTILE, T.LDS_FUSED, T.STEP} == set(T.BRANCHES)
    using = {f for f in os.listdir(csrc) if 'TH_LAUNCH(' in open(os.path.join(csrc, f)).read()}
    assert using == {'threshold.hip'}
    assert 'csrc/threshold.hip' in open(os.path.join(ROOT, 'build.sh')).read()
    assert "'csrc/threshold.hip'" in open(os.path.join(ROOT, '__graft_entry__.py')).read()
    # every arithmetic function is rounded operation by operation; the one contraction is the explicit fmaf
    assert 'asm' not in src and src.count('#pragma clang fp contract(off)') == 3 and len(re.findall(r'\bfmaf\(', src)) == 2
    assert 'buffer_load' not in src and '__builtin_amdgcn_raw_buffer' not in src and '__builtin_amdgcn_rcp' not in src
    hdr = open(os.path.join(ROOT, 'include', 'dp_hip.h')).read()
    for name, nargs in (('dp_x0_abs_quantile_workspace', 2), ('dp_x0_abs_quantile', 15), ('dp_x0_step', 14), ('dp_x0_threshold_step', 17)):
        assert len(L.SIGNATURES[name]) == nargs
        decl = re.search(r'\b%s\(([^;]*)\);' % name, hdr).group(1)
        assert decl.count(',') + 1 == nargs, name
        assert getattr(L.load(), name) is not None
    fields = re.search(r'typedef struct dp_x0_coef \{(.*?)\} dp_x0_coef;', hdr, re.S).group(1)
    names = [n for line in re.sub(r'/\*.*?\*/', '', fields).split(';') for n in re.findall(r'\b(?!float\b)([A-Za-z_0-9]+)\b', line)]
    assert tuple(names) == tuple(n for n, _ in L.X0Coef._fields_) == ops.X0_COEF == mock.X0_COEF and ctypes.sizeof(L.X0Coef) == 24
    consts = {k: int(v) for k, v in re.findall(r'#define (DP_(?:X0|THRESHOLD)_[A-Z0-9_]+) (\d+)', hdr)}
    assert consts['DP_THRESHOLD_LDS_MAX'] == ops.THRESHOLD_LDS_MAX == mock.THRESHOLD_LDS_MAX == T.LDS_MAX
    assert consts['DP_X0_STEP_MAX_BLOCKS'] == ops.X0_STEP_MAX_BLOCKS == mock.X0_STEP_MAX_BLOCKS == T.MAX_BLOCKS
    for mod in (ops, mock):
        assert (mod.X0_PRED_EPSILON, mod.X0_PRED_SAMPLE, mod.X0_PRED_V) == tuple(consts['DP_X0_PRED_' + k] for k in ('EPSILON', 'SAMPLE', 'V'))
        assert (mod.X0_TREAT_NONE, mod.X0_TREAT_CLIP, mod.X0_TREAT_THRESHOLD) == tuple(consts['DP_X0_TREAT_' + k] for k in ('NONE', 'CLIP', 'THRESHOLD'))
        assert (mod.X0_MODE_DDIM, mod.X0_MODE_DDPM, mod.X0_MODE_CONVERT) == tuple(consts['DP_X0_MODE_' + k] for k in ('DDIM', 'DDPM', 'CONVERT'))
        assert (mod.X0_ROUTE_LDS, mod.X0_ROUTE_MULTI) == (consts['DP_X0_ROUTE_LDS'], consts['DP_X0_ROUTE_MULTI'])
        assert mod.X0_PRED == {'epsilon': 0, 'sample': 1, 'v_prediction': 2}
    assert L.load().dp_x0_abs_quantile_workspace(3, 100) == 3 * 264 * 4
