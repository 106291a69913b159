"""The sigma-space schedulers on the host (`-m "not gpu"`): diffusion.EulerDiscreteScheduler, EulerAncestralDiscreteScheduler and
HeunDiscreteScheduler over the CPU stand-in of their three kernels (tests/mock_ops_sigma.py, the kernels' operation order in fp32
torch) against the fixtures that tests/golden/make_golden_sigma.py recorded from the reference's own schedulers: the timestep and
sigma tables bit for bit, every stored step and the toy-model chains bit for bit against the reference's fp32 run with every host
scalar equal to the reference's; the refusals; configs across classes; the pipeline directory round trip; LDMPipeline against the
explicit loop; and the launch-site table of csrc/sigma.hip."""
import ctypes
import json
import os
import re
import warnings
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import golden_common as gc
import sigma_ref as R
from helpers import pkg

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture()
def mocked(monkeypatch):
    import mock_ops_sigma as mock
    monkeypatch.setattr(pkg('diffusion'), 'ops', mock)
    del mock.calls[:]
    return mock


@pytest.fixture(scope='module')
def tables():
    return R.load(R.TABLES_FILE)


@pytest.fixture(scope='module')
def steps():
    return R.load(R.STEPS_FILE)


def _sched(cls, **kw):
    return getattr(pkg('diffusion'), R.CLASSES[cls])(**kw)


def _extra(cls, skw, seed):
    return dict(skw, generator=torch.Generator().manual_seed(seed)) if cls != 'heun' else {}


# ------------------------------------------------------------------------------------------------ the fixture and the launch-site table
def test_fixture_covers_what_it_must(tables, steps):
    """From the stored numbers: every table case; every setting at n = 10 (integer timesteps) and n = 7 (fractional ones); the stored
    calls reaching every instantiation of dp_sigma_step, with and without churn, first and last calls, both states of Heun; five
    chains; every file under 1 MiB."""
    assert {c[3] for c in R.TABLE_CASES} == {1, 2, 3, 5, 7, 10, 50, 1000} and len(R.TABLE_CASES) == 144
    assert {c[:3] for c in R.TABLE_CASES} == {(c, s, v) for c in R.CLASSES for s in R.SCHEDULES for v in R.VARIANTS[c]}
    for case in R.TABLE_CASES:
        name = R.table_name(case)
        ts, sig = tables[name + ':timesteps'], tables[name + ':sigmas']
        assert ts.dtype == np.float64 and sig.dtype == np.float32 and (len(ts), len(sig)) == R.table_lengths(case)
        assert np.isfinite(ts).all() and np.isfinite(sig).all()
    frac = lambda case: int((tables[R.table_name(case) + ':timesteps'] % 1 != 0).sum())               # noqa: E731
    assert frac(('euler', 'linear', 'plain', 50)) == 48 and frac(('euler', 'linear', 'karras', 10)) == 8
    assert frac(('euler', 'linear', 'plain', 10)) == 0 and frac(('euler', 'linear', 'plain', 7)) == 3
    seen, churned, states = set(), set(), set()
    for run in R.STEP_RUNS:
        sname, cls, kw, skw, n, at = run
        name = R.run_name(run)
        assert n in (10, 7) and len(steps[name + ':timesteps']) == R.n_calls(cls, n) and 0 in at and R.n_calls(cls, n) - 1 in at
        for k in at:
            key = '%s@%d' % (name, k)
            seen.add((R.mode_of_call(cls, k), R.PRED_OF[kw.get('prediction_type', 'epsilon')]))
            assert steps[key + ':prev64'].dtype == np.float64 and steps[key + ':prev32'].dtype == np.float32
            assert steps[key + ':prev32'].shape == R.STEP_SHAPE and steps[key + ':coefs'].shape == (len(R.COEF_NAMES),)
            assert float(steps[key + ':e_ref32']) == float(np.abs(steps[key + ':prev32'].astype(np.float64) - steps[key + ':prev64']).max())
            assert (key + ':x0_32' in steps) == (cls != 'heun')
            if int(steps[name + ':churn'][k]):
                churned.add(sname)
            if cls == 'heun':
                states.add(k % 2)
    assert seen == set(R.INSTANCES) == R.stored_coverage() and len(seen) == 9
    assert churned == {'euler_churn', 'euler_v_churn'} and states == {0, 1}
    # ... and the churn runs hold calls without churn too (sigma outside [s_tmin, s_tmax])
    assert any(not int(steps['run:euler_churn:10:churn'][k]) for k in R.stored_calls('euler', 10))
    assert [c[0] for c in R.CHAINS] == ['euler7', 'euler_karras10', 'euler_v7', 'ancestral7', 'heun5']
    chains, toy = R.load(R.CHAINS_FILE), R.load(R.TOY_FILE)
    for name, cls, kw, n, with_gen in R.CHAINS:
        calls = R.n_calls(cls, n)
        assert chains[name + ':xs64'].dtype == np.float64 and chains[name + ':xs64'].shape[0] == calls + 1 == len(chains[name + ':gap'])
        assert toy[name + ':xs32'].dtype == np.float32 and toy[name + ':xs32'].shape == (calls + 1,) + R.TOY_SHAPE
        assert (name + ':gen_state' in toy) == with_gen
    # what the fixture writer's table patch (sqrt / log / exp rounded once from fp64) moved against the reference without it, on the
    # host that wrote the fixtures: last bits only
    total, differing, worst_ulp = (int(v) for v in tables['unpatched:sigmas'])
    assert total == sum(R.table_lengths(c)[1] for c in R.TABLE_CASES) and 0 <= differing <= total // 100 and worst_ulp <= 1
    assert float(tables['unpatched:timesteps_worst']) <= 1e-3
    for f in (R.TABLES_FILE, R.STEPS_FILE, R.CHAINS_FILE, R.TOY_FILE):
        assert os.path.getsize(os.path.join(HERE, 'golden', f)) <= 1 << 20


def test_every_launch_site_of_sigma_hip_is_in_its_branch_table():
    """csrc/sigma.hip launches through SG_LAUNCH, a macro of its own with the body of the library's launch macro, and its sites are
    tabled in tests/test_sigma_gpu.py: a new site changes the count, a new instantiation is in no table, an entry without a case
    fails -- before a GPU is needed.  The file is in both build lists and declared with its bindings."""
    import test_sigma_gpu as T
    import mock_ops_sigma as mock
    L, ops = pkg('_lib'), pkg('ops')
    csrc = os.path.join(ROOT, 'diff-pruning_amd', 'csrc')
    assert list(T.LAUNCH_SITES) == ['sigma.hip']
    src = open(os.path.join(csrc, 'sigma.hip')).read()
    body = src.replace('#define SG_LAUNCH(', '')
    sites = re.findall(r'\bSG_LAUNCH\((\(sigma_step_kernel<DP_SIGMA_[A-Z0-9]+, DP_SIGMA_[A-Z]+>\)|sigma_scale_kernel|sigma_add_noise_kernel)', body)
    assert len(sites) == T.LAUNCH_SITES['sigma.hip'] == body.count('SG_LAUNCH(') == 11, sites
    assert 'DP_' + 'LAUNCH(' not in src
    assert re.search(r'#define SG_LAUNCH\(k, \.\.\.\).*dp_launch_names\[dp_launches\+\+ & \(DP_LAUNCH_RING - 1\)\] = #k;.*'
                     r'hipLaunchKernelGGL\(k, __VA_ARGS__\)', src)
    assert '#pragma clang fp contract(off)' in src and 'fma' not in src.replace('v_fma_f32', '') and '__fdividef' not in src
    assert 'atomic' not in src and 'asm' not in src
    assert sorted(sites) == sorted(T.BRANCHES) and len(set(T.BRANCHES)) == len(T.BRANCHES)
    assert all(e in T.CASES for e in T.BRANCHES), sorted(set(T.BRANCHES) - set(T.CASES))
    assert sorted(v for v in T.CASES.values() if v is not None) == sorted(R.INSTANCES) == sorted(ops.SIGMA_INSTANCES) == sorted(mock.SIGMA_INSTANCES)
    using = {f for f in os.listdir(csrc) if 'SG_LAUNCH(' in open(os.path.join(csrc, f)).read()}
    assert using == {'sigma.hip'}
    assert 'csrc/sigma.hip' in open(os.path.join(ROOT, 'build.sh')).read()
    assert "'csrc/sigma.hip'" in open(os.path.join(ROOT, '__graft_entry__.py')).read()
    hdr = open(os.path.join(ROOT, 'include', 'dp_hip.h')).read()
    assert len(L.SIGNATURES['dp_sigma_step']) == 12 and len(L.SIGNATURES['dp_sigma_scale']) == 5 and len(L.SIGNATURES['dp_sigma_add_noise']) == 7
    assert ('int dp_sigma_step(const float* x, const float* e, const float* z, const float* d1, const float* xs, int mode, int pred,\n'
            '                  const dp_sigma_coef* coef, float* x_next, float* aux_out, long long n, void* stream);') in hdr
    assert 'int dp_sigma_scale(const float* x, float c, float* out, long long n, void* stream);' in hdr
    assert 'int dp_sigma_add_noise(const float* x0, const float* z, const float* sigma, long long B, long long per, float* out, void* stream);' in hdr
    # the struct of scalars: the header's field order is the binding's, the wrapper's, the stand-in's and the fixture's
    fields = re.search(r'typedef struct dp_sigma_coef \{(.*?)\} dp_sigma_coef;', hdr, re.S).group(1)
    names = [n for line in re.sub(r'/\*.*?\*/', '', fields, flags=re.S).split(';') for n in re.findall(r'\b(?!float\b)([a-z_0-9]+)\b', line)]
    assert tuple(names) == tuple(n for n, _ in L.SigmaCoef._fields_) == ops.SIGMA_COEF == mock.SIGMA_COEF == R.COEF_NAMES
    assert ctypes.sizeof(L.SigmaCoef) == 4 * len(names) == 28
    for i, m in enumerate(R.MODES):
        assert int(re.search(r'#define DP_SIGMA_%s (\d+)' % m, hdr).group(1)) == getattr(ops, 'SIGMA_' + m) == getattr(mock, 'SIGMA_' + m) == i
    for i, m in enumerate(R.PREDS):
        assert int(re.search(r'#define DP_SIGMA_%s (\d+)' % m, hdr).group(1)) == getattr(ops, 'SIGMA_' + m) == getattr(mock, 'SIGMA_' + m) == i
    m = re.search(r'#define DP_SIGMA_MAX_BLOCKS (\d+)', hdr)
    assert int(m.group(1)) == ops.SIGMA_MAX_BLOCKS == T.MAX_BLOCKS
    lib = L.load()
    assert all(getattr(lib, n) is not None for n in ('dp_sigma_step', 'dp_sigma_scale', 'dp_sigma_add_noise'))


# ------------------------------------------------------------------------------------------------ tables
@pytest.mark.parametrize('case', R.TABLE_CASES, ids=R.table_name)
def test_tables_equal_the_references_bit_for_bit(case, tables):
    s = _sched(case[0], **R.table_kwargs(case))
    s.set_timesteps(case[3])
    name = R.table_name(case)
    assert s.timesteps.dtype == torch.float64 and s.sigmas.dtype == torch.float32
    assert s.timesteps.numpy().tobytes() == tables[name + ':timesteps'].tobytes()
    assert s.sigmas.numpy().tobytes() == tables[name + ':sigmas'].tobytes()
    assert np.float32(float(s.init_noise_sigma)).tobytes() == tables[name + ':init_noise_sigma'].tobytes()
    # the host's copies: what `step` and `scale_model_input` look up
    assert s._ts == tables[name + ':timesteps'].tolist() and all(type(t) is float for t in s._ts)
    assert s._sig.device.type == 'cpu' and torch.equal(s._sig, s.sigmas) and s.num_inference_steps == case[3]


def test_the_quirks_of_the_tables():
    e = _sched('euler', interpolation_type='log_linear')
    e.set_timesteps(5)
    assert len(e._ts) == 5 and len(e._sig) == 7                                    # n + 2 sigmas for n timesteps
    top = float(e.init_noise_sigma)
    e.set_timesteps(3)
    assert float(e.init_noise_sigma) == top == float(e._train_sigmas().max())      # the Euler classes: from the constructor, not updated
    h = _sched('heun')
    assert h.order == 2 and len(h._ts) == 1999 and len(h._sig) == 2000             # the constructor's table: every training timestep
    h.set_timesteps(1)
    assert h._ts == [0.0] and len(h._sig) == 2 and float(h._sig[1]) == 0.0
    assert float(h.init_noise_sigma) == float(h._sig[0])                            # Heun: follows set_timesteps
    h.set_timesteps(4)
    assert len(h._ts) == 7 and len(h._sig) == 8 and h._ts[1] == h._ts[2] and h._ts[0] == 999.0
    assert h.state_in_first_order and h.prev_derivative is None and h.sample is None
    assert vars(h.config)['beta_start'] == 0.00085 and vars(h.config)['beta_end'] == 0.012
    for cls in R.CLASSES:
        s = _sched(cls)
        assert s.sigma_space is True and len(s) == 1000 and s.order == (2 if cls == 'heun' else 1)
    with pytest.raises(ValueError, match='log_linear'):
        _sched('euler', interpolation_type='cubic').set_timesteps(5)


# ------------------------------------------------------------------------------------------------ single steps, chains: bit for bit
def _coef_names(cls, kw, churn):
    names = {'sig', 'dt'} | ({'c_out', 'c_den'} if kw.get('prediction_type') == 'v_prediction' else set())
    return names | ({'k', 's_noise'} if churn else set()) | ({'sigma_up'} if cls == 'ancestral' else set())


@pytest.mark.parametrize('run', R.STEP_RUNS, ids=R.run_name)
def test_single_steps_equal_the_references_fp32_bits(run, steps, mocked):
    sname, cls, kw, skw, n, at = run
    name = R.run_name(run)
    s = _sched(cls, **kw)
    s.set_timesteps(n)
    assert s._ts == steps[name + ':timesteps'].tolist()
    s.is_scale_input_called = True
    extra = _extra(cls, skw, R.GEN_SEED)
    for k in range(len(s._ts)):
        x, e = R.step_inputs(k)
        x0, e0 = x.clone(), e.clone()
        before = len(mocked.calls)
        out = s.step(e, s._ts[k], x, **extra)
        assert len(mocked.calls) == before + 1                                   # one kernel call per step
        op, mode, pred, churn, coef = mocked.calls[-1]
        assert (op, mode, pred) == ('step', R.mode_of_call(cls, k), R.PRED_OF[kw.get('prediction_type', 'epsilon')])
        assert churn == bool(steps[name + ':churn'][k]) and set(coef) == _coef_names(cls, kw, churn)
        assert torch.equal(x, x0) and torch.equal(e, e0)                         # a step writes none of its inputs
        assert out.prev_sample.dtype == torch.float32 and type(out).__name__ == (
            'SchedulerOutput' if cls == 'heun' else R.CLASSES[cls] + 'Output')
        if k in at:
            key = '%s@%d' % (name, k)
            stored = steps[key + ':coefs']
            differing = [c for c in coef if np.float32(coef[c]).tobytes() != stored[R.COEF_NAMES.index(c)].tobytes()]
            assert differing == [], (key, differing)                             # every host scalar as the reference formed it
            assert np.array_equal(out.prev_sample.numpy(), steps[key + ':prev32']), key
            if cls != 'heun':
                assert np.array_equal(out.pred_original_sample.numpy(), steps[key + ':x0_32']), key
    assert cls != 'heun' or not s.state_in_first_order                           # the last Heun call is a first-order one


def _chain(s, cls, model, x_T, n, with_gen):
    x = x_T * s.init_noise_sigma
    s.set_timesteps(n)
    gen = torch.Generator().manual_seed(R.NOISE_SEED) if with_gen else None
    extra = dict(generator=gen) if cls != 'heun' else {}
    xs = [x]
    for t in s._ts:
        xs.append(s.step(model(s.scale_model_input(xs[-1], t), t), t, xs[-1], **extra).prev_sample.clone())
    return xs, gen


@pytest.mark.parametrize('chain', R.CHAINS, ids=lambda c: c[0])
def test_toy_chains_equal_the_references_fp32_bits(chain, mocked):
    name, cls, kw, n, with_gen = chain
    g = R.load(R.TOY_FILE)
    s = _sched(cls, **kw)
    xs, gen = _chain(s, cls, R.toy_model, torch.from_numpy(g['x_T']), n, with_gen)
    assert s._ts == g[name + ':timesteps'].tolist()
    want = g[name + ':xs32']
    for k, x in enumerate(xs):
        assert np.array_equal(x.numpy(), want[k]), (name, k)
    assert [c[0] for c in mocked.calls] == ['scale', 'step'] * R.n_calls(cls, n) and s.is_scale_input_called
    if with_gen:                                                                 # the generator's stream advanced as the reference's did
        assert np.array_equal(gen.get_state().numpy(), g[name + ':gen_state'])


def test_the_toy_x_T_is_the_pipelines_draw():
    g = R.load(R.TOY_FILE)
    x = pkg('diffusion').randn_tensor(R.TOY_SHAPE, generator=torch.Generator().manual_seed(R.CHAIN_SEED))
    assert np.array_equal(x.numpy(), g['x_T'])


def test_euler_draws_on_every_step_and_ancestral_after_the_update(mocked):
    """A generator's stream: Euler without churn draws (and does not use) one tensor per step; the two streams stay equal."""
    x, e = R.step_inputs(0)
    for cls in ('euler', 'ancestral'):
        s = _sched(cls)
        s.set_timesteps(7)
        gen, twin = torch.Generator().manual_seed(3), torch.Generator().manual_seed(3)
        for t in s._ts[:3]:
            s.step(e, t, x, generator=gen)
            torch.randn(R.STEP_SHAPE, generator=twin)
            assert torch.equal(gen.get_state(), twin.get_state())


def test_scale_model_input_and_noise_sigmas_equal_the_references(steps, mocked):
    x, z = (torch.from_numpy(gc.det_noise(R.STEP_SHAPE, 900 + i)) for i in range(2))
    for i, (cls, kw, idx) in enumerate(R.SCALE_CASES):
        s = _sched(cls, **kw)
        s.set_timesteps(7)
        xin = x * R.X_SCALE
        keep = xin.clone()
        y = s.scale_model_input(xin, s._ts[idx])
        assert np.array_equal(y.numpy(), steps['scale:%d:out' % i]) and torch.equal(xin, keep) and y.data_ptr() != xin.data_ptr()
        assert s.scale_model_input(xin, torch.tensor(s._ts[idx], dtype=torch.float64)).data_ptr() == y.data_ptr()      # a buffer of its own
    for i, (cls, kw, idx) in enumerate(R.NOISE_CASES):
        s = _sched(cls, **kw)
        s.set_timesteps(10)
        sig = s.noise_sigmas(s.timesteps[idx])
        assert sig.dtype == torch.float32 and np.array_equal(sig.numpy(), steps['noise:%d:sigmas' % i])
        assert np.array_equal(mocked.sigma_add_noise(x, z, sig).numpy(), steps['noise:%d:out' % i])
        with pytest.raises(RuntimeError):                                        # host tensors: no fall-back
            s.add_noise(x, z, s.timesteps[idx])


# ------------------------------------------------------------------------------------------------ Heun's state
def test_heun_keeps_its_state_as_the_reference_does(mocked):
    s = _sched('heun')
    s.set_timesteps(4)
    x0, e0 = R.step_inputs(0)
    x1, e1 = R.step_inputs(1)
    assert s.index_for_timestep(s._ts[1]) == 2                                   # first-order state: the last match
    a = s.step(e0, s._ts[0], x0).prev_sample
    assert not s.state_in_first_order and s.sample is x0 and s.prev_derivative is not None      # held by reference, not copied
    assert isinstance(s.dt, torch.Tensor) and s.dt.dim() == 0 and float(s.dt) == float(s._sig[1] - s._sig[0])
    assert s.index_for_timestep(s._ts[1]) == 1                                   # second-order state: the first match
    d1 = s.prev_derivative.clone()
    b = s.step(e1, s._ts[1], a).prev_sample
    assert s.state_in_first_order and s.sample is None and s.prev_derivative is None and s.dt is None
    want, none = mocked.sigma_step(a, e1, dict(sig=float(s._sig[1]), dt=float(s._sig[1] - s._sig[0])), mocked.SIGMA_HEUN2, d1=d1, saved=x0)
    assert none is None and torch.equal(b, want)
    assert len({a.data_ptr(), b.data_ptr(), x0.data_ptr()}) == 3                 # the saved sample and the stage-1 result are not written
    assert [c[1] for c in mocked.calls[:2]] == [mocked.SIGMA_HEUN1, mocked.SIGMA_HEUN2]


def test_outputs_alternate_between_buffers_of_the_schedulers_own(mocked):
    for cls in R.CLASSES:
        s = _sched(cls)
        s.set_timesteps(5)
        s.is_scale_input_called = True
        x, e = R.step_inputs(0)
        ptrs = []
        for t in s._ts[:4]:
            keep = x.clone()
            y = s.step(e, t, x, **_extra(cls, {}, 1)).prev_sample
            assert torch.equal(x, keep) and y.data_ptr() != x.data_ptr()         # the returned prev_sample stays valid as the next input
            ptrs.append(y.data_ptr())
            x = y
        assert len(set(ptrs)) == s.order + 1
        r = s.step(e, s._ts[4], x, return_dict=False, **_extra(cls, {}, 1)) if cls != 'heun' else s.step(e, s._ts[4], x, return_dict=False)
        assert isinstance(r, tuple) and len(r) == 1


# ------------------------------------------------------------------------------------------------ refusals, configs, directories
def test_refusals_raise_and_call_no_op(mocked):
    z = torch.zeros(1, 3, 4, 4)
    for cls in R.CLASSES:
        with pytest.raises(NotImplementedError):
            _sched(cls, trained_betas=[0.1, 0.2])
        with pytest.raises(NotImplementedError):
            _sched(cls, beta_schedule='sigmoid')
        s = _sched(cls)
        s.set_timesteps(7)
        with pytest.raises(ValueError, match='not one of'):                      # 500.0 is not in the table of n = 7
            s.step(z, 500.0, z)
        with pytest.raises(ValueError):
            s.scale_model_input(z, 500.0)
        with pytest.raises(NotImplementedError):                                 # a model that predicts a variance too
            s.step(torch.zeros(1, 6, 4, 4), s._ts[0], z)
        if cls != 'heun':
            for t in (999, torch.tensor(999), torch.tensor(999, dtype=torch.int32), torch.tensor([999])):
                with pytest.raises(ValueError, match='Passing integer indices'):
                    s.step(z, t, z)
        bad = _sched(cls, prediction_type='nonsense')
        bad.set_timesteps(7)
        with pytest.raises(ValueError, match='prediction_type'):
            bad.step(z, bad._ts[0], z)
    for cls in ('ancestral', 'heun'):
        s = _sched(cls, prediction_type='sample')                                # the reference raises in `step`, not before
        s.set_timesteps(7)
        with pytest.raises(NotImplementedError, match='prediction_type not implemented yet: sample'):
            s.step(z, s._ts[0], z)
    assert mocked.calls == []
    h = _sched('heun')                                                           # Heun takes an int, as the reference does
    h.set_timesteps(10)
    h.step(z, 999, z)
    e = _sched('euler', prediction_type='original_sample')
    e.set_timesteps(10)
    e.is_scale_input_called = True
    e.step(z, 999.0, z)
    assert [c[:3] for c in mocked.calls] == [('step', mocked.SIGMA_HEUN1, 0), ('step', mocked.SIGMA_EULER, 2)]


def test_step_without_scale_model_input_warns_once(mocked):
    z = torch.zeros(1, 3, 4, 4)
    for cls, warns in (('euler', True), ('ancestral', True), ('heun', False)):
        s = _sched(cls)
        s.set_timesteps(10)
        assert s.is_scale_input_called is False
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter('always')
            s.step(z, s._ts[0], z)
            s.step(z, s._ts[1], z)
        assert len([m for m in w if 'scale_model_input' in str(m.message)]) == (1 if warns else 0)
        s2 = _sched(cls)
        s2.set_timesteps(10)
        s2.scale_model_input(z, s2._ts[0])
        assert s2.is_scale_input_called is True
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter('always')
            s2.step(z, s2._ts[0], z)
        assert not w


def test_config_keys_and_from_config_across_classes():
    import inspect
    diffusion = pkg('diffusion')
    keys = dict(euler=('num_train_timesteps', 'beta_start', 'beta_end', 'beta_schedule', 'trained_betas', 'prediction_type',
                       'interpolation_type', 'use_karras_sigmas'),
                ancestral=('num_train_timesteps', 'beta_start', 'beta_end', 'beta_schedule', 'trained_betas', 'prediction_type'),
                heun=('num_train_timesteps', 'beta_start', 'beta_end', 'beta_schedule', 'trained_betas', 'prediction_type', 'use_karras_sigmas'))
    for cls, want in keys.items():
        c = getattr(diffusion, R.CLASSES[cls])
        params = [p for p in inspect.signature(c.__init__).parameters if p != 'self']
        assert tuple(params) == c._CONFIG_KEYS == tuple(vars(c().config)) == want
        a = c(beta_schedule='scaled_linear', prediction_type='v_prediction')
        assert vars(c.from_config(a.config).config) == vars(a.config)
        assert vars(c.from_config(dict(vars(a.config), skip_type='quad')).config) == vars(a.config)      # foreign keys are dropped
        # from another scheduler's config, as a script that swaps the sampler does, and back
        b = c.from_config(diffusion.DDPMScheduler(beta_schedule='scaled_linear', beta_start=0.0015, beta_end=0.0195).config)
        assert (b.config.beta_schedule, b.config.beta_start, b.config.beta_end) == ('scaled_linear', 0.0015, 0.0195)
        for other in (diffusion.DDIMScheduler, diffusion.DPMSolverMultistepScheduler, diffusion.PNDMScheduler, diffusion.EulerDiscreteScheduler):
            assert other.from_config(b.config).config.beta_end == 0.0195
    assert vars(diffusion.HeunDiscreteScheduler().config)['beta_start'] == 0.00085
    e = diffusion.EulerDiscreteScheduler.from_config(diffusion.HeunDiscreteScheduler(use_karras_sigmas=True).config)
    assert e.config.use_karras_sigmas is True and e.use_karras_sigmas is True and e.config.interpolation_type == 'linear'
    step = inspect.signature(diffusion.EulerDiscreteScheduler.step).parameters
    assert list(step) == ['self', 'model_output', 'timestep', 'sample', 's_churn', 's_tmin', 's_tmax', 's_noise', 'generator', 'return_dict']
    assert (step['s_churn'].default, step['s_tmin'].default, step['s_tmax'].default, step['s_noise'].default) == (0.0, 0.0, float('inf'), 1.0)
    assert list(inspect.signature(diffusion.EulerAncestralDiscreteScheduler.step).parameters) == [
        'self', 'model_output', 'timestep', 'sample', 'generator', 'return_dict']
    assert list(inspect.signature(diffusion.HeunDiscreteScheduler.step).parameters) == ['self', 'model_output', 'timestep', 'sample', 'return_dict']


@pytest.mark.parametrize('cls', list(R.CLASSES))
def test_a_directory_that_names_the_class_loads_and_saves_identically(cls, tmp_path):
    """What the issue reports: model_index.json naming one of the three classes ended in NotImplementedError('scheduler class ...')."""
    diffusion = pkg('diffusion')
    unet = pkg('unet').UNet2DModel(**gc.TINY_CFG)
    d = str(tmp_path / 'pipe')
    diffusion.DDPMPipeline(unet, diffusion.DDPMScheduler()).save_pretrained(d)
    index = json.load(open(os.path.join(d, 'model_index.json')))
    index['scheduler'] = ['diffusers', R.CLASSES[cls]]
    json.dump(index, open(os.path.join(d, 'model_index.json'), 'w'))
    cfg = dict(_class_name=R.CLASSES[cls], _diffusers_version='0.17.0.dev0', num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012,
               beta_schedule='scaled_linear', trained_betas=None, prediction_type='v_prediction')
    cfg.update(dict(euler=dict(interpolation_type='log_linear', use_karras_sigmas=True), heun=dict(use_karras_sigmas=True)).get(cls, {}))
    json.dump(cfg, open(os.path.join(d, 'scheduler', 'scheduler_config.json'), 'w'))
    back = diffusion.DDPMPipeline.from_pretrained(d)
    want = {k: v for k, v in cfg.items() if not k.startswith('_')}
    assert type(back.scheduler).__name__ == R.CLASSES[cls] and vars(back.scheduler.config) == want
    alone = type(back.scheduler).from_pretrained(d, subfolder='scheduler')
    assert vars(alone.config) == want
    d2 = str(tmp_path / 'again')
    back.save_pretrained(d2)
    stored = json.load(open(os.path.join(d2, 'scheduler', 'scheduler_config.json')))
    assert stored['_class_name'] == R.CLASSES[cls] and {k: v for k, v in stored.items() if not k.startswith('_')} == want
    assert json.load(open(os.path.join(d2, 'model_index.json')))['scheduler'] == ['diffusers', R.CLASSES[cls]]
    alone.save_pretrained(str(tmp_path / 'sched'))
    assert json.load(open(str(tmp_path / 'sched' / 'scheduler_config.json'))) == stored
    with pytest.raises(ValueError, match='LDMPipeline'):                         # ... and the pixel-space pipeline refuses to sample with it
        back(batch_size=1, num_inference_steps=2)


# ------------------------------------------------------------------------------------------------ pipelines
class _ToyUNet:
    """A foreign model object: no sampling_forward, so the pipelines call it plainly."""
    config = SimpleNamespace(sample_size=8, in_channels=3)
    device = torch.device('cpu')
    dtype = torch.float32

    def __init__(self):
        self.seen = []

    def __call__(self, sample, t):
        self.seen.append(t)
        return SimpleNamespace(sample=R.toy_model(sample, t))


class _ToyVQ:
    def decode(self, z):
        return SimpleNamespace(sample=torch.tanh(z * 0.01))


@pytest.mark.parametrize('chain', [c for c in R.CHAINS if not c[4]], ids=lambda c: c[0])
def test_ldm_pipeline_equals_the_explicit_loop(chain, mocked):
    """Over the chains that take no generator: LDMPipeline passes the scheduler none, as the reference's does not."""
    name, cls, kw, n, _ = chain
    diffusion = pkg('diffusion')
    g = R.load(R.TOY_FILE)
    unet = _ToyUNet()
    pipe = diffusion.LDMPipeline(vqvae=_ToyVQ(), unet=unet, scheduler=_sched(cls, **kw))
    images = pipe(batch_size=R.CHAIN_B, generator=torch.Generator().manual_seed(R.CHAIN_SEED), num_inference_steps=n, output_type='numpy').images
    assert unet.seen == g[name + ':timesteps'].tolist() and all(type(t) is float for t in unet.seen)      # fractional timesteps as they are
    last = torch.from_numpy(g[name + ':xs32'][-1])
    want = (torch.tanh(last * 0.01) / 2 + 0.5).clamp(0, 1).permute(0, 2, 3, 1).numpy()
    assert np.array_equal(images, want) and images.min() != images.max()


class _Stop(Exception):
    pass


class _StopsAtOnce(_ToyUNet):
    def __call__(self, sample, t):
        self.seen.append(t)
        raise _Stop


def test_ldm_pipeline_keeps_the_integer_list_of_the_other_schedulers():
    diffusion = pkg('diffusion')
    for sched in (diffusion.DDIMScheduler(), diffusion.PNDMScheduler(skip_prk_steps=True), diffusion.DPMSolverMultistepScheduler()):
        unet = _StopsAtOnce()
        with pytest.raises(_Stop):
            diffusion.LDMPipeline(vqvae=_ToyVQ(), unet=unet, scheduler=sched)(batch_size=1, num_inference_steps=10)
        assert unet.seen == [int(sched.timesteps[0])] and type(unet.seen[0]) is int, (type(sched).__name__, unet.seen)


def test_host_timesteps_is_the_list_a_loop_walks():
    diffusion = pkg('diffusion')
    for cls in R.CLASSES:
        s = _sched(cls)
        s.set_timesteps(7)
        got = s.host_timesteps()
        assert got == s.timesteps.tolist() == s._ts and all(type(t) is float for t in got) and got is not s._ts
    for s in (diffusion.DDPMScheduler(), diffusion.DDIMScheduler(), diffusion.PNDMScheduler(skip_prk_steps=True),
              diffusion.DPMSolverMultistepScheduler(), diffusion.UniPCMultistepScheduler()):
        s.set_timesteps(10)
        got = s.host_timesteps()
        assert got == [int(t) for t in s.timesteps.tolist()] and all(type(t) is int for t in got), type(s).__name__


def test_ddpm_pipeline_refuses_a_sigma_space_scheduler():
    diffusion = pkg('diffusion')
    unet = _ToyUNet()
    for cls in R.CLASSES:
        with pytest.raises(ValueError, match='LDMPipeline.*explicit loop'):
            diffusion.DDPMPipeline(unet, _sched(cls))(batch_size=1, num_inference_steps=3)
    assert unet.seen == []
    # detected by an attribute of the scheduler, not by a class list
    other = diffusion.DDIMScheduler()
    other.sigma_space = True
    with pytest.raises(ValueError, match='LDMPipeline'):
        diffusion.DDPMPipeline(unet, other)(batch_size=1, num_inference_steps=3)
    # DDIMPipeline and PNDMPipeline rebuild their own scheduler from the config, as before
    assert type(diffusion.DDIMPipeline(unet, _sched('euler')).scheduler) is diffusion.DDIMScheduler
    assert type(diffusion.PNDMPipeline(unet, _sched('heun')).scheduler) is diffusion.PNDMScheduler


# ------------------------------------------------------------------------------------------------ the sampling forward's timestep kinds
def test_fractional_timesteps_are_told_from_table_indices():
    unet = pkg('unet')
    for t in (832.5, 888.0, np.float32(832.5), np.float64(832.5), torch.tensor(832.5), torch.tensor(832.5, dtype=torch.float64), torch.tensor([979.61])):
        assert unet._is_fractional(t)
    for t in (888, True, torch.tensor(888), torch.tensor([888, 3]), torch.tensor([1.5, 2.5]), np.int64(3), np.int32(3)):
        assert not unet._is_fractional(t)
    got = unet._fractional_timesteps(torch.tensor(979.61, dtype=torch.float64), 3, 'cpu')
    assert got.dtype == torch.float32 and got.tolist() == [float(np.float32(979.61))] * 3
    assert unet._fractional_timesteps(np.float32(979.61), 2, 'cpu').tolist() == [float(np.float32(979.61))] * 2
    buf = torch.zeros(3)
    assert unet._fractional_timesteps(832.5, 3, 'cpu', out=buf) is buf and buf.tolist() == [832.5] * 3
