"""LMSDiscreteScheduler, KDPM2DiscreteScheduler and KDPM2AncestralDiscreteScheduler on the host (`-m "not gpu"`): the classes of
diffusion.py over the CPU stand-in of their kernels (tests/mock_ops_kdiff.py, the kernels' operation order in fp32 torch) against the
fixtures that tests/golden/make_golden_kdiff.py recorded from the reference's own schedulers: the tables exactly, NaN positions
included; the multistep coefficients bit for bit; every stored step and the toy-model chains as numbers against the reference's fp32
run (the reference's `sum()` starts from the integer 0, which moves the sign of a zero and nothing else) with every host scalar equal
to the reference's; the refusals; configs across all twelve classes; the pipeline directory round trip; LDMPipeline against the
explicit loop; and the launch-site table of csrc/kdiff.hip."""
import ctypes
import inspect
import json
import os
import re
import warnings
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import golden_common as gc
import kdiff_ref as R
from helpers import pkg

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture()
def mocked(monkeypatch):
    import mock_ops_kdiff as mock
    monkeypatch.setattr(pkg('diffusion'), 'ops', mock)
    del mock.calls[:]
    return mock


@pytest.fixture(scope='module')
def tables():
    return R.load(R.TABLES_FILE)


@pytest.fixture(scope='module')
def steps():
    return R.load_steps()


def _sched(cls, **kw):
    return getattr(pkg('diffusion'), R.CLASSES[cls])(**kw)


def _extra(cls, skw, seed):
    return dict(skw, generator=torch.Generator().manual_seed(seed)) if cls == 'kdpm2a' else dict(skw)


def _same(a, b):
    """Equal as numbers, element by element: NaN equals NaN, -0.0 equals 0.0."""
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


# ------------------------------------------------------------------------------------------------ the fixture and the launch-site table
def test_fixture_covers_what_it_must(tables, steps):
    """From the stored numbers: every table case; every setting at n = 10 and n = 7; the stored calls reaching all 18 instantiations of
    dp_kdpm2_step and dp_lms_step, first and last calls, both states of the KDPM2 classes; five chains; every file under 1 MiB."""
    assert {c[3] for c in R.TABLE_CASES} == {1, 2, 3, 5, 7, 10, 50, 1000} and len(R.TABLE_CASES) == 96
    assert {c[:3] for c in R.TABLE_CASES} == {(c, s, v) for c in R.CLASSES for s in R.SCHEDULES for v in R.VARIANTS[c]}
    assert R.VARIANTS['lms'] == ('plain', 'karras')
    for case in R.TABLE_CASES:
        name = R.table_name(case)
        ts, sig = tables[name + ':timesteps'], tables[name + ':sigmas']
        assert ts.dtype == np.float64 and sig.dtype == np.float32 and (len(ts), len(sig)) == R.table_lengths(case)
        assert np.isfinite(sig).all() and (np.isfinite(ts).all() or case[:2] == ('kdpm2a', 'squaredcos_cap_v2'))
        for k in R.EXTRA_TABLES[case[0]]:
            assert tables[name + ':' + k].dtype == np.float32 and tables[name + ':' + k].shape == sig.shape
    for n in R.LMS_COEF_NS:
        for t in range(n):
            for order in range(1, min(t + 1, 4) + 1):
                c = tables[R.lms_coef_name(n, t, order)]
                assert c.dtype == np.float32 and c.shape == (order,) and np.isfinite(c).all()
    assert R.LMS_COEF_NS == (2, 5, 10)
    seen = set()
    for run in R.STEP_RUNS:
        sname, cls, kw, skw, n, at = run
        name = R.run_name(run)
        last = R.n_calls(cls, n) - 1
        assert n in (10, 7) and len(steps[name + ':timesteps']) == last + 1
        assert set(at) == ({0, 1, 3, 4, last} if cls == 'lms' else {0, 1, 2, last - 1, last})
        for k in at:
            key = '%s@%d' % (name, k)
            seen.add(R.instance_of_call(cls, kw, skw, k))
            assert steps[key + ':prev64'].dtype == np.float64 and steps[key + ':prev32'].dtype == np.float32
            assert steps[key + ':prev32'].shape == R.STEP_SHAPE and steps[key + ':coefs'].shape == (len(R.LMS_COEF if cls == 'lms' else R.KDPM2_COEF),)
            assert float(steps[key + ':e_ref32']) == float(np.abs(steps[key + ':prev32'].astype(np.float64) - steps[key + ':prev64']).max())
            assert (key + ':x0_32' in steps) == (cls == 'lms')
    assert seen == set(R.INSTANCES) == R.stored_coverage() and len(seen) == 18
    settings = {s[0]: s for s in R.SETTINGS}
    assert settings['lms_karras'][2] == dict(use_karras_sigmas=True) and settings['lms_order2'][3] == dict(order=2)
    assert {(s[1], s[2].get('prediction_type', 'epsilon')) for s in R.SETTINGS} == {
        ('lms', 'epsilon'), ('lms', 'v_prediction'), ('lms', 'sample'), ('kdpm2', 'epsilon'), ('kdpm2', 'v_prediction'),
        ('kdpm2a', 'epsilon'), ('kdpm2a', 'v_prediction')}
    assert any(s[2].get('beta_schedule') == 'scaled_linear' for s in R.SETTINGS)
    assert [c[0] for c in R.CHAINS] == ['lms7', 'lms_karras10', 'kdpm2_5', 'kdpm2_v5', 'kdpm2a_5']
    chains, toy = R.load(R.CHAINS_FILE), R.load(R.TOY_FILE)
    for name, cls, kw, n, with_gen in R.CHAINS:
        calls = R.n_calls(cls, n)
        assert chains[name + ':xs64'].dtype == np.float64 and chains[name + ':xs64'].shape[0] == calls + 1 == len(chains[name + ':gap'])
        assert toy[name + ':xs32'].dtype == np.float32 and toy[name + ':xs32'].shape == (calls + 1,) + R.TOY_SHAPE
        assert (name + ':gen_state' in toy) == with_gen == (cls == 'kdpm2a')
    # what the fixture writer's table patches (sqrt / log / exp rounded once from fp64) moved against the reference without them, on the
    # host that wrote the fixtures: last bits of the sigmas; more of the tables that difference neighbouring sigmas, in few places
    total, differing, worst_ulp = (int(v) for v in tables['unpatched:sigmas'])
    assert total == sum(R.table_lengths(c)[1] for c in R.TABLE_CASES) and 0 <= differing <= total // 100 and worst_ulp <= 1
    for k in ('sigmas_interpol', 'sigmas_up', 'sigmas_down'):
        total, differing, worst_ulp = (int(v) for v in tables['unpatched:' + k])
        assert total > 0 and differing <= total // 50 and worst_ulp <= 263
    assert float(tables['unpatched:timesteps_worst']) <= 1e-3
    for f in (R.TABLES_FILE, R.CHAINS_FILE, R.TOY_FILE) + tuple(R.STEPS_FILES.values()):
        assert os.path.getsize(os.path.join(HERE, 'golden', f)) <= 1 << 20


def test_every_launch_site_of_kdiff_hip_is_in_its_branch_table():
    """csrc/kdiff.hip launches through KD_LAUNCH, a macro of its own with the body of the library's launch macro, and its sites are
    tabled in tests/test_kdiff_gpu.py: a new site changes the count, a new instantiation is in no table, an entry without a case
    fails -- before a GPU is needed.  The file is in both build lists and declared with its bindings, and csrc/sigma.hip keeps its 11
    sites."""
    import test_kdiff_gpu as T
    import mock_ops_kdiff as mock
    L, ops = pkg('_lib'), pkg('ops')
    csrc = os.path.join(ROOT, 'diff-pruning_amd', 'csrc')
    assert list(T.LAUNCH_SITES) == ['kdiff.hip']
    src = open(os.path.join(csrc, 'kdiff.hip')).read()
    body = src.replace('#define KD_LAUNCH(', '')
    sites = re.findall(r'\bKD_LAUNCH\((\((?:kdpm2|lms)_step_kernel<\d, DP_KDIFF_[A-Z]+>\))', body)
    assert len(sites) == T.LAUNCH_SITES['kdiff.hip'] == body.count('KD_LAUNCH(') == 18, sites
    assert 'DP_' + 'LAUNCH(' not in src and 'SG_LAUNCH' not in src
    assert re.search(r'#define KD_LAUNCH\(k, \.\.\.\).*dp_launch_names\[dp_launches\+\+ & \(DP_LAUNCH_RING - 1\)\] = #k;.*'
                     r'hipLaunchKernelGGL\(k, __VA_ARGS__\)', src)
    assert '#pragma clang fp contract(off)' in src and 'fma' not in src.replace('v_fma_f32', '') and '__fdividef' not in src
    assert 'atomic' not in src and 'asm' not in src
    assert sorted(sites) == sorted(T.BRANCHES) and len(set(T.BRANCHES)) == len(T.BRANCHES)
    assert all(e in T.CASES for e in T.BRANCHES), sorted(set(T.BRANCHES) - set(T.CASES))
    assert sorted(T.CASES.values()) == sorted(R.INSTANCES)
    assert sorted(R.KDPM2_INSTANCES) == sorted(ops.KDPM2_INSTANCES) == sorted(mock.KDPM2_INSTANCES)
    assert sorted(R.LMS_INSTANCES) == sorted(ops.LMS_INSTANCES) == sorted(mock.LMS_INSTANCES)
    using = {f for f in os.listdir(csrc) if 'KD_LAUNCH(' in open(os.path.join(csrc, f)).read()}
    assert using == {'kdiff.hip'}
    assert open(os.path.join(csrc, 'sigma.hip')).read().replace('#define SG_LAUNCH(', '').count('SG_LAUNCH(') == 11
    assert 'csrc/kdiff.hip' in open(os.path.join(ROOT, 'build.sh')).read()
    assert "'csrc/kdiff.hip'" in open(os.path.join(ROOT, '__graft_entry__.py')).read()
    hdr = open(os.path.join(ROOT, 'include', 'dp_hip.h')).read()
    assert len(L.SIGNATURES['dp_kdpm2_step']) == 9 and len(L.SIGNATURES['dp_lms_step']) == 13
    assert ('int dp_kdpm2_step(const float* x, const float* e, const float* xs, const float* z, int pred, const dp_kdpm2_coef* coef,\n'
            '                  float* x_next, long long n, void* stream);') in hdr
    assert ('int dp_lms_step(const float* x, const float* e, const float* d1, const float* d2, const float* d3, int order, int pred,\n'
            '                const dp_lms_coef* coef, float* x_next, float* d_new, float* x0_out, long long n, void* stream);') in hdr
    # the header's parameter kinds against the ctypes table: pointers, ints, long long, in order
    kinds = {'float*': ctypes.c_void_p, 'void*': ctypes.c_void_p, 'int': ctypes.c_int, 'long long': ctypes.c_longlong}
    for fn, struct in (('dp_kdpm2_step', L.Kdpm2Coef), ('dp_lms_step', L.LmsCoef)):
        params = re.search(r'int %s\((.*?)\);' % fn, hdr, re.S).group(1).replace('\n', ' ').split(',')
        want = []
        for p in params:
            p = p.replace('const ', '').strip()
            want.append(ctypes.POINTER(struct) if 'coef*' in p else kinds[p.rsplit(' ', 1)[0]])
        assert want == L.SIGNATURES[fn], fn
    # the structs of scalars: the header's field order is the binding's, the wrapper's, the stand-in's and the fixture's
    for struct, binding, names_of in (('dp_kdpm2_coef', L.Kdpm2Coef, (ops.KDPM2_COEF, mock.KDPM2_COEF, R.KDPM2_COEF)),
                                      ('dp_lms_coef', L.LmsCoef, (ops.LMS_COEF, mock.LMS_COEF, R.LMS_COEF))):
        fields = re.search(r'typedef struct %s \{(.*?)\} %s;' % (struct, struct), hdr, re.S).group(1)
        names = [n for line in re.sub(r'/\*.*?\*/', '', fields, flags=re.S).split(';') for n in re.findall(r'\b(?!float\b)([a-z_0-9]+)\b', line)]
        assert all(tuple(names) == v for v in names_of) and tuple(names) == tuple(n for n, _ in binding._fields_)
        assert ctypes.sizeof(binding) == 4 * len(names)
    for i, m in enumerate(R.PREDS):
        assert int(re.search(r'#define DP_KDIFF_%s (\d+)' % m, hdr).group(1)) == getattr(ops, 'KDIFF_' + m) == getattr(mock, 'KDIFF_' + m) == i
    for i, m in enumerate(R.SHAPES):
        assert getattr(ops, 'KDPM2_' + m) == getattr(mock, 'KDPM2_' + m) == i
    m = re.search(r'#define DP_KDIFF_MAX_BLOCKS (\d+)', hdr)
    assert int(m.group(1)) == ops.KDIFF_MAX_BLOCKS == T.MAX_BLOCKS == int(re.search(r'#define DP_SIGMA_MAX_BLOCKS (\d+)', hdr).group(1))
    lib = L.load()
    assert all(getattr(lib, n) is not None for n in ('dp_kdpm2_step', 'dp_lms_step'))


# ------------------------------------------------------------------------------------------------ tables
@pytest.mark.parametrize('case', R.TABLE_CASES, ids=R.table_name)
def test_tables_equal_the_references(case, tables):
    """Every table equals the fixture's exactly, NaN positions included (a NaN's payload is not compared)."""
    s = _sched(case[0], **R.table_kwargs(case))
    s.set_timesteps(case[3])
    name = R.table_name(case)
    assert s.timesteps.dtype == torch.float64 and s.sigmas.dtype == torch.float32
    assert _same(s.timesteps.numpy(), tables[name + ':timesteps'])
    assert s.sigmas.numpy().tobytes() == tables[name + ':sigmas'].tobytes()
    for k in R.EXTRA_TABLES[case[0]]:
        got = getattr(s, k)
        assert got.dtype == torch.float32 and _same(got.numpy(), tables[name + ':' + k]), k
        assert np.array_equal(np.isnan(got.numpy()), np.isnan(tables[name + ':' + k]))
    assert np.float32(float(s.init_noise_sigma)).tobytes() == tables[name + ':init_noise_sigma'].tobytes()
    # the host's copies: what `step` and `scale_model_input` look up
    assert _same(s._ts, tables[name + ':timesteps']) and all(type(t) is float for t in s._ts)
    assert s._sig.device.type == 'cpu' and torch.equal(s._sig, s.sigmas) and s.num_inference_steps == case[3]


@pytest.mark.parametrize('n', R.LMS_COEF_NS)
def test_lms_coefficients_equal_the_references_bits(n, tables):
    s = _sched('lms')
    s.set_timesteps(n)
    for t in range(n):
        for order in range(1, min(t + 1, 4) + 1):
            got = np.array(s.lms_coefficients(order, t), np.float32)
            assert got.tobytes() == tables[R.lms_coef_name(n, t, order)].tobytes(), (n, t, order)
            assert all(type(v) is float for v in s.lms_coefficients(order, t))


def test_the_reference_quadrature_is_not_the_closed_form(tables):
    """Why the coefficients come from scipy's quad over the fp32 integrand: the exact integral of the Lagrange basis polynomial,
    evaluated in fp64 from the same fp32 sigmas, rounds to another fp32 value for some of them."""
    s = _sched('lms')
    s.set_timesteps(10)
    sig = s._sig.double().numpy()
    t, order = 5, 4
    exact = []
    for j in range(order):
        poly = np.poly1d([1.0])
        for k in range(order):
            if k != j:
                poly = poly * np.poly1d([1.0, -sig[t - k]]) / (sig[t - j] - sig[t - k])
        P = poly.integ()
        exact.append(P(sig[t + 1]) - P(sig[t]))
    stored = tables[R.lms_coef_name(10, t, order)]
    exact32 = np.array(exact, np.float32)
    assert np.allclose(exact32, stored, rtol=1e-5) and int((exact32 != stored).sum()) >= 1


def test_the_coefficient_cache_integrates_once_per_order_and_index(mocked, monkeypatch):
    from scipy import integrate
    counted = []
    real = integrate.quad
    monkeypatch.setattr(integrate, 'quad', lambda f, a, b, **kw: counted.append((float(a), float(b))) or real(f, a, b, **kw))
    s = _sched('lms')
    s.set_timesteps(5)
    assert counted == []                                                         # nothing is integrated before a step needs it
    s.is_scale_input_called = True
    x, e = R.step_inputs(0)
    for t in s._ts:
        s.step(e, t, x)
    assert len(counted) == 1 + 2 + 3 + 4 + 4                                     # `order` integrals per (order, index)
    s.derivatives = []
    for t in s._ts:                                                              # the same (order, index) pairs again: kept
        s.step(e, t, x)
    assert len(counted) == 14 and sorted(s._lms) == [(1, 0), (2, 1), (3, 2), (4, 3), (4, 4)]
    s.step(e, s._ts[4], x, order=2)                                              # another order at a known index: integrated
    assert len(counted) == 16
    s.set_timesteps(5)
    assert s._lms == {} and s.derivatives == []
    s.step(e, s._ts[0], x)
    assert len(counted) == 17


def test_the_quirks_of_the_tables():
    lms = _sched('lms')
    assert lms.order == 1 and len(lms._ts) == 1000 and len(lms._sig) == 1001 and lms.derivatives == []
    top = float(lms.init_noise_sigma)
    lms.set_timesteps(3)
    assert float(lms.init_noise_sigma) == top == float(lms._train_sigmas().max())  # from the constructor, not updated
    for cls in ('kdpm2', 'kdpm2a'):
        s = _sched(cls)
        assert s.order == 2 and len(s._ts) == 1999 and len(s._sig) == 2002       # the constructor's table: every training timestep
        assert vars(s.config)['beta_start'] == 0.00085 and vars(s.config)['beta_end'] == 0.012
        s.set_timesteps(1)
        assert s._ts == [0.0] and len(s._sig) == 4 and s._sig[1:].tolist() == [0.0, 0.0, 0.0]
        assert float(s.init_noise_sigma) == float(s._sig[0])                      # follows set_timesteps
        s.set_timesteps(5)
        assert len(s._ts) == 9 and len(s._sig) == 12 and s._ts[0] == 999.0 and s.state_in_first_order and s.sample is None
        assert s._interpol.shape == s._sig.shape and _same(s._interpol, s.sigmas_interpol)
        assert s.log_sigmas.dtype == torch.float32 and s.log_sigmas.shape == (1000,)
    k = _sched('kdpm2')
    k.set_timesteps(5)
    assert bool(torch.isnan(k._interpol[0])) and bool(torch.isfinite(k._interpol[1:]).all())     # a lerp towards log 0; never read
    a = _sched('kdpm2a')
    a.set_timesteps(5)
    assert a._ts[2] == 749.25 and 0 < a._ts[1] - a._ts[2] < 1e-3                  # nearly equal pairs: the lookup goes by state
    assert _same(a._up, a.sigmas_up) and torch.equal(a._down, a.sigmas_down) and bool(torch.isnan(a._up[-1]))
    a.set_timesteps(10)
    pairs = [(i, i + 1) for i in range(1, len(a._ts) - 1, 2) if a._ts[i] == a._ts[i + 1]]
    assert pairs, a._ts                                                          # ... and exactly equal ones
    i, j = pairs[0]
    assert a.index_for_timestep(a._ts[i]) == j                                   # first-order state: the last match
    a.sample = torch.zeros(1)
    assert a.index_for_timestep(a._ts[i]) == i                                   # second-order state: the first
    for cls in R.CLASSES:
        s = _sched(cls)
        assert s.sigma_space is True and len(s) == 1000


# ------------------------------------------------------------------------------------------------ single steps, chains
def _coef_names(cls, kw, inst):
    names = {'sig'} | ({'c_out', 'c_den'} if kw.get('prediction_type') == 'v_prediction' else set())
    if cls == 'lms':
        return names | {'c%d' % k for k in range(inst[1])}
    return names | {'dt'} | ({'sigma_up'} if inst[1] == 2 else set())


@pytest.mark.parametrize('run', R.STEP_RUNS, ids=R.run_name)
def test_single_steps_equal_the_references_fp32_run(run, steps, mocked):
    sname, cls, kw, skw, n, at = run
    name = R.run_name(run)
    s = _sched(cls, **kw)
    s.set_timesteps(n)
    assert s._ts == steps[name + ':timesteps'].tolist()
    s.is_scale_input_called = True
    extra = _extra(cls, skw, R.GEN_SEED)
    names = R.LMS_COEF if cls == 'lms' else R.KDPM2_COEF
    for k in range(len(s._ts)):
        x, e = R.step_inputs(k)
        x0, e0 = x.clone(), e.clone()
        before = len(mocked.calls)
        out = s.step(e, s._ts[k], x, **extra)
        assert len(mocked.calls) == before + 1                                   # one kernel call per step
        op, a, pred, _, coef = mocked.calls[-1]
        inst = R.instance_of_call(cls, kw, skw, k)
        assert (op, a, pred) == inst and set(coef) == _coef_names(cls, kw, inst)
        assert torch.equal(x, x0) and torch.equal(e, e0)                         # a step writes none of its inputs
        assert out.prev_sample.dtype == torch.float32 and type(out).__name__ == ('LMSDiscreteSchedulerOutput' if cls == 'lms' else 'SchedulerOutput')
        if k in at:
            key = '%s@%d' % (name, k)
            stored = steps[key + ':coefs']
            differing = [c for c in coef if np.float32(coef[c]).tobytes() != stored[names.index(c)].tobytes()]
            assert differing == [], (key, differing)                             # every host scalar as the reference formed it
            assert _same(out.prev_sample.numpy(), steps[key + ':prev32']), key
            bound = R.single_step_bound(steps[key + ':e_ref32'], steps[key + ':prev64'])
            assert float(np.abs(out.prev_sample.double().numpy() - steps[key + ':prev64']).max()) <= bound, key
            if cls == 'lms':
                assert _same(out.pred_original_sample.numpy(), steps[key + ':x0_32']), key
                bound = R.single_step_bound(steps[key + ':e_ref32_x0'], steps[key + ':x0_64'])
                assert float(np.abs(out.pred_original_sample.double().numpy() - steps[key + ':x0_64']).max()) <= bound, key
    if cls == 'lms':
        assert len(s.derivatives) == min(len(s._ts), skw.get('order', 4))
    else:
        assert not s.state_in_first_order and s.sample is not None             # left so after the last call, as the reference is


def _chain(s, model, x_T, n, with_gen):
    x = x_T * s.init_noise_sigma
    s.set_timesteps(n)
    gen = torch.Generator().manual_seed(R.NOISE_SEED) if with_gen else None
    extra = dict(generator=gen) if with_gen else {}
    xs = [x]
    for t in s._ts:
        xs.append(s.step(model(s.scale_model_input(xs[-1], t), t), t, xs[-1], **extra).prev_sample.clone())
    return xs, gen


@pytest.mark.parametrize('chain', R.CHAINS, ids=lambda c: c[0])
def test_toy_chains_equal_the_references_fp32_states(chain, mocked):
    name, cls, kw, n, with_gen = chain
    g = R.load(R.TOY_FILE)
    s = _sched(cls, **kw)
    xs, gen = _chain(s, R.toy_model, torch.from_numpy(g['x_T']), n, with_gen)
    assert s._ts == g[name + ':timesteps'].tolist()
    want = g[name + ':xs32']
    for k, x in enumerate(xs):
        assert _same(x.numpy(), want[k]), (name, k)
    kernel = 'lms' if cls == 'lms' else 'kdpm2'
    assert [c[0] for c in mocked.calls] == ['scale', kernel] * R.n_calls(cls, n)
    if with_gen:                                                                 # the generator's stream advanced as the reference's did
        assert np.array_equal(gen.get_state().numpy(), g[name + ':gen_state'])


def test_the_toy_x_T_is_the_pipelines_draw():
    g = R.load(R.TOY_FILE)
    x = pkg('diffusion').randn_tensor(R.TOY_SHAPE, generator=torch.Generator().manual_seed(R.CHAIN_SEED))
    assert np.array_equal(x.numpy(), g['x_T'])


def test_the_ancestral_class_draws_on_every_call(mocked):
    """A generator's stream advances once per call, first-order calls included, as the reference's does; the draw reaches the kernel
    on second-order calls only."""
    x, e = R.step_inputs(0)
    s = _sched('kdpm2a')
    s.set_timesteps(7)
    gen, twin = torch.Generator().manual_seed(3), torch.Generator().manual_seed(3)
    for k, t in enumerate(s._ts[:4]):
        s.step(e, t, x, generator=gen)
        torch.randn(R.STEP_SHAPE, generator=twin)
        assert torch.equal(gen.get_state(), twin.get_state())
        assert mocked.calls[-1][1] == (2 if k % 2 else 0)


def test_scale_model_input_and_noise_sigmas_equal_the_references(steps, mocked):
    x, z = (torch.from_numpy(gc.det_noise(R.STEP_SHAPE, 900 + i)) for i in range(2))
    for i, (cls, kw, idx, first) in enumerate(R.SCALE_CASES):
        s = _sched(cls, **kw)
        s.set_timesteps(7)
        if not first:
            s.sample = torch.zeros(1)
        xin = x * R.X_SCALE
        keep = xin.clone()
        y = s.scale_model_input(xin, s._ts[idx])
        assert np.array_equal(y.numpy(), steps['scale:%d:out' % i]) and torch.equal(xin, keep) and y.data_ptr() != xin.data_ptr(), i
        assert s.scale_model_input(xin, torch.tensor(s._ts[idx], dtype=torch.float64)).data_ptr() == y.data_ptr()      # a buffer of its own
    for i, (cls, kw, idx, first) in enumerate(R.NOISE_CASES):
        s = _sched(cls, **kw)
        s.set_timesteps(10)
        if not first:
            s.sample = torch.zeros(1)
        sig = s.noise_sigmas(s.timesteps[idx])
        assert sig.dtype == torch.float32
        assert np.array_equal(mocked.sigma_add_noise(x, z, sig).numpy(), steps['noise:%d:out' % i]), i
        with pytest.raises(RuntimeError):                                        # host tensors: no fall-back
            s.add_noise(x, z, s.timesteps[idx])
    assert {c[0] for c in mocked.calls} == {'scale', 'add_noise'}


# ------------------------------------------------------------------------------------------------ state
def test_kdpm2_keeps_its_state_as_the_reference_does(mocked):
    for cls in ('kdpm2', 'kdpm2a'):
        del mocked.calls[:]
        s = _sched(cls)
        s.set_timesteps(4)
        x0, e0 = R.step_inputs(0)
        x1, e1 = R.step_inputs(1)
        extra = _extra(cls, {}, 5)
        a = s.step(e0, s._ts[0], x0, **extra).prev_sample
        assert not s.state_in_first_order and s.sample is x0                    # held by reference, not copied
        c = s.step_coefs(s.index_for_timestep(s._ts[1]))
        b = s.step(e1, s._ts[1], a, **extra).prev_sample
        assert s.state_in_first_order and s.sample is None
        noise = None
        if cls == 'kdpm2a':
            g = torch.Generator().manual_seed(5)
            torch.randn(R.STEP_SHAPE, generator=g)
            noise = torch.randn(R.STEP_SHAPE, generator=g)                       # the second draw of the stream
        assert ('sigma_up' in c) == (cls == 'kdpm2a')
        assert torch.equal(b, mocked.kdpm2_step(a, e1, c, saved=x0, noise=noise))
        assert len({a.data_ptr(), b.data_ptr(), x0.data_ptr()}) == 3            # the saved sample and the first result are not written
        assert [c[1] for c in mocked.calls[:2]] == [0, 2 if cls == 'kdpm2a' else 1]


def test_lms_history_is_a_ring_of_four_buffers_of_the_schedulers_own(mocked):
    s = _sched('lms')
    s.set_timesteps(10)
    s.is_scale_input_called = True
    slots = []
    for k, t in enumerate(s._ts):
        x, e = R.step_inputs(k)
        out = s.step(e, t, x)
        assert len(s.derivatives) == min(k + 1, 4)
        slots.append(s.derivatives[-1].data_ptr())
        want = (x - (x - torch.tensor(float(s._sig[k])) * e)) / torch.tensor(float(s._sig[k]))
        assert torch.equal(s.derivatives[-1], want)                              # newest last, as the reference's list
        assert out.pred_original_sample.data_ptr() not in slots and out.prev_sample.data_ptr() not in slots
    assert len(set(slots)) == 4 and slots[4:] == slots[:6]                       # the new derivative takes the slot of the one dropped
    assert [d.data_ptr() for d in s.derivatives] == slots[-4:]
    s.step(e, s._ts[9], x, order=2)                                              # a smaller order drops one, as the reference does
    assert len(s.derivatives) == 4 and mocked.calls[-1][1] == 2
    s.set_timesteps(10)
    assert s.derivatives == []
    s.step(e, s._ts[5], x)                                                       # fewer derivatives than the order: zip() stops early
    assert mocked.calls[-1][1] == 1 and set(mocked.calls[-1][4]) == {'sig', 'c0'}
    assert np.float32(mocked.calls[-1][4]['c0']) == np.float32(s.lms_coefficients(4, 5)[0])


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
        r = s.step(e, s._ts[4], x, return_dict=False, **_extra(cls, {}, 1))
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
        bad = _sched(cls, prediction_type='nonsense')
        bad.set_timesteps(7)
        with pytest.raises(ValueError, match='prediction_type'):
            bad.step(z, bad._ts[0], z)
    for cls in ('kdpm2', 'kdpm2a'):
        s = _sched(cls, prediction_type='sample')                                # the reference raises in `step`, not before
        s.set_timesteps(7)
        with pytest.raises(NotImplementedError, match='prediction_type not implemented yet: sample'):
            s.step(z, s._ts[0], z)
        assert s.state_in_first_order
    lms = _sched('lms')
    lms.set_timesteps(7)
    with pytest.raises(NotImplementedError, match='order'):
        lms.step(z, lms._ts[0], z, order=5)
    with pytest.raises(ValueError, match='order'):
        lms.step(z, lms._ts[0], z, order=0)
    assert mocked.calls == [] and lms.derivatives == []
    with pytest.raises(AssertionError):                                          # the stand-in refuses what the wrapper refuses
        mocked.kdpm2_step(z, z, dict(sig=1.0, dt=1.0), pred=mocked.KDIFF_SAMPLE)
    with pytest.raises(AssertionError):
        mocked.kdpm2_step(z, z, dict(sig=1.0, dt=1.0), noise=z)
    with pytest.raises(AssertionError):
        mocked.lms_step(z, z, dict(sig=1.0, c0=1.0, c1=1.0), 2)


def test_lms_step_without_scale_model_input_warns_once(mocked):
    z = torch.zeros(1, 3, 4, 4)
    for cls, warns in (('lms', True), ('kdpm2', False), ('kdpm2a', False)):
        s = _sched(cls)
        s.set_timesteps(10)
        with warnings.catch_warnings(record=True) as w:
            warnings.simplefilter('always')
            s.step(z, s._ts[0], z)
            s.step(z, s._ts[1], z)
        assert len([m for m in w if 'scale_model_input' in str(m.message)]) == (1 if warns else 0)
    s2 = _sched('lms')
    s2.set_timesteps(10)
    assert s2.is_scale_input_called is False
    s2.scale_model_input(z, s2._ts[0])
    assert s2.is_scale_input_called is True
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        s2.step(z, s2._ts[0], z)
    assert not w


def test_signatures_and_config_defaults_equal_the_references():
    """The constructor parameters in the reference's order with its defaults (scheduling_lms_discrete.py:111-120,
    scheduling_k_dpm_2_discrete.py:86-94, scheduling_k_dpm_2_ancestral_discrete.py:87-95) and the `step` / `set_timesteps` parameters."""
    diffusion = pkg('diffusion')
    want = dict(
        lms=dict(num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule='linear', trained_betas=None,
                 use_karras_sigmas=False, prediction_type='epsilon'),
        kdpm2=dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule='linear', trained_betas=None,
                   prediction_type='epsilon'),
        kdpm2a=dict(num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule='linear', trained_betas=None,
                    prediction_type='epsilon'))
    for cls, defaults in want.items():
        c = getattr(diffusion, R.CLASSES[cls])
        params = inspect.signature(c.__init__).parameters
        assert [p for p in params if p != 'self'] == list(defaults) == list(c._CONFIG_KEYS) == list(vars(c().config))
        assert {k: params[k].default for k in defaults} == defaults == vars(c().config)
    step = inspect.signature(diffusion.LMSDiscreteScheduler.step).parameters
    assert list(step) == ['self', 'model_output', 'timestep', 'sample', 'order', 'return_dict'] and step['order'].default == 4
    assert step['return_dict'].default is True
    assert list(inspect.signature(diffusion.KDPM2DiscreteScheduler.step).parameters) == ['self', 'model_output', 'timestep', 'sample', 'return_dict']
    assert list(inspect.signature(diffusion.KDPM2AncestralDiscreteScheduler.step).parameters) == [
        'self', 'model_output', 'timestep', 'sample', 'generator', 'return_dict']
    assert list(inspect.signature(diffusion.LMSDiscreteScheduler.set_timesteps).parameters) == ['self', 'num_inference_steps', 'device']
    for c in (diffusion.KDPM2DiscreteScheduler, diffusion.KDPM2AncestralDiscreteScheduler):
        assert list(inspect.signature(c.set_timesteps).parameters) == ['self', 'num_inference_steps', 'device', 'num_train_timesteps']
    assert list(inspect.signature(diffusion.LMSDiscreteScheduler.get_lms_coefficient).parameters) == ['self', 'order', 't', 'current_order']
    out = diffusion.LMSDiscreteSchedulerOutput(prev_sample=torch.zeros(1))
    assert out.pred_original_sample is None


def test_from_config_round_trips_across_all_twelve_classes():
    diffusion = pkg('diffusion')
    classes = [getattr(diffusion, n) for n in R.ALL_CLASSES]
    assert len(classes) == 12
    for cls in R.CLASSES:
        c = getattr(diffusion, R.CLASSES[cls])
        a = c(beta_schedule='scaled_linear', beta_start=0.0015, beta_end=0.0195, prediction_type='v_prediction')
        assert vars(c.from_config(a.config).config) == vars(a.config)
        assert vars(c.from_config(dict(vars(a.config), skip_type='quad')).config) == vars(a.config)      # foreign keys are dropped
        for other in classes:
            # RePaint carries epsilon models only and no prediction_type key: it starts from its own defaults for what it lacks
            src = other() if other is diffusion.RePaintScheduler else other(beta_schedule='scaled_linear', beta_start=0.0015, beta_end=0.0195)
            there = c.from_config(src.config)                                    # from every class ...
            assert (there.config.beta_start, there.config.beta_end) == (src.config.beta_start, src.config.beta_end), other.__name__
            back = other.from_config(dict(vars(a.config), prediction_type='epsilon'))     # ... and to it (not every class carries v)
            assert (back.config.beta_schedule, back.config.beta_end) == ('scaled_linear', 0.0195), other.__name__
            assert vars(c.from_config(back.config).config)['beta_start'] == 0.0015
    lms = diffusion.LMSDiscreteScheduler.from_config(diffusion.HeunDiscreteScheduler(use_karras_sigmas=True).config)
    assert lms.config.use_karras_sigmas is True and lms.use_karras_sigmas is True
    assert vars(diffusion.KDPM2DiscreteScheduler.from_config(lms.config).config)['beta_start'] == 0.00085


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
    cfg.update(dict(lms=dict(use_karras_sigmas=True)).get(cls, {}))
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


def test_host_timesteps_and_the_ddpm_pipelines_refusal():
    diffusion = pkg('diffusion')
    unet = _ToyUNet()
    for cls in R.CLASSES:
        s = _sched(cls)
        s.set_timesteps(7)
        got = s.host_timesteps()
        assert got == s.timesteps.tolist() == s._ts and all(type(t) is float for t in got) and got is not s._ts
        with pytest.raises(ValueError, match='LDMPipeline.*explicit loop'):
            diffusion.DDPMPipeline(unet, _sched(cls))(batch_size=1, num_inference_steps=3)
    assert unet.seen == []
