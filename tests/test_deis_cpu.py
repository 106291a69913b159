"""DEISMultistepScheduler and DPMSolverSinglestepScheduler on the host (`-m "not gpu"`): the two classes of diffusion.py over the CPU
stand-in of their kernels (tests/mock_ops_deis.py, the kernels' operation order in fp32 torch) against the fixtures that
tests/golden/make_golden_deis.py recorded from the reference's own schedulers: the timestep tables, `orders` and the order every step
took entry for entry, every single step and the toy-model chains bit for bit against the reference's fp32 run -- third-order DEIS
included: its three-term sum is matched term by term, no step is held to the fp64 bound instead; the rewrites and refusals;
`from_config` to and from every other scheduler class; the pipeline directory round trip; the saved-sample rule of the singlestep
solver; and the launch-site table of csrc/deis.hip."""
import ctypes
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

import golden_common as gc
import deis_ref as R
from helpers import pkg

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OTHERS = ('DDPMScheduler', 'DDIMScheduler', 'DPMSolverMultistepScheduler', 'UniPCMultistepScheduler', 'PNDMScheduler', 'RePaintScheduler',
          'EulerDiscreteScheduler', 'EulerAncestralDiscreteScheduler', 'HeunDiscreteScheduler', 'LMSDiscreteScheduler',
          'KDPM2DiscreteScheduler', 'KDPM2AncestralDiscreteScheduler')


@pytest.fixture()
def mocked(monkeypatch):
    import mock_ops_deis as mock
    monkeypatch.setattr(pkg('diffusion'), 'ops', mock)
    del mock.calls[:]
    return mock


@pytest.fixture(scope='module')
def steps():
    return R.load_steps()


def _cls(cls):
    return getattr(pkg('diffusion'), R.CLASSES[cls])


def _sched(cls, **kw):
    return _cls(cls)(**kw)


# ------------------------------------------------------------------------------------------------ the fixture and the launch-site table
def test_fixture_covers_what_it_must(steps):
    """From the stored numbers: every table case; together the stored steps reach every launch site of both kernels with every
    model type, algorithm and treatment, midpoint and heun at orders 2 and 3; the thresholded batches straddle 1 and the maximum."""
    for cls, cases in R.TABLE_CASES.items():
        assert all(R.table_name(cls, c) in steps for c in cases)
        assert {c[2] for c in cases} == {1, 2, 3, 5, 9, 10, 14, 15, 20} and {c[0] for c in cases} == set(R.SCHEDULES)
    assert R.CLIPPED in R.TABLE_CASES['single'] and R.CLIPPED[1] > -float('inf')
    reached, orders2 = set(), set()
    for run in R.STEP_RUNS:
        cls, kw, n, at = run
        name = R.run_name(run)
        orders = steps[name + ':orders'].tolist()
        algo = kw.get('algorithm_type', 'dpmsolver++') if cls == 'single' else 'deis'
        for k in at:
            reached.add((R.run_site(run, orders[k]), kw.get('prediction_type', 'epsilon'), algo, R.run_thresholds(run)))
            if cls == 'single':
                orders2.add((orders[k], kw.get('solver_type', 'midpoint')))
            assert steps['%s@%d:prev64' % (name, k)].dtype == np.float64 and steps['%s@%d:prev32' % (name, k)].shape == R.STEP_SHAPE
        assert (name + ':scale' in steps) == R.run_thresholds(run)
    for pred in R.PREDS:
        for thr in (False, True):
            assert {(R.deis_site(o), pred, 'deis', thr) for o in (1, 2, 3)} <= reached
            for site in {R.single_site(o, h) for o in (1, 2, 3) for h in (False, True)}:
                assert (site, pred, 'dpmsolver++', thr) in reached and (thr or (site, pred, 'dpmsolver', False) in reached)
    assert {(o, s) for o in (2, 3) for s in R.STYPES} <= orders2
    assert steps['run:deis:solver_order=3:20:orders'][-2:].tolist() == [3, 3]            # no lower-order steps from 15 steps on
    names = [c[0] for c in R.CHAINS]
    assert len(set(names)) == 8 and sorted(c[3] for c in R.CHAINS) == [9, 10, 10, 10, 10, 10, 20, 20]
    for f in tuple(R.STEPS_FILES.values()) + R.CHAINS_FILES + (R.TOY_FILE,):
        assert os.path.getsize(os.path.join(HERE, 'golden', f)) <= 1 << 20
    for i, f in enumerate(R.CHAINS_FILES):
        g = R.load(f)
        for name, _, _, n, fi in R.CHAINS:
            if fi == i:
                assert g[name + ':xs64'].dtype == np.float64 and g[name + ':xs64'].shape[0] == n + 1 == len(g[name + ':gap'])


def test_thresholded_fixture_batches_straddle_one_and_the_maximum(steps):
    """Within every thresholded batch the quantile of |x0| falls below 1, inside (1, sample_max_value) and above it."""
    import threshold_ref as TR
    seen = 0
    for run in R.STEP_RUNS:
        if not R.run_thresholds(run):
            continue
        cls, kw, n, at = run
        s = _sched(cls, **kw)
        s.set_timesteps(n)
        scale = steps[R.run_name(run) + ':scale']
        for k in at:
            x, e = R.step_inputs(k, scale[k])
            t = s._ts[k]
            st = TR.abs_quantile(x, e, TR.PRED[kw.get('prediction_type', 'epsilon')], float(s.alpha_t[t]), float(s.sigma_t[t]), 0.995, R.MAX_VALUE)
            q = st[:, 2].tolist()
            assert q[0] < 1.0 < q[1] < R.MAX_VALUE < q[2], (R.run_name(run), k, q)
            assert st[:, 3].tolist() == [1.0, q[1], R.MAX_VALUE]
            seen += 1
    assert seen == 3 * 5 + 6 * 3


def test_every_launch_site_of_deis_hip_is_in_its_branch_table():
    """csrc/deis.hip launches through DE_LAUNCH, a macro of its own with the body of the library's launch macro, and its sites are
    tabled in tests/test_deis_gpu.py: a new site changes the count, a new instantiation is in no table, an entry without a case fails
    -- before a GPU is needed.  The file stays out of the older tables' census, which counts the library macro's call text per file,
    and uses no other file's macro; it is in both build lists and declared with its bindings."""
    import test_deis_gpu as T
    L, ops = pkg('_lib'), pkg('ops')
    csrc = os.path.join(ROOT, 'diff-pruning_amd', 'csrc')
    assert list(T.LAUNCH_SITES) == ['deis.hip']
    src = open(os.path.join(csrc, 'deis.hip')).read()
    body = src.replace('#define DE_LAUNCH(', '')
    sites = re.findall(r'\bDE_LAUNCH\((\((?:deis_step_kernel<\d>|dpm_single_step_kernel<\d, (?:true|false)>)\))', body)
    assert len(sites) == T.LAUNCH_SITES['deis.hip'] == body.count('DE_LAUNCH(') == 7, sites
    assert re.findall(r'\b([A-Z][A-Z0-9]*_LAUNCH)\(', src.replace('DP_LAUNCH_CHECK(', '')) == ['DE_LAUNCH'] * 8
    assert 'DP_' + 'LAUNCH(' not in src
    assert re.search(r'#define DE_LAUNCH\(k, \.\.\.\).*dp_launch_names\[dp_launches\+\+ & \(DP_LAUNCH_RING - 1\)\] = #k;.*'
                     r'hipLaunchKernelGGL\(k, __VA_ARGS__\)', src)
    assert sorted(sites) == sorted(T.BRANCHES) and len(set(T.BRANCHES)) == len(T.BRANCHES)
    assert sorted(T.BRANCHES) == sorted([R.deis_site(o) for o in (1, 2, 3)] + [R.single_site(o, False) for o in (1, 2, 3)] + [R.single_site(3, True)])
    assert all(e in T.CASES and T.CASES[e] for e in T.BRANCHES)
    using = {f for f in os.listdir(csrc) if 'DE_LAUNCH(' in open(os.path.join(csrc, f)).read()}
    assert using == {'deis.hip'}
    assert '#pragma clang fp contract(off)' in src and 'fmaf' not in src
    assert 'csrc/deis.hip' in open(os.path.join(ROOT, 'build.sh')).read()
    assert "'csrc/deis.hip'" in open(os.path.join(ROOT, '__graft_entry__.py')).read()
    hdr = open(os.path.join(ROOT, 'include', 'dp_hip.h')).read()
    assert len(L.SIGNATURES['dp_deis_step']) == 13 and len(L.SIGNATURES['dp_dpm_single_step']) == 16
    assert ('int dp_deis_step(const float* x, const float* m, const float* m1, const float* m2, const float* stats, int order, int pred,\n'
            '                 const dp_deis_coef* coef, float* x_next, float* m0_out, long long B, long long n, void* stream);') in hdr
    assert ('int dp_dpm_single_step(const float* x, const float* xs, const float* m, const float* m1, const float* m2, const float* stats,\n'
            '                       int order, int pred, int data_pred, int heun, const dp_dpm_single_coef* coef, float* x_next, float* m0_out,\n'
            '                       long long B, long long n, void* stream);') in hdr
    # the structs of scalars: the header's field order is the binding's, the wrapper's and the stand-in's
    import mock_ops_deis as mock
    for struct, binding, names_w, names_m in (('dp_deis_coef', L.DeisCoef, ops.DEIS_COEF, mock.DEIS_COEF),
                                              ('dp_dpm_single_coef', L.DpmSingleCoef, ops.DPM_SINGLE_COEF, mock.DPM_SINGLE_COEF)):
        fields = re.search(r'typedef struct %s \{(.*?)\} %s;' % (struct, struct), hdr, re.S).group(1)
        names = [n for line in re.sub(r'/\*.*?\*/', '', fields).split(';') for n in re.findall(r'\b(?!float\b)([a-z_0-9]+)\b', line)]
        assert tuple(names) == tuple(n for n, _ in binding._fields_) == names_w == names_m
        assert ctypes.sizeof(binding) == 4 * len(names)
    m = re.search(r'#define DP_DEIS_MAX_BLOCKS (\d+)', hdr)
    assert int(m.group(1)) == ops.DEIS_MAX_BLOCKS == T.MAX_BLOCKS
    assert (mock.X0_PRED_EPSILON, mock.X0_PRED_SAMPLE, mock.X0_PRED_V) == (ops.X0_PRED_EPSILON, ops.X0_PRED_SAMPLE, ops.X0_PRED_V)
    lib = L.load()
    assert lib.dp_deis_step is not None and lib.dp_dpm_single_step is not None


# ------------------------------------------------------------------------------------------------ tables and orders
@pytest.mark.parametrize('cls,case', [(c, k) for c in R.TABLE_CASES for k in R.TABLE_CASES[c]], ids=lambda v: v if isinstance(v, str) else '%s-%s-%d' % v)
def test_timestep_tables_equal_the_references(cls, case, steps):
    s = _sched(cls, **R.table_kwargs(case))
    s.set_timesteps(case[2])
    want = steps[R.table_name(cls, case)]
    assert s.timesteps.dtype == torch.int64 and s.timesteps.tolist() == want.tolist() == s._ts == s.host_timesteps()
    assert s.num_inference_steps == len(want) and s.model_outputs == [None] * 2


def test_deis_removes_duplicates_and_singlestep_refuses_them():
    d = _sched('deis')
    d.set_timesteps(1000)
    assert len(d._ts) == d.num_inference_steps < 1000 and len(set(d._ts)) == len(d._ts)
    s = _sched('single')
    with pytest.raises(ValueError, match='1000'):
        s.set_timesteps(1000)


@pytest.mark.parametrize('case', R.ORDER_CASES, ids=R.orders_name)
def test_singlestep_orders_and_the_order_each_step_takes(case, steps, mocked):
    """`orders` is get_order_list of the steps asked for; `step` takes order_list's entry, built for num_train_timesteps steps."""
    so, lof, n = case
    s = _sched('single', solver_order=so, lower_order_final=lof)
    assert s.order_list == s.get_order_list(1000)
    s.set_timesteps(n)
    assert s.orders == steps[R.orders_name(case) + ':orders'].tolist() == s.get_order_list(n)
    x = torch.zeros(1, 1, 2, 2)
    for t in s._ts:
        s.step(x, t, x)
    assert [c[1] for c in mocked.calls] == steps[R.orders_name(case) + ':taken'].tolist() == s.order_list[:n]


def test_the_last_of_nine_third_order_steps_is_third_order(steps):
    s = _sched('single', solver_order=3)
    s.set_timesteps(9)
    assert s.orders[-1] == 1 and s.order_list[8] == 3
    assert steps['orders:3:1:9:taken'][-1] == 3 and steps['orders:3:1:9:orders'][-1] == 1


def test_tables_of_the_constructors():
    ref = pkg('diffusion').DPMSolverMultistepScheduler()
    for cls in R.CLASSES:
        s = _sched(cls)
        for n in ('alphas_cumprod', 'alpha_t', 'sigma_t', 'lambda_t'):
            assert torch.equal(getattr(s, n), getattr(ref, n))
        assert s.timesteps.dtype == torch.float32 and s.timesteps[0] == 999 and s.timesteps[-1] == 0 and len(s) == 1000
        assert s.init_noise_sigma == 1.0 and s.num_inference_steps is None and s.order == 1
        x = torch.zeros(2)
        assert s.scale_model_input(x, 5) is x
        with pytest.raises(ValueError):
            s.step(x, 5, x)
        cos = _sched(cls, beta_schedule='squaredcos_cap_v2')
        assert torch.equal(cos.lambda_t, pkg('diffusion').DPMSolverMultistepScheduler(beta_schedule='squaredcos_cap_v2').lambda_t)


# ------------------------------------------------------------------------------------------------ single steps, chains: bit for bit
@pytest.mark.parametrize('run', R.STEP_RUNS, ids=R.run_name)
def test_single_steps_equal_the_references_fp32_bits(run, steps, mocked):
    cls, kw, n, at = run
    name = R.run_name(run)
    thr = R.run_thresholds(run)
    s = _sched(cls, **kw)
    s.set_timesteps(n)
    assert s._ts == steps[name + ':timesteps'].tolist()
    scale = steps.get(name + ':scale')
    taken = []
    for k in range(max(at) + 1):
        x, e = R.step_inputs(k, None if scale is None else scale[k])
        before = len(mocked.calls)
        out = s.step(e, s._ts[k], x)
        new = mocked.calls[before:]
        assert [c[0] for c in new] == (['x0_abs_quantile'] if thr else []) + ['deis_step' if cls == 'deis' else 'dpm_single_step']
        taken.append(new[-1][1])
        assert type(out).__name__ == 'SchedulerOutput' and out.prev_sample.dtype == torch.float32
        if k in at:
            key = '%s@%d' % (name, k)
            assert np.array_equal(out.prev_sample.numpy(), steps[key + ':prev32']), key
            assert np.array_equal(s.model_outputs[-1].numpy(), steps[key + ':m0_32']), key
    assert taken == steps[name + ':orders'][:max(at) + 1].tolist()


@pytest.mark.parametrize('chain', R.CHAINS, ids=lambda c: c[0])
def test_toy_chains_equal_the_references_fp32_bits(chain, mocked):
    name, cls, kw, n, _ = chain
    g = R.load(R.TOY_FILE)
    s = _sched(cls, **kw)
    s.set_timesteps(n)
    assert s._ts == g[name + ':timesteps'].tolist()
    x = torch.from_numpy(g['x_T'])
    want = g[name + ':xs32']
    for k, t in enumerate(s._ts):
        x = s.step(R.toy_model(x, t), t, x).prev_sample
        assert np.array_equal(x.numpy(), want[k + 1]), (name, k)
    assert len([c for c in mocked.calls if c[0] != 'x0_abs_quantile']) == n


def test_the_toy_x_T_is_the_pipelines_draw():
    g = R.load(R.TOY_FILE)
    x = pkg('diffusion').randn_tensor(R.TOY_SHAPE, generator=torch.Generator().manual_seed(R.CHAIN_SEED))
    assert np.array_equal(x.numpy(), g['x_T'])


# ------------------------------------------------------------------------------------------------ step forms, the saved sample
def test_step_forms_and_the_history_ring(mocked):
    """return_dict=False, a 0-d tensor timestep, a timestep that is not in the table (the reference then takes the last index), a
    captured forward's reused output buffer (the history keeps its own copy), and the ring: solver_order buffers, written in turn."""
    s = _sched('deis', solver_order=3)
    s.set_timesteps(20)
    x, e = R.step_inputs(0)
    shared = e.clone()
    a = s.step(shared, torch.tensor(s._ts[0]), x, return_dict=False)
    assert isinstance(a, tuple) and len(a) == 1
    first = s.model_outputs[-1]
    assert first.data_ptr() != shared.data_ptr()
    kept = first.clone()
    shared.copy_(R.step_inputs(1)[1])
    assert torch.equal(first, kept)
    s.step(shared, s._ts[1], x)
    s.step(shared, s._ts[2], x)
    ring = [t.data_ptr() for t in s.model_outputs]
    assert len(set(ring)) == 3 and s.lower_order_nums == 3
    s.step(shared, s._ts[3], x)
    assert [t.data_ptr() for t in s.model_outputs] == ring[1:] + ring[:1]
    s.set_timesteps(20)
    assert s.model_outputs == [None] * 3 and s.lower_order_nums == 0
    for cls in R.CLASSES:
        s2 = _sched(cls)
        s2.set_timesteps(20 if cls == 'deis' else 19)                            # singlestep: the last index must be a first-order step
        assert 7 not in s2._ts
        fn = mocked.deis_step if cls == 'deis' else mocked.dpm_single_step
        want, _ = fn(x, e, s2.step_coefs(1, 7, 0), order=1)
        assert torch.equal(s2.step(e, 7, x).prev_sample, want)


def test_singlestep_saved_sample_survives_until_it_is_read(mocked):
    """The order-1 step's input is kept by reference (no copy), no later output lands in it, and the order-2 / order-3 steps restart
    from its bits -- not from the sample they are handed."""
    s = _sched('single', solver_order=3, algorithm_type='dpmsolver', solver_type='heun')
    s.set_timesteps(9)
    x0, e0 = R.step_inputs(0)
    keep = x0.clone()
    a = s.step(e0, s._ts[0], x0).prev_sample
    assert s.sample is x0
    b = s.step(R.step_inputs(1)[1], s._ts[1], a).prev_sample
    assert s.sample is x0 and torch.equal(x0, keep)
    c = s.step(R.step_inputs(2)[1], s._ts[2], b).prev_sample
    assert s.sample is x0 and torch.equal(x0, keep)
    outs = [a, b, c] + list(s.model_outputs)
    assert all(t.data_ptr() != x0.data_ptr() for t in outs) and len({t.data_ptr() for t in outs}) == 6
    # the same three steps with garbage handed to steps 2 and 3 as `sample`: an epsilon model under dpmsolver reads only the saved one
    s2 = _sched('single', solver_order=3, algorithm_type='dpmsolver', solver_type='heun')
    s2.set_timesteps(9)
    s2.step(e0, s2._ts[0], x0)
    junk = torch.full_like(x0, 1e9)
    s2.step(R.step_inputs(1)[1], s2._ts[1], junk)
    c2 = s2.step(R.step_inputs(2)[1], s2._ts[2], junk).prev_sample
    assert torch.equal(c, c2)
    d = s.step(R.step_inputs(3)[1], s._ts[3], c).prev_sample                  # the next solver step starts over from ITS input
    assert s.sample is c and d.data_ptr() != c.data_ptr()
    # a step of order 2 without the step it completes
    s3 = _sched('single', solver_order=2)
    s3.set_timesteps(10)
    with pytest.raises(ValueError):
        s3.step(e0, s3._ts[1], x0)


def test_mock_steps_allow_the_kernels_aliases(mocked):
    gen = torch.Generator().manual_seed(3)
    x, xs, e, m1, m2 = (torch.randn(3, 37, generator=gen) for _ in range(5))
    cd, cs = R.random_coefs(mocked.DEIS_COEF, 1), R.random_coefs(mocked.DPM_SINGLE_COEF, 2)
    for order in (1, 2, 3):
        for pred in range(3):
            want, want0 = mocked.deis_step(x, e, cd, order=order, pred=pred, m1=m1, m2=m2)
            xc, old = x.clone(), (m2 if order == 3 else m1).clone()
            kw = dict(m1=old if order == 2 else m1, m2=old if order == 3 else m2)
            got, got0 = mocked.deis_step(xc, e, cd, order=order, pred=pred, out=xc, m0_out=old if order > 1 else None, **kw)
            assert got is xc and torch.equal(got, want) and torch.equal(got0, want0)
            for data in (True, False):
                want, want0 = mocked.dpm_single_step(x, e, cs, order=order, pred=pred, data_pred=data, heun=True, xs=xs, m1=m1, m2=m2)
                uc, old = (x if order == 1 else xs).clone(), (m2 if order == 3 else m1).clone()
                kw = dict(m1=old if order == 2 else m1, m2=old if order == 3 else m2)
                got, got0 = mocked.dpm_single_step(uc if order == 1 else x, e, cs, order=order, pred=pred, data_pred=data, heun=True,
                                                   xs=uc, out=uc, m0_out=old if order > 1 else None, **kw)
                assert got is uc and torch.equal(got, want) and torch.equal(got0, want0)


# ------------------------------------------------------------------------------------------------ refusals, configs, directories
def test_refusals_and_rewrites():
    for cls in R.CLASSES:
        for kw in (dict(trained_betas=[0.1, 0.2]), dict(solver_order=4), dict(algorithm_type='sde-dpmsolver'), dict(solver_type='euler'),
                   dict(beta_schedule='sigmoid')):
            with pytest.raises(NotImplementedError):
                _sched(cls, **kw)
        for kw in (dict(solver_order=0), dict(prediction_type='score')):
            with pytest.raises(ValueError):
                _sched(cls, **kw)
        s = _sched(cls)
        s.set_timesteps(10)
        with pytest.raises(NotImplementedError):                                 # a model that predicts a variance too
            s.step(torch.zeros(1, 6, 4, 4), s._ts[0], torch.zeros(1, 3, 4, 4))
    for vt in ('learned', 'learned_range'):
        with pytest.raises(NotImplementedError):
            _sched('single', variance_type=vt)
    assert _sched('single', variance_type='fixed_small').config.variance_type == 'fixed_small'
    for a in ('dpmsolver', 'dpmsolver++', 'deis'):
        assert _sched('deis', algorithm_type=a).config.algorithm_type == 'deis'
    for st in ('midpoint', 'heun', 'bh1', 'bh2', 'logrho'):
        assert _sched('deis', solver_type=st).config.solver_type == 'logrho'
    assert _sched('single', algorithm_type='deis').config.algorithm_type == 'dpmsolver++'
    for st in ('logrho', 'bh1', 'bh2'):
        assert _sched('single', solver_type=st).config.solver_type == 'midpoint'
    assert _sched('single', solver_type='heun', algorithm_type='dpmsolver').config.solver_type == 'heun'


def test_singlestep_ignores_thresholding_under_dpmsolver(mocked):
    s = _sched('single', algorithm_type='dpmsolver', thresholding=True, sample_max_value=2.0)
    s.set_timesteps(10)
    x, e = R.step_inputs(0)
    s.step(e, s._ts[0], x)
    assert [c[0] for c in mocked.calls] == ['dpm_single_step'] and mocked.calls[0][5] is False


@pytest.mark.parametrize('cls', list(R.CLASSES))
def test_config_keys_equal_the_signature_and_the_config(cls):
    c = _cls(cls)
    params = [p for p in inspect.signature(c.__init__).parameters if p != 'self']
    assert tuple(params) == c._CONFIG_KEYS == tuple(vars(c().config))
    d = inspect.signature(c.__init__).parameters
    assert d['solver_order'].default == 2 and d['prediction_type'].default == 'epsilon' and d['thresholding'].default is False
    assert d['dynamic_thresholding_ratio'].default == 0.995 and d['sample_max_value'].default == 1.0 and d['lower_order_final'].default is True
    if cls == 'deis':
        assert (d['algorithm_type'].default, d['solver_type'].default) == ('deis', 'logrho') and len(params) == 13
    else:
        assert (d['algorithm_type'].default, d['solver_type'].default) == ('dpmsolver++', 'midpoint') and len(params) == 15
        assert d['lambda_min_clipped'].default == -float('inf') and d['variance_type'].default is None
    a = c(solver_order=3, prediction_type='v_prediction', thresholding=True, sample_max_value=2.0, beta_schedule='scaled_linear')
    b = c.from_config(a.config)
    assert vars(b.config) == vars(a.config)
    assert vars(c.from_config(dict(vars(a.config), skip_type='quad')).config) == vars(a.config)       # foreign keys are dropped


@pytest.mark.parametrize('other', OTHERS)
@pytest.mark.parametrize('cls', list(R.CLASSES))
def test_from_config_to_and_from_every_other_class(cls, other):
    diffusion = pkg('diffusion')
    oc = getattr(diffusion, other)
    o = oc(beta_schedule='scaled_linear', beta_start=0.0015, beta_end=0.0195)
    mine = _cls(cls).from_config(o.config)
    assert type(mine) is _cls(cls) and mine.config.beta_schedule == 'scaled_linear' and mine.config.beta_end == 0.0195
    assert mine.config.algorithm_type == ('deis' if cls == 'deis' else 'dpmsolver++')
    assert mine.config.solver_type == ('logrho' if cls == 'deis' else 'midpoint')
    back = oc.from_config(mine.config)
    assert type(back) is oc and back.config.beta_schedule == 'scaled_linear' and back.config.beta_start == 0.0015
    mine.set_timesteps(10)
    assert len(mine._ts) == 10
    # and between the two new classes
    twin = _cls('single' if cls == 'deis' else 'deis').from_config(mine.config)
    assert twin.config.solver_order == mine.config.solver_order and twin.config.beta_end == 0.0195


def test_deis_from_the_multistep_solvers_config():
    diffusion = pkg('diffusion')
    s = diffusion.DEISMultistepScheduler.from_config(diffusion.DPMSolverMultistepScheduler().config)
    assert type(s) is diffusion.DEISMultistepScheduler and s.config.algorithm_type == 'deis' and s.config.solver_type == 'logrho'


def test_pipelines_keep_the_new_schedulers():
    diffusion = pkg('diffusion')
    unet = pkg('unet').UNet2DModel(**gc.TINY_CFG)
    for cls in R.CLASSES:
        assert type(diffusion.DDPMPipeline(unet, _sched(cls)).scheduler) is _cls(cls)
        assert type(diffusion.LDMPipeline(None, unet, _sched(cls)).scheduler) is _cls(cls)


@pytest.mark.parametrize('cls,kw', [('deis', dict()), ('single', dict()),
                                    ('deis', dict(solver_order=3, prediction_type='v_prediction', thresholding=True, sample_max_value=2.0,
                                                  beta_schedule='squaredcos_cap_v2', lower_order_final=False)),
                                    ('single', dict(algorithm_type='dpmsolver', solver_type='heun', solver_order=3, lambda_min_clipped=-5.1,
                                                    beta_schedule='squaredcos_cap_v2', lower_order_final=False, prediction_type='sample'))],
                         ids=['deis-defaults', 'single-defaults', 'deis-changed', 'single-changed'])
def test_pipeline_directory_round_trip(cls, kw, tmp_path):
    diffusion = pkg('diffusion')
    unet = pkg('unet').UNet2DModel(**gc.TINY_CFG)
    gc.det_init_(unet, 5)
    pipe = diffusion.DDPMPipeline(unet, _sched(cls, **kw))
    d = str(tmp_path / 'pipe')
    pipe.save_pretrained(d)
    with open(os.path.join(d, 'model_index.json')) as f:
        assert json.load(f)['scheduler'] == ['diffusers', R.CLASSES[cls]]      # before these classes: NotImplementedError('scheduler class ...')
    with open(os.path.join(d, 'scheduler', 'scheduler_config.json')) as f:
        stored = json.load(f)
    assert stored['_class_name'] == R.CLASSES[cls]
    assert {k: v for k, v in stored.items() if not k.startswith('_')} == vars(pipe.scheduler.config)
    back = diffusion.DDPMPipeline.from_pretrained(d)
    assert type(back.scheduler) is _cls(cls) and vars(back.scheduler.config) == vars(pipe.scheduler.config)
    back.scheduler.set_timesteps(20)
    pipe.scheduler.set_timesteps(20)
    assert back.scheduler._ts == pipe.scheduler._ts
    alone = _cls(cls).from_pretrained(d, subfolder='scheduler')
    assert vars(alone.config) == vars(pipe.scheduler.config)
    sd, sb = pipe.unet.state_dict(), back.unet.state_dict()
    assert list(sd) == list(sb) and all(torch.equal(sd[k], sb[k]) for k in sd)


def test_add_noise_goes_through_the_existing_op(monkeypatch):
    seen = []
    fake = type('Ops', (), {'add_noise': staticmethod(lambda x, n, acp, t: seen.append((acp, t)) or x)})
    monkeypatch.setattr(pkg('diffusion'), 'ops', fake)
    for cls in R.CLASSES:
        s = _sched(cls)
        with pytest.raises(RuntimeError):                                        # host tensors: no fall-back
            s.add_noise(torch.zeros(1, 3, 4, 4), torch.zeros(1, 3, 4, 4), torch.tensor([1]))
    assert seen == []
