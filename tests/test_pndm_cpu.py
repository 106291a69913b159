"""PNDMScheduler on the host (`-m "not gpu"`): diffusion.PNDMScheduler over the CPU stand-in of its one kernel
(tests/mock_ops_pndm.py, the kernel's operation order in fp32 torch) against the fixtures that tests/golden/make_golden_pndm.py
recorded from the reference's own scheduler: the timestep tables entry for entry, every stored step and the toy-model chains bit for
bit against the reference's fp32 run; the counter logic's oddities; the refusals; the pipeline directory round trip; and the
launch-site table of csrc/pndm.hip."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import golden_common as gc
import pndm_ref as R
from helpers import pkg

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture()
def mocked(monkeypatch):
    import mock_ops_pndm as mock
    monkeypatch.setattr(pkg('diffusion'), 'ops', mock)
    del mock.calls[:]
    return mock


@pytest.fixture(scope='module')
def steps():
    return R.load(R.STEPS_FILE)


def _sched(**kw):
    return pkg('diffusion').PNDMScheduler(**kw)


# ------------------------------------------------------------------------------------------------ the fixture and the launch-site table
def test_fixture_covers_what_it_must(steps):
    """From the stored numbers: every table case (the ones the reference refuses recorded as such), every setting at n = 5 and 10, the
    stored calls hitting all nine modes under both prediction types, a negative previous timestep with and without set_alpha_to_one,
    four chains."""
    assert all(R.table_name(c) in steps and R.table_name(c) + ':raises' in steps for c in R.TABLE_CASES)
    assert {c[2] for c in R.TABLE_CASES} == {1, 2, 3, 4, 5, 6, 10, 50, 1000} and len(R.TABLE_CASES) == 36
    raised = [c for c in R.TABLE_CASES if int(steps[R.table_name(c) + ':raises'])]
    assert raised == [(False, off, n) for off in (0, 1) for n in (1, 2, 3)]
    assert [name for name, _ in R.SETTINGS] == ['default', 'skip', 'alpha_one', 'v', 'v_skip', 'scaled_linear_off1']
    seen, negative = set(), set()
    for run in R.STEP_RUNS:
        sname, kw, n, at = run
        name = R.run_name(run)
        modes = [int(v) for v in steps[name + ':modes']]
        assert n in (5, 10) and len(modes) == R.n_calls(kw, n) == len(steps[name + ':timesteps'])
        assert modes == [R.mode_of_call(kw, k) for k in range(len(modes))]
        for k in at:
            key = '%s@%d' % (name, k)
            seen.add((R.MODES[modes[k]], kw.get('prediction_type') == 'v_prediction'))
            assert steps[key + ':prev64'].dtype == np.float64 and steps[key + ':prev32'].dtype == np.float32
            assert steps[key + ':prev32'].shape == R.STEP_SHAPE and steps[key + ':coefs'].shape == (5,)
            assert float(steps[key + ':e_ref32']) == float(np.abs(steps[key + ':prev32'].astype(np.float64) - steps[key + ':prev64']).max())
            if steps[name + ':t_pairs'][k][1] < 0:
                negative.add(sname)
    assert seen == {(m, v) for m in R.MODES for v in (False, True)} == R.stored_coverage() and len(seen) == 18
    assert negative == {name for name, _ in R.SETTINGS}
    assert sorted(n for _, _, n in R.CHAINS) == [5, 10, 10, 10] and [c[0] for c in R.CHAINS] == ['prk10', 'plms10', 'plms10_v', 'prk5']
    for f in (R.STEPS_FILE, R.CHAINS_FILE, R.TOY_FILE):
        assert os.path.getsize(os.path.join(HERE, 'golden', f)) <= 1 << 20
    chains, toy = R.load(R.CHAINS_FILE), R.load(R.TOY_FILE)
    for name, kw, n in R.CHAINS:
        calls = R.n_calls(kw, n)
        assert chains[name + ':xs64'].dtype == np.float64 and chains[name + ':xs64'].shape[0] == calls + 1 == len(chains[name + ':gap'])
        assert toy[name + ':xs32'].dtype == np.float32 and toy[name + ':xs32'].shape == (calls + 1,) + R.TOY_SHAPE


def test_every_launch_site_of_pndm_hip_is_in_its_branch_table():
    """csrc/pndm.hip launches through PN_LAUNCH, a macro of its own with the body of the library's launch macro, and its sites are
    tabled in tests/test_pndm_gpu.py (the discipline of tests/test_dpm_solver_cpu.py): a new site changes the count, a new
    instantiation is in no table, an entry without a case fails -- before a GPU is needed.  The file stays out of the older tables'
    census, which counts the library macro's call text per file; it is in both build lists and declared with its binding."""
    import test_pndm_gpu as T
    L, ops = pkg('_lib'), pkg('ops')
    csrc = os.path.join(ROOT, 'diff-pruning_amd', 'csrc')
    assert list(T.LAUNCH_SITES) == ['pndm.hip']
    src = open(os.path.join(csrc, 'pndm.hip')).read()
    body = src.replace('#define PN_LAUNCH(', '')
    sites = re.findall(r'\bPN_LAUNCH\((\(pndm_step_kernel<DP_PNDM_[A-Z0-9_]+, (?:true|false)>\))', body)
    assert len(sites) == T.LAUNCH_SITES['pndm.hip'] == body.count('PN_LAUNCH(') == 18, sites
    assert 'DP_' + 'LAUNCH(' not in src
    assert re.search(r'#define PN_LAUNCH\(k, \.\.\.\).*dp_launch_names\[dp_launches\+\+ & \(DP_LAUNCH_RING - 1\)\] = #k;.*'
                     r'hipLaunchKernelGGL\(k, __VA_ARGS__\)', src)
    assert '#pragma clang fp contract(off)' in src and 'fma' not in src.replace('v_fma_f32', '') and '__fdividef' not in src
    assert sorted(sites) == sorted(T.BRANCHES) and len(set(T.BRANCHES)) == len(T.BRANCHES)
    assert all(e in T.CASES for e in T.BRANCHES), sorted(set(T.BRANCHES) - set(T.CASES))
    assert sorted(T.CASES.values()) == sorted((m, v) for m in range(9) for v in (False, True))
    using = {f for f in os.listdir(csrc) if 'PN_LAUNCH(' in open(os.path.join(csrc, f)).read()}
    assert using == {'pndm.hip'}
    assert 'csrc/pndm.hip' in open(os.path.join(ROOT, 'build.sh')).read()
    assert "'csrc/pndm.hip'" in open(os.path.join(ROOT, '__graft_entry__.py')).read()
    hdr = open(os.path.join(ROOT, 'include', 'dp_hip.h')).read()
    assert len(L.SIGNATURES['dp_pndm_step']) == 13
    assert ('int dp_pndm_step(const float* x, const float* e, float* acc, const float* h1, const float* h2, const float* h3, int mode, int v_pred,\n'
            '                 const dp_pndm_coef* coef, float* x_next, float* hist_out, long long n, void* stream);') in hdr
    # the struct of scalars: the header's field order is the binding's and the wrapper's
    fields = re.search(r'typedef struct dp_pndm_coef \{(.*?)\} dp_pndm_coef;', hdr, re.S).group(1)
    names = [n for line in re.sub(r'/\*.*?\*/', '', fields, flags=re.S).split(';') for n in re.findall(r'\b(?!float\b)([a-z_0-9]+)\b', line)]
    assert tuple(names) == tuple(n for n, _ in L.PndmCoef._fields_) == ops.PNDM_COEF
    assert ctypes.sizeof(L.PndmCoef) == 4 * len(names) == 32
    # the modes: the header's values are the wrapper's, the stand-in's and the fixture's names in order
    import mock_ops_pndm as mock
    for i, m in enumerate(R.MODES):
        assert int(re.search(r'#define DP_PNDM_%s (\d+)' % m, hdr).group(1)) == getattr(ops, 'PNDM_' + m) == getattr(mock, 'PNDM_' + m) == i
    assert ops.PNDM_MODES == mock.PNDM_MODES and ops.PNDM_COEF == mock.PNDM_COEF and ops.PNDM_FRACTIONS == mock.PNDM_FRACTIONS
    m = re.search(r'#define DP_PNDM_MAX_BLOCKS (\d+)', hdr)
    assert int(m.group(1)) == ops.PNDM_MAX_BLOCKS == T.MAX_BLOCKS
    assert getattr(L.load(), 'dp_pndm_step') is not None


# ------------------------------------------------------------------------------------------------ timestep tables
@pytest.mark.parametrize('case', R.TABLE_CASES, ids=R.table_name)
def test_timestep_tables_equal_the_references(case, steps):
    s = _sched(**R.table_kwargs(case))
    name = R.table_name(case)
    if int(steps[name + ':raises']):
        with pytest.raises(ValueError, match='at least 4'):
            s.set_timesteps(case[2])
        assert s.num_inference_steps is None and s.timesteps is None
        return
    s.set_timesteps(case[2])
    want = steps[name]
    assert s.timesteps.dtype == torch.int64 and s.timesteps.tolist() == want.tolist() == s._ts
    assert len(s.prk_timesteps) == int(steps[name + ':n_prk']) == len(s._prk) and len(s.prk_timesteps) + len(s.plms_timesteps) == len(want)
    assert s.num_inference_steps == case[2] and s.ets == [] and s.counter == 0 and s.cur_sample is None


def test_the_tables_the_issue_lists(steps):
    def ts(n, **kw):
        s = _sched(**kw)
        s.set_timesteps(n)
        return s._ts
    assert len(ts(5)) == 14 and ts(5)[:6] == [800, 700, 700, 600, 600, 500] and ts(5)[-3:] == [200, 200, 0]
    assert len(ts(4)) == 13 and len(ts(1000)) == 1009
    assert ts(1, skip_prk_steps=True) == [0] and ts(2, skip_prk_steps=True) == [500, 0, 0]
    assert ts(10, skip_prk_steps=True) == [900, 800, 800, 700, 600, 500, 400, 300, 200, 100, 0]
    for n in (1, 2, 3):
        with pytest.raises(ValueError):
            ts(n)


def test_tables_of_the_constructor():
    diffusion = pkg('diffusion')
    s = _sched()
    assert torch.equal(s.alphas_cumprod, diffusion.DDPMScheduler().alphas_cumprod)
    assert torch.equal(s.final_alpha_cumprod, s.alphas_cumprod[0]) and float(_sched(set_alpha_to_one=True).final_alpha_cumprod) == 1.0
    assert s.init_noise_sigma == 1.0 and s.num_inference_steps is None and s.order == 1 and len(s) == 1000 and s.pndm_order == 4
    assert s.timesteps is None and s.prk_timesteps is None and s.plms_timesteps is None and s._timesteps.tolist() == list(range(999, -1, -1))
    x = torch.zeros(2)
    assert s.scale_model_input(x, 5) is x
    with pytest.raises(ValueError):
        s.step(x, 5, x)                                                          # before set_timesteps
    cos = _sched(beta_schedule='squaredcos_cap_v2')
    assert torch.equal(cos.betas, diffusion.DPMSolverMultistepScheduler(beta_schedule='squaredcos_cap_v2').betas)
    sl = _sched(beta_schedule='scaled_linear', beta_start=0.00085, beta_end=0.012)
    assert torch.equal(sl.betas, torch.linspace(0.00085 ** 0.5, 0.012 ** 0.5, 1000, dtype=torch.float32) ** 2)


# ------------------------------------------------------------------------------------------------ single steps, chains: bit for bit
def _coef_bits(c, stored, v_pred):
    names = ('sa', 'sb', 'sc', 'd', 'den') if v_pred else ('sc', 'd', 'den')
    assert sorted(c) == sorted(names)
    return [n for n in names if np.float32(c[n]).tobytes() != stored[('sa', 'sb', 'sc', 'd', 'den').index(n)].tobytes()]


@pytest.mark.parametrize('run', R.STEP_RUNS, ids=R.run_name)
def test_single_steps_equal_the_references_fp32_bits(run, steps, mocked):
    sname, kw, n, at = run
    name = R.run_name(run)
    v = kw.get('prediction_type') == 'v_prediction'
    s = _sched(**kw)
    s.set_timesteps(n)
    assert s._ts == steps[name + ':timesteps'].tolist()
    for k in range(len(s._ts)):
        x, e = R.step_inputs(k)
        x0, e0 = x.clone(), e.clone()
        before = len(mocked.calls)
        out = s.step(e, s._ts[k], x)
        assert len(mocked.calls) == before + 1                                   # one kernel call per step
        assert type(out).__name__ == 'SchedulerOutput' and out.prev_sample.dtype == torch.float32
        assert torch.equal(x, x0) and torch.equal(e, e0)                         # a step writes none of its inputs
        if k in at:
            key = '%s@%d' % (name, k)
            t, prev_t = (int(q) for q in steps[name + ':t_pairs'][k])
            assert _coef_bits(s.step_coefs(t, prev_t), steps[key + ':coefs'], v) == [], key
            assert np.array_equal(out.prev_sample.numpy(), steps[key + ':prev32']), key
    assert [c[0] for c in mocked.calls] == steps[name + ':modes'].tolist()
    assert all(c[1] == v for c in mocked.calls) and s.counter == len(s._ts) and len(s.ets) <= 4


@pytest.mark.parametrize('chain', R.CHAINS, ids=lambda c: c[0])
def test_toy_chains_equal_the_references_fp32_bits(chain, mocked):
    name, kw, n = chain
    g = R.load(R.TOY_FILE)
    s = _sched(**kw)
    s.set_timesteps(n)
    assert s._ts == g[name + ':timesteps'].tolist()
    x = torch.from_numpy(g['x_T'])
    want = g[name + ':xs32']
    for k, t in enumerate(s._ts):
        x = s.step(R.toy_model(x, t), t, x).prev_sample
        assert np.array_equal(x.numpy(), want[k + 1]), (name, k)
    assert len(mocked.calls) == R.n_calls(kw, n)


def test_the_toy_x_T_is_the_pipelines_draw():
    g = R.load(R.TOY_FILE)
    x = pkg('diffusion').randn_tensor(R.TOY_SHAPE, generator=torch.Generator().manual_seed(R.CHAIN_SEED))
    assert np.array_equal(x.numpy(), g['x_T'])


# ------------------------------------------------------------------------------------------------ the counter logic's oddities
def test_prk_stages_1_to_3_ignore_the_sample_they_are_handed(mocked):
    a, b = _sched(), _sched()
    a.set_timesteps(10)
    b.set_timesteps(10)
    junk = torch.full(R.STEP_SHAPE, 1e3)
    for k in range(8):
        x, e = R.step_inputs(k)
        pa = a.step(e, a._ts[k], x).prev_sample
        pb = b.step(e, b._ts[k], x if k % 4 == 0 else junk).prev_sample
        assert torch.equal(pa, pb), k
        if k % 4 == 0:
            assert a.cur_sample is x                                             # held by reference, as the reference holds it
    # ... and stage 0 does not
    x, e = R.step_inputs(8)
    assert not torch.equal(a.step(e, a._ts[8], x).prev_sample, b.step(e, b._ts[8], junk).prev_sample)


def test_the_second_plms_call_shifts_its_timesteps_and_restores_cur_sample(mocked):
    s = _sched(skip_prk_steps=True)
    s.set_timesteps(10)
    assert s._ts[:3] == [900, 800, 800]
    x0, e0 = R.step_inputs(0)
    x1, e1 = R.step_inputs(1)
    s.step(e0, 900, x0)
    assert s.cur_sample is x0 and len(s.ets) == 1 and torch.equal(s.ets[0], e0) and s.ets[0] is not e0
    got = s.step(e1, 800, x1).prev_sample
    assert s.cur_sample is None and len(s.ets) == 1 and torch.equal(s.ets[0], e0)          # e1 is not appended
    want, none = mocked.pndm_step(x0, e1, s.step_coefs(900, 800), mocked.PNDM_PLMS_AVG, hist=[e0])     # from x0, with t = 900 -> 800
    assert none is None and torch.equal(got, want)
    assert [c[0] for c in mocked.calls[:2]] == [mocked.PNDM_PLMS1, mocked.PNDM_PLMS_AVG]


def test_negative_previous_timestep_selects_final_alpha_cumprod():
    for one in (False, True):
        s = _sched(set_alpha_to_one=one)
        s.set_timesteps(10)
        a_t = s.alphas_cumprod[0]
        a_prev = torch.tensor(1.0) if one else s.alphas_cumprod[0]
        c = s.step_coefs(0, -100)
        assert c['d'] == float(a_prev - a_t) and sorted(c) == ['d', 'den', 'sc']
        assert c['sc'] == float(torch.sqrt((a_prev / a_t).double()).float())
    # the v-conversion's two square roots: correctly rounded
    s = _sched(prediction_type='v_prediction')
    c = s.step_coefs(500, 400)
    a = s.alphas_cumprod[500]
    assert c['sa'] == float(torch.sqrt(a.double()).float()) and c['sb'] == float(torch.sqrt((1 - a).double()).float())
    assert c['den'] == float(a * torch.sqrt((1 - s.alphas_cumprod[400]).double()).float()
                             + torch.sqrt((a * (1 - a) * s.alphas_cumprod[400]).double()).float())


def test_plms_before_three_history_entries_raises(mocked):
    s = _sched()
    s.set_timesteps(10)
    s.counter = 12                                                                 # past prk_timesteps with an empty history
    x, e = R.step_inputs(0)
    with pytest.raises(ValueError, match='prk'):
        s.step(e, 600, x)
    assert mocked.calls == []


def test_prk0_turns_a_negative_zero_positive(mocked):
    """The reference's first accumulation is 0 + (1/6) e on a Python 0: the accumulator of a -0.0 output has a clear sign bit."""
    e = torch.tensor([-0.0, 0.0, -1.0, 3.0]).reshape(1, 1, 2, 2)
    x = torch.ones(1, 1, 2, 2)
    s = _sched()
    s.set_timesteps(10)
    s.step(e, s._ts[0], x)
    acc = s._acc.flatten()
    assert not bool(torch.signbit(acc[0])) and not bool(torch.signbit(acc[1])) and float(acc[0]) == 0.0
    assert float(acc[2]) == -float(np.float32(1 / 6)) and float(acc[3]) == float(np.float32(np.float32(1 / 6) * np.float32(3.0)))
    assert bool(torch.signbit(s.ets[0].flatten()[0]))                             # the history keeps e itself
    # what torch does with `0 + 1 / 6 * tensor`
    ref = 0
    ref += 1 / 6 * e
    assert torch.equal(ref, s._acc) and not bool(torch.signbit(ref.flatten()[0]))


def test_step_forms_and_the_ring(mocked):
    """return_dict=False, a 0-d tensor timestep, a captured forward's reused output buffer (the history keeps its own copy), `out=`,
    and the ring: four buffers, written in turn; set_timesteps forgets them."""
    s = _sched()
    s.set_timesteps(10)
    shared = torch.empty(R.STEP_SHAPE)                                             # one buffer for every model output
    x = R.step_inputs(0)[0]
    for k in range(12):
        shared.copy_(R.step_inputs(k)[1])
        r = s.step(shared, torch.tensor(s._ts[k]), x, return_dict=False)
        assert isinstance(r, tuple) and len(r) == 1
        x = r[0]
    assert len(s.ets) == 3 and all(torch.equal(s.ets[i], R.step_inputs(4 * i)[1]) for i in range(3))
    assert all(h.data_ptr() != shared.data_ptr() for h in s.ets)
    seen = []
    for k in range(12, 19):
        shared.copy_(R.step_inputs(k)[1])
        x = s.step(shared, s._ts[k], x).prev_sample
        seen.append([h.data_ptr() for h in s.ets])
    assert len(set(seen[0])) == 4 and all(b == a[1:] + a[:1] for a, b in zip(seen, seen[1:]))       # the oldest buffer took the new output
    assert not any(c[3] for c in mocked.calls)                                     # ... which that step did not read
    # out=: prev_sample goes where the caller says, the sample's own buffer included
    s2 = _sched(skip_prk_steps=True)
    s2.set_timesteps(10)
    x, e = R.step_inputs(0)
    want = _sched(skip_prk_steps=True)
    want.set_timesteps(10)
    w = want.step(e, 900, x).prev_sample
    xc = x.clone()
    got = s2.step(e, 900, xc, out=xc).prev_sample
    assert got is xc and torch.equal(got, w) and mocked.calls[-1][2]
    s.set_timesteps(10)
    assert s.ets == [] and s.counter == 0 and s._acc is None


# ------------------------------------------------------------------------------------------------ the stand-in itself
def test_mock_step_allows_the_kernels_aliases(mocked):
    gen = torch.Generator().manual_seed(3)
    x, e, acc, h1, h2, h3 = (torch.randn(37, generator=gen) for _ in range(6))
    c = R.random_coefs(1)
    for mode, (reads_acc, writes_acc, need, appends) in mocked.PNDM_MODES.items():
        for v in (False, True):
            hist = [h1, h2, h3][:need]
            a0 = acc.clone()
            want, want_h = mocked.pndm_step(x, e, c, mode, v_pred=v, acc=a0, hist=hist)
            assert (want_h is not None) == appends and (not appends or torch.equal(want_h, e))
            assert writes_acc or torch.equal(a0, acc)
            # out is x; hist_out is the oldest entry the step reads (h3 in PLMS4, while it is being read); acc in place
            xc, a1 = x.clone(), acc.clone()
            hc = [h.clone() for h in hist]
            got, got_h = mocked.pndm_step(xc, e, c, mode, v_pred=v, acc=a1, hist=hc, out=xc, hist_out=hc[-1] if hc and appends else None)
            assert got is xc and torch.equal(got, want) and torch.equal(a1, a0), (mode, v)
            if hc and appends:
                assert got_h is hc[-1] and torch.equal(got_h, e)


# ------------------------------------------------------------------------------------------------ refusals, configs, directories
def test_refusals_raise(mocked):
    with pytest.raises(NotImplementedError):
        _sched(trained_betas=[0.1, 0.2])
    with pytest.raises(NotImplementedError):
        _sched(beta_schedule='sigmoid')
    for pt in ('sample', 'nonsense'):
        s = _sched(prediction_type=pt)                                           # the reference raises in `step`, not before
        s.set_timesteps(10)
        with pytest.raises(ValueError, match='prediction_type'):
            s.step(torch.zeros(1, 3, 4, 4), s._ts[0], torch.zeros(1, 3, 4, 4))
        with pytest.raises(ValueError, match='prediction_type'):
            s.step_coefs(900, 850)
    s = _sched()
    s.set_timesteps(10)
    with pytest.raises(NotImplementedError):                                     # a model that predicts a variance too
        s.step(torch.zeros(1, 6, 4, 4), s._ts[0], torch.zeros(1, 3, 4, 4))
    assert mocked.calls == [] and s.counter == 0


def test_config_keys_and_from_config():
    import inspect
    diffusion = pkg('diffusion')
    cls = diffusion.PNDMScheduler
    params = [p for p in inspect.signature(cls.__init__).parameters if p != 'self']
    assert tuple(params) == cls._CONFIG_KEYS == tuple(vars(_sched().config))
    assert cls._CONFIG_KEYS == ('num_train_timesteps', 'beta_start', 'beta_end', 'beta_schedule', 'trained_betas', 'skip_prk_steps',
                                'set_alpha_to_one', 'prediction_type', 'steps_offset')
    s = _sched()
    assert vars(s.config) == dict(num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule='linear', trained_betas=None,
                                  skip_prk_steps=False, set_alpha_to_one=False, prediction_type='epsilon', steps_offset=0)
    a = _sched(beta_schedule='scaled_linear', skip_prk_steps=True, set_alpha_to_one=True, prediction_type='v_prediction', steps_offset=1)
    b = cls.from_config(a.config)
    assert vars(b.config) == vars(a.config)
    assert vars(cls.from_config(dict(vars(a.config), skip_type='quad')).config) == vars(a.config)       # foreign keys are dropped
    # from a DDIM scheduler's config, as a script that swaps the sampler does
    c = cls.from_config(diffusion.DDIMScheduler(beta_schedule='scaled_linear', steps_offset=1, set_alpha_to_one=False).config)
    assert c.config.beta_schedule == 'scaled_linear' and c.config.steps_offset == 1 and c.config.skip_prk_steps is False
    params = inspect.signature(cls.step).parameters                              # the pipelines' `inspect`: neither generator nor eta
    assert 'generator' not in params and 'eta' not in params and list(params)[:5] == ['self', 'model_output', 'timestep', 'sample', 'return_dict']


def test_pipelines_and_the_scheduler_they_keep():
    diffusion = pkg('diffusion')
    unet = pkg('unet').UNet2DModel(**gc.TINY_CFG)
    assert type(diffusion.DDIMPipeline(unet, _sched()).scheduler) is diffusion.DDIMScheduler        # still replaced by a DDIM one
    mine = _sched(skip_prk_steps=True)
    assert diffusion.DDPMPipeline(unet, mine).scheduler is mine
    p = diffusion.PNDMPipeline(unet, diffusion.DDIMScheduler(beta_schedule='scaled_linear', steps_offset=1))
    assert type(p.scheduler) is diffusion.PNDMScheduler and p.scheduler.config.beta_schedule == 'scaled_linear'
    q = diffusion.PNDMPipeline(unet, mine)
    assert q.scheduler is not mine and vars(q.scheduler.config) == vars(mine.config)                  # re-created from its config


@pytest.mark.parametrize('kw', [dict(), dict(beta_schedule='squaredcos_cap_v2', skip_prk_steps=True, set_alpha_to_one=True,
                                             prediction_type='v_prediction', steps_offset=1, beta_start=0.001, beta_end=0.01,
                                             num_train_timesteps=500)], ids=['defaults', 'all_changed'])
def test_pipeline_directory_round_trip(kw, tmp_path):
    diffusion = pkg('diffusion')
    unet = pkg('unet').UNet2DModel(**gc.TINY_CFG)
    gc.det_init_(unet, 5)
    pipe = diffusion.PNDMPipeline(unet, _sched(**kw))
    d = str(tmp_path / 'pipe')
    pipe.save_pretrained(d)
    with open(os.path.join(d, 'model_index.json')) as f:
        index = json.load(f)
    assert index['scheduler'] == ['diffusers', 'PNDMScheduler'] and index['_class_name'] == 'PNDMPipeline'
    with open(os.path.join(d, 'scheduler', 'scheduler_config.json')) as f:
        stored = json.load(f)
    assert stored['_class_name'] == 'PNDMScheduler'
    # the reference's JSON keys: the arguments of its register_to_config constructor
    assert sorted(k for k in stored if not k.startswith('_')) == sorted(
        ['num_train_timesteps', 'beta_start', 'beta_end', 'beta_schedule', 'trained_betas', 'skip_prk_steps', 'set_alpha_to_one',
         'prediction_type', 'steps_offset'])
    assert {k: v for k, v in stored.items() if not k.startswith('_')} == vars(pipe.scheduler.config) and stored['trained_betas'] is None
    for cls in (diffusion.PNDMPipeline, diffusion.DDPMPipeline):
        back = cls.from_pretrained(d)
        assert type(back) is cls and type(back.scheduler) is diffusion.PNDMScheduler
        assert vars(back.scheduler.config) == vars(pipe.scheduler.config)
    back.scheduler.set_timesteps(20)
    pipe.scheduler.set_timesteps(20)
    assert back.scheduler._ts == pipe.scheduler._ts
    alone = diffusion.PNDMScheduler.from_pretrained(d, subfolder='scheduler')
    assert vars(alone.config) == vars(pipe.scheduler.config)
    sd, sb = pipe.unet.state_dict(), back.unet.state_dict()
    assert list(sd) == list(sb) and all(torch.equal(sd[k], sb[k]) for k in sd)


def test_a_directory_that_names_the_scheduler_no_longer_ends_in_not_implemented(tmp_path):
    """What the issue reports: model_index.json naming PNDMScheduler ended in NotImplementedError('scheduler class PNDMScheduler')."""
    diffusion = pkg('diffusion')
    unet = pkg('unet').UNet2DModel(**gc.TINY_CFG)
    d = str(tmp_path / 'pipe')
    diffusion.DDPMPipeline(unet, diffusion.DDPMScheduler()).save_pretrained(d)
    index = json.load(open(os.path.join(d, 'model_index.json')))
    index['scheduler'] = ['diffusers', 'PNDMScheduler']
    json.dump(index, open(os.path.join(d, 'model_index.json'), 'w'))
    cfg = dict(_class_name='PNDMScheduler', _diffusers_version='0.17.0.dev0', num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02,
               beta_schedule='linear', trained_betas=None, skip_prk_steps=True, set_alpha_to_one=False, prediction_type='epsilon',
               steps_offset=0)
    json.dump(cfg, open(os.path.join(d, 'scheduler', 'scheduler_config.json'), 'w'))
    back = diffusion.DDPMPipeline.from_pretrained(d)
    assert type(back.scheduler) is diffusion.PNDMScheduler and back.scheduler.config.skip_prk_steps is True


def test_add_noise_goes_through_the_existing_op(monkeypatch):
    seen = []
    fake = type('Ops', (), {'add_noise': staticmethod(lambda x, n, acp, t: seen.append((acp, t)) or x)})
    monkeypatch.setattr(pkg('diffusion'), 'ops', fake)
    s = _sched()
    with pytest.raises(RuntimeError):                                            # host tensors: no fall-back
        s.add_noise(torch.zeros(1, 3, 4, 4), torch.zeros(1, 3, 4, 4), torch.tensor([1]))
    assert seen == []
