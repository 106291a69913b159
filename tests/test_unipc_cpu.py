"""UniPCMultistepScheduler on the host (`-m "not gpu"`): diffusion.UniPCMultistepScheduler over the CPU stand-in of its one kernel
(tests/mock_ops_unipc.py, the kernel's operation order in fp32 torch) against the fixtures that tests/golden/make_golden_unipc.py
recorded from the reference's own scheduler: the timestep tables and the three scalar tables entry for entry, the order / corrector
decisions of whole runs, every single step from its recorded entering state -- bit for bit against the reference's fp32 result
where at most one history difference enters each sum (pc <= 2 and pp <= 2; torch.einsum adds the two terms of a third-order sum
in an order of its own), within max(4 e_ref32, 4 * 2^-24 * max|y64|) of the fp64 result otherwise -- the toy-model chains; the
refusals; the directory round trips of both pipelines; and the launch-site table of csrc/unipc.hip."""
import ctypes
import json
import os
import re

import numpy as np
import pytest
import torch

import golden_common as gc
import unipc_ref as R
from helpers import pkg

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture()
def mocked(monkeypatch):
    import mock_ops_unipc as mock
    monkeypatch.setattr(pkg('diffusion'), 'ops', mock)
    del mock.calls[:]
    return mock


@pytest.fixture(scope='module')
def steps():
    return R.load(R.STEPS_FILE)


def _sched(**kw):
    return pkg('diffusion').UniPCMultistepScheduler(**kw)


# ------------------------------------------------------------------------------------------------ the fixture and the launch-site table
def test_fixture_covers_what_it_must(steps):
    """From the stored numbers: every table case, both solver types, predict_x0 on and off, solver_order 1 .. 3, lower_order_final on
    and off, a disable_corrector list, every (pc, pp) pair a run can produce, the duplicate removal, four chains."""
    assert all(R.table_name(c) in steps for c in R.TABLE_CASES)
    assert len(steps[R.table_name(('linear', 1000))]) == 999 and ('linear', 1000) in R.TABLE_CASES
    seen, settings = set(), set()
    for run in R.STEP_RUNS:
        st, x0, so, lof, dc, sched, n, at = run
        name = R.run_name(run)
        dec = [tuple(v) for v in steps[name + ':decisions'].tolist()]
        assert dec == R.decisions(so, n, lof, dc)
        for k in at:
            key = '%s@%d' % (name, k)
            assert (int(steps[key + ':pc']), int(steps[key + ':pp'])) == dec[k]
            seen.add(dec[k])
            settings.add((st, x0, so, lof, bool(dc)))
            assert steps[key + ':prev64'].dtype == np.float64 and steps[key + ':prev32'].shape == R.STEP_SHAPE
    assert seen == R.reachable_pairs() and len(seen) == 10 and (1, 3) not in seen and (3, 1) not in seen
    assert {s[0] for s in settings} == {'bh1', 'bh2'} and {s[1] for s in settings} == {True, False}
    assert {s[2] for s in settings} == {1, 2, 3} and {s[3] for s in settings} == {True, False} and {s[4] for s in settings} == {True, False}
    for f in (R.STEPS_FILE, R.CHAINS_FILE, R.TOY_FILE):
        assert os.path.getsize(os.path.join(HERE, 'golden', f)) <= 1 << 20
    chains = R.load(R.CHAINS_FILE)
    for name, _, n in R.CHAINS:
        assert chains[name + ':xs64'].dtype == np.float64 and chains[name + ':xs64'].shape[0] == n + 1 == len(chains[name + ':gap'])
    assert sorted(R.CHAIN_LOW.values()) == [False, False, True, True]


def test_every_launch_site_of_unipc_hip_is_in_its_branch_table():
    """csrc/unipc.hip launches through UP_LAUNCH, a macro of its own with the body of the library's launch macro, and its sites are
    tabled in tests/test_unipc_gpu.py: a new site changes the count, a new instantiation is in no table, an entry without a case
    fails -- before a GPU is needed.  The file is in both build lists, and its entry point is declared and bound."""
    import test_unipc_gpu as T
    L, ops = pkg('_lib'), pkg('ops')
    csrc = os.path.join(ROOT, 'diff-pruning_amd', 'csrc')
    assert list(T.LAUNCH_SITES) == ['unipc.hip']
    src = open(os.path.join(csrc, 'unipc.hip')).read()
    body = src.replace('#define UP_LAUNCH(', '')
    sites = re.findall(r'\bUP_LAUNCH\((\(unipc_step_kernel<\d, \d, (?:true|false)>\))', body)
    assert len(sites) == T.LAUNCH_SITES['unipc.hip'] == body.count('UP_LAUNCH(') == 24, sites
    assert 'DP_' + 'LAUNCH(' not in src
    assert re.search(r'#define UP_LAUNCH\(k, \.\.\.\).*dp_launch_names\[dp_launches\+\+ & \(DP_LAUNCH_RING - 1\)\] = #k;.*'
                     r'hipLaunchKernelGGL\(k, __VA_ARGS__\)', src)
    assert sorted(sites) == sorted(T.BRANCHES) and len(set(T.BRANCHES)) == len(T.BRANCHES)
    assert all(e in T.CASES for e in T.BRANCHES), sorted(set(T.BRANCHES) - set(T.CASES))
    assert sorted(T.CASES.values()) == sorted((pc, pp, d) for pc in (0, 1, 2, 3) for pp in (1, 2, 3) for d in (False, True))
    using = {f for f in os.listdir(csrc) if 'UP_LAUNCH(' in open(os.path.join(csrc, f)).read()}
    assert using == {'unipc.hip'}
    assert 'csrc/unipc.hip' in open(os.path.join(ROOT, 'build.sh')).read()
    assert "'csrc/unipc.hip'" in open(os.path.join(ROOT, '__graft_entry__.py')).read()
    assert 'asm' not in src and 'atomic' not in src.lower() and 'fp contract(off)' in src
    hdr = open(os.path.join(ROOT, 'include', 'dp_hip.h')).read()
    assert len(L.SIGNATURES['dp_unipc_step']) == 15
    assert ('int dp_unipc_step(const float* e, const float* x_pred, const float* x_last, const float* m0, const float* m1, const float* m2,\n'
            '                  int pc, int pp, int predict_x0, const dp_unipc_coef* coef, float* m_new, float* x_c, float* x_next, long long n,\n'
            '                  void* stream);') in hdr
    # the struct of scalars: the header's field order is the binding's and the wrapper's
    fields = re.search(r'typedef struct dp_unipc_coef \{(.*?)\} dp_unipc_coef;', hdr, re.S).group(1)
    names = [n for line in re.sub(r'/\*.*?\*/', '', fields).split(';') for n in re.findall(r'\b(?!float\b)([A-Za-z_0-9]+)\b', line)]
    assert tuple(names) == tuple(n for n, _ in L.UniPCCoef._fields_) == ops.UNIPC_COEF
    import mock_ops_unipc
    assert mock_ops_unipc.UNIPC_COEF == ops.UNIPC_COEF
    assert ctypes.sizeof(L.UniPCCoef) == 4 * len(names) == 68
    m = re.search(r'#define DP_UNIPC_MAX_BLOCKS (\d+)', hdr)
    assert int(m.group(1)) == ops.UNIPC_MAX_BLOCKS == T.MAX_BLOCKS
    assert getattr(L.load(), 'dp_unipc_step') is not None


# ------------------------------------------------------------------------------------------------ timestep tables, scalar tables
@pytest.mark.parametrize('case', R.TABLE_CASES, ids=R.table_name)
def test_timestep_tables_equal_the_references(case, steps):
    s = _sched(beta_schedule=case[0], solver_order=3)
    s.last_sample, s.lower_order_nums, s.model_outputs = torch.zeros(1), 2, [torch.zeros(1)] * 3
    s.set_timesteps(case[1])
    want = steps[R.table_name(case)]
    assert s.timesteps.dtype == torch.int64 and s.timesteps.tolist() == want.tolist() == s._ts
    assert s.num_inference_steps == len(want) and s.model_outputs == [None] * 3 and s.lower_order_nums == 0 and s.last_sample is None


@pytest.mark.parametrize('sched', R.SCHEDULES)
def test_alpha_sigma_lambda_tables_equal_the_references_bits(sched, steps):
    s = _sched(beta_schedule=sched)
    for n in ('alpha_t', 'sigma_t', 'lambda_t'):
        assert np.array_equal(getattr(s, n).numpy(), steps['tables:%s:%s' % (sched, n)]), n


def test_state_of_the_constructor():
    s = _sched(solver_order=3)
    d = pkg('diffusion').DPMSolverMultistepScheduler()
    assert torch.equal(s.alpha_t, d.alpha_t) and torch.equal(s.sigma_t, d.sigma_t) and torch.equal(s.lambda_t, d.lambda_t)
    assert s.timesteps.dtype == torch.float32 and s.timesteps[0] == 999 and s.timesteps[-1] == 0 and len(s) == 1000
    assert s.init_noise_sigma == 1.0 and s.num_inference_steps is None and s.order == 1
    assert s.model_outputs == [None] * 3 and s.timestep_list == [None] * 3 and s.last_sample is None and s.lower_order_nums == 0
    assert s.predict_x0 is True and s.disable_corrector == [] and s.solver_p is None
    x = torch.zeros(2)
    assert s.scale_model_input(x, 5) is x
    with pytest.raises(ValueError):
        s.step(x, 5, x)


# ------------------------------------------------------------------------------------------------ decisions of whole runs
@pytest.mark.parametrize('run', R.STEP_RUNS, ids=R.run_name)
def test_order_and_corrector_decisions_of_whole_runs_equal_the_references(run, steps, mocked):
    st, x0, so, lof, dc, sched, n, at = run
    name = R.run_name(run)
    s = _sched(**R.run_kwargs(run))
    s.set_timesteps(n)
    assert s._ts == steps[name + ':timesteps'].tolist()
    for k in range(n):
        x, e = R.step_inputs(k)
        s.step(e, s._ts[k], x)
        assert len(mocked.calls) == k + 1                                         # one kernel call per step
    assert [list(c[:2]) for c in mocked.calls] == steps[name + ':decisions'].tolist()
    assert all(c[2] == x0 for c in mocked.calls)


# ------------------------------------------------------------------------------------------------ single steps from the recorded state
def _check_step(key, s, g, out):
    """-> (pc, pp, bit-equal, {what: (err, bound)}) of one fixture step just taken by `s`."""
    pc, pp = int(g[key + ':pc']), int(g[key + ':pp'])
    got = dict(prev=out, last=s.last_sample, m=s.model_outputs[-1])
    same, errs = True, {}
    for what, v in got.items():
        a = v.detach().cpu().numpy()
        same = same and np.array_equal(a, g['%s:%s32' % (key, what)])
        y64 = g['%s:%s64' % (key, what)]
        errs[what] = (float(np.abs(a.astype(np.float64) - y64).max()), R.single_step_bound(g['%s:e_ref32_%s' % (key, what)], y64))
    return pc, pp, same, errs


@pytest.mark.parametrize('key', R.step_case_ids())
def test_single_steps_from_the_recorded_state(key, steps, mocked):
    run = [r for r in R.STEP_RUNS if key.startswith(R.run_name(r) + '@')][0]
    s = _sched(**R.run_kwargs(run))
    s.set_timesteps(run[6])
    x, e, t = R.place(s, steps, key)
    x0, e0 = x.clone(), e.clone()
    out = s.step(e, t, x)
    assert type(out).__name__ == 'SchedulerOutput' and out.prev_sample.dtype == torch.float32
    assert len(mocked.calls) == 1 and torch.equal(x, x0) and torch.equal(e, e0)
    pc, pp, same, errs = _check_step(key, s, steps, out.prev_sample)
    assert mocked.calls[0][:3] == (pc, pp, run[1]) and s.this_order == pp
    for what, (err, bound) in errs.items():
        assert err <= bound, (key, what, err, bound)
    if pc <= 2 and pp <= 2:
        assert same, key                                                          # the reference's fp32 bits


def test_step_forms_and_entry_points(mocked):
    """return_dict=False, a 0-d tensor timestep, a timestep that is not in the table (the reference then takes the last index), a
    captured forward's reused output buffer (the history keeps its own copy), the ring of solver_order buffers written in turn,
    and the corrected sample in a buffer of the scheduler's own that later steps update in place."""
    s = _sched(predict_x0=False, solver_order=3, lower_order_final=False)
    s.set_timesteps(20)
    x, e = R.step_inputs(0)
    shared = e.clone()                                                             # one buffer for every model output
    a = s.step(shared, torch.tensor(s._ts[0]), x, return_dict=False)
    assert isinstance(a, tuple) and len(a) == 1
    first = s.model_outputs[-1]
    assert first is not shared and first.data_ptr() != shared.data_ptr() and torch.equal(first, e)
    assert s.last_sample is x and s.timestep_list == [None, None, 999] and s.this_order == 1     # no corrector: the sample itself
    shared.copy_(R.step_inputs(1)[1])
    assert torch.equal(first, e)                                                   # the history did not move with the buffer
    x1 = a[0].clone()
    s.step(shared, s._ts[1], a[0])
    assert torch.equal(a[0], x1) and s.last_sample is not a[0]                     # the corrected sample is not written over the caller's
    own = s.last_sample
    s.step(shared, s._ts[2], x)
    ring = [t.data_ptr() for t in s.model_outputs]
    assert len(set(ring)) == 3 and s.lower_order_nums == 3 and s.last_sample is own and mocked.calls[-1][4]
    s.step(shared, s._ts[3], x)
    assert [t.data_ptr() for t in s.model_outputs] == ring[1:] + ring[:1] and mocked.calls[-1][5]      # the oldest buffer took the new output
    assert [c[:2] for c in mocked.calls] == [(0, 1), (1, 2), (2, 3), (3, 3)]
    s.set_timesteps(20)
    assert s.model_outputs == [None] * 3 and s.lower_order_nums == 0 and s.last_sample is None
    # unknown timestep -> last index -> prev_timestep 0, no corrector on a fresh scheduler
    s2 = _sched()
    s2.set_timesteps(20)
    assert 7 not in s2._ts
    want, _, _ = mocked.unipc_step(e, x, s2.step_coefs(0, 1, 7, 0, [None, None]), pc=0, pp=1, predict_x0=True)
    assert torch.equal(s2.step(e, 7, x).prev_sample, want)


@pytest.mark.parametrize('chain', R.CHAINS, ids=lambda c: c[0])
def test_toy_chains_against_the_reference(chain, mocked):
    name, kw, n = chain
    g = R.load(R.TOY_FILE)
    s = _sched(**kw)
    s.set_timesteps(n)
    assert s._ts == g[name + ':timesteps'].tolist()
    x = torch.from_numpy(g['x_T'])
    want32, want64, gaps = g[name + ':xs32'], g[name + ':xs64'], g[name + ':gap']
    for k, t in enumerate(s._ts):
        x = s.step(R.toy_model(x, t), t, x).prev_sample
        if R.CHAIN_LOW[name]:
            assert np.array_equal(x.numpy(), want32[k + 1]), (name, k)
        err = float(np.abs(x.double().numpy() - want64[k + 1]).max())
        assert err <= R.CHAIN_FACTOR * float(gaps[k + 1]) + R.CHAIN_FLOOR, (name, k, err, float(gaps[k + 1]))
    assert [list(c[:2]) for c in mocked.calls] == g[name + ':decisions'].tolist()


def test_the_toy_x_T_is_the_pipelines_draw():
    g = R.load(R.TOY_FILE)
    x = pkg('diffusion').randn_tensor(R.TOY_SHAPE, generator=torch.Generator().manual_seed(R.CHAIN_SEED))
    assert np.array_equal(x.numpy(), g['x_T'])


# ------------------------------------------------------------------------------------------------ the stand-in itself
def test_mock_step_allows_the_kernels_aliases(mocked):
    gen = torch.Generator().manual_seed(3)
    e, x, xl, m0, m1, m2 = (torch.randn(37, generator=gen) for _ in range(6))
    c = R.random_coefs(1)
    for pc in (0, 1, 2, 3):
        for pp in (1, 2, 3):
            for x0 in (True, False):
                nh = max(pc, pp - 1)
                want, want_c, want_m = mocked.unipc_step(e, x, c, pc=pc, pp=pp, predict_x0=x0, x_last=xl, hist=[m0, m1, m2])
                assert (want_c is None) == (pc == 0)
                hist = [m0.clone(), m1.clone(), m2.clone()]
                xp, la = x.clone(), xl.clone()
                got, got_c, got_m = mocked.unipc_step(e, xp, c, pc=pc, pp=pp, predict_x0=x0, x_last=la, hist=hist, out=xp,
                                                      x_c=la if pc else None, m_new=hist[nh - 1] if nh else None)
                assert got is xp and torch.equal(got, want) and torch.equal(got_m, want_m)
                assert nh == 0 or got_m is hist[nh - 1]
                assert pc == 0 or (got_c is la and torch.equal(got_c, want_c))


# ------------------------------------------------------------------------------------------------ refusals, configs, directories
def test_refusals_raise_and_name_the_option():
    for kw, word in ((dict(thresholding=True), 'thresholding'), (dict(solver_p=object()), 'solver_p'),
                     (dict(trained_betas=[0.1, 0.2]), 'trained_betas'), (dict(prediction_type='sample'), 'prediction_type'),
                     (dict(prediction_type='v_prediction'), 'prediction_type'), (dict(solver_order=4), 'solver_order'),
                     (dict(solver_type='euler'), 'solver_type'), (dict(beta_schedule='sigmoid'), 'sigmoid')):
        with pytest.raises(NotImplementedError, match=word):
            _sched(**kw)
    s = _sched()
    s.set_timesteps(10)
    with pytest.raises(NotImplementedError, match='channels'):                    # a model that predicts a variance too
        s.step(torch.zeros(1, 6, 4, 4), s._ts[0], torch.zeros(1, 3, 4, 4))


def test_config_keys_rewrites_and_from_config():
    import inspect
    cls = pkg('diffusion').UniPCMultistepScheduler
    params = [p for p in inspect.signature(cls.__init__).parameters if p != 'self']
    assert tuple(params) == cls._CONFIG_KEYS == tuple(vars(_sched().config))
    assert cls._CONFIG_KEYS == ('num_train_timesteps', 'beta_start', 'beta_end', 'beta_schedule', 'trained_betas', 'solver_order',
                                'prediction_type', 'thresholding', 'dynamic_thresholding_ratio', 'sample_max_value', 'predict_x0',
                                'solver_type', 'lower_order_final', 'disable_corrector', 'solver_p')
    assert [p for p in inspect.signature(cls.step).parameters] == ['self', 'model_output', 'timestep', 'sample', 'return_dict']
    s = _sched()
    assert s.config.solver_order == 2 and s.config.predict_x0 is True and s.config.solver_type == 'bh2'
    assert s.config.lower_order_final is True and s.config.disable_corrector == [] and s.config.solver_p is None
    for st in ('midpoint', 'heun', 'logrho'):
        assert _sched(solver_type=st).config.solver_type == 'bh1'
    a = _sched(predict_x0=False, solver_type='bh1', solver_order=3, lower_order_final=False, disable_corrector=[0, 2])
    b = cls.from_config(a.config)
    assert vars(b.config) == vars(a.config) and b.predict_x0 is False and b.disable_corrector == [0, 2]
    assert vars(cls.from_config(dict(vars(a.config), skip_type='quad')).config) == vars(a.config)       # foreign keys are dropped
    # from a DDPM scheduler's config, as a script that swaps the sampler does; from the DPM scheduler's (its solver_type is rewritten)
    diffusion = pkg('diffusion')
    c = cls.from_config(diffusion.DDPMScheduler(beta_schedule='scaled_linear').config)
    assert c.config.beta_schedule == 'scaled_linear' and c.config.solver_order == 2
    assert cls.from_config(diffusion.DPMSolverMultistepScheduler(solver_order=3).config).config.solver_type == 'bh1'
    with pytest.raises(NotImplementedError):                                     # the DPM scheduler's refusal stays
        diffusion.DPMSolverMultistepScheduler(algorithm_type='unipc')


def test_pipelines_take_the_scheduler_and_ddim_still_replaces_it():
    diffusion = pkg('diffusion')
    unet = pkg('unet').UNet2DModel(**gc.TINY_CFG)
    pipe = diffusion.DDPMPipeline(unet, diffusion.DDPMScheduler())
    swapped = diffusion.DDPMPipeline(unet, diffusion.UniPCMultistepScheduler.from_config(pipe.scheduler.config))
    assert type(swapped.scheduler) is diffusion.UniPCMultistepScheduler
    assert type(diffusion.DDIMPipeline(unet, _sched()).scheduler) is diffusion.DDIMScheduler


@pytest.mark.parametrize('kw', [dict(), dict(predict_x0=False, solver_type='bh1', solver_order=3, disable_corrector=[0, 1],
                                             beta_schedule='squaredcos_cap_v2', lower_order_final=False)],
                         ids=['defaults', 'all_changed'])
def test_ddpm_pipeline_directory_round_trip(kw, tmp_path):
    diffusion = pkg('diffusion')
    unet = pkg('unet').UNet2DModel(**gc.TINY_CFG)
    gc.det_init_(unet, 5)
    pipe = diffusion.DDPMPipeline(unet, _sched(**kw))
    d = str(tmp_path / 'pipe')
    pipe.save_pretrained(d)
    with open(os.path.join(d, 'model_index.json')) as f:
        assert json.load(f)['scheduler'] == ['diffusers', 'UniPCMultistepScheduler']
    with open(os.path.join(d, 'scheduler', 'scheduler_config.json')) as f:
        stored = json.load(f)
    assert stored['_class_name'] == 'UniPCMultistepScheduler'
    assert {k: v for k, v in stored.items() if not k.startswith('_')} == vars(pipe.scheduler.config)
    back = diffusion.DDPMPipeline.from_pretrained(d)                              # resolved by name from `diffusion`
    assert type(back.scheduler) is diffusion.UniPCMultistepScheduler and vars(back.scheduler.config) == vars(pipe.scheduler.config)
    back.scheduler.set_timesteps(10)
    pipe.scheduler.set_timesteps(10)
    assert back.scheduler._ts == pipe.scheduler._ts
    alone = diffusion.UniPCMultistepScheduler.from_pretrained(d, subfolder='scheduler')
    assert vars(alone.config) == vars(pipe.scheduler.config)
    sd, sb = pipe.unet.state_dict(), back.unet.state_dict()
    assert list(sd) == list(sb) and all(torch.equal(sd[k], sb[k]) for k in sd)


def test_ldm_pipeline_directory_round_trip(tmp_path):
    """The micro LDM pipeline directory of the fixtures with the scheduler swapped: saved, its model_index.json names the class,
    loaded back with the same config."""
    diffusion = pkg('diffusion')
    pipe = R.micro_pipe(_sched(**R.micro_scheduler_kwargs(solver_order=3, solver_type='bh1')))
    d = str(tmp_path / 'ldm')
    pipe.save_pretrained(d)
    with open(os.path.join(d, 'model_index.json')) as f:
        index = json.load(f)
    assert index['scheduler'] == ['diffusers', 'UniPCMultistepScheduler'] and index['_class_name'] == 'LDMPipeline' and 'vqvae' in index
    back = diffusion.LDMPipeline.from_pretrained(d)
    assert type(back.scheduler) is diffusion.UniPCMultistepScheduler and vars(back.scheduler.config) == vars(pipe.scheduler.config)
    assert back.vqvae is not None and type(back.unet) is type(pipe.unet)


def test_add_noise_goes_through_the_existing_op(monkeypatch):
    seen = []
    fake = type('Ops', (), {'add_noise': staticmethod(lambda x, n, acp, t: seen.append((acp, t)) or x)})
    monkeypatch.setattr(pkg('diffusion'), 'ops', fake)
    s = _sched()
    with pytest.raises(RuntimeError):                                            # host tensors: no fall-back
        s.add_noise(torch.zeros(1, 3, 4, 4), torch.zeros(1, 3, 4, 4), torch.tensor([1]))
    assert seen == []
