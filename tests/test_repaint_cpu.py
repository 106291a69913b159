"""RePaintScheduler and RePaintPipeline on the host (`-m "not gpu"`): diffusion.RePaintScheduler over the CPU stand-in of its two
kernels (tests/mock_ops_repaint.py, the kernels' operation order in fp32 torch) against the fixtures that
tests/golden/make_golden_repaint.py recorded from the reference's own scheduler and pipeline: the timestep tables entry for entry,
every stored step, undo step and toy-model pipeline chain bit for bit against the reference's fp32 run (the chains also prove that the
generator is consumed as the reference consumes it); the signed zero of the unknown part; `eta` as an attribute; the refusals; the
pipeline directory round trip; the preprocessors; and the launch-site table of csrc/repaint.hip."""
import ctypes
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

import golden_common as gc
import repaint_ref as R
from helpers import pkg

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture()
def mocked(monkeypatch):
    import mock_ops_repaint as mock
    monkeypatch.setattr(pkg('diffusion'), 'ops', mock)
    del mock.calls[:]
    return mock


@pytest.fixture(scope='module')
def steps():
    return R.load(R.STEPS_FILE)


@pytest.fixture(scope='module')
def tables():
    return R.load(R.TABLES_FILE)


def _sched(**kw):
    return pkg('diffusion').RePaintScheduler(**kw)


# ------------------------------------------------------------------------------------------------ the fixture and the launch-site table
def test_fixture_covers_what_it_must(steps, tables):
    assert R.TABLE_CASES == [(10, 3, 2), (8, 2, 3), (6, 1, 2), (4, 10, 10), (250, 10, 10), (1000, 10, 10), (2000, 10, 10), (1, 1, 1)]
    assert all(len(tables[R.table_name(c)]) == n for c, n in R.TABLE_LENGTHS.items()) and len(R.TABLE_LENGTHS) == 6
    assert R.TABLE_LENGTHS[(250, 10, 10)] == 4570 and R.TABLE_LENGTHS[(1000, 10, 10)] == 18820
    names = [c[0] for c in R.STEP_CASES]
    assert len(set(names)) == len(names) == 105 and R.STEP_SHAPE == (2, 3, 5, 7)
    # every eta x clip x timestep x mask form
    assert {(c[3], c[1]['clip_sample'], c[4], c[5]) for c in R.STEP_CASES[:90]} == {
        (eta, clip, t, form) for eta in (0.0, 0.5, 1.0) for clip in (True, False) for t in (900, 500, 0) for form in R.MASK_FORMS}
    assert R.MASK_FORMS == ('full', 'B1HW', '11HW', '1CHW', '1HW')
    for name in names:
        key = 'step:' + name
        assert steps[key + ':prev32'].dtype == np.float32 and steps[key + ':prev64'].dtype == np.float64
        assert steps[key + ':x0_32'].shape == steps[key + ':prev64'].shape == R.STEP_SHAPE and steps[key + ':coefs'].shape == (6,)
        assert float(steps[key + ':e_ref32']) == float(np.abs(steps[key + ':prev32'].astype(np.float64) - steps[key + ':prev64']).max())
        assert float(steps[key + ':e_ref32_x0']) == float(np.abs(steps[key + ':x0_32'].astype(np.float64) - steps[key + ':x0_64']).max())
    assert [1000 // n for n, _ in R.UNDO_CASES] == list(R.UNDO_N) == [1, 4, 9, 100]
    for case, n in zip(R.UNDO_CASES, R.UNDO_N):
        assert steps[R.undo_name(case) + ':coefs'].shape == (n, 2) and steps[R.undo_name(case) + ':out64'].dtype == np.float64
    assert [(c[1], c[2]) for c in R.CHAINS] == [((10, 3, 2), 0.0), ((10, 3, 2), 1.0), ((8, 2, 3), 0.5)] and R.CHAIN_B == 2
    toy = R.load(R.TOY_FILE)
    files = [R.TABLES_FILE, R.STEPS_FILE, R.TOY_FILE]
    for name, st, _ in R.CHAINS:
        g = R.load(R.CHAIN_FILE % name)
        files.append(R.CHAIN_FILE % name)
        n = R.TABLE_LENGTHS[st]
        assert g[name + ':xs64'].dtype == np.float64 and g[name + ':xs64'].shape[0] == n + 1 == len(g[name + ':gap'])
        assert toy[name + ':xs32'].dtype == np.float32 and toy[name + ':xs32'].shape == (n + 1,) + R.TOY_SHAPE
    for f in files:
        assert os.path.getsize(os.path.join(HERE, 'golden', f)) <= 1 << 20, f


def test_every_launch_site_of_repaint_hip_is_in_its_branch_table():
    """csrc/repaint.hip launches through RP_LAUNCH, a macro of its own with the body of the library's launch macro, and its sites are
    tabled in tests/test_repaint_gpu.py (the discipline of tests/test_pndm_cpu.py): a new site changes the count, a new
    instantiation is in no table, an entry without a case fails -- before a GPU is needed."""
    import test_repaint_gpu as T
    import mock_ops_repaint as mock
    L, ops = pkg('_lib'), pkg('ops')
    csrc = os.path.join(ROOT, 'diff-pruning_amd', 'csrc')
    assert list(T.LAUNCH_SITES) == ['repaint.hip']
    src = open(os.path.join(csrc, 'repaint.hip')).read()
    body = src.replace('#define RP_LAUNCH(', '')
    sites = re.findall(r'\bRP_LAUNCH\((\(repaint_(?:step_kernel<(?:true|false)(?:, (?:true|false)){3}>|undo_kernel<\d>)\))', body)
    assert len(sites) == T.LAUNCH_SITES['repaint.hip'] == body.count('RP_LAUNCH(') == 24, sites
    assert 'DP_' + 'LAUNCH(' not in src
    assert re.search(r'#define RP_LAUNCH\(k, \.\.\.\).*dp_launch_names\[dp_launches\+\+ & \(DP_LAUNCH_RING - 1\)\] = #k;.*'
                     r'hipLaunchKernelGGL\(k, __VA_ARGS__\)', src)
    assert '#pragma clang fp contract(off)' in src and 'fma' not in src.replace('v_fma_f32', '') and '__fdividef' not in src
    assert 'asm' not in src and '__builtin_amdgcn' not in src                      # plain C++ loads and stores only
    assert sorted(sites) == sorted(T.BRANCHES) and len(set(T.BRANCHES)) == len(T.BRANCHES)
    assert all(e in T.CASES for e in T.BRANCHES), sorted(set(T.BRANCHES) - set(T.CASES))
    assert sorted(v for v in T.CASES.values() if v[0] == 'step') == sorted(
        ('step', c, z, f, x0) for c in (False, True) for z in (False, True) for f in (False, True) for x0 in (False, True))
    assert sorted(v for v in T.CASES.values() if v[0] == 'undo') == [('undo', k) for k in range(1, 9)]
    using = {f for f in os.listdir(csrc) if 'RP_LAUNCH(' in open(os.path.join(csrc, f)).read()}
    assert using == {'repaint.hip'}
    assert 'csrc/repaint.hip' in open(os.path.join(ROOT, 'build.sh')).read()
    assert "'csrc/repaint.hip'" in open(os.path.join(ROOT, '__graft_entry__.py')).read()
    hdr = open(os.path.join(ROOT, 'include', 'dp_hip.h')).read()
    assert len(L.SIGNATURES['dp_repaint_step']) == 15 and len(L.SIGNATURES['dp_repaint_undo']) == 6
    assert ('int dp_repaint_step(const float* x, const float* e, const float* z, const float* o, const float* m, long long m_outer,\n'
            '                    long long m_stride, long long m_inner, int clip, int noise, const dp_repaint_coef* coef, float* out,\n'
            '                    float* x0_out, long long n, void* stream);') in hdr
    assert 'int dp_repaint_undo(const float* x, const dp_repaint_undo_coef* coef, int k, float* out, long long n, void* stream);' in hdr
    # the struct of scalars: the header's field order is the binding's, the wrapper's and the stand-in's
    fields = re.search(r'typedef struct dp_repaint_coef \{(.*?)\} dp_repaint_coef;', hdr, re.S).group(1)
    names = [n for line in re.sub(r'/\*.*?\*/', '', fields, flags=re.S).split(';') for n in re.findall(r'\b(?!float\b)([a-z_0-9]+)\b', line)]
    assert tuple(names) == tuple(n for n, _ in L.RepaintCoef._fields_) == ops.REPAINT_COEF == mock.REPAINT_COEF
    assert ctypes.sizeof(L.RepaintCoef) == 4 * len(names) == 24
    undo = re.search(r'typedef struct dp_repaint_undo_coef \{(.*?)\} dp_repaint_undo_coef;', hdr, re.S).group(1)
    assert re.findall(r'(\w+)\[DP_REPAINT_UNDO_MAX\]', undo) == [n for n, _ in L.RepaintUndoCoef._fields_] == ['z', 'a', 'b']
    assert ctypes.sizeof(L.RepaintUndoCoef) == 8 * 8 + 4 * 8 + 4 * 8
    assert int(re.search(r'#define DP_REPAINT_UNDO_MAX (\d+)', hdr).group(1)) == ops.REPAINT_UNDO_MAX == mock.REPAINT_UNDO_MAX == 8
    assert int(re.search(r'#define DP_REPAINT_MAX_BLOCKS (\d+)', hdr).group(1)) == ops.REPAINT_MAX_BLOCKS == T.MAX_BLOCKS
    lib = L.load()
    assert getattr(lib, 'dp_repaint_step') is not None and getattr(lib, 'dp_repaint_undo') is not None


def test_mask_geometry_of_the_wrapper_and_the_stand_in():
    """The three numbers: every form the kernel reads in place gathers what broadcasting gives; the others are the caller's."""
    import mock_ops_repaint as mock
    ops = pkg('ops')
    cases = [((2, 3, 5, 7), f) for f in R.MASK_FORMS] + [((3, 2, 4, 4), f) for f in R.MASK_FORMS] + [((1, 1, 1, 1), f) for f in R.MASK_FORMS]
    for shape, form in cases:
        ms = R.mask_shape(form, shape)
        geo = ops.repaint_mask_geometry(shape, ms)
        assert geo == mock.repaint_mask_geometry(shape, ms) and geo is not None
        outer, stride, inner = geo
        n = int(np.prod(shape))
        assert 1 <= inner <= outer and outer % inner == 0 and stride >= 0
        m = torch.arange(int(np.prod(ms)), dtype=torch.float32).reshape(ms)
        assert torch.equal(mock.mask_values(m, geo, n).reshape(shape), m.expand(shape))
    assert ops.repaint_mask_geometry((2, 3, 5, 7), (2, 3, 5, 7)) == (210, 0, 210)
    assert ops.repaint_mask_geometry((2, 3, 5, 7), (2, 1, 5, 7)) == (105, 35, 35)
    assert ops.repaint_mask_geometry((2, 3, 5, 7), (1, 5, 7)) == ops.repaint_mask_geometry((2, 3, 5, 7), (5, 7)) == (210, 0, 35)
    assert ops.repaint_mask_geometry((2, 3, 5, 7), (1, 3, 5, 7)) == (210, 0, 105)
    assert ops.repaint_mask_geometry((2, 3, 5, 7), (7,)) == (210, 0, 7) and ops.repaint_mask_geometry((2, 3, 5, 7), (1,)) == (210, 0, 1)
    for other in ((2, 3, 1, 7), (1, 3, 1, 1), (2, 3, 5, 1), (1, 3, 5, 1)):
        assert ops.repaint_mask_geometry((2, 3, 5, 7), other) is None and mock.repaint_mask_geometry((2, 3, 5, 7), other) is None
    for bad in ((2, 3, 5, 6), (3, 1, 5, 7), (1, 2, 3, 5, 7)):
        with pytest.raises(AssertionError):
            ops.repaint_mask_geometry((2, 3, 5, 7), bad)


# ------------------------------------------------------------------------------------------------ timestep tables
@pytest.mark.parametrize('case', R.TABLE_CASES, ids=R.table_name)
def test_timestep_tables_equal_the_references(case, tables):
    s = _sched()
    s.set_timesteps(*case)
    want = tables[R.table_name(case)]
    assert s.timesteps.dtype == torch.int64 and s.timesteps.tolist() == want.tolist() == s._ts
    assert s.num_inference_steps == min(case[0], 1000)
    if case in R.TABLE_LENGTHS:
        assert len(s._ts) == R.TABLE_LENGTHS[case]


def test_the_tables_the_issue_lists():
    def ts(*a):
        s = _sched()
        s.set_timesteps(*a)
        return s._ts
    assert [len(ts(*c)) for c in R.TABLE_CASES[:6]] == [28, 32, 16, 4, 4570, 18820]
    assert ts(2000, 10, 10) == ts(1000, 10, 10) and ts(1, 1, 1) == [0] and ts(4, 10, 10) == [750, 500, 250, 0]
    assert ts(250) == ts(250, 10, 10)                                              # the defaults
    d = ts(250)
    assert R.n_model_calls(d) == 2410 and len(d) - R.n_model_calls(d) == 2160       # UNet calls and re-noising calls
    assert ts(6, 1, 2) == [166 * v for v in (5, 4, 5, 4, 3, 4, 3, 2, 3, 2, 1, 2, 1, 0, 1, 0)]      # 1000 // 6 = 166


def test_tables_of_the_constructor():
    diffusion = pkg('diffusion')
    s = _sched()
    assert torch.equal(s.alphas_cumprod, diffusion.DDPMScheduler().alphas_cumprod) and float(s.final_alpha_cumprod) == 1.0
    assert s.init_noise_sigma == 1.0 and s.num_inference_steps is None and s.order == 1 and len(s) == 1000 and s.eta == 0.0
    assert s.timesteps.tolist() == list(range(999, -1, -1))
    x = torch.zeros(2)
    assert s.scale_model_input(x, 5) is x
    with pytest.raises(ValueError):
        s.step(x, 5, x, x, x)                                                      # before set_timesteps
    cos = _sched(beta_schedule='squaredcos_cap_v2')
    assert torch.equal(cos.betas, diffusion.DPMSolverMultistepScheduler(beta_schedule='squaredcos_cap_v2').betas)
    sg = _sched(beta_schedule='sigmoid', beta_start=0.001, beta_end=0.03)
    want = torch.sigmoid(torch.linspace(-6, 6, 1000).double()).float() * (0.03 - 0.001) + 0.001
    assert torch.equal(sg.betas, want) and sg.betas.dtype == torch.float32
    with pytest.raises(NotImplementedError):
        _sched(beta_schedule='nonsense')


# ------------------------------------------------------------------------------------------------ single steps, undo steps: bit for bit
def _differing(c, stored):
    return [n for i, n in enumerate(('sa', 'sb', 'sap', 's1', 'cd', 'sd')) if np.float32(c[n]).tobytes() != stored[i].tobytes()]


@pytest.mark.parametrize('k', range(len(R.STEP_CASES)), ids=[c[0] for c in R.STEP_CASES])
def test_single_steps_equal_the_references_fp32_bits(k, steps, mocked):
    name, kw, n, eta, t, form = R.STEP_CASES[k]
    key = 'step:' + name
    s = _sched(**kw)
    s.set_timesteps(n)
    s.eta = eta                                                                    # as the pipeline sets it
    x, e, o, m = R.step_inputs(k, form)
    kept = [v.clone() for v in (x, e, o, m)]
    assert _differing(s.step_coefs(t), steps[key + ':coefs']) == [], key
    out = s.step(e, torch.tensor(t), x, o, m, generator=R.noise_generator(k))
    assert type(out).__name__ == 'RePaintSchedulerOutput' and out.prev_sample.dtype == torch.float32
    assert len(mocked.calls) == 1 and mocked.calls[0] == ('step', kw.get('clip_sample', True), t > 0 and eta > 0, form == 'full', True, False)
    assert all(torch.equal(a, b) for a, b in zip((x, e, o, m), kept))              # a step writes none of its inputs
    assert np.array_equal(out.prev_sample.numpy(), steps[key + ':prev32']), key
    assert np.array_equal(out.pred_original_sample.numpy(), steps[key + ':x0_32']), key


@pytest.mark.parametrize('k', range(len(R.UNDO_CASES)), ids=[R.undo_name(c) for c in R.UNDO_CASES])
def test_undo_steps_equal_the_references_fp32_bits(k, steps, mocked):
    case = R.UNDO_CASES[k]
    n_inf, t = case
    key = R.undo_name(case)
    s = _sched()
    s.set_timesteps(n_inf)
    x = R.undo_input(k)
    x0 = x.clone()
    c = np.array(s.undo_coefs(t), np.float32)
    assert c.shape == (R.UNDO_N[k], 2) and c.tobytes() == steps[key + ':coefs'].tobytes()
    y = s.undo_step(x, t, generator=R.noise_generator(1000 + k))
    assert torch.equal(x, x0) and np.array_equal(y.numpy(), steps[key + ':out32'])
    n = R.UNDO_N[k]
    assert [c[1] for c in mocked.calls] == [8] * (n // 8) + ([n % 8] if n % 8 else []) and len(mocked.calls) == -(-n // 8)


def test_step_draws_once_per_call_even_where_the_noise_is_not_added(mocked):
    """One randn_tensor draw per `step`, at t == 0 and with eta == 0 too; n separate draws per `undo_step`, in order."""
    s = _sched()
    s.set_timesteps(10)
    x, e, o, m = R.step_inputs(0, 'full')
    for eta, t in ((0.0, 500), (1.0, 0), (0.5, 500)):
        s.eta = eta
        g, ref = torch.Generator().manual_seed(5), torch.Generator().manual_seed(5)
        s.step(e, t, x, o, m, generator=g)
        torch.randn(R.STEP_SHAPE, generator=ref)
        assert torch.equal(g.get_state(), ref.get_state()), (eta, t)
    s.set_timesteps(250)
    g, ref = torch.Generator().manual_seed(6), torch.Generator().manual_seed(6)
    y = s.undo_step(x, 496, generator=g)
    zs = [torch.randn(R.STEP_SHAPE, generator=ref) for _ in range(4)]
    assert torch.equal(g.get_state(), ref.get_state())
    assert torch.equal(y, mocked.repaint_undo(x, zs, s.undo_coefs(496)))


def test_the_unknown_part_turns_a_negative_zero_positive(mocked):
    """Without added noise the reference adds a Python 0 to the unknown part: (a + b) + 0.  Where a + b is -0 the sum is +0, and with
    a mask of 0 the output, 0 * k + 1 * u, keeps that sign: a kernel that skipped the addition would return -0."""
    x, e, o, m, z, c = R.signed_zero_case()
    got, x0 = mocked.repaint_step(x, e, z, o, m, c, clip=False, add_noise=False, x0_out=True)
    assert torch.signbit(x0.flatten()).tolist() == [True, False]                                    # x0 = -0: sap * x0 + cd * e = -0 + -0
    assert torch.signbit(got.flatten()).tolist() == [False, False] and float(got.abs().max()) == 0.0   # ... and (-0) + 0 = +0
    # with added noise the reference adds sd * z instead: a -0 there keeps the sign
    got, _ = mocked.repaint_step(x, e, -z, o, m, dict(c, sd=1.0), clip=False, add_noise=True)
    assert torch.signbit(got.flatten()).tolist() == [True, False]
    a = torch.tensor(-0.0)
    assert bool(torch.signbit(a + a)) and not bool(torch.signbit((a + a) + 0))                     # what torch does with `+ 0`


def test_eta_is_read_from_the_attribute_the_pipeline_sets(mocked):
    s = _sched(eta=0.0)
    s.set_timesteps(10)
    x, e, o, m = R.step_inputs(3, 'full')
    a = s.step(e, 500, x, o, m, generator=torch.Generator().manual_seed(1)).prev_sample
    assert mocked.calls[-1][2] is False and s.step_coefs(500)['sd'] == 0.0
    s.eta = 1.0
    b = s.step(e, 500, x, o, m, generator=torch.Generator().manual_seed(1)).prev_sample
    assert mocked.calls[-1][2] is True and s.step_coefs(500)['sd'] > 0.0 and not torch.equal(a, b)
    assert s.config.eta == 0.0
    want = _sched(eta=1.0)
    want.set_timesteps(10)
    assert torch.equal(b, want.step(e, 500, x, o, m, generator=torch.Generator().manual_seed(1)).prev_sample)


def test_step_forms(mocked):
    """return_dict=False, `out=` (the sample's own buffer included), need_x0=False, a mask the kernel does not index in place."""
    s = _sched()
    s.set_timesteps(10)
    s.eta = 0.5
    x, e, o, m = R.step_inputs(7, 'B1HW')
    g = lambda: torch.Generator().manual_seed(2)                                   # noqa: E731
    want = s.step(e, 500, x, o, m, generator=g())
    r = s.step(e, 500, x, o, m, generator=g(), return_dict=False)
    assert isinstance(r, tuple) and len(r) == 2 and torch.equal(r[0], want.prev_sample) and torch.equal(r[1], want.pred_original_sample)
    xc = x.clone()
    got = s.step(e, 500, xc, o, m, generator=g(), out=xc, need_x0=False)
    assert got.prev_sample is xc and torch.equal(xc, want.prev_sample) and got.pred_original_sample is None
    assert mocked.calls[-1] == ('step', True, True, False, False, True)
    # [B,C,1,W]: expanded once by the scheduler, then read as a full mask
    m2 = (torch.arange(2 * 3 * 7).reshape(2, 3, 1, 7) % 2).float()
    a = s.step(e, 500, x, o, m2, generator=g()).prev_sample
    assert mocked.calls[-1][3] is True and s._mask[0] is m2
    held = s._mask[1]
    b = s.step(e, 500, x, o, m2.expand(2, 3, 5, 7).contiguous(), generator=g()).prev_sample
    assert torch.equal(a, b)
    s.step(e, 500, x, o, m2, generator=g())
    assert s._mask[1] is held                                                      # once per mask


# ------------------------------------------------------------------------------------------------ the pipeline: toy chains, bit for bit
def _spied(sched):
    states = []
    real_step, real_undo = sched.step, sched.undo_step

    def step(model_output, timestep, sample, *a, **k):
        if not states:
            states.append(sample.clone())
        out = real_step(model_output, timestep, sample, *a, **k)
        states.append(out.prev_sample.clone())
        return out

    def undo(sample, timestep, *a, **k):
        out = real_undo(sample, timestep, *a, **k)
        states.append(out.clone())
        return out
    sched.step, sched.undo_step = step, undo
    return states


@pytest.mark.parametrize('chain', R.CHAINS, ids=lambda c: c[0])
def test_toy_pipeline_chains_equal_the_references_fp32_bits(chain, mocked):
    """The whole call -- x_T, one draw per step, n per re-noising step, from one generator -- against the reference pipeline's fp32
    states: equal bits at every state prove the arithmetic, the `t < t_last` logic and the order of the draws."""
    diffusion = pkg('diffusion')
    name, st, eta = chain
    g = R.load(R.TOY_FILE)
    pipe = diffusion.RePaintPipeline(R.ToyUNet(), _sched())
    states = _spied(pipe.scheduler)
    image, mask = R.chain_inputs(R.TOY_SHAPE)
    image0, mask0 = image.clone(), mask.clone()
    images = pipe(image, mask, num_inference_steps=st[0], eta=eta, jump_length=st[1], jump_n_sample=st[2],
                  generator=torch.Generator().manual_seed(R.CHAIN_SEED), output_type='numpy').images
    ts = g[name + ':timesteps'].tolist()
    assert pipe.scheduler._ts == ts and pipe.scheduler.eta == eta and len(states) == len(ts) + 1
    want = g[name + ':xs32']
    for k, x in enumerate(states):
        assert np.array_equal(x.numpy(), want[k]), (name, k)
    assert np.array_equal(images, g[name + ':images'])
    assert torch.equal(image, image0) and torch.equal(mask, mask0)
    kinds = [c[0] for c in mocked.calls]
    per_undo = -(-(1000 // st[0]) // mocked.REPAINT_UNDO_MAX)                        # launches per undo_step: ceil(n / 8)
    assert kinds.count('step') == R.n_model_calls(ts) and kinds.count('undo') == (len(ts) - R.n_model_calls(ts)) * per_undo
    # in place, without the x0 prediction, on the [1, H, W] mask as it lies
    assert all(c[3:] == (False, False, True) for c in mocked.calls if c[0] == 'step') and all(c[2] for c in mocked.calls if c[0] == 'undo')
    # the known region of the result is the original image: the last entry is t = 0 with alpha_prod_t_prev = 1
    known = mask0.expand(R.TOY_SHAPE) == 1
    assert torch.equal(states[-1][known], image0[known]) and not torch.equal(states[-1][~known], image0[~known])


def test_pipeline_call_forms(mocked):
    diffusion = pkg('diffusion')
    pipe = diffusion.RePaintPipeline(R.ToyUNet(), _sched())
    image, mask = R.chain_inputs(R.TOY_SHAPE)
    kw = dict(num_inference_steps=4, jump_length=2, jump_n_sample=2, output_type='numpy')
    with pytest.raises(ValueError, match='generators'):
        pipe(image, mask, generator=[torch.Generator().manual_seed(0)] * 3, **kw)
    # a list of generators: x_T from one generator per image, every later draw from the first
    gens = [torch.Generator().manual_seed(11), torch.Generator().manual_seed(12)]
    states = _spied(pipe.scheduler)
    pipe(image, mask, generator=gens, **kw)
    ref = [torch.Generator().manual_seed(11), torch.Generator().manual_seed(12)]
    assert torch.equal(states[0], torch.cat([torch.randn((1,) + R.TOY_SHAPE[1:], generator=r) for r in ref]))
    assert torch.equal(gens[1].get_state(), ref[1].get_state()) and not torch.equal(gens[0].get_state(), ref[0].get_state())
    r = pipe(image, mask, generator=torch.Generator().manual_seed(1), return_dict=False, **kw)
    assert isinstance(r, tuple) and r[0].shape == (2, 8, 8, 3)
    pil = pipe(image, mask, generator=torch.Generator().manual_seed(1), **dict(kw, output_type='pil')).images
    assert len(pil) == 2 and pil[0].size == (8, 8)
    sig = inspect.signature(diffusion.RePaintPipeline.__call__)
    assert list(sig.parameters)[1:] == ['image', 'mask_image', 'num_inference_steps', 'eta', 'jump_length', 'jump_n_sample', 'generator',
                                        'output_type', 'return_dict']
    assert [sig.parameters[p].default for p in ('num_inference_steps', 'eta', 'jump_length', 'jump_n_sample', 'output_type')] == [
        250, 0.0, 10, 10, 'pil']


def test_preprocessors_equal_the_references(steps):
    diffusion = pkg('diffusion')
    image, mask = R.pre_inputs()
    assert image.size == (37, 45) and mask.size == (70, 70)
    a, b = diffusion._preprocess_image(image), diffusion._preprocess_mask(mask)
    assert np.array_equal(a.numpy(), steps['pre:image']) and tuple(a.shape) == (1, 3, 40, 32) and a.dtype == torch.float32
    assert np.array_equal(b.numpy(), steps['pre:mask']) and tuple(b.shape) == (1, 64, 64) and b.dtype == torch.float32
    t = torch.zeros(1, 3, 8, 8)
    assert diffusion._preprocess_image(t) is t and diffusion._preprocess_mask(t) is t
    assert diffusion._preprocess_image([t, t]).shape == (2, 3, 8, 8) and diffusion._preprocess_mask([t[0], t[0]]).shape == (6, 8, 8)
    assert diffusion._preprocess_image([image, image]).shape == (2, 3, 40, 32) and diffusion._preprocess_mask([mask]).shape == (1, 64, 64)


# ------------------------------------------------------------------------------------------------ refusals, configs, directories
def test_refusals_raise(mocked):
    with pytest.raises(NotImplementedError, match='trained_betas'):
        _sched(trained_betas=[0.1, 0.2])
    s = _sched()
    s.set_timesteps(10)
    z = torch.zeros(1, 3, 4, 4)
    g = torch.Generator().manual_seed(0)
    state = g.get_state()
    with pytest.raises(NotImplementedError, match='variance'):                  # a model that predicts a variance too
        s.step(torch.zeros(1, 6, 4, 4), 500, z, z, z, generator=g)
    assert mocked.calls == [] and torch.equal(g.get_state(), state)
    with pytest.raises(NotImplementedError, match=r'Use `DDPMScheduler.add_noise\(\)` to train for sampling with RePaint.'):
        s.add_noise(z, z, torch.tensor([1]))
    with pytest.raises(AssertionError):                                          # a mask that does not broadcast
        s.step(z, 500, z, z, torch.zeros(1, 3, 4, 5))


def test_config_keys_and_from_config():
    diffusion = pkg('diffusion')
    cls = diffusion.RePaintScheduler
    params = [p for p in inspect.signature(cls.__init__).parameters if p != 'self']
    assert tuple(params) == cls._CONFIG_KEYS == tuple(vars(_sched().config))
    assert cls._CONFIG_KEYS == ('num_train_timesteps', 'beta_start', 'beta_end', 'beta_schedule', 'eta', 'trained_betas', 'clip_sample')
    assert vars(_sched().config) == dict(num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule='linear', eta=0.0,
                                         trained_betas=None, clip_sample=True)
    a = _sched(beta_schedule='sigmoid', eta=0.25, clip_sample=False, num_train_timesteps=500)
    b = cls.from_config(a.config)
    assert vars(b.config) == vars(a.config) and b.eta == 0.25
    assert vars(cls.from_config(dict(vars(a.config), skip_type='quad')).config) == vars(a.config)       # foreign keys are dropped
    c = cls.from_config(diffusion.DDPMScheduler(beta_schedule='scaled_linear', clip_sample=False).config)
    assert c.config.beta_schedule == 'scaled_linear' and c.config.clip_sample is False and c.config.eta == 0.0
    assert list(inspect.signature(cls.step).parameters)[:8] == ['self', 'model_output', 'timestep', 'sample', 'original_image', 'mask',
                                                                 'generator', 'return_dict']
    assert list(inspect.signature(cls.set_timesteps).parameters) == ['self', 'num_inference_steps', 'jump_length', 'jump_n_sample', 'device']
    assert list(inspect.signature(cls.undo_step).parameters)[:4] == ['self', 'sample', 'timestep', 'generator']


@pytest.mark.parametrize('kw', [dict(), dict(beta_schedule='sigmoid', eta=0.75, clip_sample=False, beta_start=0.001, beta_end=0.01,
                                             num_train_timesteps=500)], ids=['defaults', 'all_changed'])
def test_pipeline_directory_round_trip(kw, tmp_path):
    diffusion = pkg('diffusion')
    unet = pkg('unet').UNet2DModel(**gc.TINY_CFG)
    gc.det_init_(unet, 5)
    pipe = diffusion.RePaintPipeline(unet, _sched(**kw))
    d = str(tmp_path / 'pipe')
    pipe.save_pretrained(d)
    with open(os.path.join(d, 'model_index.json')) as f:
        index = json.load(f)
    assert index['scheduler'] == ['diffusers', 'RePaintScheduler'] and index['_class_name'] == 'RePaintPipeline'
    with open(os.path.join(d, 'scheduler', 'scheduler_config.json')) as f:
        stored = json.load(f)
    assert stored['_class_name'] == 'RePaintScheduler'
    assert sorted(k for k in stored if not k.startswith('_')) == sorted(
        ['num_train_timesteps', 'beta_start', 'beta_end', 'beta_schedule', 'eta', 'trained_betas', 'clip_sample'])
    assert {k: v for k, v in stored.items() if not k.startswith('_')} == vars(pipe.scheduler.config) and stored['trained_betas'] is None
    back = diffusion.RePaintPipeline.from_pretrained(d)
    assert type(back) is diffusion.RePaintPipeline and type(back.scheduler) is diffusion.RePaintScheduler
    assert vars(back.scheduler.config) == vars(pipe.scheduler.config) and back.scheduler.eta == kw.get('eta', 0.0)      # eta round-trips
    back.scheduler.set_timesteps(20, 4, 3)
    pipe.scheduler.set_timesteps(20, 4, 3)
    assert back.scheduler._ts == pipe.scheduler._ts and torch.equal(back.scheduler.betas, pipe.scheduler.betas)
    alone = diffusion.RePaintScheduler.from_pretrained(d, subfolder='scheduler')
    assert vars(alone.config) == vars(pipe.scheduler.config)
    sd, sb = pipe.unet.state_dict(), back.unet.state_dict()
    assert list(sd) == list(sb) and all(torch.equal(sd[k], sb[k]) for k in sd)


def test_a_directory_that_names_the_scheduler_no_longer_ends_in_not_implemented(tmp_path):
    """What the issue reports: model_index.json naming RePaintScheduler ended in NotImplementedError('scheduler class RePaintScheduler')."""
    diffusion = pkg('diffusion')
    unet = pkg('unet').UNet2DModel(**gc.TINY_CFG)
    d = str(tmp_path / 'pipe')
    diffusion.DDPMPipeline(unet, diffusion.DDPMScheduler()).save_pretrained(d)
    index = json.load(open(os.path.join(d, 'model_index.json')))
    index['scheduler'] = ['diffusers', 'RePaintScheduler']
    index['_class_name'] = 'RePaintPipeline'
    json.dump(index, open(os.path.join(d, 'model_index.json'), 'w'))
    cfg = dict(_class_name='RePaintScheduler', _diffusers_version='0.17.0.dev0', num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02,
               beta_schedule='linear', eta=0.5, trained_betas=None, clip_sample=True)
    json.dump(cfg, open(os.path.join(d, 'scheduler', 'scheduler_config.json'), 'w'))
    back = diffusion.RePaintPipeline.from_pretrained(d)
    assert type(back.scheduler) is diffusion.RePaintScheduler and back.scheduler.config.eta == 0.5 and back.scheduler.eta == 0.5
