"""DPMSolverMultistepScheduler on the MI355X: dp_dpm_solver_step (csrc/dpm_solver.hip) and diffusion.DPMSolverMultistepScheduler on the
HIP UNet2DModel, against the fixtures the reference wrote (tests/golden/make_golden_dpm_solver.py).

Bounds (none fixed by hand):
  * the kernel equals the stand-in tests/mock_ops_dpm_solver.py bit for bit: both are the same sequence of correctly rounded fp32
    operations (the stand-in runs torch's eager fp32 ops on the device, one rounding each, scalars as 0-d device tensors);
  * a fixture step lies within max(4 e_ref32, 4 * 2^-24 * max|y64|) of the fixture's fp64 result y64, e_ref32 being the reference's
    own fp32 distance stored beside it (the rule of tests/test_ddpm_exp_sampler_gpu.py); bit equality with the reference's fp32
    result is reported beside it;
  * a chain state lies within 10 x the reference fp32 chain's own gap at that state + 1e-5 of the fp64 chain.
Measured on one MI355X (profiles/dpm_solver_gpu_tests.txt holds every value beside its bound): all 50 fixture steps equal the
reference's fp32 result bit for bit (worst error 0.25 of the bound), the chains at most 0.15 of theirs (worst state 2.9e-4 from fp64 at
magnitude 375)."""
import ctypes

import numpy as np
import pytest
import torch

import golden_common as gc
import dpm_solver_ref as R
import mock_ops_dpm_solver as mock
from helpers import make_model, pkg

pytestmark = pytest.mark.gpu
DEV = 'cuda'

# ---- the launch sites of csrc/dpm_solver.hip (tests/test_dpm_solver_cpu.py compares this table with the source)
LAUNCH_SITES = {'dpm_solver.hip': 6}
BRANCHES = ['(dpm_solver_step_kernel<%d, %s>)' % (o, d) for o in (1, 2, 3) for d in ('false', 'true')]
# branch -> (order, data_pred): test_kernel_equals_the_stand_in runs every one of them at every size
CASES = {'(dpm_solver_step_kernel<%d, %s>)' % (o, 'true' if d else 'false'): (o, d) for o in (1, 2, 3) for d in (False, True)}
MAX_BLOCKS = 4096                                  # DP_DPM_SOLVER_MAX_BLOCKS
CAP = MAX_BLOCKS * 256 * 4                         # elements one launch covers without a second grid-stride trip (16-byte path)
SIZES = [1, 3, 4, 5, 255, 1024, 1027, CAP + 1029]


def _branch(order, data_pred):
    return '(dpm_solver_step_kernel<%d, %s>)' % (order, 'true' if data_pred else 'false')


def _launched(lib, before):
    n = lib.dp_launch_count() - before
    arr = (ctypes.c_char_p * 256)()
    k = lib.dp_recent_launches(arr, 256)
    return [arr[i].decode() for i in range(k)][k - n:] if n else []


def _line(report, key, **kw):
    report['dpm_solver/' + key] = kw
    print('dpm_solver/%s %s' % (key, ' '.join('%s=%.3e' % (k, v) if isinstance(v, float) else '%s=%s' % (k, v) for k, v in kw.items())))


def _sched(**kw):
    return pkg('diffusion').DPMSolverMultistepScheduler(**kw)


# ---------------------------------------------------------------------------------------------- kernel against stand-in
@pytest.fixture(scope='module')
def seeded():
    n = SIZES[-1] + 1
    gen = torch.Generator().manual_seed(13)
    return tuple(torch.randn(n, generator=gen).to(DEV) for _ in range(4))


def _scheduler_coefs():
    """{(order, algorithm, solver_type): the scheduler's own fp32 scalars at a middle step of a 20-step table}."""
    out = {}
    for algo in R.ALGOS:
        for stype in ('midpoint', 'heun'):
            s = _sched(algorithm_type=algo, solver_type=stype, solver_order=3)
            s.set_timesteps(20)
            ts = s._ts
            for order in (1, 2, 3):
                out[(order, algo, stype)] = s.step_coefs(order, ts[7], ts[8], ts[6], ts[5])
    return out


@pytest.mark.parametrize('n', SIZES)
def test_kernel_equals_the_stand_in(n, seeded, report):
    """Every order x algorithm x solver type at element offsets 0 (16-byte aligned) and 1 (a scalar head of 3), out of place and with
    x_next aliasing x and m0_out aliasing the oldest history buffer the step reads; one pointer of another alignment (all 4-byte
    accesses); nothing written outside [0, n)."""
    ops, L = pkg('ops'), pkg('_lib')
    lib = L.load()
    coefs = _scheduler_coefs()
    assert len(coefs) == 12
    ran = set()
    for (order, algo, stype), c in sorted(coefs.items()):
        data = algo == 'dpmsolver++'
        for off in (0, 1):
            x, e, m1, m2 = (t[off:off + n] for t in seeded)
            assert x.data_ptr() % 16 == 4 * off
            want, want0 = mock.dpm_solver_step(x, e, c, order=order, data_pred=data, m1=m1, m2=m2)
            buf = torch.full((n + 2,), 7.0, device=DEV)
            buf0 = torch.full((n + 2,), 7.0, device=DEV)
            before = lib.dp_launch_count()
            got, got0 = ops.dpm_solver_step(x, e, c, order=order, data_pred=data, m1=m1, m2=m2, out=buf[off:off + n], m0_out=buf0[off:off + n])
            assert _launched(lib, before) == [_branch(order, data)]
            ran.add(_branch(order, data))
            assert torch.equal(got, want) and torch.equal(got0, want0), (n, order, algo, stype, off)
            for b in (buf, buf0):                                                # nothing written before the start or past the end
                assert float(b[off + n]) == 7.0 and (off == 0 or float(b[0]) == 7.0) and float(b[n + 1]) == 7.0
            # in place: x_next is x, m0_out is the oldest history buffer this step reads
            xc = torch.empty(n + 1, device=DEV)[off:off + n].copy_(x)
            old = torch.empty(n + 1, device=DEV)[off:off + n].copy_(m2 if order == 3 else m1)
            kw = dict(m1=old if order == 2 else m1, m2=old if order == 3 else m2)
            got, got0 = ops.dpm_solver_step(xc, e, c, order=order, data_pred=data, out=xc, m0_out=old if order > 1 else None, **kw)
            assert got is xc and torch.equal(xc, want) and torch.equal(got0, want0), (n, order, algo, stype, off, 'in place')
            assert order == 1 or got0 is old
        # pointers of two alignments: every access is a 4-byte one
        x, e, m1, m2 = (t[:n] for t in seeded)
        want, want0 = mock.dpm_solver_step(x, e, c, order=order, data_pred=data, m1=m1, m2=m2)
        got, got0 = ops.dpm_solver_step(x, e, c, order=order, data_pred=data, m1=m1, m2=m2, out=torch.empty(n + 1, device=DEV)[1:])
        assert torch.equal(got, want) and torch.equal(got0, want0), (n, order, algo, stype, 'two alignments')
    assert ran == set(BRANCHES) == set(CASES)
    _line(report, 'kernel_vs_stand_in/n%d' % n, cases=len(coefs) * 5, differing_elements=0)


def test_the_wrapper_and_the_library_refuse_what_the_kernel_is_not_written_for(seeded):
    ops, L = pkg('ops'), pkg('_lib')
    x, e, m1, m2 = (t[:64].clone() for t in seeded)
    c = R.random_coefs(2)
    for bad in (dict(out=e), dict(m0_out=x), dict(m0_out=e), dict(order=2), dict(order=3, m1=m1), dict(order=2, m1=m1, out=m1),
                dict(order=1, out=x, m0_out=x)):
        kw = dict(order=1)
        kw.update(bad)
        with pytest.raises(AssertionError):
            ops.dpm_solver_step(x, e, c, **kw)
    with pytest.raises(AssertionError):
        ops.dpm_solver_step(x, e.double(), c)
    with pytest.raises(AssertionError):
        ops.dpm_solver_step(x, e[:32], c)
    big = torch.zeros(256, device=DEV)
    lib = L.load()
    before = lib.dp_launch_count()
    for xx, bad in ((x, dict(out=big[8:72], m0_out=big[40:104])),                # the two outputs overlap in part
                    (x, dict(order=2, m1=big[0:64], m0_out=big[4:68])),          # m0_out overlaps the history without being it
                    (big[128:192], dict(out=big[130:194]))):                     # x_next overlaps x without being it
        kw = dict(order=1)
        kw.update(bad)
        with pytest.raises(L.DpHipError) as err:
            ops.dpm_solver_step(xx, e, c, **kw)
        assert err.value.code == 1                                               # hipErrorInvalidValue, before any launch
    assert lib.dp_launch_count() == before


# ---------------------------------------------------------------------------------------------- kernel against reference
@pytest.fixture(scope='module')
def steps():
    return R.load(R.STEPS_FILE)


def test_host_tables_on_this_machine_equal_the_fixtures(steps):
    """The scalars of a step are host arithmetic: on the GPU machine's host too, the tables are the fixture's bit for bit."""
    for sched in ('linear', 'squaredcos_cap_v2'):
        s = _sched(beta_schedule=sched)
        for n in ('alpha_t', 'sigma_t', 'lambda_t'):
            assert np.array_equal(getattr(s, n).numpy(), steps['tables:%s:%s' % (sched, n)]), (sched, n)


@pytest.mark.parametrize('run', R.STEP_RUNS, ids=R.run_name)
def test_scheduler_steps_on_the_reference_single_steps(run, steps, report):
    """The teacher-forced run of the fixture through scheduler.step on the device: step k is handed the seeded x_k, e_k."""
    L = pkg('_lib')
    lib = L.load()
    algo, stype, so, n, at = run
    name = R.run_name(run)
    s = _sched(algorithm_type=algo, solver_type=stype, solver_order=so)
    s.set_timesteps(n)
    assert s._ts == steps[name + ':timesteps'].tolist()
    orders = steps[name + ':orders'].tolist()
    for k in range(max(at) + 1):
        x, e = (t.to(DEV) for t in R.step_inputs(k))
        before = lib.dp_launch_count()
        prev = s.step(e, s._ts[k], x).prev_sample
        assert _launched(lib, before) == [_branch(orders[k], algo == 'dpmsolver++')]
        if k not in at:
            continue
        key = '%s@%d' % (name, k)
        m0 = s.model_outputs[-1]
        e_prev = float(np.abs(prev.double().cpu().numpy() - steps[key + ':prev64']).max())
        e_m0 = float(np.abs(m0.double().cpu().numpy() - steps[key + ':m0_64']).max())
        b_prev = R.single_step_bound(steps[key + ':e_ref32_prev'], steps[key + ':prev64'])
        b_m0 = R.single_step_bound(steps[key + ':e_ref32_m0'], steps[key + ':m0_64'])
        same32 = bool(np.array_equal(prev.cpu().numpy(), steps[key + ':prev32']) and np.array_equal(m0.cpu().numpy(), steps[key + ':m0_32']))
        _line(report, 'step/' + key, order=orders[k], err_prev=e_prev, bound_prev=b_prev, err_m0=e_m0, bound_m0=b_m0, equals_reference_fp32=same32)
        assert e_prev <= b_prev and e_m0 <= b_m0, (key, e_prev, b_prev, e_m0, b_m0)


# ---------------------------------------------------------------------------------------------- no read-back, one launch
def test_step_is_one_launch_and_reads_nothing_back():
    L = pkg('_lib')
    lib = L.load()
    s = _sched(solver_order=3)
    s.set_timesteps(20)
    x, e = (t.to(DEV) for t in R.step_inputs(0))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        for k in range(4):                                                       # orders 1, 2, 3 and a step on a full ring
            before = lib.dp_launch_count()
            x = s.step(e, s._ts[k], x).prev_sample
            assert lib.dp_launch_count() == before + 1
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert torch.isfinite(x).all()


# ---------------------------------------------------------------------------------------------- chains on the HIP UNet
@pytest.fixture(scope='module')
def tiny():
    return make_model(gc.TINY_CFG, R.MODEL_SEED)


@pytest.fixture(scope='module')
def chains():
    return R.load(R.CHAINS_FILE)


def _loop(model, sched, x_T, n, replay):
    sched.set_timesteps(n)
    fwd = model.sampling_forward(tuple(x_T.shape), n, replay=replay)
    assert type(fwd).__name__ == ('_CapturedForward' if replay else '_EagerForward')
    xs = [x_T]
    try:
        with torch.no_grad():
            for t in sched._ts:
                xs.append(sched.step(fwd(xs[-1], t), t, xs[-1]).prev_sample)
    finally:
        fwd.close()
    return xs


@pytest.mark.parametrize('chain', R.CHAINS, ids=lambda c: c[0])
def test_pipeline_chains_on_the_hip_unet_against_the_reference(chain, tiny, chains, report):
    diffusion = pkg('diffusion')
    name, kw, n = chain
    g = chains
    sched = _sched(**kw)
    pipe = diffusion.DDPMPipeline(tiny, sched)
    seen = []
    real = sched.step

    def spy(model_output, timestep, sample, **k):
        out = real(model_output, timestep, sample, **k)
        seen.append((int(timestep), sample, out.prev_sample))
        return out
    sched.step = spy
    try:
        images = pipe(batch_size=R.CHAIN_B, generator=torch.Generator().manual_seed(R.CHAIN_SEED), num_inference_steps=n,
                      output_type='numpy').images
    finally:
        del sched.step
    assert [t for t, _, _ in seen] == g[name + ':timesteps'].tolist() == sched._ts and len(seen) == n
    assert np.array_equal(seen[0][1].cpu().numpy(), g['x_T'])                    # the pipeline draws the fixture's x_T bit for bit
    xs = [seen[0][1]] + [p for _, _, p in seen]
    y64, gaps = g[name + ':xs64'], g[name + ':gap']
    errs = [float(np.abs(t.double().cpu().numpy() - y64[k]).max()) for k, t in enumerate(xs)]
    bounds = [R.CHAIN_FACTOR * float(gaps[k]) + R.CHAIN_FLOOR for k in range(len(xs))]
    _line(report, 'chain/' + name, steps=n, worst_err=max(errs), worst_err_over_bound=max(e / b for e, b in zip(errs, bounds)),
          errs=' '.join('%.1e' % v for v in errs), bounds=' '.join('%.1e' % v for v in bounds))
    assert all(e <= b for e, b in zip(errs, bounds)), (name, errs, bounds)
    want = (xs[-1] / 2 + 0.5).clamp(0, 1).cpu().permute(0, 2, 3, 1).numpy()
    assert np.array_equal(images, want)
    # replayed and eager forwards: the same bits, and the pipeline's
    x_T = torch.from_numpy(g['x_T']).to(DEV)
    replayed, eager = _loop(tiny, _sched(**kw), x_T, n, True), _loop(tiny, _sched(**kw), x_T, n, False)
    for a, b, c in zip(replayed, eager, xs):
        assert torch.equal(a, b) and torch.equal(a, c)


# ---------------------------------------------------------------------------------------------- LDMPipeline
def test_ldm_pipeline_with_the_solver_equals_the_loop_and_decode(tiny):
    import vq_ref
    diffusion, vq, syn = pkg('diffusion'), pkg('vq'), pkg('synthetic')
    vqm = vq.VQModel(**syn.VQ_TINY_CFG)
    vqm.load_state_dict({k: v.float() for k, v in vq_ref.params(syn.VQ_TINY_CFG, 3).items()})
    vqm = vqm.to(DEV).eval()
    kw = dict(solver_order=3, beta_schedule='scaled_linear', beta_start=0.0015, beta_end=0.0195)
    n, B = 6, 2
    pipe = diffusion.LDMPipeline(vqvae=vqm, unet=tiny, scheduler=_sched(**kw))
    images = pipe(batch_size=B, generator=torch.Generator().manual_seed(9), num_inference_steps=n, output_type='numpy').images
    ss = gc.TINY_CFG['sample_size']
    x_T = diffusion.randn_tensor((B, gc.TINY_CFG['in_channels'], ss, ss), generator=torch.Generator().manual_seed(9)).to(DEV)
    lat = _loop(tiny, _sched(**kw), x_T, n, True)[-1]
    with torch.no_grad():
        dec = vqm.decode(lat).sample
    want = (dec / 2 + 0.5).clamp(0, 1).cpu().permute(0, 2, 3, 1).numpy()
    assert images.shape == want.shape and images.shape[0] == B and np.isfinite(images).all()
    assert np.array_equal(images, want) and images.min() != images.max()
