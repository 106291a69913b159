"""UniPCMultistepScheduler on the MI355X: dp_unipc_step (csrc/unipc.hip) and diffusion.UniPCMultistepScheduler on the HIP UNet2DModel,
against the fixtures the reference wrote (tests/golden/make_golden_unipc.py).

Bounds (none fixed by hand):
  * the kernel equals the stand-in tests/mock_ops_unipc.py bit for bit: both are the same sequence of correctly rounded fp32
    operations (the stand-in runs torch's eager fp32 ops on the device, one rounding each, scalars as 0-d device tensors);
  * a fixture step, taken from its recorded entering state, lies within max(4 e_ref32, 4 * 2^-24 * max|y64|) of the fixture's fp64
    result y64, e_ref32 being the reference's own fp32 distance stored beside it (the rule of tests/test_dpm_solver_gpu.py); bit
    equality with the reference's fp32 result is asserted where at most one history difference enters each sum (pc <= 2 and
    pp <= 2) and reported for the third-order steps, whose two-term sums torch.einsum adds in an order of its own;
  * a chain state lies within 10 x the reference fp32 chain's own gap at that state + 1e-5 of the fp64 chain.
profiles/unipc_gpu_tests.txt holds every measured value beside its bound."""
import ctypes

import numpy as np
import pytest
import torch

import golden_common as gc
import unipc_ref as R
import mock_ops_unipc as mock
from helpers import make_model, pkg

pytestmark = pytest.mark.gpu
DEV = 'cuda'

# ---- the launch sites of csrc/unipc.hip (tests/test_unipc_cpu.py compares this table with the source)
LAUNCH_SITES = {'unipc.hip': 24}
# branch -> (pc, pp, predict_x0): test_kernel_equals_the_stand_in runs every one of them at every size
CASES = {'(unipc_step_kernel<%d, %d, %s>)' % (pc, pp, 'true' if d else 'false'): (pc, pp, d)
         for pc in (0, 1, 2, 3) for pp in (1, 2, 3) for d in (False, True)}
BRANCHES = sorted(CASES)
MAX_BLOCKS = 4096                                  # DP_UNIPC_MAX_BLOCKS
CAP = MAX_BLOCKS * 256 * 4                         # elements one launch covers without a second grid-stride trip (16-byte path)
SIZES = [1, 3, 4, 5, 255, 1024, 1027, CAP + 1029]
INVALID = 1                                        # hipErrorInvalidValue


def _branch(pc, pp, x0):
    return '(unipc_step_kernel<%d, %d, %s>)' % (pc, pp, 'true' if x0 else 'false')


def _launched(lib, before):
    n = lib.dp_launch_count() - before
    arr = (ctypes.c_char_p * 256)()
    k = lib.dp_recent_launches(arr, 256)
    return [arr[i].decode() for i in range(k)][k - n:] if n else []


def _line(report, key, **kw):
    report['unipc/' + key] = kw
    print('unipc/%s %s' % (key, ' '.join('%s=%.3e' % (k, v) if isinstance(v, float) else '%s=%s' % (k, v) for k, v in kw.items())))


def _sched(**kw):
    return pkg('diffusion').UniPCMultistepScheduler(**kw)


# ---------------------------------------------------------------------------------------------- kernel against stand-in
@pytest.fixture(scope='module')
def seeded():
    n = SIZES[-1] + 1
    gen = torch.Generator().manual_seed(13)
    return tuple(torch.randn(n, generator=gen).to(DEV) for _ in range(6))          # e, x_pred, x_last, m0, m1, m2


def _scheduler_coefs():
    """{(pc, pp, predict_x0): the scheduler's own fp32 scalars at a middle step of a 20-step table}, the two solver types in turn."""
    out = {}
    for pc, pp, x0 in sorted(CASES.values()):
        s = _sched(solver_type=('bh1', 'bh2')[(pc + pp) % 2], predict_x0=x0, solver_order=3)
        s.set_timesteps(20)
        ts = s._ts
        out[(pc, pp, x0)] = s.step_coefs(pc, pp, ts[7], ts[8], [ts[4], ts[5], ts[6]])
    return out


@pytest.mark.parametrize('n', SIZES)
def test_kernel_equals_the_stand_in(n, seeded, report):
    """Every (pc, pp, predict_x0) instantiation at element offsets 0 (16-byte aligned) and 1 (a scalar head of 3), out of place with
    guard words around every output, and with every allowed alias at once (x_next on x_pred, x_c on x_last, m_new on the oldest
    history buffer the step reads); one pointer of another alignment (all 4-byte accesses); exactly one launch, of the expected
    instantiation."""
    ops, L = pkg('ops'), pkg('_lib')
    lib = L.load()
    coefs = _scheduler_coefs()
    assert len(coefs) == 24
    ran = set()
    for (pc, pp, x0), c in sorted(coefs.items()):
        nh = max(pc, pp - 1)
        kw = dict(pc=pc, pp=pp, predict_x0=x0)
        for off in (0, 1):
            e, x, xl, m0, m1, m2 = (t[off:off + n] for t in seeded)
            assert x.data_ptr() % 16 == 4 * off
            want, want_c, want_m = mock.unipc_step(e, x, c, x_last=xl, hist=[m0, m1, m2], **kw)
            bufs = [torch.full((n + 2,), 7.0, device=DEV) for _ in range(3)]
            before = lib.dp_launch_count()
            got, got_c, got_m = ops.unipc_step(e, x, c, x_last=xl, hist=[m0, m1, m2], out=bufs[0][off:off + n],
                                               x_c=bufs[1][off:off + n], m_new=bufs[2][off:off + n], **kw)
            assert _launched(lib, before) == [_branch(pc, pp, x0)]
            ran.add(_branch(pc, pp, x0))
            assert torch.equal(got, want) and torch.equal(got_m, want_m), (n, pc, pp, x0, off)
            assert (got_c is None and want_c is None) if pc == 0 else torch.equal(got_c, want_c), (n, pc, pp, x0, off)
            if pc == 0:
                assert bool((bufs[1] == 7.0).all())                               # x_c is not written without a corrector
            for b in bufs:                                                       # nothing written before the start or past the end
                assert float(b[off + n]) == 7.0 and (off == 0 or float(b[0]) == 7.0) and float(b[n + 1]) == 7.0
            # in place: every allowed alias at once
            xp, la = (torch.empty(n + 1, device=DEV)[off:off + n].copy_(t) for t in (x, xl))
            hist = [torch.empty(n + 1, device=DEV)[off:off + n].copy_(t) for t in (m0, m1, m2)]
            before = lib.dp_launch_count()
            got, got_c, got_m = ops.unipc_step(e, xp, c, x_last=la, hist=hist, out=xp, x_c=la if pc else None,
                                               m_new=hist[nh - 1] if nh else None, **kw)
            assert _launched(lib, before) == [_branch(pc, pp, x0)]
            assert got is xp and torch.equal(xp, want) and torch.equal(got_m, want_m), (n, pc, pp, x0, off, 'in place')
            assert nh == 0 or got_m is hist[nh - 1]
            assert pc == 0 or (got_c is la and torch.equal(la, want_c)), (n, pc, pp, x0, off, 'in place')
            for j in range(3):                                                   # the history buffers that took no output are unchanged
                assert j == nh - 1 or torch.equal(hist[j], (m0, m1, m2)[j])
        # pointers of two alignments: every access is a 4-byte one
        e, x, xl, m0, m1, m2 = (t[:n] for t in seeded)
        want, want_c, want_m = mock.unipc_step(e, x, c, x_last=xl, hist=[m0, m1, m2], **kw)
        got, got_c, got_m = ops.unipc_step(e, x, c, x_last=xl, hist=[m0, m1, m2], out=torch.empty(n + 1, device=DEV)[1:], **kw)
        assert torch.equal(got, want) and torch.equal(got_m, want_m) and (pc == 0 or torch.equal(got_c, want_c)), (n, pc, pp, x0, 'two alignments')
    assert ran == set(BRANCHES) == set(CASES)
    _line(report, 'kernel_vs_stand_in/n%d' % n, cases=len(coefs) * 5, differing_elements=0)


def test_the_wrapper_and_the_library_refuse_what_the_kernel_is_not_written_for(seeded):
    ops, L = pkg('ops'), pkg('_lib')
    n = 64
    e, x, xl, m0, m1, m2 = (t[:n].clone() for t in seeded)
    c = R.random_coefs(2)
    full = dict(pc=3, pp=3, x_last=xl, hist=[m0, m1, m2])
    for bad in (dict(out=e), dict(out=xl), dict(out=m0), dict(m_new=x), dict(m_new=e), dict(m_new=xl), dict(x_c=x), dict(x_c=e),
                dict(x_c=m1), dict(out=x, m_new=x), dict(hist=[m0, m1]), dict(x_last=None), dict(pc=4), dict(pp=0)):
        kw = dict(full)
        kw.update(bad)
        with pytest.raises(AssertionError):
            ops.unipc_step(e, x, c, **kw)
    with pytest.raises(AssertionError):
        ops.unipc_step(e.double(), x, c)
    with pytest.raises(AssertionError):
        ops.unipc_step(e[:32], x, c)
    # the entry point itself: every disallowed overlap, null pointers and orders out of range return the invalid-value code
    lib = L.load()
    big = torch.zeros(1024, device=DEV)
    out, xc, mn = (torch.empty(n, device=DEV) for _ in range(3))
    good = dict(e=e, x_pred=x, x_last=xl, m0=m0, m1=m1, m2=m2, pc=3, pp=3, m_new=mn, x_c=xc, x_next=out)
    coef = L.UniPCCoef(**c)

    def call(**change):
        a = dict(good)
        a.update(change)

        def p(t):
            return None if t is None else ctypes.c_void_p(t.data_ptr())
        return lib.dp_unipc_step(p(a['e']), p(a['x_pred']), p(a['x_last']), p(a['m0']), p(a['m1']), p(a['m2']), a['pc'], a['pp'], 1,
                                 ctypes.byref(coef), p(a['m_new']), p(a['x_c']), p(a['x_next']), n, None)
    part = dict(x_pred=big[128:192], x_next=big[130:194])
    bad_calls = [dict(x_next=e), dict(x_next=xl), dict(x_next=m0), dict(x_next=m1), dict(x_next=m2), dict(x_next=mn), dict(x_next=xc),
                 dict(m_new=e), dict(m_new=x), dict(m_new=xl), dict(m_new=xc), dict(x_c=e), dict(x_c=x), dict(x_c=m0), dict(x_c=m1),
                 dict(x_c=m2), part, dict(x_last=big[0:64], x_c=big[4:68]), dict(m2=big[256:320], m_new=big[260:324]),
                 dict(m0=big[256:320], m_new=big[252:316]), dict(m_new=big[400:464], x_next=big[432:496]),
                 dict(x_c=big[400:464], x_next=big[463:527]), dict(e=big[600:664], x_c=big[663:727]),
                 dict(e=None), dict(x_pred=None), dict(x_last=None), dict(x_c=None), dict(m_new=None), dict(x_next=None), dict(m0=None),
                 dict(m2=None), dict(pc=4), dict(pc=-1), dict(pp=0), dict(pp=4)]
    torch.cuda.synchronize()
    before = lib.dp_launch_count()
    for change in bad_calls:
        assert call(**change) == INVALID, sorted(change)
    assert lib.dp_launch_count() == before                                       # refused before any launch
    # what an instantiation does not read is not looked at: m_new on a history buffer beyond max(pc, pp - 1), null unused pointers
    assert call(pc=0, pp=1, x_last=None, x_c=None, m0=None, m1=None, m2=None) == 0
    assert call(pc=1, pp=2, m1=None, m2=None) == 0
    assert call(m_new=m2, x_c=xl, x_next=x) == 0                                  # the three allowed aliases
    assert lib.dp_launch_count() == before + 3
    with pytest.raises(L.DpHipError) as err:                                     # through the wrapper: a partial overlap
        ops.unipc_step(e, big[128:192], c, out=big[130:194])
    assert err.value.code == INVALID
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- kernel against reference
@pytest.fixture(scope='module')
def steps():
    return R.load(R.STEPS_FILE)


def test_host_tables_on_this_machine_equal_the_fixtures(steps):
    """The scalars of a step are host arithmetic: on the GPU machine's host too, the tables are the fixture's bit for bit."""
    for sched in R.SCHEDULES:
        s = _sched(beta_schedule=sched)
        for n in ('alpha_t', 'sigma_t', 'lambda_t'):
            assert np.array_equal(getattr(s, n).numpy(), steps['tables:%s:%s' % (sched, n)]), (sched, n)


@pytest.mark.parametrize('run', R.STEP_RUNS, ids=R.run_name)
def test_scheduler_steps_from_the_recorded_states(run, steps, report):
    """Every listed step of the run through scheduler.step on the device, from the state the fixture recorded entering it."""
    L = pkg('_lib')
    lib = L.load()
    name = R.run_name(run)
    for k in run[7]:
        key = '%s@%d' % (name, k)
        s = _sched(**R.run_kwargs(run))
        s.set_timesteps(run[6])
        assert s._ts == steps[name + ':timesteps'].tolist()
        x, e, t = R.place(s, steps, key, device=DEV)
        x0, e0 = x.clone(), e.clone()
        pc, pp = int(steps[key + ':pc']), int(steps[key + ':pp'])
        before = lib.dp_launch_count()
        prev = s.step(e, t, x).prev_sample
        assert _launched(lib, before) == [_branch(pc, pp, run[1])]
        assert torch.equal(x, x0) and torch.equal(e, e0) and s.this_order == pp
        got = dict(prev=prev, last=s.last_sample, m=s.model_outputs[-1])
        same, vals = True, {}
        for what, v in got.items():
            a = v.cpu().numpy()
            y64 = steps['%s:%s64' % (key, what)]
            same = same and bool(np.array_equal(a, steps['%s:%s32' % (key, what)]))
            vals['err_' + what] = float(np.abs(a.astype(np.float64) - y64).max())
            vals['bound_' + what] = R.single_step_bound(steps['%s:e_ref32_%s' % (key, what)], y64)
        _line(report, 'step/' + key, pc=pc, pp=pp, equals_reference_fp32=same, **vals)
        for what in got:
            assert vals['err_' + what] <= vals['bound_' + what], (key, what, vals)
        if pc <= 2 and pp <= 2:
            assert same, key


# ---------------------------------------------------------------------------------------------- no read-back, one launch, no side effects
def test_step_is_one_launch_reads_nothing_back_and_leaves_its_inputs():
    L = pkg('_lib')
    lib = L.load()
    s = _sched(solver_order=3)
    s.set_timesteps(20)
    x, e = (t.to(DEV) for t in R.step_inputs(0))
    e0 = e.clone()
    kept = []
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        for k in range(5):                                                       # (0,1) (1,2) (2,3) and two steps on a full ring
            before = lib.dp_launch_count()
            kept.append((x, x.clone()))
            x = s.step(e, s._ts[k], x).prev_sample
            assert lib.dp_launch_count() == before + 1
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert torch.isfinite(x).all() and torch.equal(e, e0)
    for given, copy in kept:                                                     # no sample handed to `step` was written, then or later
        assert torch.equal(given, copy)


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

    def spy(model_output, timestep, sample, return_dict=True):                    # the scheduler's own signature: no generator
        out = real(model_output, timestep, sample, return_dict=return_dict)
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
def test_ldm_pipeline_on_the_micro_directory_equals_the_loop_written_out():
    diffusion = pkg('diffusion')
    kw = R.micro_scheduler_kwargs(solver_order=3)
    n, B = 6, 2
    pipe = R.micro_pipe(_sched(**kw), device=DEV)
    images = pipe(batch_size=B, generator=torch.Generator().manual_seed(9), num_inference_steps=n, output_type='numpy').images
    ss = pipe.unet.config.sample_size
    x = diffusion.randn_tensor((B, pipe.unet.config.in_channels, ss, ss), generator=torch.Generator().manual_seed(9)).to(DEV)
    s = _sched(**kw)
    s.set_timesteps(n)
    with torch.no_grad():
        for t in s._ts:
            x = s.step(pipe.unet(x, t).sample, t, x).prev_sample
        dec = pipe.vqvae.decode(x).sample
    want = (dec / 2 + 0.5).clamp(0, 1).cpu().permute(0, 2, 3, 1).numpy()
    assert images.shape == want.shape and images.shape[0] == B and np.isfinite(images).all()
    assert np.array_equal(images, want) and images.min() != images.max()
