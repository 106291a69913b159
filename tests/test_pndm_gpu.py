"""PNDMScheduler on the MI355X: dp_pndm_step (csrc/pndm.hip) and diffusion.PNDMScheduler / PNDMPipeline on the HIP UNet2DModel,
against the fixtures the reference wrote (tests/golden/make_golden_pndm.py).

Bounds (none fixed by hand):
  * the kernel equals the stand-in tests/mock_ops_pndm.py bit for bit: both are the same sequence of correctly rounded fp32
    operations (the stand-in runs torch's eager fp32 ops on the device, one rounding each, scalars as 0-d device tensors);
  * a fixture step lies within max(4 e_ref32, 4 * 2^-24 * max|y64|) of the fixture's fp64 result y64, e_ref32 being the reference's
    own fp32 distance stored beside it (the rule of tests/test_dpm_solver_gpu.py), without exclusions; and it equals the
    reference's fp32 result bit for bit -- a step that does not is named in the report with the scalar that differs, and fails;
  * a chain state lies within 10 x the reference fp32 chain's own gap at that state + 1e-5 of the fp64 chain.
Measured on one MI355X (profiles/pndm_gpu_tests.txt holds every value beside its bound): all 104 fixture steps equal the reference's
fp32 result bit for bit with every host scalar equal to the reference's (worst error 0.25 of the bound), the chains at most 0.13 of
theirs (worst state 5.6e-5 from fp64 at magnitude 260)."""
import ctypes

import numpy as np
import pytest
import torch

import golden_common as gc
import pndm_ref as R
import mock_ops_pndm as mock
from helpers import make_model, pkg

pytestmark = pytest.mark.gpu
DEV = 'cuda'

# ---- the launch sites of csrc/pndm.hip (tests/test_pndm_cpu.py compares this table with the source)
LAUNCH_SITES = {'pndm.hip': 18}
BRANCHES = ['(pndm_step_kernel<DP_PNDM_%s, %s>)' % (m, v) for m in R.MODES for v in ('false', 'true')]
# branch -> (mode, v_pred): test_kernel_equals_the_stand_in runs every one of them at every size
CASES = {'(pndm_step_kernel<DP_PNDM_%s, %s>)' % (m, 'true' if v else 'false'): (i, v) for i, m in enumerate(R.MODES) for v in (False, True)}
MAX_BLOCKS = 4096                                  # DP_PNDM_MAX_BLOCKS
CAP = MAX_BLOCKS * 256 * 4                         # elements one launch covers without a second grid-stride trip (16-byte path)
SIZES = [1, 3, 4, 5, 255, 1024, 1027, CAP + 1029]
GUARD = 7.0


def _branch(mode, v_pred):
    return '(pndm_step_kernel<DP_PNDM_%s, %s>)' % (R.MODES[mode], 'true' if v_pred else 'false')


def _launched(lib, before):
    n = lib.dp_launch_count() - before
    arr = (ctypes.c_char_p * 256)()
    k = lib.dp_recent_launches(arr, 256)
    return [arr[i].decode() for i in range(k)][k - n:] if n else []


def _line(report, key, **kw):
    report['pndm/' + key] = kw
    print('pndm/%s %s' % (key, ' '.join('%s=%.3e' % (k, v) if isinstance(v, float) else '%s=%s' % (k, v) for k, v in kw.items())))


def _sched(**kw):
    return pkg('diffusion').PNDMScheduler(**kw)


# ---------------------------------------------------------------------------------------------- kernel against stand-in
@pytest.fixture(scope='module')
def seeded():
    n = SIZES[-1] + 1
    gen = torch.Generator().manual_seed(17)
    return tuple(torch.randn(n, generator=gen).to(DEV) for _ in range(6))           # x, e, acc, h1, h2, h3


def _scheduler_coefs(v_pred):
    """The scheduler's own fp32 scalars at a middle step of a 20-step table."""
    s = _sched(prediction_type='v_prediction' if v_pred else 'epsilon')
    return s.step_coefs(650, 600)


def _guarded(n, off):
    """A view of n elements at element offset `off` inside a buffer of guard words."""
    buf = torch.full((n + 2,), GUARD, device=DEV)
    return buf, buf[off:off + n]


def _guards_intact(buf, n, off):
    return float(buf[off + n]) == GUARD and (off == 0 or float(buf[0]) == GUARD) and float(buf[n + 1]) == GUARD


def _copy_at(t, n, off):
    """A copy of t[:n] whose first element sits at element offset `off` of a fresh allocation, with guard words either side."""
    buf, view = _guarded(n, off)
    view.copy_(t[:n])
    return buf, view


@pytest.mark.parametrize('n', SIZES)
def test_kernel_equals_the_stand_in(n, seeded, report):
    """All 18 instantiations with every pointer 16-byte aligned, with every pointer at element offset 1 (a scalar head of 3) and with
    pointers of two phases (all 4-byte accesses), out of place and under every permitted alias at once (x_next is x, acc in place,
    hist_out is the oldest history entry the step reads); the guard words either side of every output stay untouched, and the
    launch ring names the instantiation that was asked for."""
    ops, L = pkg('ops'), pkg('_lib')
    lib = L.load()
    ran, cases = set(), 0
    for mode, (reads_acc, writes_acc, need, appends) in sorted(ops.PNDM_MODES.items()):
        for v in (False, True):
            c = _scheduler_coefs(v)
            for off in (0, 1):
                x, e, acc, h1, h2, h3 = (t[off:off + n] for t in seeded)
                assert x.data_ptr() % 16 == 4 * off
                hist = [h1, h2, h3][:need]
                acc_want = acc.clone()
                want, want_h = mock.pndm_step(x, e, c, mode, v_pred=v, acc=acc_want, hist=hist)
                # out of place (acc: a guarded copy)
                obuf, out = _guarded(n, off)
                hbuf, hout = _guarded(n, off)
                abuf, a = _copy_at(acc, n, off)
                before = lib.dp_launch_count()
                got, got_h = ops.pndm_step(x, e, c, mode, v_pred=v, acc=a, hist=hist, out=out, hist_out=hout)
                assert _launched(lib, before) == [_branch(mode, v)]
                ran.add(_branch(mode, v))
                assert torch.equal(got, want) and torch.equal(a, acc_want if writes_acc else acc), (n, mode, v, off)
                assert (got_h is None) == (not appends) and (not appends or torch.equal(got_h, e)), (n, mode, v, off)
                assert appends or bool((hout == GUARD).all())                    # a mode that appends nothing leaves hist_out alone
                assert all(_guards_intact(b, n, off) for b in (obuf, hbuf, abuf)), (n, mode, v, off)
                # every permitted alias at once
                xbuf, xc = _copy_at(x, n, off)
                abuf, a = _copy_at(acc, n, off)
                hcopies = [_copy_at(h, n, off) for h in hist]
                hc = [view for _, view in hcopies]
                got, got_h = ops.pndm_step(xc, e, c, mode, v_pred=v, acc=a, hist=hc, out=xc, hist_out=hc[-1] if hc and appends else None)
                assert got is xc and torch.equal(xc, want) and torch.equal(a, acc_want if writes_acc else acc), (n, mode, v, off, 'aliased')
                if hc and appends:
                    assert got_h is hc[-1] and torch.equal(got_h, e)
                    assert all(torch.equal(hv, h) for hv, h in zip(hc[:-1], hist[:-1]))               # the newer entries are not written
                assert all(_guards_intact(b, n, off) for b in [xbuf, abuf] + [b for b, _ in hcopies]), (n, mode, v, off, 'aliased')
                cases += 2
            # pointers of two phases: every access is a 4-byte one
            x, e, acc, h1, h2, h3 = (t[:n] for t in seeded)
            hist = [h1, h2, h3][:need]
            acc_want = acc.clone()
            want, want_h = mock.pndm_step(x, e, c, mode, v_pred=v, acc=acc_want, hist=hist)
            obuf, out = _guarded(n, 1)
            abuf, a = _copy_at(acc, n, 0)
            got, got_h = ops.pndm_step(x, e, c, mode, v_pred=v, acc=a, hist=hist, out=out)
            assert torch.equal(got, want) and torch.equal(a, acc_want if writes_acc else acc), (n, mode, v, 'two phases')
            assert (not appends or torch.equal(got_h, e)) and _guards_intact(obuf, n, 1) and _guards_intact(abuf, n, 0)
            cases += 1
    assert ran == set(BRANCHES) == set(CASES) and cases == 90
    _line(report, 'kernel_vs_stand_in/n%d' % n, cases=cases, differing_elements=0)


def test_prk0_turns_a_negative_zero_positive_on_the_device():
    ops = pkg('ops')
    e = torch.tensor([-0.0, 0.0, -1.0, 3.0, -0.0], device=DEV)
    x = torch.ones(5, device=DEV)
    acc = torch.full((5,), -5.0, device=DEV)
    _, h = ops.pndm_step(x, e, R.random_coefs(4), ops.PNDM_PRK0, acc=acc)
    assert not bool(torch.signbit(acc[0])) and not bool(torch.signbit(acc[4])) and float(acc[0]) == 0.0
    assert bool(torch.signbit(h[0])) and torch.equal(h, e)                        # the history keeps e itself


def test_the_wrapper_and_the_library_refuse_what_the_kernel_is_not_written_for(seeded):
    ops, L = pkg('ops'), pkg('_lib')
    x, e, acc, h1, h2, h3 = (t[:64].clone() for t in seeded)
    c = R.random_coefs(2)
    P = ops
    lib = L.load()
    before = lib.dp_launch_count()
    # the wrapper: missing pointers, shared buffers
    for bad in (dict(mode=P.PNDM_PRK0), dict(mode=P.PNDM_PRK1), dict(mode=P.PNDM_PRK3),                  # no accumulator
                dict(mode=P.PNDM_PLMS2), dict(mode=P.PNDM_PLMS_AVG), dict(mode=P.PNDM_PLMS3, hist=[h1]),   # history below the mode
                dict(mode=P.PNDM_PLMS4, hist=[h1, h2]), dict(mode=P.PNDM_PLMS4, hist=[h1, None, h3]),
                dict(mode=P.PNDM_PLMS1, out=e), dict(mode=P.PNDM_PLMS1, hist_out=x), dict(mode=P.PNDM_PLMS1, hist_out=e),
                dict(mode=P.PNDM_PLMS1, out=x, hist_out=x), dict(mode=P.PNDM_PLMS2, hist=[h1], out=h1),
                dict(mode=P.PNDM_PRK0, acc=x), dict(mode=P.PNDM_PRK1, acc=e), dict(mode=P.PNDM_PRK0, acc=acc, hist_out=acc),
                dict(mode=P.PNDM_PRK1, acc=acc, out=acc), dict(mode=9), dict(mode=-1)):
        with pytest.raises(AssertionError):
            ops.pndm_step(x, e, c, **bad)
    with pytest.raises(AssertionError):
        ops.pndm_step(x, e.double(), c, P.PNDM_PLMS1)
    with pytest.raises(AssertionError):
        ops.pndm_step(x, e[:32], c, P.PNDM_PLMS1)
    with pytest.raises(AssertionError):
        ops.pndm_step(x, e, dict(c, nonsense=1.0), P.PNDM_PLMS1)
    # the library: partial overlaps, which the wrapper's pointer comparison does not see
    big = torch.zeros(256, device=DEV)
    for xx, bad in ((x, dict(mode=P.PNDM_PLMS1, out=big[8:72], hist_out=big[40:104])),                   # the two outputs overlap in part
                    (x, dict(mode=P.PNDM_PLMS2, hist=[big[0:64]], hist_out=big[4:68])),                  # hist_out overlaps h1 without being it
                    (x, dict(mode=P.PNDM_PLMS4, hist=[h1, h2, big[0:64]], hist_out=big[4:68])),          # ... h3
                    (x, dict(mode=P.PNDM_PLMS4, hist=[h1, h2, big[0:64]], out=big[60:124])),             # x_next overlaps h3
                    (big[128:192], dict(mode=P.PNDM_PLMS1, out=big[130:194])),                           # x_next overlaps x without being it
                    (x, dict(mode=P.PNDM_PRK1, acc=big[0:64], out=big[32:96])),                          # x_next overlaps acc
                    (big[0:64], dict(mode=P.PNDM_PRK0, acc=big[32:96])),                                 # acc overlaps x
                    (x, dict(mode=P.PNDM_PRK0, acc=big[0:64], hist_out=big[60:124]))):                   # acc overlaps hist_out
        with pytest.raises(L.DpHipError) as err:
            ops.pndm_step(xx, e, c, **bad)
        assert err.value.code == 1                                               # hipErrorInvalidValue, before any launch
    # the library alone: null pointers that the mode reads or writes, a mode outside 0 .. 8
    coef = L.PndmCoef(**dict(ops.PNDM_FRACTIONS, **c))
    out, hout = torch.empty_like(x), torch.empty_like(x)

    def raw(mode, x_=x, e_=e, acc_=None, h=(None, None, None), out_=out, hout_=None, coef_=coef):
        p = ops._p
        return lib.dp_pndm_step(p(x_), p(e_), p(acc_), p(h[0]), p(h[1]), p(h[2]), mode, 0, ctypes.byref(coef_) if coef_ is not None else None,
                                p(out_), p(hout_), 64, None)
    for rc in (raw(P.PNDM_PLMS1, x_=None, hout_=hout), raw(P.PNDM_PLMS1, e_=None, hout_=hout), raw(P.PNDM_PLMS1, out_=None, hout_=hout),
               raw(P.PNDM_PLMS1), raw(P.PNDM_PLMS1, hout_=hout, coef_=None), raw(P.PNDM_PRK0, hout_=hout), raw(P.PNDM_PRK0, acc_=acc),
               raw(P.PNDM_PRK2), raw(P.PNDM_PRK3), raw(P.PNDM_PLMS_AVG), raw(P.PNDM_PLMS2, hout_=hout),
               raw(P.PNDM_PLMS3, h=(h1, None, None), hout_=hout), raw(P.PNDM_PLMS4, h=(h1, h2, None), hout_=hout),
               raw(P.PNDM_PLMS4, h=(h1, h2, h3)), raw(9, hout_=hout), raw(-1, hout_=hout)):
        assert rc == 1
    assert lib.dp_launch_count() == before
    torch.cuda.synchronize()
    assert bool((big == 0).all())
    # what a mode neither reads nor writes may be anything, null included: one launch
    assert raw(P.PNDM_PLMS_AVG, h=(h1, None, None)) == 0 and raw(P.PNDM_PRK3, acc_=acc, h=(out, out, out), hout_=out) == 0
    assert lib.dp_launch_count() == before + 2


# ---------------------------------------------------------------------------------------------- kernel against reference
@pytest.fixture(scope='module')
def steps():
    return R.load(R.STEPS_FILE)


@pytest.mark.parametrize('case', [c for c in R.TABLE_CASES if c[2] in (4, 5, 10, 1000)], ids=R.table_name)
def test_host_tables_on_this_machine_equal_the_fixtures(case, steps):
    s = _sched(**R.table_kwargs(case))
    s.set_timesteps(case[2])
    assert s._ts == steps[R.table_name(case)].tolist()


def _differing_scalars(c, stored, v_pred):
    names = ('sa', 'sb', 'sc', 'd', 'den')
    return [n for n in (names if v_pred else names[2:]) if np.float32(c[n]).tobytes() != stored[names.index(n)].tobytes()]


@pytest.mark.parametrize('run', R.STEP_RUNS, ids=R.run_name)
def test_scheduler_steps_on_the_reference_single_steps(run, steps, report):
    """The teacher-forced run of the fixture through scheduler.step on the device: call k is handed the seeded x_k, e_k.  Every stored
    call: the host's scalars equal the fixture's bits, the result lies within the bound of fp64 and equals the reference's fp32 bits."""
    L = pkg('_lib')
    lib = L.load()
    sname, kw, n, at = run
    name = R.run_name(run)
    v = kw.get('prediction_type') == 'v_prediction'
    s = _sched(**kw)
    s.set_timesteps(n)
    assert s._ts == steps[name + ':timesteps'].tolist()
    modes = steps[name + ':modes'].tolist()
    failed = []
    for k in range(len(s._ts)):
        x, e = (t.to(DEV) for t in R.step_inputs(k))
        before = lib.dp_launch_count()
        prev = s.step(e, s._ts[k], x).prev_sample
        assert _launched(lib, before) == [_branch(modes[k], v)]
        if k not in at:
            continue
        key = '%s@%d' % (name, k)
        t, prev_t = (int(q) for q in steps[name + ':t_pairs'][k])
        differing = _differing_scalars(s.step_coefs(t, prev_t), steps[key + ':coefs'], v)
        got = prev.cpu().numpy()
        err = float(np.abs(got.astype(np.float64) - steps[key + ':prev64']).max())
        bound = R.single_step_bound(steps[key + ':e_ref32'], steps[key + ':prev64'])
        same32 = bool(np.array_equal(got, steps[key + ':prev32']))
        _line(report, 'step/' + key, mode=R.MODES[modes[k]], err=err, bound=bound, e_ref32=float(steps[key + ':e_ref32']),
              equals_reference_fp32=same32, differing_scalars=','.join(differing) or 'none')
        if err > bound or not same32 or differing:
            failed.append((key, err, bound, same32, differing))
    assert not failed, failed


# ---------------------------------------------------------------------------------------------- no read-back, one launch
@pytest.mark.parametrize('kw', [dict(), dict(skip_prk_steps=True, prediction_type='v_prediction')], ids=['prk', 'skip_v'])
def test_step_is_one_launch_and_reads_nothing_back(kw):
    L = pkg('_lib')
    lib = L.load()
    s = _sched(**kw)
    s.set_timesteps(5)
    x, e = (t.to(DEV) for t in R.step_inputs(0))
    first, x0 = x, x.clone()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        for t in s._ts:                                                          # every mode of the run, the ring turning over
            before = lib.dp_launch_count()
            x = s.step(e, t, x).prev_sample
            assert lib.dp_launch_count() == before + 1
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert torch.isfinite(x).all() and torch.equal(first, x0)                    # a step writes none of its inputs


# ---------------------------------------------------------------------------------------------- chains on the HIP UNet
@pytest.fixture(scope='module')
def tiny():
    return make_model(gc.TINY_CFG, R.MODEL_SEED)


@pytest.fixture(scope='module')
def chains():
    return R.load(R.CHAINS_FILE)


def _loop(model, sched, x_T, n, replay):
    sched.set_timesteps(n)
    fwd = model.sampling_forward(tuple(x_T.shape), len(sched._ts), replay=replay)
    assert type(fwd).__name__ == ('_CapturedForward' if replay else '_EagerForward')
    xs = [x_T]
    try:
        with torch.no_grad():
            for t in sched._ts:
                xs.append(sched.step(fwd(xs[-1], t), t, xs[-1]).prev_sample)
    finally:
        fwd.close()
    return xs


def _spied(sched):
    seen = []
    real = sched.step

    def spy(model_output, timestep, sample, **k):
        out = real(model_output, timestep, sample, **k)
        seen.append((int(timestep), sample, out.prev_sample))
        return out
    sched.step = spy
    return seen


@pytest.mark.parametrize('chain', R.CHAINS, ids=lambda c: c[0])
def test_pipeline_chains_on_the_hip_unet_against_the_reference(chain, tiny, chains, report):
    diffusion = pkg('diffusion')
    name, kw, n = chain
    g = chains
    pipe = diffusion.PNDMPipeline(tiny, _sched(**kw))
    sched = pipe.scheduler
    seen = _spied(sched)
    try:
        images = pipe(batch_size=R.CHAIN_B, generator=torch.Generator().manual_seed(R.CHAIN_SEED), num_inference_steps=n,
                      output_type='numpy').images
    finally:
        del sched.step
    calls = R.n_calls(kw, n)
    assert [t for t, _, _ in seen] == g[name + ':timesteps'].tolist() == sched._ts and len(seen) == calls
    assert np.array_equal(seen[0][1].cpu().numpy(), g['x_T'])                    # the pipeline draws the fixture's x_T bit for bit
    xs = [seen[0][1]] + [p for _, _, p in seen]
    y64, gaps = g[name + ':xs64'], g[name + ':gap']
    errs = [float(np.abs(t.double().cpu().numpy() - y64[k]).max()) for k, t in enumerate(xs)]
    bounds = [R.CHAIN_FACTOR * float(gaps[k]) + R.CHAIN_FLOOR for k in range(len(xs))]
    _line(report, 'chain/' + name, calls=calls, worst_err=max(errs), worst_err_over_bound=max(e / b for e, b in zip(errs, bounds)),
          errs=' '.join('%.1e' % v for v in errs), bounds=' '.join('%.1e' % v for v in bounds))
    assert all(e <= b for e, b in zip(errs, bounds)), (name, errs, bounds)
    want = (xs[-1] / 2 + 0.5).clamp(0, 1).cpu().permute(0, 2, 3, 1).numpy()
    assert np.array_equal(images, want)
    # the hand-written loop, on replayed and on eager forwards: the same bits, and the pipeline's
    x_T = torch.from_numpy(g['x_T']).to(DEV)
    replayed, eager = _loop(tiny, _sched(**kw), x_T, n, True), _loop(tiny, _sched(**kw), x_T, n, False)
    assert len(replayed) == len(eager) == len(xs)
    for a, b, c in zip(replayed, eager, xs):
        assert torch.equal(a, b) and torch.equal(a, c)


def test_ddpm_pipeline_with_the_scheduler_equals_the_loop(tiny, chains):
    diffusion = pkg('diffusion')
    kw, n = dict(steps_offset=1), 5
    mine = _sched(**kw)
    pipe = diffusion.DDPMPipeline(tiny, mine)
    assert pipe.scheduler is mine
    images = pipe(batch_size=R.CHAIN_B, generator=torch.Generator().manual_seed(R.CHAIN_SEED), num_inference_steps=n,
                  output_type='numpy').images
    x_T = torch.from_numpy(chains['x_T']).to(DEV)
    last = _loop(tiny, _sched(**kw), x_T, n, True)[-1]
    want = (last / 2 + 0.5).clamp(0, 1).cpu().permute(0, 2, 3, 1).numpy()
    assert np.array_equal(images, want) and images.min() != images.max() and mine.counter == 14


def test_ldm_pipeline_with_the_scheduler_equals_the_loop_and_decode(tiny):
    import vq_ref
    diffusion, vq, syn = pkg('diffusion'), pkg('vq'), pkg('synthetic')
    vqm = vq.VQModel(**syn.VQ_TINY_CFG)
    vqm.load_state_dict({k: v.float() for k, v in vq_ref.params(syn.VQ_TINY_CFG, 3).items()})
    vqm = vqm.to(DEV).eval()
    kw = dict(skip_prk_steps=True, beta_schedule='scaled_linear', beta_start=0.0015, beta_end=0.0195)
    n, B = 6, 2
    pipe = diffusion.LDMPipeline(vqvae=vqm, unet=tiny, scheduler=_sched(**kw))
    images = pipe(batch_size=B, generator=torch.Generator().manual_seed(9), num_inference_steps=n, output_type='numpy').images
    assert pipe.scheduler.counter == n + 1
    ss = gc.TINY_CFG['sample_size']
    x_T = diffusion.randn_tensor((B, gc.TINY_CFG['in_channels'], ss, ss), generator=torch.Generator().manual_seed(9)).to(DEV)
    lat = _loop(tiny, _sched(**kw), x_T, n, True)[-1]
    with torch.no_grad():
        dec = vqm.decode(lat).sample
    want = (dec / 2 + 0.5).clamp(0, 1).cpu().permute(0, 2, 3, 1).numpy()
    assert images.shape == want.shape and images.shape[0] == B and np.isfinite(images).all()
    assert np.array_equal(images, want) and images.min() != images.max()
