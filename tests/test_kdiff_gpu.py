"""LMSDiscreteScheduler, KDPM2DiscreteScheduler and KDPM2AncestralDiscreteScheduler on the MI355X: dp_kdpm2_step / dp_lms_step
(csrc/kdiff.hip), the three classes of diffusion.py, the HIP UNet2DModel's sampling forward under them and LDMPipeline, against the
fixtures the reference wrote (tests/golden/make_golden_kdiff.py).

Bounds (none fixed by hand; all of tests/pndm_ref.py, not retuned):
  * the kernels equal the stand-in tests/mock_ops_kdiff.py bit for bit: both are the same sequence of correctly rounded fp32
    operations (the stand-in runs torch's eager fp32 ops on the device, one rounding each, scalars as 0-d device tensors);
  * a fixture step lies within max(4 e_ref32, 4 * 2^-24 * max|y64|) of the fixture's fp64 result y64, e_ref32 being the reference's
    own fp32 distance stored beside it, without exclusions; and it equals the reference's fp32 result as numbers (the reference's
    `sum()` starts from the integer 0, which can move the sign of a zero and nothing else);
  * a chain state lies within 10 x the reference fp32 chain's own gap at that state + 1e-5 of the fp64 chain.
profiles/kdiff_gpu_tests.txt holds every measured value beside its bound."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import golden_common as gc
import kdiff_ref as R
import mock_ops_kdiff as mock
from helpers import make_model, pkg

pytestmark = pytest.mark.gpu
DEV = 'cuda'

# ---- the launch sites of csrc/kdiff.hip (tests/test_kdiff_cpu.py compares this table with the source)
LAUNCH_SITES = {'kdiff.hip': 18}
BRANCHES = [R.branch(i) for i in R.INSTANCES]
# branch -> ('kdpm2', shape, pred) | ('lms', order, pred): test_kernels_equal_the_stand_in runs every one at every size
CASES = {R.branch(i): i for i in R.INSTANCES}
MAX_BLOCKS = 4096                                  # DP_KDIFF_MAX_BLOCKS
CAP = MAX_BLOCKS * 256 * 4                         # elements one launch covers without a second grid-stride trip (16-byte path)
SIZES = [1, 3, 4, 5, 255, 1027, CAP + 7]
OFFSETS = (0, 1, 2, 3)                             # elements from 16-byte alignment: a scalar head of 0, 3, 2, 1
GUARD = 7.0


def _launched(lib, before):
    n = lib.dp_launch_count() - before
    arr = (ctypes.c_char_p * 256)()
    k = lib.dp_recent_launches(arr, 256)
    return [arr[i].decode() for i in range(k)][k - n:] if n else []


def _line(report, key, **kw):
    report['kdiff/' + key] = kw
    print('kdiff/%s %s' % (key, ' '.join('%s=%.3e' % (k, v) if isinstance(v, float) else '%s=%s' % (k, v) for k, v in kw.items())))


def _sched(cls, **kw):
    return getattr(pkg('diffusion'), R.CLASSES[cls])(**kw)


# ---------------------------------------------------------------------------------------------- kernels against stand-in
@pytest.fixture(scope='module')
def seeded():
    n = SIZES[-1] + 4
    gen = torch.Generator().manual_seed(23)
    return tuple(torch.randn(n, generator=gen).to(DEV) for _ in range(5))           # x, e, and three more streams


def _guarded(n, off):
    """A view of n elements at element offset `off` inside a buffer of guard words."""
    buf = torch.full((n + 4,), GUARD, device=DEV)
    return buf, buf[off:off + n]


def _guards_intact(buf, n, off):
    return bool((buf[:off] == GUARD).all()) and bool((buf[off + n:] == GUARD).all())


def _copy_at(t, n, off):
    buf, view = _guarded(n, off)
    view.copy_(t[:n])
    return buf, view


@pytest.mark.parametrize('n', SIZES)
def test_kdpm2_kernel_equals_the_stand_in(n, seeded, report):
    """All 6 instantiations with every pointer at element offset 0 .. 3 from 16-byte alignment (a scalar head of 0, 3, 2, 1) and with
    pointers of two phases (all 4-byte accesses), out of place and under both permitted aliases (x_next is x; x_next is the saved
    sample); the guard words either side of every output stay untouched, and the launch ring names the instantiation asked for."""
    ops, L = pkg('ops'), pkg('_lib')
    lib = L.load()
    ran, cases = set(), 0
    for i, (shape, pred) in enumerate(R.KDPM2_INSTANCES):
        c = R.kdpm2_coefs(R.random_coefs(10 + i))
        for off in OFFSETS + ('mixed',):
            src = 0 if off == 'mixed' else off
            dst = 1 if off == 'mixed' else off
            x, e, xs, z = (t[src:src + n] for t in seeded[:4])
            assert x.data_ptr() % 16 == 4 * src
            kw = dict(saved=xs if shape else None, noise=z if shape == 2 else None)
            want = mock.kdpm2_step(x, e, c, pred, **kw)
            obuf, out = _guarded(n, dst)
            before = lib.dp_launch_count()
            got = ops.kdpm2_step(x, e, c, pred, out=out, **kw)
            assert _launched(lib, before) == [R.branch(('kdpm2', shape, pred))]
            ran.add(R.branch(('kdpm2', shape, pred)))
            assert got is out and torch.equal(got, want) and _guards_intact(obuf, n, dst), (n, shape, pred, off)
            cases += 1
            if off == 'mixed':
                continue
            xbuf, xc = _copy_at(x, n, off)                                       # x_next is x
            assert ops.kdpm2_step(xc, e, c, pred, out=xc, **kw) is xc and torch.equal(xc, want) and _guards_intact(xbuf, n, off), (n, shape, pred, off, 'x')
            cases += 1
            if shape:                                                            # x_next is the saved sample
                sbuf, sc = _copy_at(xs, n, off)
                got = ops.kdpm2_step(x, e, c, pred, saved=sc, noise=kw['noise'], out=sc)
                assert got is sc and torch.equal(sc, want) and _guards_intact(sbuf, n, off), (n, shape, pred, off, 'saved')
                cases += 1
    assert ran == set(BRANCHES[:6]) and cases == 6 * 5 + 6 * 4 + 4 * 4
    _line(report, 'kdpm2_kernel_vs_stand_in/n%d' % n, cases=cases, differing_elements=0)


@pytest.mark.parametrize('n', SIZES)
def test_lms_kernel_equals_the_stand_in(n, seeded, report):
    """All 12 instantiations at the same alignments, out of place and with x_next being x: the next state, the new derivative and x0
    bit for bit, the guard words either side of all three outputs untouched, the launch ring naming the instantiation."""
    ops, L = pkg('ops'), pkg('_lib')
    lib = L.load()
    ran, cases = set(), 0
    for i, (order, pred) in enumerate(R.LMS_INSTANCES):
        c = R.lms_coefs(R.random_coefs(40 + i), order)
        for off in OFFSETS + ('mixed',):
            src = 0 if off == 'mixed' else off
            dst = 1 if off == 'mixed' else off
            x, e, d1, d2, d3 = (t[src:src + n] for t in seeded)
            history = [d1, d2, d3][:order - 1]
            want = mock.lms_step(x, e, c, order, pred, history=history)
            bufs = [_guarded(n, dst) for _ in range(3)]
            before = lib.dp_launch_count()
            got = ops.lms_step(x, e, c, order, pred, history=history, out=bufs[0][1], d_out=bufs[1][1], x0_out=bufs[2][1])
            assert _launched(lib, before) == [R.branch(('lms', order, pred))]
            ran.add(R.branch(('lms', order, pred)))
            assert all(torch.equal(g, w) for g, w in zip(got, want)), (n, order, pred, off)
            assert all(_guards_intact(b, n, dst) for b, _ in bufs), (n, order, pred, off)
            cases += 1
            if off == 'mixed':
                continue
            xbuf, xc = _copy_at(x, n, off)                                       # x_next is x
            got = ops.lms_step(xc, e, c, order, pred, history=history, out=xc, d_out=bufs[1][1], x0_out=bufs[2][1])
            assert got[0] is xc and all(torch.equal(g, w) for g, w in zip(got, want)) and _guards_intact(xbuf, n, off), (n, order, pred, off, 'x')
            cases += 1
    assert ran == set(BRANCHES[6:]) and cases == 12 * 9
    _line(report, 'lms_kernel_vs_stand_in/n%d' % n, cases=cases, differing_elements=0)


def test_the_wrapper_and_the_library_refuse_what_the_kernels_are_not_written_for(seeded):
    """Nothing here launches: every call is refused by the wrapper's assertions or by the library's checks before the launch."""
    ops, L = pkg('ops'), pkg('_lib')
    x, e, a, b, c3 = (t[:64].clone() for t in seeded)
    c = R.random_coefs(2)
    kc, lc = R.kdpm2_coefs(c), R.lms_coefs(c, 4)
    lib = L.load()
    before = lib.dp_launch_count()
    # the wrapper: unknown instantiations, missing pointers, shared buffers
    for bad in (dict(pred=ops.KDIFF_SAMPLE), dict(pred=3), dict(pred=-1), dict(noise=a), dict(out=e), dict(saved=a, noise=b, out=b)):
        with pytest.raises(AssertionError):
            ops.kdpm2_step(x, e, kc, **bad)
    for bad in (dict(order=0), dict(order=5, history=[a, b, c3, a]), dict(order=2), dict(order=4, history=[a, b]), dict(order=1, pred=3),
                dict(order=2, history=[a], out=e), dict(order=2, history=[a], out=a), dict(order=2, history=[a], d_out=x),
                dict(order=2, history=[a], d_out=a), dict(order=1, out=x, d_out=x), dict(order=1, x0_out=e),
                dict(order=1, d_out=b, x0_out=b)):
        with pytest.raises(AssertionError):
            ops.lms_step(x, e, lc, **bad)
    with pytest.raises(AssertionError):
        ops.kdpm2_step(x, e.double(), kc)
    with pytest.raises(AssertionError):
        ops.lms_step(x, e[:32], lc, 1)
    with pytest.raises(AssertionError):
        ops.kdpm2_step(x, e, dict(kc, nonsense=1.0))
    with pytest.raises(AssertionError):
        ops.lms_step(x, e, dict(lc, dt=1.0), 1)
    # the library: partial overlaps, which the wrapper's pointer comparison does not see
    big = torch.zeros(256, device=DEV)
    for xx, bad in ((big[128:192], dict(out=big[130:194])),                                  # x_next overlaps x without being it
                    (x, dict(saved=big[0:64], out=big[4:68])),                                # ... the saved sample
                    (x, dict(saved=a, noise=big[0:64], out=big[32:96]))):                     # x_next overlaps the noise
        with pytest.raises(L.DpHipError) as err:
            ops.kdpm2_step(xx, e, kc, **bad)
        assert err.value.code == 1                                               # hipErrorInvalidValue, before any launch
    with pytest.raises(L.DpHipError) as err:
        ops.kdpm2_step(x, big[0:64], kc, out=big[60:124])                        # x_next overlaps e
    assert err.value.code == 1
    for xx, bad in ((big[128:192], dict(order=1, out=big[130:194])),                         # x_next overlaps x without being it
                    (x, dict(order=2, history=[big[0:64]], out=big[60:124])),                # x_next overlaps d1
                    (x, dict(order=4, history=[a, b, big[0:64]], out=big[60:124])),          # ... d3
                    (x, dict(order=1, out=big[8:72], d_out=big[40:104])),                    # two outputs overlap in part
                    (x, dict(order=1, out=big[8:72], x0_out=big[40:104])),
                    (x, dict(order=1, d_out=big[8:72], x0_out=big[40:104])),
                    (big[0:64], dict(order=1, d_out=big[32:96])),                            # d_new overlaps x
                    (x, dict(order=3, history=[a, big[0:64]], x0_out=big[32:96]))):          # x0_out overlaps d2
        with pytest.raises(L.DpHipError) as err:
            ops.lms_step(xx, e, lc, **bad)
        assert err.value.code == 1
    with pytest.raises(L.DpHipError) as err:
        ops.lms_step(x, big[0:64], lc, 1, d_out=big[60:124])                     # d_new overlaps e
    assert err.value.code == 1
    # the library alone: null pointers that the call reads or writes, types and orders outside the table
    kcoef, lcoef = L.Kdpm2Coef(**kc), L.LmsCoef(**lc)
    out, dn, p0 = torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)
    p = ops._p

    def kraw(pred=0, x_=x, e_=e, xs_=None, z_=None, out_=out, coef_=kcoef, n=64):
        return lib.dp_kdpm2_step(p(x_), p(e_), p(xs_), p(z_), pred, ctypes.byref(coef_) if coef_ is not None else None, p(out_), n, None)

    def lraw(order=1, pred=0, x_=x, e_=e, d_=(None, None, None), out_=out, dn_=dn, p0_=p0, coef_=lcoef, n=64):
        return lib.dp_lms_step(p(x_), p(e_), p(d_[0]), p(d_[1]), p(d_[2]), order, pred, ctypes.byref(coef_) if coef_ is not None else None,
                               p(out_), p(dn_), p(p0_), n, None)
    for rc in (kraw(x_=None), kraw(e_=None), kraw(out_=None), kraw(coef_=None), kraw(pred=2), kraw(pred=3), kraw(pred=-1), kraw(z_=a),
               lraw(x_=None), lraw(e_=None), lraw(out_=None), lraw(dn_=None), lraw(p0_=None), lraw(coef_=None), lraw(order=0), lraw(order=5),
               lraw(order=-1), lraw(pred=3), lraw(pred=-1), lraw(order=2), lraw(order=3, d_=(a, None, None)), lraw(order=4, d_=(a, b, None)),
               lraw(order=4, d_=(None, a, b))):
        assert rc == 1
    assert lib.dp_launch_count() == before
    torch.cuda.synchronize()
    assert bool((big == 0).all())
    # what an order does not read may be anything, null included: one launch each; n <= 0 is a no-op
    assert lraw(order=1, d_=(out, out, out)) == 0 and lraw(order=2, d_=(a, None, dn)) == 0 and kraw(xs_=a, z_=b) == 0
    assert lib.dp_launch_count() == before + 3
    assert kraw(x_=None, e_=None, out_=None, n=0) == 0 and lraw(x_=None, e_=None, out_=None, dn_=None, p0_=None, n=0) == 0 and lraw(order=9, n=-1) == 0
    assert lib.dp_launch_count() == before + 3
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- schedulers against reference
@pytest.fixture(scope='module')
def steps():
    return R.load_steps()


@pytest.mark.parametrize('case', [c for c in R.TABLE_CASES if c[3] in (7, 10) and c[1] == 'linear'], ids=R.table_name)
def test_host_tables_on_this_machine_equal_the_fixtures(case):
    g = R.load(R.TABLES_FILE)
    s = _sched(case[0], **R.table_kwargs(case))
    s.set_timesteps(case[3], device=DEV)
    name = R.table_name(case)
    assert s._ts == g[name + ':timesteps'].tolist() and s._sig.numpy().tobytes() == g[name + ':sigmas'].tobytes()
    assert s.timesteps.device.type == 'cuda' and s.sigmas.device.type == 'cuda' and s._sig.device.type == 'cpu'
    for k in R.EXTRA_TABLES[case[0]]:
        assert getattr(s, k).device.type == 'cuda' and np.array_equal(getattr(s, k).cpu().numpy(), g[name + ':' + k], equal_nan=True)
    if case[0] == 'lms' and case[3] == 10 and case[2] == 'plain':
        for t in range(10):
            for order in range(1, min(t + 1, 4) + 1):
                assert np.array(s.lms_coefficients(order, t), np.float32).tobytes() == g[R.lms_coef_name(10, t, order)].tobytes()


@pytest.mark.parametrize('run', R.STEP_RUNS, ids=R.run_name)
def test_scheduler_steps_on_the_reference_single_steps(run, steps, report):
    """The teacher-forced run of the fixture through scheduler.step on the device: call k is handed the seeded x_k, e_k.  Every call is
    one launch of the instantiation the fixture names; every stored output lies within the bound of fp64 and equals the reference's
    fp32 result as numbers (prev_sample, and for LMS pred_original_sample)."""
    L = pkg('_lib')
    lib = L.load()
    sname, cls, kw, skw, n, at = run
    name = R.run_name(run)
    s = _sched(cls, **kw)
    s.set_timesteps(n)
    s.is_scale_input_called = True
    assert s._ts == steps[name + ':timesteps'].tolist()
    extra = dict(skw, generator=torch.Generator().manual_seed(R.GEN_SEED)) if cls == 'kdpm2a' else dict(skw)
    failed = []
    for k in range(len(s._ts)):
        x, e = (t.to(DEV) for t in R.step_inputs(k))
        x_keep, e_keep = x.clone(), e.clone()
        before = lib.dp_launch_count()
        o = s.step(e, s._ts[k], x, **extra)
        inst = R.instance_of_call(cls, kw, skw, k)
        assert _launched(lib, before) == [R.branch(inst)]
        assert torch.equal(x, x_keep) and torch.equal(e, e_keep)
        if k not in at:
            continue
        key = '%s@%d' % (name, k)
        outs = [('prev', o.prev_sample, '')] + ([('x0', o.pred_original_sample, '_x0')] if cls == 'lms' else [])
        for what, t, suffix in outs:
            got = t.cpu().numpy()
            y64 = steps[key + (':prev64' if what == 'prev' else ':x0_64')]
            e_ref = float(steps[key + ':e_ref32' + suffix])
            err = float(np.abs(got.astype(np.float64) - y64).max())
            bound = R.single_step_bound(e_ref, y64)
            same32 = bool(np.array_equal(got, steps[key + (':prev32' if what == 'prev' else ':x0_32')]))
            _line(report, 'step/%s/%s' % (key, what), kernel=R.branch(inst), err=err, bound=bound, e_ref32=e_ref, equals_reference_fp32=same32)
            if err > bound or not same32:
                failed.append((key, what, err, bound, same32))
    assert not failed, failed


def test_scale_model_input_and_add_noise_equal_the_references(steps):
    x, z = (torch.from_numpy(gc.det_noise(R.STEP_SHAPE, 900 + i)).to(DEV) for i in range(2))
    for i, (cls, kw, idx, first) in enumerate(R.SCALE_CASES):
        s = _sched(cls, **kw)
        s.set_timesteps(7)
        if not first:
            s.sample = x
        y = s.scale_model_input(x * R.X_SCALE, s._ts[idx])
        assert np.array_equal(y.cpu().numpy(), steps['scale:%d:out' % i]), i
    for i, (cls, kw, idx, first) in enumerate(R.NOISE_CASES):
        s = _sched(cls, **kw)
        s.set_timesteps(10)
        if not first:
            s.sample = x
        x_keep = x.clone()
        y = s.add_noise(x, z, s.timesteps[idx])
        assert np.array_equal(y.cpu().numpy(), steps['noise:%d:out' % i]) and torch.equal(x, x_keep), i


# ---------------------------------------------------------------------------------------------- no read-back, one launch
@pytest.mark.parametrize('cls,kw', [('lms', dict()), ('lms', dict(prediction_type='v_prediction', use_karras_sigmas=True)),
                                    ('kdpm2', dict()), ('kdpm2a', dict(prediction_type='v_prediction'))],
                         ids=['lms', 'lms_v_karras', 'kdpm2', 'kdpm2a_v'])
def test_step_is_one_launch_scaling_one_more_and_neither_reads_back(cls, kw):
    L = pkg('_lib')
    lib = L.load()
    s = _sched(cls, **kw)
    s.set_timesteps(5)
    x, e = (t.to(DEV) for t in R.step_inputs(0))
    first, x0 = x, x.clone()
    s.scale_model_input(x, s._ts[0])                                            # the buffers of its own exist
    if cls == 'lms':
        for t in s._ts:                                                          # ... and the coefficients are integrated (host work)
            s.lms_coefficients(min(s._ts.index(t) + 1, 4), s._ts.index(t))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        for t in s._ts:
            before = lib.dp_launch_count()
            xin = s.scale_model_input(x, t)
            assert _launched(lib, before) == ['sigma_scale_kernel'] and xin.data_ptr() != x.data_ptr()
            x = s.step(e, t, x).prev_sample                                      # no generator: nothing crosses the bus
            assert lib.dp_launch_count() == before + 2
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert torch.isfinite(x).all() and torch.equal(first, x0)                    # the caller's sample is never written


def test_the_ancestral_class_uploads_noise_for_the_second_call_only(monkeypatch):
    """The draw of a first-order call is made where the generator lives (its stream advances as the reference's does) and not
    uploaded."""
    diffusion = pkg('diffusion')
    s = _sched('kdpm2a')
    s.set_timesteps(5)
    x, e = (t.to(DEV) for t in R.step_inputs(0))
    gen, twin = torch.Generator().manual_seed(5), torch.Generator().manual_seed(5)
    drawn = []
    real = diffusion.randn_tensor
    monkeypatch.setattr(diffusion, 'randn_tensor', lambda *a, **k: drawn.append(real(*a, **k)) or drawn[-1])
    y = s.step(e, s._ts[0], x, generator=gen).prev_sample
    torch.randn(R.STEP_SHAPE, generator=twin)
    assert len(drawn) == 1 and drawn[0].device.type == 'cpu' and torch.equal(gen.get_state(), twin.get_state())
    s.step(e, s._ts[1], y, generator=gen)
    assert len(drawn) == 2 and drawn[1].device.type == 'cuda'


# ---------------------------------------------------------------------------------------------- chains on the HIP UNet
@pytest.fixture(scope='module')
def tiny():
    return make_model(gc.TINY_CFG, R.MODEL_SEED)


@pytest.fixture(scope='module')
def chains():
    return R.load(R.CHAINS_FILE)


def _loop(model, cls, kw, x_T, n, with_gen, replay):
    s = _sched(cls, **kw)
    x = x_T * s.init_noise_sigma
    s.set_timesteps(n)
    extra = dict(generator=torch.Generator().manual_seed(R.NOISE_SEED)) if with_gen else {}
    fwd = model.sampling_forward(tuple(x_T.shape), len(s._ts), replay=replay)
    xs = [x]
    try:
        with torch.no_grad():
            for t in s._ts:
                xs.append(s.step(fwd(s.scale_model_input(xs[-1], t), t), t, xs[-1], **extra).prev_sample.clone())
    finally:
        fwd.close()
    return xs, s


@pytest.mark.parametrize('chain', R.CHAINS, ids=lambda c: c[0])
def test_chains_on_the_hip_unet_against_the_reference(chain, tiny, chains, report):
    """The canonical loop -- scale_model_input, the model, step -- over replayed and over eager forwards: the same bits, and every
    state within CHAIN_FACTOR x the reference fp32 chain's own gap + CHAIN_FLOOR of the fixture's fp64 chain."""
    name, cls, kw, n, with_gen = chain
    g = chains
    x_T = torch.from_numpy(g['x_T']).to(DEV)
    xs, s = _loop(tiny, cls, kw, x_T, n, with_gen, True)
    eager, _ = _loop(tiny, cls, kw, x_T, n, with_gen, False)
    assert s._ts == g[name + ':timesteps'].tolist() and len(xs) == R.n_calls(cls, n) + 1 == len(eager)
    assert all(torch.equal(a, b) for a, b in zip(xs, eager))
    y64, gaps = g[name + ':xs64'], g[name + ':gap']
    errs = [float(np.abs(t.double().cpu().numpy() - y64[k]).max()) for k, t in enumerate(xs)]
    bounds = [R.CHAIN_FACTOR * float(gaps[k]) + R.CHAIN_FLOOR for k in range(len(xs))]
    _line(report, 'chain/' + name, calls=len(xs) - 1, fractional=sum(t != round(t) for t in s._ts), worst_err=max(errs),
          worst_err_over_bound=max(e / b for e, b in zip(errs, bounds)), errs=' '.join('%.1e' % v for v in errs),
          bounds=' '.join('%.1e' % v for v in bounds))
    assert all(e <= b for e, b in zip(errs, bounds)), (name, errs, bounds)


def test_ldm_pipeline_equals_the_loop_and_decode(tiny):
    import vq_ref
    diffusion, vq, syn = pkg('diffusion'), pkg('vq'), pkg('synthetic')
    vqm = vq.VQModel(**syn.VQ_TINY_CFG)
    vqm.load_state_dict({k: v.float() for k, v in vq_ref.params(syn.VQ_TINY_CFG, 3).items()})
    vqm = vqm.to(DEV).eval()
    ss, B = gc.TINY_CFG['sample_size'], 2
    for cls, kw, n in (('lms', dict(beta_schedule='scaled_linear', beta_start=0.0015, beta_end=0.0195), 6), ('kdpm2a', dict(), 4)):
        pipe = diffusion.LDMPipeline(vqvae=vqm, unet=tiny, scheduler=_sched(cls, **kw))
        torch.manual_seed(31)                                                    # the ancestral noise of both runs: the device's own stream
        images = pipe(batch_size=B, generator=torch.Generator().manual_seed(9), num_inference_steps=n, output_type='numpy').images
        assert any(t != round(t) for t in pipe.scheduler._ts)                    # fractional timesteps reached the model
        x_T = diffusion.randn_tensor((B, gc.TINY_CFG['in_channels'], ss, ss), generator=torch.Generator().manual_seed(9)).to(DEV)
        torch.manual_seed(31)
        lat = _loop(tiny, cls, kw, x_T, n, False, True)[0][-1]                   # the pipeline hands the scheduler no generator
        with torch.no_grad():
            dec = vqm.decode(lat).sample
        want = (dec / 2 + 0.5).clamp(0, 1).cpu().permute(0, 2, 3, 1).numpy()
        assert images.shape == want.shape and images.shape[0] == B and np.isfinite(images).all()
        assert np.array_equal(images, want) and images.min() != images.max()


@pytest.mark.parametrize('cls', list(R.CLASSES))
def test_a_saved_pipeline_directory_naming_the_class_loads(cls, tiny, tmp_path):
    diffusion = pkg('diffusion')
    d = str(tmp_path / 'pipe')
    diffusion.DDPMPipeline(tiny, diffusion.DDPMScheduler()).save_pretrained(d)
    index = json.load(open(os.path.join(d, 'model_index.json')))
    index['scheduler'] = ['diffusers', R.CLASSES[cls]]
    json.dump(index, open(os.path.join(d, 'model_index.json'), 'w'))
    cfg = dict(vars(_sched(cls).config), _class_name=R.CLASSES[cls], _diffusers_version='0.17.0.dev0')
    json.dump(cfg, open(os.path.join(d, 'scheduler', 'scheduler_config.json'), 'w'))
    back = diffusion.DDPMPipeline.from_pretrained(d)
    assert type(back.scheduler).__name__ == R.CLASSES[cls] and vars(back.scheduler.config) == vars(_sched(cls).config)
    s = back.scheduler
    s.set_timesteps(3)
    x, e = (t.to(DEV) for t in R.step_inputs(0))
    s.scale_model_input(x, s._ts[0])
    y = s.step(e, s._ts[0], x).prev_sample
    assert y.device.type == 'cuda' and bool(torch.isfinite(y).all())
