"""The sigma-space schedulers on the MI355X: dp_sigma_step / dp_sigma_scale / dp_sigma_add_noise (csrc/sigma.hip), diffusion's
EulerDiscreteScheduler, EulerAncestralDiscreteScheduler and HeunDiscreteScheduler, fractional timesteps through the sampling forward of
the HIP UNet2DModel, and LDMPipeline, against the fixtures the reference wrote (tests/golden/make_golden_sigma.py).

Bounds (none fixed by hand; all of tests/pndm_ref.py, not retuned):
  * the kernels equal the stand-in tests/mock_ops_sigma.py bit for bit: both are the same sequence of correctly rounded fp32
    operations (the stand-in runs torch's eager fp32 ops on the device, one rounding each, scalars as 0-d device tensors);
  * a fixture step lies within max(4 e_ref32, 4 * 2^-24 * max|y64|) of the fixture's fp64 result y64, e_ref32 being the reference's
    own fp32 distance stored beside it, without exclusions; and it equals the reference's fp32 result bit for bit;
  * a chain state lies within 10 x the reference fp32 chain's own gap at that state + 1e-5 of the fp64 chain.
profiles/sigma_gpu_tests.txt holds every measured value beside its bound."""
import ctypes

import numpy as np
import pytest
import torch

import golden_common as gc
import sigma_ref as R
import mock_ops_sigma as mock
from helpers import make_model, pkg

pytestmark = pytest.mark.gpu
DEV = 'cuda'

# ---- the launch sites of csrc/sigma.hip (tests/test_sigma_cpu.py compares this table with the source)
LAUNCH_SITES = {'sigma.hip': 11}


def _branch(mode, pred):
    return '(sigma_step_kernel<DP_SIGMA_%s, DP_SIGMA_%s>)' % (R.MODES[mode], R.PREDS[pred])


BRANCHES = [_branch(m, p) for m, p in R.INSTANCES] + ['sigma_scale_kernel', 'sigma_add_noise_kernel']
# branch -> (mode, pred) (None: the two kernels without instantiations): test_kernels_equal_the_stand_in runs every one at every size
CASES = dict({_branch(m, p): (m, p) for m, p in R.INSTANCES}, sigma_scale_kernel=None, sigma_add_noise_kernel=None)
MAX_BLOCKS = 4096                                  # DP_SIGMA_MAX_BLOCKS
CAP = MAX_BLOCKS * 256 * 4                         # elements one launch covers without a second grid-stride trip (16-byte path)
SIZES = [1, 3, 4, 5, 255, 1024, 1027, CAP + 1029]
GUARD = 7.0


def _launched(lib, before):
    n = lib.dp_launch_count() - before
    arr = (ctypes.c_char_p * 256)()
    k = lib.dp_recent_launches(arr, 256)
    return [arr[i].decode() for i in range(k)][k - n:] if n else []


def _line(report, key, **kw):
    report['sigma/' + key] = kw
    print('sigma/%s %s' % (key, ' '.join('%s=%.3e' % (k, v) if isinstance(v, float) else '%s=%s' % (k, v) for k, v in kw.items())))


def _sched(cls, **kw):
    return getattr(pkg('diffusion'), R.CLASSES[cls])(**kw)


# ---------------------------------------------------------------------------------------------- kernels against stand-in
@pytest.fixture(scope='module')
def seeded():
    n = SIZES[-1] + 1
    gen = torch.Generator().manual_seed(19)
    return tuple(torch.randn(n, generator=gen).to(DEV) for _ in range(5))           # x, e, z, d1, saved


def _guarded(n, off):
    """A view of n elements at element offset `off` inside a buffer of guard words."""
    buf = torch.full((n + 2,), GUARD, device=DEV)
    return buf, buf[off:off + n]


def _guards_intact(buf, n, off):
    return float(buf[off + n]) == GUARD and (off == 0 or float(buf[0]) == GUARD) and float(buf[n + 1]) == GUARD


def _copy_at(t, n, off):
    buf, view = _guarded(n, off)
    view.copy_(t[:n])
    return buf, view


def _variants(mode):
    """(with noise) per mode: the Euler step with and without churn."""
    return (False, True) if mode == mock.SIGMA_EULER else (mode == mock.SIGMA_ANCESTRAL,)


@pytest.mark.parametrize('n', SIZES)
def test_step_kernel_equals_the_stand_in(n, seeded, report):
    """All 9 instantiations (the Euler ones with and without churn) with every pointer 16-byte aligned, with every pointer at element
    offset 1 (a scalar head of 3) and with pointers of two phases (all 4-byte accesses), out of place and under every permitted alias
    (x_next is x; in HEUN2 also x_next is the saved sample); the guard words either side of every output stay untouched, and the
    launch ring names the instantiation that was asked for."""
    ops, L = pkg('ops'), pkg('_lib')
    lib = L.load()
    ran, cases = set(), 0
    for i, (mode, pred) in enumerate(R.INSTANCES):
        c = R.random_coefs(10 + i)
        heun2, has_aux = mode == mock.SIGMA_HEUN2, mode != mock.SIGMA_HEUN2
        for noisy in _variants(mode):
            for off in (0, 1):
                x, e, z, d1, saved = (t[off:off + n] for t in seeded)
                assert x.data_ptr() % 16 == 4 * off
                kw = dict(noise=z if noisy else None, d1=d1 if heun2 else None, saved=saved if heun2 else None)
                want, want_aux = mock.sigma_step(x, e, c, mode, pred, **kw)
                obuf, out = _guarded(n, off)
                abuf, aux = _guarded(n, off)
                before = lib.dp_launch_count()
                got, got_aux = ops.sigma_step(x, e, c, mode, pred, out=out, aux_out=aux, **kw)
                assert _launched(lib, before) == [_branch(mode, pred)]
                ran.add(_branch(mode, pred))
                assert torch.equal(got, want), (n, mode, pred, noisy, off)
                assert (got_aux is None) == heun2 and (heun2 or torch.equal(got_aux, want_aux)), (n, mode, pred, noisy, off)
                assert has_aux or bool((aux == GUARD).all())                      # HEUN2 leaves aux_out alone
                assert _guards_intact(obuf, n, off) and _guards_intact(abuf, n, off), (n, mode, pred, noisy, off)
                # x_next is x
                xbuf, xc = _copy_at(x, n, off)
                got, got_aux = ops.sigma_step(xc, e, c, mode, pred, out=xc, **kw)
                assert got is xc and torch.equal(xc, want) and (heun2 or torch.equal(got_aux, want_aux)), (n, mode, pred, noisy, off, 'x')
                assert _guards_intact(xbuf, n, off)
                cases += 2
                if heun2:                                                        # x_next is the saved sample
                    sbuf, sc = _copy_at(saved, n, off)
                    got, _ = ops.sigma_step(x, e, c, mode, pred, d1=d1, saved=sc, out=sc)
                    assert got is sc and torch.equal(sc, want) and _guards_intact(sbuf, n, off), (n, mode, pred, off, 'saved')
                    cases += 1
            # pointers of two phases: every access is a 4-byte one
            x, e, z, d1, saved = (t[:n] for t in seeded)
            kw = dict(noise=z if noisy else None, d1=d1 if heun2 else None, saved=saved if heun2 else None)
            want, want_aux = mock.sigma_step(x, e, c, mode, pred, **kw)
            obuf, out = _guarded(n, 1)
            got, got_aux = ops.sigma_step(x, e, c, mode, pred, out=out, **kw)
            assert torch.equal(got, want) and (heun2 or torch.equal(got_aux, want_aux)) and _guards_intact(obuf, n, 1), (n, mode, pred, 'two phases')
            cases += 1
    assert ran == set(BRANCHES[:9]) and cases == 12 * 5 + 2 * 2
    _line(report, 'step_kernel_vs_stand_in/n%d' % n, cases=cases, differing_elements=0)


def _splits(n):
    return [b for b in (1, 2, 3, 5, 13, n) if n % b == 0 and (b == n or b < n)]


@pytest.mark.parametrize('n', SIZES)
def test_scale_and_add_noise_kernels_equal_the_stand_in(n, seeded, report):
    """dp_sigma_scale (out of place and in place) and dp_sigma_add_noise (every split of n into images in _splits: one image, images
    that a 16-byte group straddles, one element per image) at the three alignments, guard words intact, the ring naming the kernel."""
    ops, L = pkg('ops'), pkg('_lib')
    lib = L.load()
    cases = 0
    for off_in, off_out in ((0, 0), (1, 1), (0, 1)):
        x, z = (t[off_in:off_in + n] for t in seeded[:2])
        for c in (1.0000305, 157.41072):
            want = mock.sigma_scale(x, c)
            obuf, out = _guarded(n, off_out)
            before = lib.dp_launch_count()
            got = ops.sigma_scale(x, c, out=out)
            assert _launched(lib, before) == ['sigma_scale_kernel']
            assert torch.equal(got, want) and _guards_intact(obuf, n, off_out), (n, off_in, off_out, c)
            xbuf, xc = _copy_at(x, n, off_out)
            assert ops.sigma_scale(xc, c, out=xc) is xc and torch.equal(xc, want) and _guards_intact(xbuf, n, off_out)
            cases += 2
        for B in sorted(set(_splits(n))):
            sig = (seeded[2][:B].abs() * 20 + 0.01).contiguous()
            x0, zz = x.reshape(B, n // B), z.reshape(B, n // B)
            want = mock.sigma_add_noise(x0, zz, sig)
            obuf, out = _guarded(n, off_out)
            before = lib.dp_launch_count()
            got = ops.sigma_add_noise(x0, zz, sig, out=out.reshape(B, n // B))
            assert _launched(lib, before) == ['sigma_add_noise_kernel']
            assert torch.equal(got, want) and _guards_intact(obuf, n, off_out), (n, off_in, off_out, B)
            cases += 1
    _line(report, 'scale_add_noise_vs_stand_in/n%d' % n, cases=cases, differing_elements=0)


def test_the_wrapper_and_the_library_refuse_what_the_kernels_are_not_written_for(seeded):
    ops, L = pkg('ops'), pkg('_lib')
    x, e, z, d1, saved = (t[:64].clone() for t in seeded)
    c = R.random_coefs(2)
    P = ops
    lib = L.load()
    before = lib.dp_launch_count()
    # the wrapper: unknown instantiations, missing pointers, shared buffers
    for bad in (dict(mode=4), dict(mode=-1), dict(mode=P.SIGMA_EULER, pred=3), dict(mode=P.SIGMA_ANCESTRAL, pred=P.SIGMA_SAMPLE, noise=z),
                dict(mode=P.SIGMA_HEUN1, pred=P.SIGMA_SAMPLE), dict(mode=P.SIGMA_HEUN2, pred=P.SIGMA_SAMPLE, d1=d1, saved=saved),
                dict(mode=P.SIGMA_ANCESTRAL), dict(mode=P.SIGMA_HEUN2), dict(mode=P.SIGMA_HEUN2, d1=d1), dict(mode=P.SIGMA_HEUN2, saved=saved),
                dict(mode=P.SIGMA_EULER, out=e), dict(mode=P.SIGMA_EULER, noise=z, out=z), dict(mode=P.SIGMA_HEUN2, d1=d1, saved=saved, out=d1),
                dict(mode=P.SIGMA_EULER, aux_out=x), dict(mode=P.SIGMA_EULER, aux_out=e), dict(mode=P.SIGMA_EULER, out=x, aux_out=x),
                dict(mode=P.SIGMA_ANCESTRAL, noise=z, aux_out=z), dict(mode=P.SIGMA_HEUN1, aux_out=e)):
        with pytest.raises(AssertionError):
            ops.sigma_step(x, e, c, **bad)
    with pytest.raises(AssertionError):
        ops.sigma_step(x, e.double(), c, P.SIGMA_EULER)
    with pytest.raises(AssertionError):
        ops.sigma_step(x, e[:32], c, P.SIGMA_EULER)
    with pytest.raises(AssertionError):
        ops.sigma_step(x, e, dict(c, nonsense=1.0), P.SIGMA_EULER)
    with pytest.raises(AssertionError):
        ops.sigma_scale(x.double(), 2.0)
    with pytest.raises(AssertionError):
        ops.sigma_add_noise(x.reshape(2, 32), z.reshape(2, 32), d1[:3])
    with pytest.raises(AssertionError):
        ops.sigma_add_noise(x.reshape(2, 32), z.reshape(2, 32), d1[:2], out=x.reshape(2, 32))
    # the library: partial overlaps, which the wrapper's pointer comparison does not see
    big = torch.zeros(256, device=DEV)
    for xx, bad in ((x, dict(mode=P.SIGMA_EULER, out=big[8:72], aux_out=big[40:104])),                    # the two outputs overlap in part
                    (big[128:192], dict(mode=P.SIGMA_EULER, out=big[130:194])),                          # x_next overlaps x without being it
                    (x, dict(mode=P.SIGMA_HEUN2, d1=d1, saved=big[0:64], out=big[4:68])),                # ... the saved sample
                    (x, dict(mode=P.SIGMA_HEUN2, d1=big[0:64], saved=saved, out=big[60:124])),           # x_next overlaps d1
                    (x, dict(mode=P.SIGMA_ANCESTRAL, noise=big[0:64], out=big[32:96])),                  # x_next overlaps the noise
                    (big[0:64], dict(mode=P.SIGMA_HEUN1, aux_out=big[32:96]))):                          # aux_out overlaps x
        with pytest.raises(L.DpHipError) as err:
            ops.sigma_step(xx, e, c, **bad)
        assert err.value.code == 1                                               # hipErrorInvalidValue, before any launch
    with pytest.raises(L.DpHipError) as err:
        ops.sigma_scale(big[0:64], 2.0, out=big[2:66])
    assert err.value.code == 1
    with pytest.raises(L.DpHipError) as err:
        ops.sigma_add_noise(big[0:64].reshape(2, 32), z.reshape(2, 32), d1[:2].contiguous(), out=big[32:96].reshape(2, 32))
    assert err.value.code == 1
    # the library alone: null pointers that the mode reads or writes, modes and types outside the table
    coef = L.SigmaCoef(**c)
    out, aux = torch.empty_like(x), torch.empty_like(x)

    def raw(mode, pred=0, x_=x, e_=e, z_=None, d1_=None, xs_=None, out_=out, aux_=aux, coef_=coef):
        p = ops._p
        return lib.dp_sigma_step(p(x_), p(e_), p(z_), p(d1_), p(xs_), mode, pred, ctypes.byref(coef_) if coef_ is not None else None, p(out_),
                                 p(aux_), 64, None)
    for rc in (raw(P.SIGMA_EULER, x_=None), raw(P.SIGMA_EULER, e_=None), raw(P.SIGMA_EULER, out_=None), raw(P.SIGMA_EULER, aux_=None),
               raw(P.SIGMA_EULER, coef_=None), raw(P.SIGMA_ANCESTRAL), raw(P.SIGMA_HEUN1, aux_=None), raw(P.SIGMA_HEUN2),
               raw(P.SIGMA_HEUN2, d1_=d1), raw(P.SIGMA_HEUN2, xs_=saved), raw(4), raw(-1), raw(P.SIGMA_EULER, pred=3), raw(P.SIGMA_EULER, pred=-1),
               raw(P.SIGMA_ANCESTRAL, pred=2, z_=z), raw(P.SIGMA_HEUN1, pred=2), raw(P.SIGMA_HEUN2, pred=2, d1_=d1, xs_=saved),
               lib.dp_sigma_scale(None, 2.0, ops._p(out), 64, None), lib.dp_sigma_scale(ops._p(x), 2.0, None, 64, None),
               lib.dp_sigma_add_noise(ops._p(x), ops._p(z), None, 2, 32, ops._p(out), None),
               lib.dp_sigma_add_noise(ops._p(x), None, ops._p(d1), 2, 32, ops._p(out), None)):
        assert rc == 1
    assert lib.dp_launch_count() == before
    torch.cuda.synchronize()
    assert bool((big == 0).all())
    # what a mode neither reads nor writes may be anything, null included: one launch each; n <= 0 is a no-op
    assert raw(P.SIGMA_HEUN2, d1_=d1, xs_=saved, aux_=None) == 0 and raw(P.SIGMA_HEUN1, z_=out, d1_=out, xs_=out) == 0
    assert lib.dp_launch_count() == before + 2
    assert lib.dp_sigma_scale(None, 2.0, None, 0, None) == 0 and lib.dp_sigma_add_noise(None, None, None, 0, 5, None, None) == 0
    assert lib.dp_launch_count() == before + 2


# ---------------------------------------------------------------------------------------------- schedulers against reference
@pytest.fixture(scope='module')
def steps():
    return R.load(R.STEPS_FILE)


@pytest.mark.parametrize('case', [c for c in R.TABLE_CASES if c[3] in (7, 10) and c[1] == 'linear'], ids=R.table_name)
def test_host_tables_on_this_machine_equal_the_fixtures(case):
    g = R.load(R.TABLES_FILE)
    s = _sched(case[0], **R.table_kwargs(case))
    s.set_timesteps(case[3], device=DEV)
    name = R.table_name(case)
    assert s._ts == g[name + ':timesteps'].tolist() and s._sig.numpy().tobytes() == g[name + ':sigmas'].tobytes()
    assert s.timesteps.device.type == 'cuda' and s.sigmas.device.type == 'cuda' and s._sig.device.type == 'cpu'


@pytest.mark.parametrize('run', R.STEP_RUNS, ids=R.run_name)
def test_scheduler_steps_on_the_reference_single_steps(run, steps, report):
    """The teacher-forced run of the fixture through scheduler.step on the device: call k is handed the seeded x_k, e_k.  Every call is
    one launch of the instantiation the fixture names; every stored call lies within the bound of fp64 and equals the reference's fp32
    bits (prev_sample, and pred_original_sample where there is one)."""
    L = pkg('_lib')
    lib = L.load()
    sname, cls, kw, skw, n, at = run
    name = R.run_name(run)
    pred = R.PRED_OF[kw.get('prediction_type', 'epsilon')]
    s = _sched(cls, **kw)
    s.set_timesteps(n)
    s.is_scale_input_called = True
    assert s._ts == steps[name + ':timesteps'].tolist()
    extra = dict(skw, generator=torch.Generator().manual_seed(R.GEN_SEED)) if cls != 'heun' else {}
    failed = []
    for k in range(len(s._ts)):
        x, e = (t.to(DEV) for t in R.step_inputs(k))
        x_keep, e_keep = x.clone(), e.clone()
        before = lib.dp_launch_count()
        o = s.step(e, s._ts[k], x, **extra)
        assert _launched(lib, before) == [_branch(R.mode_of_call(cls, k), pred)]
        assert torch.equal(x, x_keep) and torch.equal(e, e_keep)
        if k not in at:
            continue
        key = '%s@%d' % (name, k)
        outs = [('prev', o.prev_sample, '')] + ([('x0', o.pred_original_sample, '_x0')] if cls != 'heun' else [])
        for what, t, suffix in outs:
            got = t.cpu().numpy()
            y64 = steps[key + (':prev64' if what == 'prev' else ':x0_64')]
            e_ref = float(steps[key + ':e_ref32' + suffix])
            err = float(np.abs(got.astype(np.float64) - y64).max())
            bound = R.single_step_bound(e_ref, y64)
            same32 = bool(np.array_equal(got, steps[key + (':prev32' if what == 'prev' else ':x0_32')]))
            _line(report, 'step/%s/%s' % (key, what), mode=R.MODES[R.mode_of_call(cls, k)], churn=int(steps[name + ':churn'][k]), err=err, bound=bound,
                  e_ref32=e_ref, equals_reference_fp32=same32)
            if err > bound or not same32:
                failed.append((key, what, err, bound, same32))
    assert not failed, failed


def test_scale_model_input_and_add_noise_equal_the_references(steps):
    x, z = (torch.from_numpy(gc.det_noise(R.STEP_SHAPE, 900 + i)).to(DEV) for i in range(2))
    for i, (cls, kw, idx) in enumerate(R.SCALE_CASES):
        s = _sched(cls, **kw)
        s.set_timesteps(7)
        y = s.scale_model_input(x * R.X_SCALE, s._ts[idx])
        assert np.array_equal(y.cpu().numpy(), steps['scale:%d:out' % i])
    for i, (cls, kw, idx) in enumerate(R.NOISE_CASES):
        s = _sched(cls, **kw)
        s.set_timesteps(10)
        x_keep = x.clone()
        y = s.add_noise(x, z, s.timesteps[idx])
        assert np.array_equal(y.cpu().numpy(), steps['noise:%d:out' % i]) and torch.equal(x, x_keep)


# ---------------------------------------------------------------------------------------------- no read-back, one launch
@pytest.mark.parametrize('cls,kw', [('euler', dict()), ('euler', dict(prediction_type='v_prediction', use_karras_sigmas=True)),
                                    ('ancestral', dict()), ('heun', dict())], ids=['euler', 'euler_v_karras', 'ancestral', 'heun'])
def test_step_is_one_launch_scaling_one_more_and_neither_reads_back(cls, kw):
    L = pkg('_lib')
    lib = L.load()
    s = _sched(cls, **kw)
    s.set_timesteps(5)
    x, e = (t.to(DEV) for t in R.step_inputs(0))
    first, x0 = x, x.clone()
    s.scale_model_input(x, s._ts[0])                                            # the buffers of its own exist
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


def test_euler_without_churn_uploads_no_noise(monkeypatch):
    """With gamma == 0 the draw is made where the generator lives (its stream advances as the reference's does) and not uploaded."""
    diffusion = pkg('diffusion')
    s = _sched('euler')
    s.set_timesteps(5)
    x, e = (t.to(DEV) for t in R.step_inputs(0))
    gen, twin = torch.Generator().manual_seed(5), torch.Generator().manual_seed(5)
    drawn = []
    real = diffusion.randn_tensor
    monkeypatch.setattr(diffusion, 'randn_tensor', lambda *a, **k: drawn.append(real(*a, **k)) or drawn[-1])
    s.step(e, s._ts[0], x, generator=gen)
    torch.randn(R.STEP_SHAPE, generator=twin)
    assert len(drawn) == 1 and drawn[0].device.type == 'cpu' and torch.equal(gen.get_state(), twin.get_state())
    s.step(e, s._ts[1], x, generator=gen, s_churn=3.0)                           # with churn it is uploaded and read
    assert len(drawn) == 2 and drawn[1].device.type == 'cuda'


# ---------------------------------------------------------------------------------------------- fractional timesteps on the HIP UNet
@pytest.fixture(scope='module')
def tiny():
    return make_model(gc.TINY_CFG, R.MODEL_SEED)


@pytest.fixture(scope='module')
def chains():
    return R.load(R.CHAINS_FILE)


def _x(seed=7):
    ss = gc.TINY_CFG['sample_size']
    return torch.from_numpy(gc.det_noise((R.CHAIN_B, gc.TINY_CFG['in_channels'], ss, ss), seed)).to(DEV)


def test_fractional_timesteps_through_both_sampling_forwards(tiny):
    x = _x()
    with torch.no_grad():
        want = tiny(x, torch.tensor([832.5, 832.5], device=DEV)).sample.clone()
        want_int = tiny(x, 888).sample.clone()
        assert not torch.equal(want, tiny(x, 832).sample) and not torch.equal(want, tiny(x, 833).sample)
        got = {}
        for replay in (False, True):
            fwd = tiny.sampling_forward(tuple(x.shape), 4, replay=replay)
            assert type(fwd).__name__ == ('_CapturedForward' if replay else '_EagerForward')
            try:
                got[replay] = [fwd(x, 832.5).clone(), fwd(x, torch.tensor(832.5, dtype=torch.float64)).clone(),
                               fwd(x, torch.tensor(832.5, device=DEV)).clone(), fwd(x, 888.0).clone(), fwd(x, 832.5).clone()]
                if replay:
                    first = fwd.call_f
                    assert first is not None and fwd.tf.dtype == torch.float32 and fwd.t.dtype == torch.long
                    fwd(x, 100.25)
                    assert fwd.call_f is first                                  # captured at most once per kind of timestep
            finally:
                fwd.close()
    for replay in (False, True):
        a, b, c, d, e = got[replay]
        assert torch.equal(a, want) and torch.equal(b, want) and torch.equal(c, want) and torch.equal(e, want), replay
        assert torch.equal(d, want_int), replay                                  # 888.0 as a float: the bits of 888 as an int


def test_the_integer_path_is_unchanged_by_a_float_call(tiny):
    x = _x(8)
    with torch.no_grad():
        for replay in (False, True):
            alone = tiny.sampling_forward(tuple(x.shape), 4, replay=replay)
            try:
                want = [alone(x, 500).clone(), alone(x, torch.tensor(3, device=DEV)).clone(), alone(x, torch.tensor([7, 900], device=DEV)).clone()]
                assert getattr(alone, 'call_f', None) is None                    # no float capture without a float call
            finally:
                alone.close()
            fwd = tiny.sampling_forward(tuple(x.shape), 4, replay=replay)
            try:
                a = fwd(x, 500).clone()
                fwd(x, 979.61)
                b, c, d = fwd(x, 500).clone(), fwd(x, torch.tensor(3, device=DEV)).clone(), fwd(x, torch.tensor([7, 900], device=DEV)).clone()
            finally:
                fwd.close()
            assert torch.equal(a, want[0]) and torch.equal(b, want[0]) and torch.equal(c, want[1]) and torch.equal(d, want[2]), replay
        assert torch.equal(tiny(x, 979.6).sample, tiny(x, 979).sample)           # a bare Python float to forward(): truncated, as before


# ---------------------------------------------------------------------------------------------- chains on the HIP UNet
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
    for cls, kw, n in (('euler', dict(beta_schedule='scaled_linear', beta_start=0.0015, beta_end=0.0195), 6), ('heun', dict(use_karras_sigmas=True), 4)):
        pipe = diffusion.LDMPipeline(vqvae=vqm, unet=tiny, scheduler=_sched(cls, **kw))
        images = pipe(batch_size=B, generator=torch.Generator().manual_seed(9), num_inference_steps=n, output_type='numpy').images
        assert any(t != round(t) for t in pipe.scheduler._ts)                    # fractional timesteps reached the model
        x_T = diffusion.randn_tensor((B, gc.TINY_CFG['in_channels'], ss, ss), generator=torch.Generator().manual_seed(9)).to(DEV)
        lat = _loop(tiny, cls, kw, x_T, n, False, True)[0][-1]
        with torch.no_grad():
            dec = vqm.decode(lat).sample
        want = (dec / 2 + 0.5).clamp(0, 1).cpu().permute(0, 2, 3, 1).numpy()
        assert images.shape == want.shape and images.shape[0] == B and np.isfinite(images).all()
        assert np.array_equal(images, want) and images.min() != images.max()
