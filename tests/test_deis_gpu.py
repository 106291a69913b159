"""DEISMultistepScheduler and DPMSolverSinglestepScheduler on the MI355X: dp_deis_step and dp_dpm_single_step (csrc/deis.hip) and the two
classes of diffusion.py on the HIP UNet2DModel, against the fixtures the reference wrote (tests/golden/make_golden_deis.py).

Bounds (the project's existing ones, tests/test_dpm_solver_gpu.py; none fixed by hand):
  * the kernels equal the stand-in tests/mock_ops_deis.py bit for bit: both are the same sequence of correctly rounded fp32
    operations (the stand-in runs torch's eager fp32 ops on the device, one rounding each, scalars as 0-d device tensors);
  * a fixture step lies within max(4 e_ref32, 4 * 2^-24 * max|y64|) of the fixture's fp64 result y64, e_ref32 being the reference's
    own fp32 distance stored beside it; bit equality with the reference's fp32 result is reported beside it;
  * a chain state lies within 10 x the reference fp32 chain's own gap at that state + 1e-5 of the fp64 chain.
Measured on one MI355X (profiles/deis_gpu_tests.txt holds every value beside its bound; 64 cases in 3.8 s): all 106 fixture steps
equal the reference's fp32 result bit for bit (worst error 0.25 of the bound), the chains at most 0.13 of theirs."""
import ctypes

import numpy as np
import pytest
import torch

import golden_common as gc
import deis_ref as R
import mock_ops_deis as mock
from helpers import make_model, pkg

pytestmark = pytest.mark.gpu
DEV = 'cuda'

# ---- the launch sites of csrc/deis.hip (tests/test_deis_cpu.py compares this table with the source)
LAUNCH_SITES = {'deis.hip': 7}
BRANCHES = ['(deis_step_kernel<1>)', '(deis_step_kernel<2>)', '(deis_step_kernel<3>)', '(dpm_single_step_kernel<1, false>)',
            '(dpm_single_step_kernel<2, false>)', '(dpm_single_step_kernel<3, false>)', '(dpm_single_step_kernel<3, true>)']
# branch -> the (model type, data_pred) pairs run through it (data_pred None: dp_deis_step); every pair runs untreated, and
# treated (with stats) unless data_pred is False
_PAIRS = [(p, d) for d in (True, False) for p in range(3)]
CASES = {b: ([(p, None) for p in range(3)] if b.startswith('(deis') else list(_PAIRS)) for b in BRANCHES}
MAX_BLOCKS = 4096                                  # DP_DEIS_MAX_BLOCKS
CAP = MAX_BLOCKS * 256 * 4                         # elements one launch covers without a second grid-stride trip (16-byte path)
SIZES = [1, 3, 4, 5, 255, 1024, 1027]
BIG = CAP + 1029
BIG_BRANCHES = [b for b in BRANCHES if b != '(dpm_single_step_kernel<3, true>)']          # one site per kernel and order
ROWS = [5, 48, 1027]                               # B = 3 rows: not divisible by 4 (rows of differing phase, all scalar), divisible, odd
LDS_MAX = 16384                                    # DP_THRESHOLD_LDS_MAX: a longer row takes the quantile's multi-block route


def _parse(branch):
    """(entry point, order, heun) of a launch site."""
    if branch.startswith('(deis'):
        return 'deis', int(branch[len('(deis_step_kernel<')]), False
    return 'single', int(branch[len('(dpm_single_step_kernel<')]), branch.endswith('true>)')


def _launched(lib, before):
    n = lib.dp_launch_count() - before
    arr = (ctypes.c_char_p * 256)()
    k = lib.dp_recent_launches(arr, 256)
    return [arr[i].decode() for i in range(k)][k - n:] if n else []


def _line(report, key, **kw):
    report['deis/' + key] = kw
    print('deis/%s %s' % (key, ' '.join('%s=%.3e' % (k, v) if isinstance(v, float) else '%s=%s' % (k, v) for k, v in kw.items())))


def _sched(cls, **kw):
    return getattr(pkg('diffusion'), R.CLASSES[cls])(**kw)


def _call(mod, entry, order, heun, pred, data, bufs, coef, **kw):
    """One step through `mod` (ops or the stand-in) with the buffers (x, xs, m, m1, m2)."""
    x, xs, m, m1, m2 = bufs
    if entry == 'deis':
        return mod.deis_step(x, m, coef, order=order, pred=pred, m1=m1, m2=m2, **kw)
    return mod.dpm_single_step(x, m, coef, order=order, pred=pred, data_pred=data, heun=heun, xs=xs, m1=m1, m2=m2, **kw)


def _coef(entry, seed):
    return R.random_coefs(mock.DEIS_COEF if entry == 'deis' else mock.DPM_SINGLE_COEF, seed)


# ---------------------------------------------------------------------------------------------- kernel against stand-in
@pytest.fixture(scope='module')
def seeded():
    gen = torch.Generator().manual_seed(17)
    return tuple(torch.randn(BIG + 1, generator=gen).to(DEV) for _ in range(5))


def _compare_flat(ops, lib, branch, n, seeded, offsets, aliases):
    entry, order, heun = _parse(branch)
    done = 0
    for pred, data in CASES[branch]:
        c = _coef(entry, 10 * order + pred)
        for off in offsets:
            bufs = tuple(t[off:off + n] for t in seeded)
            assert bufs[0].data_ptr() % 16 == 4 * off
            want, want0 = _call(mock, entry, order, heun, pred, data, bufs, c)
            buf = torch.full((n + 2,), 7.0, device=DEV)
            buf0 = torch.full((n + 2,), 7.0, device=DEV)
            before = lib.dp_launch_count()
            got, got0 = _call(ops, entry, order, heun, pred, data, bufs, c, out=buf[off:off + n], m0_out=buf0[off:off + n])
            assert _launched(lib, before) == [branch]
            assert torch.equal(got, want) and torch.equal(got0, want0), (branch, n, pred, data, off)
            for b in (buf, buf0):                                                # nothing written before the start or past the end
                assert float(b[off + n]) == 7.0 and (off == 0 or float(b[0]) == 7.0) and float(b[n + 1]) == 7.0
            done += 1
            if not aliases:
                continue
            # in place: x_next is x (dp_dpm_single_step: then xs), m0_out is the oldest history buffer this step reads
            x, xs, m, m1, m2 = bufs
            for target in ((0,) if entry == 'deis' or order == 1 else (0, 1)):
                own = torch.empty(n + 1, device=DEV)[off:off + n].copy_(bufs[target])
                old = torch.empty(n + 1, device=DEV)[off:off + n].copy_(m2 if order == 3 else m1)
                al = (own if target == 0 else x, own if target == 1 else xs, m, old if order == 2 else m1, old if order == 3 else m2)
                got, got0 = _call(ops, entry, order, heun, pred, data, al, c, out=own, m0_out=old if order > 1 else None)
                assert got is own and torch.equal(own, want) and torch.equal(got0, want0), (branch, n, pred, data, off, 'in place', target)
                assert order == 1 or got0 is old
                done += 1
        # pointers of two alignments: every access is a 4-byte one
        bufs = tuple(t[:n] for t in seeded)
        want, want0 = _call(mock, entry, order, heun, pred, data, bufs, c)
        got, got0 = _call(ops, entry, order, heun, pred, data, bufs, c, out=torch.empty(n + 1, device=DEV)[1:])
        assert torch.equal(got, want) and torch.equal(got0, want0), (branch, n, pred, data, 'two alignments')
        done += 1
    return done


@pytest.mark.parametrize('branch', BRANCHES)
def test_kernel_equals_the_stand_in(branch, seeded, report):
    """Every launch site with every model type (and both algorithms) at every flat size, element offsets 0 (16-byte aligned) and 1
    (a scalar head of 3), out of place and with each permitted alias; one pointer of another alignment (all 4-byte accesses);
    nothing written outside [0, n)."""
    ops, lib = pkg('ops'), pkg('_lib').load()
    done = sum(_compare_flat(ops, lib, branch, n, seeded, (0, 1), True) for n in SIZES)
    _line(report, 'kernel_vs_stand_in/%s' % branch, sizes=len(SIZES), cases=done, differing_elements=0)


@pytest.mark.parametrize('branch', BIG_BRANCHES)
def test_kernel_equals_the_stand_in_on_the_second_grid_stride_trip(branch, seeded, report):
    """4096 * 256 * 4 + 1029 elements: the grid is capped and every lane makes a second trip; one model type per site."""
    ops, lib = pkg('ops'), pkg('_lib').load()
    entry, order, heun = _parse(branch)
    pred, data = CASES[branch][order % 3]
    c = _coef(entry, 40 + order)
    bufs = tuple(t[:BIG] for t in seeded)
    want, want0 = _call(mock, entry, order, heun, pred, data, bufs, c)
    before = lib.dp_launch_count()
    got, got0 = _call(ops, entry, order, heun, pred, data, bufs, c)
    assert _launched(lib, before) == [branch]
    assert torch.equal(got, want) and torch.equal(got0, want0)
    _line(report, 'kernel_vs_stand_in_big/%s' % branch, n=BIG, differing_elements=0)


@pytest.mark.parametrize('branch', BRANCHES)
def test_thresholded_rows_equal_the_stand_in(branch, seeded, report):
    """With `stats` the data is [B, n] rows: B = 3 with n = 5, 48 and 1027 at element offsets 0 and 1, every model type, s from the
    quantile kernel; the three images are scaled so that s is 1, between and the maximum.  One row length above DP_THRESHOLD_LDS_MAX
    goes through the quantile's multi-block route."""
    ops, lib = pkg('ops'), pkg('_lib').load()
    entry, order, heun = _parse(branch)
    done = 0
    for n in ROWS + ([LDS_MAX + 4] if order == 2 else []):
        for pred, data in CASES[branch]:
            if data is False:
                continue
            c = _coef(entry, 20 * order + pred)
            for off in (0, 1):
                scale = torch.tensor([0.2, 1.0, 4.0], device=DEV).reshape(3, 1)
                x, xs, m, m1, m2 = (t[off:off + 3 * n].reshape(3, n) for t in seeded)
                x, m = (x * scale).contiguous(), (m * scale).contiguous()
                if off:                                                          # the products are fresh buffers: put them back at the offset
                    x, m = (torch.empty(3 * n + 1, device=DEV)[1:].reshape(3, n).copy_(t) for t in (x, m))
                stats = ops.x0_abs_quantile(x, m, pred, c['sa'], c['sb'], 0.9, 2.0)
                s = stats[:, 3].tolist()
                assert 1.0 <= s[0] <= s[1] <= s[2] <= 2.0 and s[0] < s[2], s
                bufs = (x, xs, m, m1, m2)
                want, want0 = _call(mock, entry, order, heun, pred, data, bufs, c, stats=stats)
                buf = torch.full((3 * n + 2,), 7.0, device=DEV)
                before = lib.dp_launch_count()
                got, got0 = _call(ops, entry, order, heun, pred, data, bufs, c, stats=stats, out=buf[off:off + 3 * n].reshape(3, n))
                assert _launched(lib, before) == [branch]
                assert torch.equal(got, want) and torch.equal(got0, want0), (branch, n, pred, off)
                assert float(buf[off + 3 * n]) == 7.0 and (off == 0 or float(buf[0]) == 7.0) and float(buf[3 * n + 1]) == 7.0
                done += 1
    _line(report, 'rows_vs_stand_in/%s' % branch, cases=done, differing_elements=0)


def test_the_wrappers_and_the_library_refuse_what_the_kernels_are_not_written_for(seeded):
    ops, L = pkg('ops'), pkg('_lib')
    x, xs, e, m1, m2 = (t[:64].clone() for t in seeded)
    cd, cs = _coef('deis', 1), _coef('single', 2)
    for bad in (dict(out=e), dict(m0_out=x), dict(m0_out=e), dict(order=2), dict(order=3, m1=m1), dict(order=2, m1=m1, out=m1),
                dict(order=1, out=x, m0_out=x), dict(order=3, m1=m1, m2=m2, m0_out=m1), dict(order=4), dict(order=0), dict(pred=3)):
        kw = dict(order=1)
        kw.update(bad)
        with pytest.raises(AssertionError):
            ops.deis_step(x, e, cd, **kw)
        with pytest.raises(AssertionError):
            ops.dpm_single_step(x, e, cs, xs=xs, **kw)
    for bad in (dict(order=2, m1=m1), dict(order=2, m1=m1, xs=xs, m0_out=xs), dict(order=1, data_pred=False, stats=torch.ones(1, 4, device=DEV))):
        with pytest.raises(AssertionError):
            ops.dpm_single_step(x, e, cs, **bad)
    with pytest.raises(AssertionError):
        ops.deis_step(x, e.double(), cd)
    with pytest.raises(AssertionError):
        ops.deis_step(x, e[:32], cd)
    with pytest.raises(AssertionError):
        ops.deis_step(x.reshape(2, 32), e.reshape(2, 32), cd, stats=torch.ones(3, 4, device=DEV))
    big = torch.zeros(256, device=DEV)
    lib = L.load()
    before = lib.dp_launch_count()
    for fn, extra in ((ops.deis_step, {}), (ops.dpm_single_step, dict(xs=xs))):
        c = cd if fn is ops.deis_step else cs
        for xx, bad in ((x, dict(out=big[8:72], m0_out=big[40:104])),            # the two outputs overlap in part
                        (x, dict(order=2, m1=big[0:64], m0_out=big[4:68])),      # m0_out overlaps the history without being it
                        (big[128:192], dict(out=big[130:194]))):                 # x_next overlaps x without being it
            kw = dict(order=1)
            kw.update(extra)
            kw.update(bad)
            with pytest.raises(L.DpHipError) as err:
                fn(xx, e, c, **kw)
            assert err.value.code == 1                                           # hipErrorInvalidValue, before any launch
    with pytest.raises(L.DpHipError) as err:                                     # x_next overlaps the saved sample without being it
        ops.dpm_single_step(x, e, cs, order=2, xs=big[128:192], m1=m1, out=big[130:194])
    assert err.value.code == 1
    st = torch.ones(256, device=DEV)
    with pytest.raises(L.DpHipError) as err:                                     # stats inside an output
        ops.deis_step(x.reshape(1, 64), e.reshape(1, 64), cd, stats=st[:4].reshape(1, 4), out=st[:64].reshape(1, 64))
    assert err.value.code == 1
    assert lib.dp_launch_count() == before


# ---------------------------------------------------------------------------------------------- kernel against reference
@pytest.fixture(scope='module')
def steps():
    return R.load_steps()


@pytest.mark.parametrize('run', R.STEP_RUNS, ids=R.run_name)
def test_scheduler_steps_on_the_reference_single_steps(run, steps, report):
    """The teacher-forced run of the fixture through scheduler.step on the device: step k is handed the seeded x_k, e_k.  A step is
    one launch of csrc/deis.hip, and with thresholding one of threshold.hip before it."""
    lib = pkg('_lib').load()
    cls, kw, n, at = run
    name = R.run_name(run)
    thr = R.run_thresholds(run)
    s = _sched(cls, **kw)
    s.set_timesteps(n)
    assert s._ts == steps[name + ':timesteps'].tolist()
    orders = steps[name + ':orders'].tolist()
    scale = steps.get(name + ':scale')
    for k in range(max(at) + 1):
        x, e = (t.to(DEV) for t in R.step_inputs(k, None if scale is None else scale[k]))
        before = lib.dp_launch_count()
        prev = s.step(e, s._ts[k], x).prev_sample
        assert _launched(lib, before) == (['(th_lds_kernel<false>)'] if thr else []) + [R.run_site(run, orders[k])]
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


# ---------------------------------------------------------------------------------------------- no read-back, launch counts
@pytest.mark.parametrize('cls', list(R.CLASSES))
@pytest.mark.parametrize('thr', [False, True], ids=['plain', 'thresholded'])
def test_step_launch_counts_and_nothing_read_back(cls, thr):
    L = pkg('_lib')
    lib = L.load()
    s = _sched(cls, solver_order=3, **(dict(thresholding=True, sample_max_value=2.0) if thr else {}))
    s.set_timesteps(20)
    x, e = (t.to(DEV) for t in R.step_inputs(0))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        for k in range(4):                                                       # orders 1, 2, 3 and a step on a full ring
            before = lib.dp_launch_count()
            x = s.step(e, s._ts[k], x).prev_sample
            names = _launched(lib, before)
            assert len(names) == (2 if thr else 1) and names[-1] in BRANCHES and names[:-1] == ['(th_lds_kernel<false>)'][:len(names) - 1]
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert torch.isfinite(x).all()


# ---------------------------------------------------------------------------------------------- chains on the HIP UNet
@pytest.fixture(scope='module')
def tiny():
    return make_model(gc.TINY_CFG, R.MODEL_SEED)


@pytest.fixture(scope='module')
def chains():
    return [R.load(f) for f in R.CHAINS_FILES]


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
    name, cls, kw, n, fi = chain
    g = chains[fi]
    sched = _sched(cls, **kw)
    pipe = diffusion.DDPMPipeline(tiny, sched)
    seen = []
    real = sched.step

    def spy(model_output, timestep, sample, return_dict=True):             # the step's own signature: the pipeline passes no generator
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
    replayed, eager = _loop(tiny, _sched(cls, **kw), x_T, n, True), _loop(tiny, _sched(cls, **kw), x_T, n, False)
    for a, b, c in zip(replayed, eager, xs):
        assert torch.equal(a, b) and torch.equal(a, c)


# ---------------------------------------------------------------------------------------------- LDMPipeline, pipeline directory
@pytest.mark.parametrize('cls', list(R.CLASSES))
def test_ldm_pipeline_and_a_loaded_pipeline_directory_sample(cls, tiny, tmp_path):
    import vq_ref
    diffusion, vq, syn = pkg('diffusion'), pkg('vq'), pkg('synthetic')
    vqm = vq.VQModel(**syn.VQ_TINY_CFG)
    vqm.load_state_dict({k: v.float() for k, v in vq_ref.params(syn.VQ_TINY_CFG, 3).items()})
    vqm = vqm.to(DEV).eval()
    kw = dict(solver_order=3, beta_schedule='scaled_linear', beta_start=0.0015, beta_end=0.0195)
    n, B = 6, 2
    pipe = diffusion.LDMPipeline(vqvae=vqm, unet=tiny, scheduler=_sched(cls, **kw))
    images = pipe(batch_size=B, generator=torch.Generator().manual_seed(9), num_inference_steps=n, output_type='numpy').images
    ss = gc.TINY_CFG['sample_size']
    x_T = diffusion.randn_tensor((B, gc.TINY_CFG['in_channels'], ss, ss), generator=torch.Generator().manual_seed(9)).to(DEV)
    lat = _loop(tiny, _sched(cls, **kw), x_T, n, True)[-1]
    with torch.no_grad():
        dec = vqm.decode(lat).sample
    want = (dec / 2 + 0.5).clamp(0, 1).cpu().permute(0, 2, 3, 1).numpy()
    assert images.shape == want.shape and images.shape[0] == B and np.isfinite(images).all()
    assert np.array_equal(images, want) and images.min() != images.max()
    # a pipeline directory naming the class loads and samples the explicit loop's bits
    d = str(tmp_path / 'pipe')
    diffusion.DDPMPipeline(tiny, _sched(cls, **kw)).save_pretrained(d)
    back = diffusion.DDPMPipeline.from_pretrained(d).to(DEV)
    assert type(back.scheduler).__name__ == R.CLASSES[cls]
    got = back(batch_size=B, generator=torch.Generator().manual_seed(9), num_inference_steps=n, output_type='numpy').images
    loop = _loop(tiny, _sched(cls, **kw), x_T, n, False)[-1]
    assert np.array_equal(got, (loop / 2 + 0.5).clamp(0, 1).cpu().permute(0, 2, 3, 1).numpy())
