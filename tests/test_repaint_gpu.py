"""RePaintScheduler on the MI355X: dp_repaint_step / dp_repaint_undo (csrc/repaint.hip) and diffusion.RePaintScheduler /
RePaintPipeline on the HIP UNet2DModel, against the fixtures the reference wrote (tests/golden/make_golden_repaint.py).

Bounds (none fixed by hand):
  * the kernels equal the stand-in tests/mock_ops_repaint.py bit for bit: both are the same sequence of correctly rounded fp32
    operations (the stand-in runs torch's eager fp32 ops on the device, one rounding each, scalars as 0-d device tensors);
  * a fixture step lies within max(4 e_ref32, 4 * 2^-24 * max|y64|) of the fixture's fp64 result y64, e_ref32 being the reference's
    own fp32 distance stored beside it (pndm_ref.single_step_bound), without exclusions, and it equals the reference's fp32 result
    bit for bit;
  * a chain state lies within 10 x the reference fp32 chain's own gap at that state + 1e-5 of the fp64 chain (the constants of
    tests/pndm_ref.py)."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import golden_common as gc
import repaint_ref as R
import mock_ops_repaint as mock
from helpers import make_model, pkg

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def _tf(v):
    return 'true' if v else 'false'


def _step_branch(clip, noise, full, x0):
    return '(repaint_step_kernel<%s, %s, %s, %s>)' % (_tf(clip), _tf(noise), _tf(full), _tf(x0))


def _undo_branch(k):
    return '(repaint_undo_kernel<%d>)' % k


# ---- the launch sites of csrc/repaint.hip (tests/test_repaint_cpu.py compares this table with the source)
LAUNCH_SITES = {'repaint.hip': 24}
FLAGS = list(itertools.product((False, True), repeat=4))                          # (clip, noise, full mask, x0 written)
BRANCHES = [_step_branch(*f) for f in FLAGS] + [_undo_branch(k) for k in range(1, 9)]
# branch -> what asks for it: the kernel tests below run every one of them
CASES = dict([(_step_branch(*f), ('step',) + f) for f in FLAGS] + [(_undo_branch(k), ('undo', k)) for k in range(1, 9)])
MAX_BLOCKS = 4096                                  # DP_REPAINT_MAX_BLOCKS
CAP = MAX_BLOCKS * 256 * 4                         # elements one launch covers without a second grid-stride trip (16-byte path)
SIZES = [1, 3, 4, 5, 255, 1027, CAP + 1029]
GUARD = 7.0


def _launched(lib, before):
    n = lib.dp_launch_count() - before
    arr = (ctypes.c_char_p * 256)()
    k = lib.dp_recent_launches(arr, 256)
    return [arr[i].decode() for i in range(k)][k - n:] if n else []


def _line(report, key, **kw):
    report['repaint/' + key] = kw
    print('repaint/%s %s' % (key, ' '.join('%s=%.3e' % (k, v) if isinstance(v, float) else '%s=%s' % (k, v) for k, v in kw.items())))


def _sched(**kw):
    return pkg('diffusion').RePaintScheduler(**kw)


def _coefs(eta=0.5, t=500):
    """The scheduler's own fp32 scalars at a middle step of the 10-step table."""
    s = _sched()
    s.set_timesteps(10)
    s.eta = eta
    return s.step_coefs(t)


# ---------------------------------------------------------------------------------------------- kernels against stand-in
@pytest.fixture(scope='module')
def seeded():
    n = SIZES[-1] + 8
    gen = torch.Generator().manual_seed(23)
    x, e, z, o = (torch.randn(n, generator=gen).to(DEV) for _ in range(4))
    m = torch.rand(n, generator=gen).to(DEV)
    m[::3] = 0.0
    m[1::3] = 1.0
    return x, e, z, o, m


def _guarded(n, off):
    """A view of n elements at element offset `off` inside a buffer of guard words."""
    buf = torch.full((n + 2,), GUARD, device=DEV)
    return buf, buf[off:off + n]


def _guards_intact(buf, n, off):
    return float(buf[off + n]) == GUARD and (off == 0 or float(buf[0]) == GUARD) and float(buf[n + 1]) == GUARD


def _copy_at(t, n, off):
    buf, view = _guarded(n, off)
    view.copy_(t.reshape(-1)[:n])
    return buf, view


@pytest.mark.parametrize('n', SIZES)
def test_step_kernel_equals_the_stand_in_on_flat_data(n, seeded, report):
    """The eight full-mask instantiations with every pointer 16-byte aligned, with every pointer at element offset 1 (a scalar head
    of 3) and with pointers of two phases (all 4-byte accesses), out of place and with `out is x`; the guard words either side of
    every output stay untouched, and the launch ring names the instantiation that was asked for."""
    ops, L = pkg('ops'), pkg('_lib')
    lib = L.load()
    c = _coefs()
    ran, cases = set(), 0
    for clip, noise, want_x0 in itertools.product((False, True), repeat=3):
        for phase in ('aligned', 'offset1', 'mixed'):
            off = 1 if phase == 'offset1' else 0
            x, e, z, o, m = (t[off:off + n] for t in seeded)
            if phase == 'mixed':
                e, m = seeded[1][1:1 + n], seeded[4][1:1 + n]
            assert x.data_ptr() % 16 == 4 * off
            want, want_x0v = mock.repaint_step(x, e, z, o, m, c, clip, noise, x0_out=True)
            out_off = 1 if phase != 'aligned' else 0
            obuf, out = _guarded(n, out_off)
            pbuf, p = _guarded(n, off)
            before = lib.dp_launch_count()
            got, got_x0 = ops.repaint_step(x, e, z, o, m, c, clip, noise, out=out, x0_out=p if want_x0 else None)
            assert _launched(lib, before) == [_step_branch(clip, noise, True, want_x0)]
            ran.add(_step_branch(clip, noise, True, want_x0))
            assert got is out and torch.equal(got, want), (n, clip, noise, want_x0, phase)
            assert (got_x0 is p and torch.equal(p, want_x0v)) if want_x0 else (got_x0 is None and bool((p == GUARD).all()))
            assert _guards_intact(obuf, n, out_off) and _guards_intact(pbuf, n, off)
            # out is x
            xbuf, xc = _copy_at(x, n, off)
            got, _ = ops.repaint_step(xc, e, z, o, m, c, clip, noise, out=xc, x0_out=p if want_x0 else None)
            assert got is xc and torch.equal(xc, want) and _guards_intact(xbuf, n, off), (n, clip, noise, want_x0, phase, 'in place')
            assert not want_x0 or torch.equal(p, want_x0v)
            cases += 2
    assert cases == 48 and ran == {b for b, v in CASES.items() if v[0] == 'step' and v[3]}           # the eight full-mask ones
    _line(report, 'step_kernel_vs_stand_in/n%d' % n, cases=cases, differing_elements=0)


BROADCAST_SHAPES = [((2, 3, 5, 7), 0), ((3, 2, 4, 4), 0), ((1, 1, 1, 1), 0), ((2, 3, 8, 8), 1), ((2, 3, 33, 35), 0)]


@pytest.mark.parametrize('shape,off', BROADCAST_SHAPES, ids=lambda v: 'x'.join(map(str, v)) if isinstance(v, tuple) else 'off%d' % v)
def test_step_kernel_equals_the_stand_in_on_broadcast_masks(shape, off, seeded, report):
    """Every mask form at every flag combination: (2,3,5,7) has H*W = 35, so 16-byte groups straddle planes and images; (2,3,33,35)
    does the same over several blocks; (1,1,1,1) makes every form the full one; (2,3,8,8) sits at element offset 1 (a scalar head)."""
    ops, L = pkg('ops'), pkg('_lib')
    lib = L.load()
    c = _coefs(eta=1.0)
    n = int(np.prod(shape))
    x, e, z, o = (t[off:off + n].view(shape) for t in seeded[:4])
    ran, cases = set(), 0
    for form in R.MASK_FORMS:
        ms = R.mask_shape(form, shape)
        m = seeded[4][2:2 + int(np.prod(ms))].view(ms)                              # its own phase: a broadcast mask is read 4 bytes at a time
        geo = ops.repaint_mask_geometry(shape, ms)
        full = geo[2] >= n
        if full:
            m = seeded[4][off:off + n].view(ms)
        assert torch.equal(mock.mask_values(m, geo, n).view(shape), m.expand(shape))
        for clip, noise, want_x0 in itertools.product((False, True), repeat=3):
            want, want_x0v = mock.repaint_step(x, e, z, o, m, c, clip, noise, x0_out=True)
            obuf, out = _guarded(n, off)
            pbuf, p = _guarded(n, off)
            before = lib.dp_launch_count()
            got, got_x0 = ops.repaint_step(x, e, z, o, m, c, clip, noise, out=out.view(shape), x0_out=p.view(shape) if want_x0 else None)
            assert _launched(lib, before) == [_step_branch(clip, noise, full, want_x0)]
            ran.add(_step_branch(clip, noise, full, want_x0))
            assert torch.equal(got, want) and (not want_x0 or torch.equal(got_x0, want_x0v)), (shape, form, clip, noise, want_x0)
            assert _guards_intact(obuf, n, off) and _guards_intact(pbuf, n, off)
            xbuf, xc = _copy_at(x, n, off)
            got, _ = ops.repaint_step(xc.view(shape), e, z, o, m, c, clip, noise, out=xc.view(shape))
            assert torch.equal(got, want) and _guards_intact(xbuf, n, off), (shape, form, clip, noise, 'in place')
            cases += 2
    assert cases == 80 and ran == {b for b, v in CASES.items() if v[0] == 'step' and (v[3] or n > 1)}  # n = 1: every form is full
    _line(report, 'step_kernel_broadcast/%s' % 'x'.join(map(str, shape)), cases=cases, differing_elements=0)


def test_the_mask_index_in_64_bits(seeded):
    """An `outer` of 2^31 or more takes the kernel's 64-bit index arithmetic: [1,1,H,W] read with outer = 35 * 2^26 (i / outer is 0 all
    the same) equals the 32-bit result."""
    ops, L = pkg('ops'), pkg('_lib')
    lib = L.load()
    shape = (2, 3, 5, 7)
    n = 210
    x, e, z, o = (t[:n].view(shape) for t in seeded[:4])
    m = seeded[4][:35].view(1, 1, 5, 7)
    c = _coefs()
    want, _ = mock.repaint_step(x, e, z, o, m, c, True, True)
    out = torch.empty_like(x)
    coef = L.RepaintCoef(**c)
    p = ops._p
    before = lib.dp_launch_count()
    assert lib.dp_repaint_step(p(x), p(e), p(z), p(o), p(m), 35 << 26, 0, 35, 1, 1, ctypes.byref(coef), p(out), None, n, None) == 0
    assert _launched(lib, before) == [_step_branch(True, True, False, False)]
    assert torch.equal(out, want)


@pytest.mark.parametrize('n', [1, 5, 1027, CAP + 1029])
def test_undo_kernel_equals_the_stand_in(n, seeded, report):
    """k = 1 .. 8 re-noising steps in one launch, aligned, at element offset 1 and with two phases, out of place and in place."""
    ops, L = pkg('ops'), pkg('_lib')
    lib = L.load()
    s = _sched()
    s.set_timesteps(111)
    coefs = s.undo_coefs(450)[:8]
    noise_src = [seeded[1 + j % 4] for j in range(8)]
    ran, cases = set(), 0
    for k in range(1, 9):
        for phase in ('aligned', 'offset1', 'mixed'):
            off = 1 if phase == 'offset1' else 0
            x = seeded[0][off:off + n]
            zs = [noise_src[j][off + 4 * (j // 4):off + 4 * (j // 4) + n] if phase != 'mixed' else noise_src[j][j % 3:j % 3 + n] for j in range(k)]
            want = mock.repaint_undo(x, zs, coefs[:k])
            obuf, out = _guarded(n, off)
            before = lib.dp_launch_count()
            got = ops.repaint_undo(x, zs, coefs[:k], out=out)
            assert _launched(lib, before) == [_undo_branch(k)]
            ran.add(_undo_branch(k))
            assert got is out and torch.equal(got, want) and _guards_intact(obuf, n, off), (n, k, phase)
            xbuf, xc = _copy_at(x, n, off)
            assert ops.repaint_undo(xc, zs, coefs[:k], out=xc) is xc and torch.equal(xc, want) and _guards_intact(xbuf, n, off)
            cases += 2
    assert cases == 48 and ran == {b for b, v in CASES.items() if v[0] == 'undo'}
    _line(report, 'undo_kernel_vs_stand_in/n%d' % n, cases=cases, differing_elements=0)


@pytest.mark.parametrize('n_noise', [9, 100])
def test_undo_op_chains_its_launches(n_noise, seeded):
    ops, L = pkg('ops'), pkg('_lib')
    lib = L.load()
    s = _sched()
    s.set_timesteps(1000 // n_noise)
    coefs = s.undo_coefs(300)
    assert len(coefs) == n_noise
    n = 1027
    gen = torch.Generator().manual_seed(n_noise)
    zs = [torch.randn(n, generator=gen).to(DEV) for _ in range(n_noise)]
    x = seeded[0][:n].clone()
    x0 = x.clone()
    want = mock.repaint_undo(x, zs, coefs)
    before = lib.dp_launch_count()
    got = ops.repaint_undo(x, zs, coefs)
    assert _launched(lib, before) == [_undo_branch(8)] * (n_noise // 8) + ([_undo_branch(n_noise % 8)] if n_noise % 8 else [])
    assert lib.dp_launch_count() - before == -(-n_noise // 8)
    assert torch.equal(got, want) and torch.equal(x, x0)
    assert ops.repaint_undo(x, zs, coefs, out=x) is x and torch.equal(x, want)


def test_the_unknown_part_turns_a_negative_zero_positive_on_the_device():
    ops = pkg('ops')
    x, e, o, m, z, c = R.signed_zero_case()
    x, e, o, m, z = (t.to(DEV) for t in (x, e, o, m, z))
    got, x0 = ops.repaint_step(x, e, z, o, m, c, clip=False, add_noise=False, x0_out=True)
    assert torch.signbit(x0.flatten()).tolist() == [True, False]
    assert torch.signbit(got.flatten()).tolist() == [False, False] and float(got.abs().max()) == 0.0
    got, _ = ops.repaint_step(x, e, -z, o, m, dict(c, sd=1.0), clip=False, add_noise=True)
    assert torch.signbit(got.flatten()).tolist() == [True, False]


def test_the_wrapper_and_the_library_refuse_what_the_kernels_are_not_written_for(seeded):
    ops, L = pkg('ops'), pkg('_lib')
    shape = (2, 2, 4, 4)
    x, e, z, o, m = (t[:64].clone().view(shape) for t in seeded)
    c = _coefs()
    lib = L.load()
    before = lib.dp_launch_count()
    # the wrapper: dtypes, layouts, devices, shared buffers, scalars, a mask that is the caller's to expand
    for bad in (dict(e=e.double()), dict(e=e[:1]), dict(x=x.transpose(2, 3)), dict(m=m.cpu()), dict(m=m[:, :, :1, :].contiguous()),
                dict(out=e), dict(out=m), dict(x0_out=x), dict(x0_out=z), dict(out=x, x0_out=x), dict(coef=dict(c, nonsense=1.0)),
                dict(coef={k: v for k, v in c.items() if k != 'sd'}), dict(out=torch.empty(63, device=DEV))):
        a = dict(x=x, e=e, noise=z, original=o, mask=m, coef=c, clip=True, add_noise=True)
        a.update({'noise' if k == 'z' else 'original' if k == 'o' else 'mask' if k == 'm' else k: v for k, v in bad.items()})
        with pytest.raises(AssertionError):
            ops.repaint_step(**a)
    with pytest.raises(AssertionError):
        ops.repaint_mask_geometry(shape, (2, 2, 4, 5))
    for bad in (dict(noises=[], coefs=[]), dict(noises=[z], coefs=[(1.0, 0.0)] * 2), dict(noises=[z.double()], coefs=[(1.0, 0.0)]),
                dict(noises=[z[:1]], coefs=[(1.0, 0.0)]), dict(noises=[z], coefs=[(1.0, 0.0)], out=z)):
        with pytest.raises(AssertionError):
            ops.repaint_undo(x, **bad)
    # the library: partial overlaps, which the wrapper's pointer comparison does not see
    big = torch.zeros(256, device=DEV)
    v = lambda a: big[a:a + 64].view(shape)                                       # noqa: E731
    for a in (dict(x=v(128), out=v(130)),                                            # out overlaps x without being it
              dict(e=v(0), out=v(32)), dict(noise=v(0), out=v(60)), dict(original=v(0), out=v(4)), dict(mask=v(0), out=v(63)),
              dict(out=v(8), x0_out=v(40)), dict(x=v(0), x0_out=v(32)), dict(mask=v(0), x0_out=v(32)),
              dict(mask=big[0:16].view(1, 1, 4, 4), out=v(12))):                   # the broadcast mask's own 16 elements
        b = dict(x=x, e=e, noise=z, original=o, mask=m, coef=c, clip=True, add_noise=True)
        b.update(a)
        with pytest.raises(L.DpHipError) as err:
            ops.repaint_step(**b)
        assert err.value.code == 1                                               # hipErrorInvalidValue, before any launch
    for a in (dict(x=v(0), out=v(32)), dict(noises=[v(0)], out=v(60)), dict(noises=[z, v(0)], out=v(4))):
        b = dict(x=x, noises=[z], coefs=[(0.5, 0.5)] * len(a.get('noises', [z])))
        b.update(a)
        with pytest.raises(L.DpHipError) as err:
            ops.repaint_undo(**b)
        assert err.value.code == 1
    # the library alone: null pointers, a mask geometry outside the rule, k outside 1 .. 8
    coef = L.RepaintCoef(**c)
    out = torch.empty_like(x)
    p = ops._p

    def raw(x_=x, e_=e, z_=z, o_=o, m_=m, geo=(64, 0, 64), coef_=coef, out_=out):
        return lib.dp_repaint_step(p(x_), p(e_), p(z_), p(o_), p(m_), geo[0], geo[1], geo[2], 1, 1,
                                   ctypes.byref(coef_) if coef_ is not None else None, p(out_), None, 64, None)
    for rc in (raw(x_=None), raw(e_=None), raw(z_=None), raw(o_=None), raw(m_=None), raw(coef_=None), raw(out_=None),
               raw(geo=(64, 0, 0)), raw(geo=(0, 0, 0)), raw(geo=(16, 0, 32)), raw(geo=(48, 0, 32)), raw(geo=(64, -16, 16)),
               raw(geo=(32, 8, 16)), raw(geo=(64, 0, -1))):
        assert rc == 1
    uc = L.RepaintUndoCoef()
    uc.z[0], uc.a[0], uc.b[0] = z.data_ptr(), 0.5, 0.5

    def raw_undo(k, x_=x, coef_=uc, out_=out):
        return lib.dp_repaint_undo(p(x_), ctypes.byref(coef_) if coef_ is not None else None, k, p(out_), 64, None)
    for rc in (raw_undo(0), raw_undo(9), raw_undo(-1), raw_undo(1, x_=None), raw_undo(1, coef_=None), raw_undo(1, out_=None),
               raw_undo(2)):                                                      # z[1] is null
        assert rc == 1
    assert lib.dp_launch_count() == before
    torch.cuda.synchronize()
    assert bool((big == 0).all())
    # what is in the rule launches: one image of a strided mask, entries past k ignored, n = 0 a no-op
    assert raw(geo=(64, 8, 16)) == 0 and raw_undo(1) == 0 and lib.dp_launch_count() == before + 2
    assert lib.dp_repaint_step(None, None, None, None, None, 0, 0, 0, 1, 1, None, None, None, 0, None) == 0
    assert lib.dp_repaint_undo(None, None, 0, None, 0, None) == 0 and lib.dp_launch_count() == before + 2
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- scheduler against reference
@pytest.fixture(scope='module')
def steps():
    return R.load(R.STEPS_FILE)


@pytest.mark.parametrize('case', [c for c in R.TABLE_CASES if c[0] <= 250], ids=R.table_name)
def test_host_tables_on_this_machine_equal_the_fixtures(case):
    s = _sched()
    s.set_timesteps(*case)
    assert s._ts == R.load(R.TABLES_FILE)[R.table_name(case)].tolist()


def test_scheduler_steps_on_the_reference_single_steps(steps, report):
    """Every fixture step through scheduler.step on the device, the noise drawn from the fixture's CPU generator: the host's scalars
    equal the fixture's bits, prev_sample and pred_original_sample equal the reference's fp32 bits and lie within the bound of fp64,
    in exactly one launch of the instantiation the case asks for, and no input is written."""
    L = pkg('_lib')
    lib = L.load()
    failed = []
    for k, (name, kw, n, eta, t, form) in enumerate(R.STEP_CASES):
        key = 'step:' + name
        s = _sched(**kw)
        s.set_timesteps(n)
        s.eta = eta
        host = R.step_inputs(k, form)
        x, e, o, m = (v.to(DEV) for v in host)
        differing = [nm for i, nm in enumerate(pkg('ops').REPAINT_COEF) if np.float32(s.step_coefs(t)[nm]).tobytes() != steps[key + ':coefs'][i].tobytes()]
        before = lib.dp_launch_count()
        r = s.step(e, t, x, o, m, generator=R.noise_generator(k))
        assert _launched(lib, before) == [_step_branch(kw.get('clip_sample', True), t > 0 and eta > 0, form == 'full', True)]
        assert all(torch.equal(a.cpu(), b) for a, b in zip((x, e, o, m), host))     # a step writes none of its inputs
        line = {}
        for tag, got, e_ref in (('prev', r.prev_sample, 'e_ref32'), ('x0', r.pred_original_sample, 'e_ref32_x0')):
            got = got.cpu().numpy()
            y64 = steps['%s:%s64' % (key, 'prev' if tag == 'prev' else 'x0_')]
            y32 = steps['%s:%s32' % (key, 'prev' if tag == 'prev' else 'x0_')]
            err = float(np.abs(got.astype(np.float64) - y64).max())
            bound = R.single_step_bound(steps[key + ':' + e_ref], y64)
            same32 = bool(np.array_equal(got, y32))
            line.update({tag + '_err': err, tag + '_bound': bound, tag + '_equals_reference_fp32': same32})
            if err > bound or not same32:
                failed.append((key, tag, err, bound, same32))
        _line(report, key, differing_scalars=','.join(differing) or 'none', **line)
        if differing:
            failed.append((key, differing))
    assert not failed, failed


def test_scheduler_undo_steps_on_the_reference(steps, report):
    L = pkg('_lib')
    lib = L.load()
    for k, case in enumerate(R.UNDO_CASES):
        n_inf, t = case
        key = R.undo_name(case)
        s = _sched()
        s.set_timesteps(n_inf)
        assert np.array(s.undo_coefs(t), np.float32).tobytes() == steps[key + ':coefs'].tobytes()
        x = R.undo_input(k).to(DEV)
        x0 = x.clone()
        before = lib.dp_launch_count()
        y = s.undo_step(x, t, generator=R.noise_generator(1000 + k))
        n = R.UNDO_N[k]
        assert lib.dp_launch_count() - before == -(-n // 8) and torch.equal(x, x0)
        got = y.cpu().numpy()
        err = float(np.abs(got.astype(np.float64) - steps[key + ':out64']).max())
        bound = R.single_step_bound(steps[key + ':e_ref32'], steps[key + ':out64'])
        same32 = bool(np.array_equal(got, steps[key + ':out32']))
        _line(report, key, n=n, err=err, bound=bound, equals_reference_fp32=same32)
        assert err <= bound and same32, (key, err, bound, same32)


# ---------------------------------------------------------------------------------------------- no read-back, one launch
def test_step_and_undo_step_read_nothing_back():
    """With the noise drawn on the device by a device generator, `step` and `undo_step` run under sync debug mode 'error': one launch
    per step, ceil(n / 8) per undo step, for every mask form the kernel reads in place."""
    L = pkg('_lib')
    lib = L.load()
    s = _sched()
    s.set_timesteps(250)
    s.eta = 1.0
    gen = torch.Generator(device=DEV).manual_seed(3)
    forms = [tuple(v.to(DEV) for v in R.step_inputs(0, form)) for form in R.MASK_FORMS]
    s.step_coefs(496), s.step_coefs(0), s.undo_coefs(496)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode('error')
    try:
        for x, e, o, m in forms:
            for t in (496, 0):
                before = lib.dp_launch_count()
                y = s.step(e, t, x, o, m, generator=gen).prev_sample
                assert lib.dp_launch_count() == before + 1
                before = lib.dp_launch_count()
                y = s.step(e, t, y, o, m, generator=gen, out=y, need_x0=False).prev_sample
                assert lib.dp_launch_count() == before + 1
            before = lib.dp_launch_count()
            y = s.undo_step(y, 496, generator=gen, out=y)
            assert lib.dp_launch_count() == before + 1
    finally:
        torch.cuda.set_sync_debug_mode('default')
    assert torch.isfinite(y).all()


# ---------------------------------------------------------------------------------------------- chains on the HIP UNet
@pytest.fixture(scope='module')
def tiny():
    return make_model(gc.TINY_CFG, R.MODEL_SEED)


def _spied(sched):
    states = []
    real_step, real_undo = sched.step, sched.undo_step

    def step(model_output, timestep, sample, *a, **k):
        if not states:
            states.append(sample.clone())
        out = real_step(model_output, timestep, sample, *a, **k)
        states.append(out.prev_sample.clone())                                    # the pipeline works in place
        return out

    def undo(sample, timestep, *a, **k):
        out = real_undo(sample, timestep, *a, **k)
        states.append(out.clone())
        return out
    sched.step, sched.undo_step = step, undo
    return states


def _loop(model, shape, st, eta, replay):
    """The pipeline's loop written out, on a replayed or an eager forward, out of place: the same draws from the same generator."""
    diffusion = pkg('diffusion')
    image, mask = (t.to(DEV) for t in R.chain_inputs(shape))
    gen = torch.Generator().manual_seed(R.CHAIN_SEED)
    x = diffusion.randn_tensor(shape, generator=gen, device=DEV)
    sched = _sched()
    sched.set_timesteps(*st)
    sched.eta = eta
    ts = sched._ts
    fwd = model.sampling_forward(tuple(shape), R.n_model_calls(ts), replay=replay)
    assert type(fwd).__name__ == ('_CapturedForward' if replay else '_EagerForward')
    xs, t_last = [x], ts[0] + 1
    try:
        with torch.no_grad():
            for t in ts:
                if t < t_last:
                    xs.append(sched.step(fwd(xs[-1], t), t, xs[-1], image, mask, gen).prev_sample)
                else:
                    xs.append(sched.undo_step(xs[-1], t_last, gen))
                t_last = t
    finally:
        fwd.close()
    return xs


@pytest.mark.parametrize('chain', R.CHAINS, ids=lambda c: c[0])
def test_pipeline_chains_on_the_hip_unet_against_the_reference(chain, tiny, report):
    diffusion = pkg('diffusion')
    name, st, eta = chain
    g = R.load(R.CHAIN_FILE % name)
    ss = gc.TINY_CFG['sample_size']
    shape = (R.CHAIN_B, gc.TINY_CFG['in_channels'], ss, ss)
    image, mask = R.chain_inputs(shape)
    pipe = diffusion.RePaintPipeline(tiny, _sched())
    xs = _spied(pipe.scheduler)
    try:
        images = pipe(image, mask, num_inference_steps=st[0], eta=eta, jump_length=st[1], jump_n_sample=st[2],
                      generator=torch.Generator().manual_seed(R.CHAIN_SEED), output_type='numpy').images
    finally:
        del pipe.scheduler.step, pipe.scheduler.undo_step
    ts = g[name + ':timesteps'].tolist()
    assert pipe.scheduler._ts == ts and len(xs) == len(ts) + 1
    y64, gaps = g[name + ':xs64'], g[name + ':gap']
    assert np.array_equal(xs[0].cpu().numpy().astype(np.float64), y64[0])          # the pipeline draws the fixture's x_T bit for bit
    errs = [float(np.abs(t.double().cpu().numpy() - y64[k]).max()) for k, t in enumerate(xs)]
    bounds = [R.CHAIN_FACTOR * float(gaps[k]) + R.CHAIN_FLOOR for k in range(len(xs))]
    _line(report, 'chain/' + name, entries=len(ts), model_calls=R.n_model_calls(ts), worst_err=max(errs),
          worst_err_over_bound=max(e / b for e, b in zip(errs, bounds)), errs=' '.join('%.1e' % v for v in errs),
          bounds=' '.join('%.1e' % v for v in bounds))
    assert all(e <= b for e, b in zip(errs, bounds)), (name, errs, bounds)
    want = (xs[-1] / 2 + 0.5).clamp(0, 1).cpu().permute(0, 2, 3, 1).numpy()
    assert np.array_equal(images, want)
    # the known region of the final state is the original image: the last entry is t = 0 with alpha_prod_t_prev = 1, k = 1 * o + 0 * z
    # (the stand-in and the reference's toy chains show the same on the host, tests/test_repaint_cpu.py)
    known = (mask.expand(shape) == 1)
    assert torch.equal(xs[-1].cpu()[known], image[known]) and not torch.equal(xs[-1].cpu()[~known], image[~known])
    # the loop written out, on replayed and on eager forwards: the same bits, and the pipeline's
    replayed, eager = _loop(tiny, shape, st, eta, True), _loop(tiny, shape, st, eta, False)
    assert len(replayed) == len(eager) == len(xs)
    for a, b, c in zip(replayed, eager, xs):
        assert torch.equal(a, b) and torch.equal(a, c)
