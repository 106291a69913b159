"""Dynamic thresholding and x0 / v-prediction in DDPMScheduler and DDIMScheduler on the MI355X: dp_x0_abs_quantile, dp_x0_step and
dp_x0_threshold_step (csrc/threshold.hip) and the two schedulers on the HIP UNet2DModel, against the stand-in tests/threshold_ref.py
and the fixtures the reference wrote (tests/golden/make_golden_threshold.py).

Bounds (none fixed by hand):
  * the selection is exact: v_lo and v_hi equal torch.sort's order statistics bit for bit, the quantile (one fma, restated exactly on
    the host) and s too -- a NaN standing for any NaN -- on both routes, and two calls give equal bits;
  * the step kernel equals the stand-in bit for bit: both are the same sequence of correctly rounded fp32 operations (the stand-in
    runs torch's eager fp32 ops on the device, one rounding each, scalars as 0-d device tensors); the fused launch equals the
    quantile followed by the step bit for bit;
  * a fixture step lies within max(4 e_ref32, 4 * 2^-24 * max|y64|) of the fixture's fp64 result y64, e_ref32 being the reference's own
    fp32 distance stored beside it; how many steps equal the reference's fp32 bits is reported, every exception by name;
  * a chain state lies within 10 x the reference fp32 chain's own gap at that state + 1e-5 of the fp64 chain.
profiles/threshold_gpu_tests.txt holds every measured value beside its bound."""
import ctypes

import numpy as np
import pytest
import torch

import golden_common as gc
import threshold_ref as R
from helpers import make_model, pkg

pytestmark = pytest.mark.gpu
DEV = 'cuda'

# ---- the launch sites of csrc/threshold.hip (tests/test_threshold_cpu.py compares this table with the source)
LAUNCH_SITES = {'threshold.hip': 8}
LDS_QUANTILE, LDS_FUSED, STEP = '(th_lds_kernel<false>)', '(th_lds_kernel<true>)', 'th_step_kernel'
MULTI = ['th_init_kernel'] + ['th_hist_kernel', 'th_pick_kernel'] * 4 + ['th_minabove_kernel', 'th_stats_kernel']
# branch -> the test that launches it
CASES = {LDS_QUANTILE: 'test_quantile_is_exact_on_both_routes', LDS_FUSED: 'test_fused_launch_equals_quantile_then_step',
         STEP: 'test_step_equals_the_stand_in', 'th_init_kernel': 'test_quantile_is_exact_on_both_routes',
         'th_hist_kernel': 'test_quantile_is_exact_on_both_routes', 'th_pick_kernel': 'test_quantile_is_exact_on_both_routes',
         'th_minabove_kernel': 'test_quantile_is_exact_on_both_routes', 'th_stats_kernel': 'test_quantile_is_exact_on_both_routes'}
BRANCHES = sorted(CASES)
LDS_MAX = 16384                                    # DP_THRESHOLD_LDS_MAX
MAX_BLOCKS = 4096                                  # DP_X0_STEP_MAX_BLOCKS
CAP = MAX_BLOCKS * 256 * 4                         # elements of one image one launch covers without a second strided trip (16-byte path)
HIST_BLOCK = 4096                                  # elements of a row one block of the multi-block route covers
QUANTILE_N = [1, 2, 5, 48, 255, 3072, LDS_MAX, LDS_MAX + 1, 5 * HIST_BLOCK + 1029]
RATIOS = [0.0, 0.3, 0.5, 0.995, 1.0]
STEP_SIZES = [(3, 1), (3, 3), (3, 4), (3, 5), (3, 255), (3, 1027), (MAX_BLOCKS + 5, 4), (1, CAP + 1028)]      # (B, n)
INVALID = 1                                        # hipErrorInvalidValue
SA, SB = 0.8, 0.6


def _launched(lib, before):
    n = lib.dp_launch_count() - before
    arr = (ctypes.c_char_p * 256)()
    k = lib.dp_recent_launches(arr, 256)
    return [arr[i].decode() for i in range(k)][k - n:] if n else []


def _line(report, key, **kw):
    report['threshold/' + key] = kw
    print('threshold/%s %s' % (key, ' '.join('%s=%.3e' % (k, v) if isinstance(v, float) else '%s=%s' % (k, v) for k, v in kw.items())))


def _at(t, off, B, n):
    """[B, n] view at element offset `off` of a flat buffer."""
    return t[off:off + B * n].view(B, n)


def _rows(kind, B, n, seed):
    """[B, n] fp32 rows of one kind, on the host."""
    gen = torch.Generator().manual_seed(seed)
    v = torch.randn(B, n, generator=gen) * torch.linspace(0.4, 2.5, B).reshape(B, 1)
    if kind == 'ties':
        v = torch.round(v.clamp(-2, 1.5) * 2) / 2                                 # 8 levels: -2, -1.5 .. 1.5
    elif kind == 'zeros':
        v = torch.where(torch.rand(B, n, generator=gen) < 0.7, torch.zeros(()), v)
        v = torch.where(torch.rand(B, n, generator=gen) < 0.5, -v, v)             # zeros of both signs
    elif kind == 'denormals':
        v = v * 1e-41
        assert n < 4 or bool(((v != 0) & (v.abs() < 1.17e-38)).any())
    elif kind == 'inf':
        v[:, n // 2] = float('inf')
        v[0, 0] = -float('inf')
    elif kind == 'nan':
        v[B // 2, n // 3] = float('nan')                                           # one NaN row between clean rows
    return v


# ---------------------------------------------------------------------------------------------- the quantile
@pytest.mark.parametrize('n', QUANTILE_N)
def test_quantile_is_exact_on_both_routes(n, report):
    """B in 1, 3, 17, every ratio, the three model types, element offsets 0 and 1, both routes wherever the length allows; rows with
    heavy ties, zeros of both signs, denormals, infinities and a NaN row; two calls; the launch ring names the route."""
    ops, L = pkg('ops'), pkg('_lib')
    lib = L.load()
    assert ops.THRESHOLD_LDS_MAX == LDS_MAX
    routes = [ops.X0_ROUTE_MULTI] + ([ops.X0_ROUTE_LDS] if n <= LDS_MAX else [])
    ran, checked = set(), 0

    def check(x, m, pred, ratio, max_value, what):
        nonlocal checked
        want = R.abs_quantile(x, m, pred, SA, SB, ratio, max_value)
        for route in routes:
            before = lib.dp_launch_count()
            got = ops.x0_abs_quantile(x, m, pred, SA, SB, ratio, max_value, route=route)
            names = _launched(lib, before)
            assert names == ([LDS_QUANTILE] if route == ops.X0_ROUTE_LDS else MULTI), names
            ran.update(names)
            again = ops.x0_abs_quantile(x, m, pred, SA, SB, ratio, max_value, route=route)
            assert got.shape == (m.shape[0], 4) and R.same_bits(got, want), (what, route, got.cpu(), want.cpu())
            assert R.same_bits(got, again), (what, route, 'two calls')
            checked += 1
        auto = ops.x0_abs_quantile(x, m, pred, SA, SB, ratio, max_value)
        assert R.same_bits(auto, want), (what, 'auto')

    for B in (1, 3, 17):
        bufs = [_rows('normal', 1, B * n + 1, 10 * B + j)[0].to(DEV) for j in (0, 1)]
        for off in (0, 1):
            x, m = (_at(t, off, B, n) for t in bufs)
            assert m.data_ptr() % 16 == 4 * off
            for pred in (R.EPSILON, R.SAMPLE, R.V):
                for ratio in RATIOS:
                    check(x, m, pred, ratio, 1.5, (B, n, off, pred, ratio))
    for kind in ('ties', 'zeros', 'denormals', 'inf', 'nan'):
        m = _rows(kind, 3, n, 77).to(DEV)
        for ratio in RATIOS:
            check(None, m, R.SAMPLE, ratio, 4.0, (kind, n, ratio))
        if kind == 'nan' and n >= 3:
            st = ops.x0_abs_quantile(None, m, R.SAMPLE, SA, SB, 0.5, 4.0).cpu()
            assert bool(torch.isnan(st[1, 2:]).all()) and not bool(torch.isnan(st[0]).any()) and not bool(torch.isnan(st[2]).any())
    torch.cuda.synchronize()
    assert ran == set(MULTI) | ({LDS_QUANTILE} if n <= LDS_MAX else set())
    _line(report, 'quantile/n%d' % n, calls=checked, differing_values=0, undecided=0)


def test_quantile_refusals():
    ops, L = pkg('ops'), pkg('_lib')
    m = torch.zeros(2, LDS_MAX + 1, device=DEV)
    with pytest.raises(ValueError):
        ops.x0_abs_quantile(None, m, R.SAMPLE, SA, SB, 0.5, 1.0, route=ops.X0_ROUTE_LDS)
    with pytest.raises(ValueError):
        ops.x0_abs_quantile(None, m, R.SAMPLE, SA, SB, 1.5, 1.0)
    lib = L.load()
    st = torch.zeros(2, 4, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())                                   # noqa: E731
    args = (2, LDS_MAX + 1, R.SAMPLE, SA, SB)
    assert lib.dp_x0_abs_quantile(None, p(m), *args, 0, 1, 0.5, 1.0, ops.X0_ROUTE_LDS, None, p(st), None) == INVALID      # too long for LDS
    assert lib.dp_x0_abs_quantile(None, p(m), *args, 0, 1, 0.5, 1.0, ops.X0_ROUTE_MULTI, None, p(st), None) == INVALID    # no workspace
    assert lib.dp_x0_abs_quantile(None, p(m), *args, 3, 5, 0.5, 1.0, 0, None, p(st), None) == INVALID                     # hi > lo + 1
    assert lib.dp_x0_abs_quantile(None, p(m), 2, 8, R.SAMPLE, SA, SB, 7, 8, 0.5, 1.0, 0, None, p(st), None) == INVALID    # hi == n
    assert lib.dp_x0_abs_quantile(None, p(m), 2, 8, R.EPSILON, SA, SB, 3, 4, 0.5, 1.0, 0, None, p(st), None) == INVALID   # epsilon model without x
    assert lib.dp_x0_abs_quantile(None, p(m), 2, 8, R.SAMPLE, SA, SB, 3, 4, 0.5, 1.0, 0, None, p(m), None) == INVALID     # stats on m
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- the step
COEF = dict(sa=SA, sb=SB, range=1.0, c0=0.9, c1=0.3, cz=0.2, ratio=0.995, max_value=1.5)


def _combos():
    out = []
    for mode in (R.DDIM, R.DDPM, R.CONVERT):
        for pred in (R.EPSILON, R.SAMPLE, R.V):
            for treat in (R.NONE, R.CLIP, R.THRESHOLD):
                if mode == R.CONVERT:
                    out.append((mode, pred, treat, False, False))
                else:
                    out += [(mode, pred, treat, rc, hz) for rc in (False, True) for hz in (False, True)]
    return out


@pytest.mark.parametrize('shape', STEP_SIZES, ids=lambda s: 'B%d_n%d' % s)
def test_step_equals_the_stand_in(shape, report):
    """Every (mode, model type, treatment, reclip, with / without z) combination at element offsets 0 and 1, out of place with guard
    words around both outputs, with prev on x, and with one pointer of another alignment; exactly one launch."""
    ops, L = pkg('ops'), pkg('_lib')
    lib = L.load()
    B, n = shape
    N = B * n
    big = N > (1 << 20)
    src = [_rows('normal', 1, N + 1, 20 + j)[0].to(DEV) for j in range(3)]
    combos = _combos()
    assert len(combos) == 2 * 3 * 3 * 4 + 9
    checked = 0
    for off in (0, 1):
        x, m, z = (_at(t, off, B, n) for t in src)
        stats = {pred: R.abs_quantile(x, m, pred, SA, SB, COEF['ratio'], COEF['max_value']) for pred in (R.EPSILON, R.SAMPLE, R.V)}
        for mode, pred, treat, reclip, has_z in (combos if not big or off == 0 else combos[::7]):
            st = stats[pred] if treat == R.THRESHOLD else None
            zz = z if has_z else None
            want, want0 = R.step(x, m, mode, pred, treat, COEF, stats=st, z=zz, reclip=reclip)
            gp, g0 = torch.full((N + 2,), 7.0, device=DEV), torch.full((N + 2,), 7.0, device=DEV)
            before = lib.dp_launch_count()
            got, got0, _ = ops.x0_step(x, m, mode, pred, treat, COEF, stats=st, z=zz, out=_at(gp, off, B, n),
                                       x0_out=None if mode == R.CONVERT else _at(g0, off, B, n), reclip=reclip)
            assert _launched(lib, before) == [STEP]
            what = (shape, off, mode, pred, treat, reclip, has_z)
            assert R.same_bits(got, want), what
            assert mode == R.CONVERT or R.same_bits(got0, want0), what
            for b in (gp, g0):                                                       # nothing written before the start or past the end
                assert float(b[off + N]) == 7.0 and (off == 0 or float(b[0]) == 7.0) and float(b[N + 1]) == 7.0
            if mode == R.CONVERT:
                assert bool((g0 == 7.0).all())
            checked += 1
            if big:
                continue
            # prev on x
            xa = torch.empty(N + 1, device=DEV)[off:off + N].view(B, n).copy_(x)
            got, _, _ = ops.x0_step(xa, m, mode, pred, treat, COEF, stats=st, z=zz, out=xa, reclip=reclip)
            assert got is xa and R.same_bits(xa, want), (what, 'in place')
            # pointers of two alignments: every access is a 4-byte one
            got, _, _ = ops.x0_step(x, m, mode, pred, treat, COEF, stats=st, z=zz, out=torch.empty(N + 1, device=DEV)[1 - off:1 - off + N].view(B, n),
                                    reclip=reclip)
            assert R.same_bits(got, want), (what, 'two alignments')
            checked += 2
    torch.cuda.synchronize()
    _line(report, 'step_vs_stand_in/B%d_n%d' % shape, cases=checked, differing_elements=0)


@pytest.mark.parametrize('shape', [(3, 1), (3, 5), (17, 48), (5, 3072), (2, LDS_MAX)], ids=lambda s: 'B%d_n%d' % s)
def test_fused_launch_equals_quantile_then_step(shape, report):
    """ops.x0_step without `stats`: ONE launch where the row fits in LDS, the quantile's launches and the step when the multi-block
    route is asked for -- and both equal the quantile followed by the step, output, treated x0 and table alike."""
    ops, L = pkg('ops'), pkg('_lib')
    lib = L.load()
    B, n = shape
    N = B * n
    src = [_rows('normal', 1, N + 1, 40 + j)[0].to(DEV) for j in range(3)]
    checked = 0
    for off in (0, 1):
        x, m, z = (_at(t, off, B, n) for t in src)
        for mode, pred, treat, reclip, has_z in _combos():
            if treat != R.THRESHOLD:
                continue
            zz = z if has_z else None
            kw = dict(z=zz, reclip=reclip)
            st = ops.x0_abs_quantile(x, m, pred, SA, SB, COEF['ratio'], COEF['max_value'], route=ops.X0_ROUTE_LDS)
            assert R.same_bits(st, R.abs_quantile(x, m, pred, SA, SB, COEF['ratio'], COEF['max_value']))
            x0s = [None if mode == R.CONVERT else torch.empty(B, n, device=DEV) for _ in range(3)]
            two, two0, _ = ops.x0_step(x, m, mode, pred, treat, COEF, stats=st, x0_out=x0s[0], **kw)
            gp = torch.full((N + 2,), 7.0, device=DEV)
            before = lib.dp_launch_count()
            one, one0, one_st = ops.x0_step(x, m, mode, pred, treat, COEF, out=_at(gp, off, B, n), x0_out=x0s[1], **kw)
            assert _launched(lib, before) == [LDS_FUSED]
            assert float(gp[off + N]) == 7.0 and (off == 0 or float(gp[0]) == 7.0) and float(gp[N + 1]) == 7.0
            before = lib.dp_launch_count()
            far, far0, far_st = ops.x0_step(x, m, mode, pred, treat, COEF, x0_out=x0s[2], route=ops.X0_ROUTE_MULTI, **kw)
            assert _launched(lib, before) == MULTI + [STEP]
            what = (shape, off, mode, pred, reclip, has_z)
            assert R.same_bits(one, two) and R.same_bits(far, two) and R.same_bits(one_st, st) and R.same_bits(far_st, st), what
            assert mode == R.CONVERT or (R.same_bits(one0, two0) and R.same_bits(far0, two0)), what
            want, _ = R.step(x, m, mode, pred, treat, COEF, stats=st, **kw)
            assert R.same_bits(one, want), what
            # in place
            xa = torch.empty(N + 1, device=DEV)[off:off + N].view(B, n).copy_(x)
            got, _, _ = ops.x0_step(xa, m, mode, pred, treat, COEF, out=xa, **kw)
            assert got is xa and R.same_bits(xa, two), (what, 'in place')
            checked += 1
    torch.cuda.synchronize()
    _line(report, 'fused_vs_two_kernels/B%d_n%d' % shape, cases=checked, differing_elements=0)


def test_dynamic_threshold_is_the_references_threshold_sample(report):
    ops = pkg('ops')
    x = (_rows('normal', 5, 3 * 16 * 16, 3) * 1.3).reshape(5, 3, 16, 16).to(DEV)
    for max_value in (1.0, 2.0):
        got = ops.dynamic_threshold(x, 0.995, max_value)
        B, xc = x.shape[0], x.cpu()
        # the reference's expressions in torch's fp32 ops on the host: torch.quantile there is the stand-in's quantile bit for bit
        # (tests/test_threshold_cpu.py), clamp and the division are correctly rounded
        s = torch.clamp(torch.quantile(xc.reshape(B, -1).abs(), 0.995, dim=1), min=1, max=max_value).reshape(B, 1, 1, 1)
        want = torch.clamp(xc, -s, s) / s
        assert got.shape == x.shape and torch.equal(got.cpu(), want), max_value
        if max_value == 1.0:
            assert torch.equal(got, x.clamp(-1, 1))                               # the default: a clip to [-1, 1]
        else:
            assert float(s.min()) > 1.0 and float(s.max()) == 2.0
    _line(report, 'dynamic_threshold', differing_elements=0)


def test_the_library_refuses_overlaps_and_bad_arguments():
    ops, L = pkg('ops'), pkg('_lib')
    lib = L.load()
    n = 64
    buf = torch.zeros(8 * n, device=DEV)
    x, m, z, out, x0 = (buf[i * n:(i + 1) * n].view(2, n // 2) for i in range(5))
    st = torch.ones(2, 4, device=DEV)

    def refused(call):
        with pytest.raises(L.DpHipError) as e:
            call()
        return e.value.code == INVALID
    ok = ops.x0_step(x, m, R.DDIM, R.EPSILON, R.CLIP, COEF, out=x)                # the one alias
    assert ok[0] is x
    shifted = buf[n + 4:2 * n + 4].view(2, n // 2)                               # half on m, half on z
    assert refused(lambda: ops.x0_step(x, m, R.DDIM, R.EPSILON, R.CLIP, COEF, out=m))
    assert refused(lambda: ops.x0_step(x, m, R.DDIM, R.EPSILON, R.CLIP, COEF, out=shifted))
    assert refused(lambda: ops.x0_step(x, m, R.DDIM, R.EPSILON, R.CLIP, COEF, z=z, out=z))
    assert refused(lambda: ops.x0_step(x, m, R.DDIM, R.EPSILON, R.CLIP, COEF, out=out, x0_out=out))
    assert refused(lambda: ops.x0_step(x, m, R.DDIM, R.EPSILON, R.CLIP, COEF, out=out, x0_out=x))
    assert refused(lambda: ops.x0_step(x, m, R.DDIM, R.EPSILON, R.CLIP, COEF, out=buf[4:n + 4].view(2, n // 2)))      # partly on x
    assert refused(lambda: ops.x0_step(x, m, R.DDPM, R.V, R.THRESHOLD, COEF, out=out, x0_out=m))                       # the fused form too
    assert refused(lambda: ops.x0_step(x, m, R.DDPM, R.V, R.THRESHOLD, COEF, out=m))
    assert refused(lambda: ops.x0_step(x, m, R.DDPM, R.V, R.THRESHOLD, COEF, stats=st, out=m))
    p = lambda t: ctypes.c_void_p(t.data_ptr())                                   # noqa: E731
    c = L.X0Coef(sa=SA, sb=SB, range=1.0, c0=0.9, c1=0.3, cz=0.2)
    assert lib.dp_x0_step(p(x), p(m), None, None, 3, 0, 0, 0, ctypes.byref(c), p(out), None, 2, n // 2, None) == INVALID      # mode
    assert lib.dp_x0_step(p(x), p(m), None, None, 0, 0, 2, 0, ctypes.byref(c), p(out), None, 2, n // 2, None) == INVALID      # threshold without stats
    assert lib.dp_x0_step(p(x), p(m), p(z), None, 2, 0, 0, 0, ctypes.byref(c), p(out), None, 2, n // 2, None) == INVALID      # CONVERT with z
    assert lib.dp_x0_step(None, p(m), None, None, 1, 1, 0, 0, ctypes.byref(c), p(out), None, 2, n // 2, None) == INVALID      # DDPM needs x
    assert lib.dp_x0_threshold_step(p(x), p(m), None, 0, 0, 0, ctypes.byref(c), 0, 1, 0.5, 1.0, p(out), None, p(st), 1, LDS_MAX + 1, None) == INVALID
    torch.cuda.synchronize()
    assert bool((out == 0).all()) and bool((x0 == 0).all())


# ---------------------------------------------------------------------------------------------- the fixtures' single steps
def _step_cases():
    return [('ddpm', R.ddpm_file(), [c for c in R.ddpm_cases()])] + \
           [('ddim', R.ddim_file(p, e), [c for c in R.ddim_cases() if c[0] == p and c[3] == e]) for p in R.PREDS for e in (0.0, 0.5)]


def run_fixture_step(diffusion, sched, case, g, device):
    """One fixture step by this project's scheduler; -> (key, prev, x0)."""
    pred, treat, where = case[:3]
    cls = diffusion.DDPMScheduler if sched == 'ddpm' else diffusion.DDIMScheduler
    s = cls(**R.sched_kwargs(pred, treat))
    s.set_timesteps(R.N_STEPS)
    t = R.timestep_at(s.timesteps, where)
    x, m, z = (v.to(device) if device else v for v in R.scaled_inputs(sched, pred, where, g[R.scale_key(sched, pred, where)]))
    if sched == 'ddpm':
        key = R.ddpm_key(case)
        out = s.step(m, t, x, variance_noise=z)
    else:
        key = R.ddim_key(case)
        out = s.step(m, t, x, eta=case[3], use_clipped_model_output=case[4], variance_noise=z if case[3] > 0 else None)
    assert int(g[key + ':t']) == t
    return key, out.prev_sample, out.pred_original_sample


@pytest.mark.parametrize('group', _step_cases(), ids=lambda g: g[1][:-4])
def test_fixture_steps_against_the_reference(group, report):
    diffusion = pkg('diffusion')
    sched, fname, cases = group
    g = R.load(fname)
    equal, worst, exceptions = 0, 0.0, []
    for case in cases:
        key, prev, x0 = run_fixture_step(diffusion, sched, case, g, DEV)
        if x0 is None:                                                            # the default path: an epsilon model, no thresholding, no reclip
            assert case[0] == 'epsilon' and not case[1].startswith('thr') and (sched == 'ddpm' or not case[4]), key
            got = dict(prev=prev)
        else:
            got = dict(prev=prev, x0=x0)
        same = True
        for what, v in got.items():
            a = v.cpu().numpy()
            y64 = g['%s:%s64' % (key, what)]
            err, bound = float(np.abs(a.astype(np.float64) - y64).max()), R.single_step_bound(g['%s:e_ref32_%s' % (key, what)], y64)
            worst = max(worst, err / bound)
            assert err <= bound, (key, what, err, bound)
            same = same and np.array_equal(a, g['%s:%s32' % (key, what)])
        equal += same
        if not same:
            exceptions.append(key)
    _line(report, 'fixture_steps/' + fname[:-4], steps=len(cases), equal_to_reference_fp32_bits=equal, worst_err_over_bound=worst,
          not_bit_equal=' '.join(exceptions) or 'none')


# ---------------------------------------------------------------------------------------------- chains on the HIP UNet, through the pipelines
@pytest.fixture(scope='module')
def tiny():
    return make_model(gc.TINY_CFG, R.MODEL_SEED)


@pytest.mark.parametrize('chain', R.CHAINS, ids=lambda c: c[0])
def test_pipeline_chains_on_the_hip_unet_against_the_reference(chain, tiny, report):
    diffusion = pkg('diffusion')
    name, which, kw, step_kw = chain
    g = R.load(R.CHAINS_FILE)
    if which == 'ddim':
        pipe = diffusion.DDIMPipeline(tiny, diffusion.DDIMScheduler(**kw))
    else:
        pipe = diffusion.DDPMPipeline(tiny, diffusion.DDPMScheduler(**kw))
    sched = pipe.scheduler
    assert sched.config.thresholding and sched.config.sample_max_value == 2.0
    seen = []
    real = sched.step

    def spy(model_output, timestep, sample, **k):
        out = real(model_output, timestep, sample, **k)
        seen.append((int(timestep), sample, out.prev_sample, out.pred_original_sample, k))
        return out
    sched.step = spy
    try:
        call = dict(batch_size=R.CHAIN_B, generator=torch.Generator().manual_seed(R.CHAIN_SEED), num_inference_steps=R.CHAIN_STEPS,
                    output_type='numpy')
        if which == 'ddim':
            call.update(eta=step_kw['eta'], use_clipped_model_output=step_kw.get('use_clipped_model_output'))
        images = pipe(**call).images
    finally:
        del sched.step
    assert [s[0] for s in seen] == g[name + ':timesteps'].tolist() and len(seen) == R.CHAIN_STEPS
    assert all(bool(s[4].get('use_clipped_model_output')) == bool(step_kw.get('use_clipped_model_output')) for s in seen)
    assert np.array_equal(seen[0][1].cpu().numpy(), g['x_T'])                    # the pipeline draws the fixture's x_T bit for bit
    assert all(s[3] is not None and s[3].shape == s[2].shape and float(s[3].abs().max()) <= 1.0 for s in seen)     # pred_original_sample
    xs = [seen[0][1]] + [s[2] for s in seen]
    y64, gaps = g[name + ':xs64'], g[name + ':gap']
    errs = [float(np.abs(t.double().cpu().numpy() - y64[k]).max()) for k, t in enumerate(xs)]
    bounds = [R.CHAIN_FACTOR * float(gaps[k]) + R.CHAIN_FLOOR for k in range(len(xs))]
    _line(report, 'chain/' + name, steps=R.CHAIN_STEPS, worst_err=max(errs), worst_err_over_bound=max(e / b for e, b in zip(errs, bounds)),
          errs=' '.join('%.1e' % v for v in errs), bounds=' '.join('%.1e' % v for v in bounds))
    assert all(e <= b for e, b in zip(errs, bounds)), (name, errs, bounds)
    want = (xs[-1] / 2 + 0.5).clamp(0, 1).cpu().permute(0, 2, 3, 1).numpy()
    assert np.array_equal(images, want)
