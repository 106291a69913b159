"""AutoencoderKL on the MI355X: the two kernels of csrc/vae.hip against fp64 and against their torch stand-ins (tests/kl_ref.py, which
tests/test_vae_cpu.py holds to the reference's own fp32 results bit for bit), and the model on the fixtures the reference wrote
(tests/golden/make_golden_kl.py).

Bounds (none fixed by hand):
  * clamped log-variance, sample and blend: bit equality with torch's eager fp32 expression;
  * std / var: within max(4 e_ref32, 4 * 2^-24 * max|y64|) of fp64, and per element a relative error of at most 4 times the worst
    per-element relative error of torch's CPU fp32 expression on the same inputs (the reference expression is the yardstick);
  * kl: within max(4 e_ref32, 1e-5 |y64|) of fp64, e_ref32 the CPU fp32 expression's distance; two calls give the same bits;
  * the model: within max(4 e_ref32, 2e-5 max|y64|) of the reference's fp64, e_ref32 the reference's own fp32 distance (the bound of
    tests/test_vq_gpu.py).
profiles/vae_gpu_tests.txt holds every measured value beside its bound."""
import ctypes
import itertools
import json
import os

import numpy as np
import pytest
import torch

import golden_common as gc
import kl_ref as R
import ldm_finetune_ref as FR
from helpers import pkg

pytestmark = pytest.mark.gpu
DEV = 'cuda'
INVALID = 1                                        # hipErrorInvalidValue

# ---- the launch sites of csrc/vae.hip (tests/test_vae_cpu.py compares this table with the source)
LAUNCH_SITES = {'vae.hip': 4}
VEC, SCALAR, COMBINE, BLEND = ('(gaussian_posterior_kernel<true>)', '(gaussian_posterior_kernel<false>)', 'gaussian_kl_combine_kernel',
                               'tile_blend_kernel')
# branch -> the test that runs it and asserts, per case, that dp_recent_launches names it
CASES = {VEC: 'test_posterior_kernel[vec16 | past_cap | special]', SCALAR: 'test_posterior_kernel[strided | offset1 | past_cap_offset1]',
         COMBINE: 'test_posterior_kernel (every case with kl)', BLEND: 'test_tile_blend_kernel'}
BRANCHES = sorted(CASES)
MAX_BLOCKS = 4096                                  # DP_VAE_MAX_BLOCKS
CAP = MAX_BLOCKS * 256 * 4                         # elements one launch covers without a second grid-stride trip (16-byte path)
SCALES = (1.0, 0.18215)
NAMES = ('logvar', 'std', 'var', 'z', 'kl')


def _launched(lib, before):
    n = lib.dp_launch_count() - before
    arr = (ctypes.c_char_p * 256)()
    k = lib.dp_recent_launches(arr, 256)
    return [arr[i].decode() for i in range(k)][k - n:] if n else []


def _line(report, key, **kw):
    report['vae/' + key] = kw
    print('vae/%s %s' % (key, ' '.join('%s=%.3e' % (k, v) if isinstance(v, float) else '%s=%s' % (k, v) for k, v in kw.items())))


# ---------------------------------------------------------------------------------------------- posterior kernel
def _moments(case):
    """(moments on the device, expected branch).  Seeded; the log-variance half is spread over a few units."""
    g = torch.Generator().manual_seed(17)
    if case == 'strided':                          # [3, 2 * 3, 5, 7] inside [3, 8, 5, 7]: images are not contiguous, chw = 105
        big = torch.randn(3, 8, 5, 7, generator=g) * 2
        m = big.to(DEV)[:, 1:7]
        assert not m.is_contiguous()
        return m, SCALAR
    if case in ('vec16', 'offset1'):               # [2, 2 * 4, 20, 14]: chw = 1120
        flat = torch.randn(2 * 8 * 20 * 14 + 1, generator=g) * 2
        d = flat.to(DEV)
        m = (d[1:] if case == 'offset1' else d[:-1].clone()).view(2, 8, 20, 14)
        assert m.data_ptr() % 16 == (4 if case == 'offset1' else 0)
        return m, SCALAR if case == 'offset1' else VEC
    if case in ('past_cap', 'past_cap_offset1'):   # one image of CAP + 1028 elements: a second grid-stride trip on either path
        chw = CAP + 1028
        flat = torch.randn(2 * chw + 1, generator=g) * 2
        d = flat.to(DEV)
        m = (d[1:] if case == 'past_cap_offset1' else d[:-1].clone()).view(1, 2, 4, chw // 4)
        return m, SCALAR if case == 'past_cap_offset1' else VEC
    assert case == 'special'                       # log-variances over -40 .. 30 with exact -30 and 20, a NaN, and zeros
    m = torch.randn(2, 4, 4, 8, generator=g)
    lv = torch.linspace(-40.0, 30.0, 2 * 2 * 4 * 8).view(2, 2, 4, 8).clone()
    lv[0, 0, 0, :4] = torch.tensor([-30.0, 20.0, 0.0, -0.0])
    lv[0, 1, 1, :2] = torch.tensor([-30.000002, 20.000002])
    lv[1, 1, 3, 5] = float('nan')
    lv[1, 0, 2, :] = 0.0
    m[:, 2:] = lv
    m[1, 0, 0, :4] = 0.0                           # zeros in the mean too
    return m.to(DEV), VEC


def _guarded(shape):
    """(view of `shape`, its buffer): 4 guard words of 7.0 on either side; the view stays 16-byte aligned."""
    n = int(np.prod(shape))
    buf = torch.full((n + 8,), 7.0, device=DEV)
    return buf[4:4 + n].view(shape), buf


def _guards_ok(buf):
    return bool((buf[:4] == 7.0).all()) and bool((buf[-4:] == 7.0).all())


def _same(a, b):
    return np.array_equal(a.detach().cpu().numpy(), b.detach().cpu().numpy(), equal_nan=True)


@pytest.mark.parametrize('case', ['strided', 'vec16', 'offset1', 'past_cap', 'past_cap_offset1', 'special'])
def test_posterior_kernel(case, report):
    ops, L = pkg('ops'), pkg('_lib')
    lib = L.load()
    m, branch = _moments(case)
    N, C = m.shape[0], m.shape[1] // 2
    shape = (N, C) + tuple(m.shape[2:])
    noise = torch.randn(shape, generator=torch.Generator().manual_seed(19)).to(DEV)
    # the yardsticks: torch's CPU fp32 expression, and fp64 on the same fp32 inputs
    mc = m.cpu().contiguous()
    ref32 = R.posterior(mc)
    ref64 = R.posterior(mc.double())
    outs, bufs = {}, {}
    for name in NAMES:
        outs[name], bufs[name] = _guarded((N,) if name == 'kl' else shape)
    before = lib.dp_launch_count()
    got = ops.gaussian_posterior(m, noise=noise, scale=1.0, **outs)
    assert _launched(lib, before) == [branch, COMBINE]
    assert all(got[k] is outs[k] for k in NAMES) and all(_guards_ok(b) for b in bufs.values())
    # the clamped log-variance: torch.clamp's bits, a NaN kept
    assert _same(got['logvar'], ref32['logvar'])
    if case == 'special':
        lvc = got['logvar'].cpu()
        assert float(lvc[~lvc.isnan()].min()) == -30.0 and float(lvc[~lvc.isnan()].max()) == 20.0 and int(lvc.isnan().sum()) == 1
        assert bool(got['std'].cpu().isnan()[1, 1, 3, 5]) and bool(got['var'].cpu().isnan()[1, 1, 3, 5]) and bool(got['z'].cpu().isnan()[1, 1, 3, 5])
    # std / var against fp64
    for name in ('std', 'var'):
        y64, y32, yk = ref64[name], ref32[name].double(), got[name].cpu().double()
        ok = ~y64.isnan()
        assert bool((yk.isnan() == y64.isnan()).all())
        err, e_ref = float((yk - y64)[ok].abs().max()), float((y32 - y64)[ok].abs().max())
        bound = max(4 * e_ref, 4 * 2.0 ** -24 * float(y64[ok].abs().max()))
        rel, rel_ref = float(((yk - y64)[ok] / y64[ok]).abs().max()), float(((y32 - y64)[ok] / y64[ok]).abs().max())
        _line(report, 'posterior/%s/%s' % (case, name), err=err, bound=bound, rel=rel, rel_ref32=rel_ref, rel_bound=4 * rel_ref)
        assert err <= bound and rel <= 4 * rel_ref, (case, name, err, bound, rel, rel_ref)
    # the sample: the fp32 expression on the kernel's own std, bit for bit, at either scale, out of place and onto the noise
    for scale in SCALES:
        want = R.posterior(m, noise, scale=scale, std=got['std'])['z']
        z, zb = _guarded(shape)
        before = lib.dp_launch_count()
        ops.gaussian_posterior(m, noise=noise, scale=scale, z=z)
        assert _launched(lib, before) == [branch]
        assert _same(z, want) and _guards_ok(zb), (case, scale)
        alias, ab = _guarded(shape)
        alias.copy_(noise)
        assert ops.gaussian_posterior(m, noise=alias, scale=scale, z=alias)['z'] is alias
        assert _same(alias, want) and _guards_ok(ab), (case, scale, 'z on noise')
    assert _same(got['z'], R.posterior(m, noise, std=got['std'])['z'])
    # kl against fp64; the same bits twice
    y64, y32, yk = ref64['kl'], ref32['kl'].double(), got['kl'].cpu().double()
    ok = ~y64.isnan()
    assert bool((yk.isnan() == y64.isnan()).all())
    err, e_ref = float((yk - y64)[ok].abs().max()), float((y32 - y64)[ok].abs().max())
    bound = max(4 * e_ref, 1e-5 * float(y64[ok].abs().max()))
    _line(report, 'posterior/%s/kl' % case, err=err, bound=bound, e_ref32=e_ref)
    assert bool(((yk - y64)[ok].abs() <= torch.clamp(1e-5 * y64[ok].abs(), min=4 * e_ref)).all()), (case, err, bound)
    again = ops.gaussian_posterior(m, kl=True)['kl']
    assert _same(again, got['kl'])
    # every subset of the outputs gives the same bits (the large cases: single outputs only)
    subsets = [s for r in range(1, 6) for s in itertools.combinations(NAMES, r)] if m.numel() < 1 << 20 else [(n,) for n in NAMES]
    for sub in subsets:
        before = lib.dp_launch_count()
        part = ops.gaussian_posterior(m, noise=noise if 'z' in sub else None, **{n: True for n in sub})
        assert _launched(lib, before) == [branch] + ([COMBINE] if 'kl' in sub else [])
        assert sorted(part) == sorted(sub) and all(_same(part[n], got[n]) for n in sub), (case, sub)


def test_posterior_refuses_overlaps_and_the_2_gib_extent():
    ops, L = pkg('ops'), pkg('_lib')
    lib = L.load()
    N, chw = 2, 64
    big = torch.zeros(4096, device=DEV)
    m = big[0:256].view(2, 2, 8, 8)                 # moments: 256 floats
    noise = big[512:640]
    free = [big[1024 + 256 * i:1024 + 256 * i + 128] for i in range(4)]
    kl, ws = big[3000:3002], torch.zeros(64, dtype=torch.float64, device=DEV)

    def call(**change):
        a = dict(noise=noise, logvar=free[0], std=free[1], var=free[2], z=free[3], kl=kl, ws=ws)
        a.update(change)

        def p(t):
            return None if t is None else ctypes.c_void_p(t.data_ptr())
        return lib.dp_gaussian_posterior(p(m), 128, N, chw, p(a['noise']), 1.0, p(a['logvar']), p(a['std']), p(a['var']), p(a['z']),
                                         p(a['kl']), p(a['ws']), None)
    bad = [dict(logvar=big[0:128]), dict(std=big[128:256]), dict(var=big[200:328]), dict(z=big[64:192]), dict(kl=big[10:12]),
           dict(logvar=noise), dict(std=noise), dict(var=big[600:728]), dict(z=big[516:644]), dict(z=big[508:636]), dict(kl=big[520:522]),
           dict(std=free[0]), dict(var=big[1024 + 100:1024 + 228]), dict(z=free[2]), dict(kl=free[3][5:7]),
           dict(noise=None), dict(ws=None), dict(z=big[1024 + 127:1024 + 255])]
    torch.cuda.synchronize()
    before = lib.dp_launch_count()
    for change in bad:
        assert call(**change) == INVALID, sorted(change)
    assert lib.dp_launch_count() == before                                      # refused before any launch
    assert call() == 0 and call(z=noise) == 0                                   # the one allowed alias: z on the noise itself
    assert call(logvar=None, std=None, var=None, z=None, noise=None) == 0 and call(kl=None, ws=None, z=None, noise=None) == 0
    with pytest.raises(L.DpHipError) as err:                                    # through the wrapper
        ops.gaussian_posterior(m, logvar=big[128:256].view(2, 1, 8, 8))
    assert err.value.code == INVALID
    with pytest.raises(AssertionError):
        ops.gaussian_posterior(m, z=True)                                       # a sample without noise
    torch.cuda.synchronize()
    # an extent of 2 GiB: refused on the host, before any launch
    huge = torch.empty(1, 2, 1 << 14, 1 << 14, device=DEV)
    before = lib.dp_launch_count()
    with pytest.raises(ValueError, match='2 GiB'):
        ops.gaussian_posterior(huge, logvar=True)
    with pytest.raises(ValueError, match='2 GiB'):
        ops.tile_blend(huge, out=huge)
    assert lib.dp_launch_count() == before
    del huge


# ---------------------------------------------------------------------------------------------- blend kernel
# (planes N x C, tile Hb x Wb, rows of the tile above | None, columns of the tile to the left | None, extent, row_limit, canvas
#  offset, canvas size)
BLEND_CASES = {
    'none':            ((2, 3), (7, 9), None, None, 3, 5, (1, 3), (9, 11)),
    'above':           ((2, 3), (7, 9), 7, None, 3, 5, (1, 3), (9, 11)),
    'left':            ((2, 3), (7, 9), None, 9, 3, 5, (1, 3), (9, 11)),
    'both_e1':         ((2, 3), (7, 9), 7, 9, 1, 6, (0, 1), (7, 8)),
    'both_e3':         ((3, 5), (7, 9), 7, 9, 3, 5, (2, 1), (9, 7)),
    'both_e4':         ((1, 4), (16, 16), 16, 16, 4, 12, (12, 12), (40, 28)),
    'both_e128':       ((1, 2), (130, 131), 130, 131, 128, 100, (3, 5), (110, 107)),
    'tile_below_e':    ((2, 8), (2, 2), 8, 8, 4, 6, (18, 12), (20, 14)),
    'neighbour_below_e': ((1, 3), (8, 9), 3, 2, 4, 6, (0, 0), (6, 6)),
    'row_limit_above': ((2, 3), (4, 5), 16, 16, 4, 12, (36, 23), (40, 28)),
    'many_planes':     ((40, 300), (3, 5), 3, 5, 2, 2, (1, 1), (4, 4)),
}


@pytest.mark.parametrize('case', sorted(BLEND_CASES))
def test_tile_blend_kernel(case):
    ops, L = pkg('ops'), pkg('_lib')
    lib = L.load()
    (N, C), (Hb, Wb), Ha, Wl, extent, row_limit, (oy, ox), (Ho, Wo) = BLEND_CASES[case]
    g = torch.Generator().manual_seed(23)
    b0 = torch.randn(N, C, Hb, Wb, generator=g).to(DEV)
    a = torch.randn(N, C, Ha, Wb, generator=g).to(DEV) if Ha else None
    l = torch.randn(N, C, Hb, Wl, generator=g).to(DEV) if Wl else None
    # the stand-in, on the device: torch's eager fp32 ops
    want_b, want_out = b0.clone(), torch.full((N, C, Ho, Wo), 7.0, device=DEV)
    R.tile_blend(want_b, a, l, extent, want_out, oy, ox, row_limit)
    b, bb = _guarded((N, C, Hb, Wb))
    b.copy_(b0)
    out, ob = _guarded((N, C, Ho, Wo))
    out.fill_(7.0)
    a0, l0 = (None if t is None else t.clone() for t in (a, l))
    before = lib.dp_launch_count()
    assert ops.tile_blend(b, a, l, extent, out, oy, ox, row_limit) is b
    assert _launched(lib, before) == [BLEND]
    assert torch.equal(b, want_b) and torch.equal(out, want_out), case         # the untouched canvas keeps its 7.0 in both
    assert _guards_ok(bb) and _guards_ok(ob)
    assert (a is None or torch.equal(a, a0)) and (l is None or torch.equal(l, l0))
    if a is not None or l is not None:
        assert not torch.equal(b, b0)
    # without a canvas: the same tile
    b2 = b0.clone()
    ops.tile_blend(b2, a, l, extent)
    assert torch.equal(b2, want_b)


def test_tile_blend_refuses_what_leaves_the_canvas_or_overlaps():
    ops, L = pkg('ops'), pkg('_lib')
    lib = L.load()
    b, a, out = torch.zeros(1, 2, 4, 4, device=DEV), torch.zeros(1, 2, 4, 4, device=DEV), torch.zeros(1, 2, 6, 6, device=DEV)
    torch.cuda.synchronize()
    before = lib.dp_launch_count()
    for kw in (dict(oy=3), dict(ox=3), dict(oy=-1), dict(row_limit=0)):
        with pytest.raises(L.DpHipError) as err:
            ops.tile_blend(b, a, None, 2, out, **dict(dict(oy=0, ox=0, row_limit=4), **kw))
        assert err.value.code == INVALID
    for above, left, canvas in ((b, None, out), (None, b, out), (a, None, b)):
        with pytest.raises(L.DpHipError) as err:
            ops.tile_blend(b, above, left, 2, canvas, 0, 0, 4)
        assert err.value.code == INVALID
    with pytest.raises(AssertionError):
        ops.tile_blend(b, torch.zeros(1, 2, 4, 5, device=DEV), None, 2)           # the tile above has another width
    assert lib.dp_launch_count() == before
    ops.tile_blend(b, a, None, 2, out, 2, 2, 4)                                   # the crop ends at the canvas's edge
    assert lib.dp_launch_count() == before + 1


# ---------------------------------------------------------------------------------------------- the model on the fixtures
def _tiny(latent_channels=None):
    vae, syn = pkg('vae'), pkg('synthetic')
    if latent_channels is None:
        model = vae.AutoencoderKL(**syn.KL_TINY_CFG)
        model.load_state_dict(R.params([(k, s) for k, s in R.keys()['state_dict']]), strict=True)
    else:                                              # the LDM fixtures' UNets take 3 latent channels
        model = vae.AutoencoderKL(**dict(syn.KL_TINY_CFG, latent_channels=latent_channels))
        model.load_state_dict(R.params([(k, tuple(v.shape)) for k, v in model.state_dict().items()]), strict=True)
    return model.to(DEV).eval()


@pytest.fixture(scope='module')
def tiny():
    return _tiny()


def _within(report, key, got, fx, name):
    e, b = R.err(got, fx[name + '64']), R.bound(fx[name + '32'], fx[name + '64'])
    _line(report, key, err=e, bound=b)
    assert e <= b, (key, e, b)


def test_model_on_the_reference_fixture(tiny, report):
    vae = pkg('vae')
    fx = R.load('kl_tiny.npz')
    x = torch.from_numpy(fx['x']).to(DEV)
    out = tiny.encode(x)
    post = out.latent_dist
    assert isinstance(out, vae.AutoencoderKLOutput) and out[0] is post and isinstance(tiny.encode(x, return_dict=False)[0], vae.DiagonalGaussianDistribution)
    assert tuple(post.parameters.shape) == (2, 8, 8, 8)
    _within(report, 'model/moments', post.parameters, fx, 'moments')
    assert torch.equal(post.mode(), post.parameters[:, :4]) and post.mean.data_ptr() == post.parameters.data_ptr()
    for name in ('logvar', 'std', 'var'):
        _within(report, 'model/' + name, getattr(post, name), fx, name)
    _within(report, 'model/mode', post.mode(), fx, 'mode')
    s = post.sample(generator=torch.Generator().manual_seed(R.NOISE_SEED))
    _within(report, 'model/sample', s, fx, 'sample')
    assert torch.equal(s, R.posterior(post.parameters, torch.from_numpy(fx['noise']).to(DEV), std=post.std)['z'])
    _within(report, 'model/kl', post.kl(), fx, 'kl')
    det = vae.DiagonalGaussianDistribution(post.parameters, deterministic=True)
    assert float(det.std.abs().max()) == 0.0 and float(det.var.abs().max()) == 0.0 and torch.equal(det.logvar, post.logvar)
    assert torch.equal(det.sample(generator=torch.Generator().manual_seed(1)), post.mode()) and float(det.kl()) == 0.0
    z_in = torch.from_numpy(fx['z_in']).to(DEV)
    dec = tiny.decode(z_in)
    assert tuple(dec.sample.shape) == (2, 3, 16, 16) and tiny.decode(z_in, return_dict=False)[0].shape == dec.sample.shape
    _within(report, 'model/decode', dec.sample, fx, 'decode')
    _within(report, 'model/forward', tiny(x).sample, fx, 'forward')
    sp = tiny(x, sample_posterior=True, generator=torch.Generator().manual_seed(R.FORWARD_SEED)).sample
    _within(report, 'model/forward_sample_posterior', sp, fx, 'forward_sp')
    # slicing: one image per call, within the same bound
    tiny.enable_slicing()
    try:
        _within(report, 'model/decode_sliced', tiny.decode(z_in).sample, fx, 'decode')
    finally:
        tiny.disable_slicing()


def test_tiled_encode_and_decode_on_the_reference_fixture(tiny, report, monkeypatch):
    vae, L = pkg('vae'), pkg('_lib')
    lib = L.load()
    fx = R.load('kl_tiled.npz')
    x, z_in = torch.from_numpy(fx['x']).to(DEV), torch.from_numpy(fx['z_in']).to(DEV)
    seen = []
    real = vae.blend_tiles

    def spy(rows, blend_extent, row_limit, blend=None):
        kept = [[t.clone() for t in row] for row in rows]
        before = lib.dp_launch_count()
        out = real(rows, blend_extent, row_limit, blend)
        launched = _launched(lib, before)
        seen.append((kept, blend_extent, row_limit, out, launched))
        return out
    monkeypatch.setattr(vae, 'blend_tiles', spy)
    tiny.enable_tiling()
    try:
        assert tiny.encode(torch.zeros(1, 3, 16, 16, device=DEV)).latent_dist.parameters.shape == (1, 8, 8, 8) and not seen   # at the tile size
        m = tiny.encode(x).latent_dist.parameters
        d = tiny.decode(z_in).sample
    finally:
        tiny.disable_tiling()
    assert tuple(m.shape) == (2, 8, 20, 14) and tuple(d.shape) == (2, 3, 40, 28) and len(seen) == 2
    _within(report, 'tiled/moments', m, fx, 'moments')
    _within(report, 'tiled/decode', d, fx, 'decode')
    for (kept, blend_extent, row_limit, out, launched), side in zip(seen, ('enc', 'dec')):
        assert [len(r) for r in kept] == [3] * 4 and launched == [BLEND] * 12                      # one launch per tile
        assert tuple(kept[3][2].shape) == tuple(fx[side + '_pre_3_2'].shape)
        worst = max(R.err(kept[i][j], fx['%s_pre_%d_%d' % (side, i, j)]) for i in range(4) for j in range(3))
        _line(report, 'tiled/%s_tiles_before_blend' % side, worst_err_to_reference_fp32=worst)
        want = real(kept, blend_extent, row_limit, R.tile_blend)                                     # blends `kept` in place
        assert torch.equal(out, want), side                                                          # the engine's own tiles, the stand-in's blend


def test_first_stage_encoding_and_decoding_with_a_scale_factor(tiny, report):
    ldm_sweep = pkg('ldm_sweep')
    fx = R.load('kl_tiny.npz')
    x = torch.from_numpy(fx['x']).to(DEV)
    sf = 0.18215
    z = ldm_sweep.encode_first_stage(tiny, x, sf, generator=torch.Generator().manual_seed(R.NOISE_SEED))
    want32 = (sf * torch.from_numpy(fx['sample32'])).numpy()
    want64 = float(np.float32(sf)) * fx['sample64']
    e, b = R.err(z, want64), R.bound(want32, want64)
    _line(report, 'first_stage/encode', err=e, bound=b)
    assert tuple(z.shape) == (2, 4, 8, 8) and e <= b
    post = tiny.encode(x).latent_dist
    assert torch.equal(z, R.posterior(post.parameters, torch.from_numpy(fx['noise']).to(DEV), scale=sf, std=post.std)['z'])
    z_in = torch.from_numpy(fx['z_in']).to(DEV)
    dec = ldm_sweep.decode_first_stage(tiny, z_in * 0.5, scale_factor=0.5, force_not_quantize=True)     # 1 / 0.5 * z: exact in fp32
    _within(report, 'first_stage/decode', dec, fx, 'decode')
    assert torch.equal(dec, ldm_sweep.decode_first_stage(tiny, z_in))


def test_ldm_finetune_step_images_on_a_kl_first_stage():
    """One step of the LDM finetune engine on images through the KL first stage: a finite loss, and the bits of step() on latents
    formed by hand from the same (global) generator state."""
    ldm, ldm_sweep, ldm_train, syn = pkg('ldm'), pkg('ldm_sweep'), pkg('ldm_train'), pkg('synthetic')
    cfg = syn.LDM_TINY_CFG
    kl = _tiny(latent_channels=3)
    images = torch.from_numpy(syn.det_clean((2, 3, 32, 32), 3)).to(DEV)
    ids = torch.tensor([1, 0])
    ts = torch.tensor([10, 700])
    noise = torch.from_numpy(syn.det_noise((2, 3, 16, 16), 4))

    def build():
        m = ldm.UNetModel(**cfg)
        gc.det_init_(m, FR.UNET_SEED)
        emb = ldm_sweep.ClassEmbedder(cfg['context_dim'], FR.N_CLASSES)
        with torch.no_grad():
            emb.embedding.weight.copy_(torch.from_numpy(gc.det_param('embedding.weight', (FR.N_CLASSES, cfg['context_dim']), FR.EMB_SEED)))
        return ldm_train.LdmFinetuneEngine(m.to(DEV).eval(), emb.to(DEV), lr=FR.LR, first_stage=kl, scale_factor=0.18215)
    a, b = build(), build()
    torch.manual_seed(31)
    loss_a = float(a.step_images(images, ids, timesteps=ts, noise=noise))
    torch.manual_seed(31)
    z = ldm_sweep.encode_first_stage(kl, images, 0.18215)
    assert tuple(z.shape) == (2, 3, 16, 16)
    loss_b = float(b.step(z, ids, timesteps=ts, noise=noise))
    assert np.isfinite(loss_a) and loss_a == loss_b
    assert torch.equal(a.flat_p, b.flat_p)
    torch.manual_seed(32)                                                           # another draw: other latents
    assert not torch.equal(ldm_sweep.encode_first_stage(kl, images, 0.18215), z)


def test_ldm_pipeline_with_a_kl_first_stage_round_trips(tmp_path):
    diffusion, unet, syn = pkg('diffusion'), pkg('unet'), pkg('synthetic')
    micro = os.path.join(R.GOLD, 'ldm_pipeline_micro')
    with open(os.path.join(micro, 'unet', 'config.json')) as f:
        u = unet.UNet2DModel(**{k: v for k, v in json.load(f).items() if not k.startswith('_')})
    syn.det_init_(u, 81)
    pipe = diffusion.LDMPipeline(vqvae=_tiny(latent_channels=3), unet=u, scheduler=diffusion.DDIMScheduler(
        beta_schedule='scaled_linear', beta_start=0.0015, beta_end=0.0195, clip_sample=False)).to(DEV)
    kw = dict(batch_size=2, num_inference_steps=4, output_type='numpy')
    img = pipe(generator=torch.Generator().manual_seed(82), **kw).images
    assert img.shape == (2, 16, 16, 3) and np.isfinite(img).all() and img.min() != img.max()
    pipe.save_pretrained(str(tmp_path / 'p'))
    with open(str(tmp_path / 'p' / 'model_index.json')) as f:
        assert json.load(f)['vqvae'] == ['diffusers', 'AutoencoderKL']
    back = diffusion.LDMPipeline.from_pretrained(str(tmp_path / 'p')).to(DEV)
    assert type(back.vqvae).__name__ == 'AutoencoderKL'
    img2 = back(generator=torch.Generator().manual_seed(82), **kw).images
    assert img2.tobytes() == img.tobytes()
