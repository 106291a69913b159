"""dp_ups9_dgrad (csrc/ups9.hip) against fp64 autograd of conv2d(interpolate(x, 2, 'nearest'), w, padding=1); the class path's error on the
same inputs is printed next to it.  Bar: 3e-6 of the reference's max-abs (the figure the sibling Winograd kernels' tests use), two runs
bit-equal.  The forward and the weight gradient of the nine-product form are not built: they keep the class launches."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

import golden_common as gc
from helpers import load_npz, make_model, pkg, relerr

pytestmark = pytest.mark.gpu
DEV = 'cuda'
TOL = 3e-6

# N, Cin, Cout, low-resolution H = W
SHAPES = {
    'n3_c16_k40_4x4': (3, 16, 40, 4),       # a 32-pixel block spans two images, the last block is half empty, 40-row K / 16-row M tails
    'n2_c24_k96_8x8': (2, 24, 96, 8),       # channel counts that are no multiple of 16
    'n1_c8_k16_16x16': (1, 8, 16, 16),      # the smallest channel counts
    'n2_c256_k64_16x16': (2, 256, 64, 16),  # two row tiles, 8 .. 16 K tiles through the single LDS stage
    'n2_c20_k7_5x3': (2, 20, 7, 5),         # odd everything (W = 3 below): K tail inside a K tile, columns beyond ld
}


@functools.lru_cache(maxsize=None)
def _case(key):
    N, Cin, Cout, H = SHAPES[key]
    W = 3 if key.endswith('5x3') else H
    g = torch.Generator().manual_seed(1234 + len(key))
    x = torch.randn(N, Cin, H, W, dtype=torch.float64, generator=g, requires_grad=True)
    w = torch.randn(Cout, Cin, 3, 3, dtype=torch.float64, generator=g) / (3.0 * Cin ** 0.5)
    dy = torch.randn(N, Cout, 2 * H, 2 * W, dtype=torch.float64, generator=g)
    add = torch.randn(N, Cin, H, W, dtype=torch.float64, generator=g)
    F.conv2d(F.interpolate(x, scale_factor=2, mode='nearest'), w, padding=1).backward(dy)
    ops = pkg('ops')
    wd, dyd = w.float().to(DEV), ops.empty_act(tuple(dy.shape), DEV).copy_(dy.float())
    up, ldu = ops.pack_weight(ops.ups9_u(wd), 1)
    return dict(ref=x.grad.clone(), add=add, w=wd, dy=dyd, up=up, ldu=ldu, Cin=Cin)


def _class_path(c, accumulate_into=None):
    """Today's four class launches (engine._ups_conv_bwd): de-interleave + one 2x2 convolution per parity class."""
    ops = pkg('ops')
    dyq = ops.deinterleave2x2(c['dy'])
    weff = ops.ups_weff(c['w'])
    dx = accumulate_into
    for k, spec in enumerate(ops.UPS_CLASS_SPECS):
        wd, ldd = ops.pack_weight(weff[k], 1)
        dx = ops.conv_dgrad(dyq[k], wd, ldd, c['Cin'], spec, tuple(c['ref'].shape[2:]), out=dx, accumulate=dx is not None)
    return dx


def _err(got, ref):
    return float((got.double().cpu() - ref).abs().max() / ref.abs().max())


@pytest.mark.parametrize('tile', [0, 1, 2])
@pytest.mark.parametrize('accumulate', [False, True])
@pytest.mark.parametrize('key', sorted(SHAPES))
def test_dgrad_matches_fp64_autograd(key, accumulate, tile):
    ops = pkg('ops')
    c = _case(key)
    ref = c['ref'] + c['add'] if accumulate else c['ref']

    def run():
        out = ops.empty_act(tuple(c['ref'].shape), DEV).copy_(c['add'].float()) if accumulate else None
        return ops.ups9_dgrad(c['dy'], c['up'], c['ldu'], c['Cin'], out=out, accumulate=accumulate, tile=tile)
    a, b = run(), run()
    cls = _class_path(c, ops.empty_act(tuple(c['ref'].shape), DEV).copy_(c['add'].float()) if accumulate else None)
    e9, ecls = _err(a, ref), _err(cls, ref)
    print('ups9 dgrad %s accumulate=%d tile=%d: error %.3e of max-abs (class path %.3e)' % (key, accumulate, tile, e9, ecls))
    assert torch.equal(a, b), 'two runs differ'
    assert e9 < TOL, (key, e9, ecls)


def test_default_tile_and_the_engine_operand():
    """ups9_dgrad without `tile` (ops.ups9_tile) and the operand the engine's pack cache builds give the bits of the explicit launch."""
    ops, engine = pkg('ops'), pkg('engine')
    c = _case('n2_c256_k64_16x16')
    N, Cin, H, W = c['ref'].shape
    a = ops.ups9_dgrad(c['dy'], c['up'], c['ldu'], Cin)
    b = ops.ups9_dgrad(c['dy'], c['up'], c['ldu'], Cin, tile=ops.ups9_tile(N, Cin, H, W))
    packs = engine._Packs()
    up, ldu = packs.get('conv', c['w'], ('up9', 0, 1))
    assert ldu == c['ldu'] and torch.equal(up, c['up']) and ('conv', ('up9', 0, 1)) in packs.lazy
    assert torch.equal(a, b) and torch.equal(a, ops.ups9_dgrad(c['dy'], up, ldu, Cin))


def test_refused_launch_is_an_error_not_a_silent_fallback():
    """What the predicate refuses (here: a dy extent of 2 GiB, beyond the 32-bit byte offsets) is refused by the host rule too, and
    the launcher returns hipErrorInvalidValue without launching."""
    ops, L = pkg('ops'), pkg('_lib')
    c = _case('n1_c8_k16_16x16')
    out = ops.empty_act(tuple(c['ref'].shape), DEV)
    p = ops._ups9_params(c['dy'], c['up'], c['ldu'], c['Cin'], out, False, 0)
    lib = L.load()
    assert lib.dp_ups9_dgrad_supported(ctypes.byref(p)) == 1
    before = lib.dp_launch_count()
    for field, bad in (('dy_bytes', 1 << 31), ('dy_bytes', 64), ('tile', 3), ('ldu', 6), ('u_bytes', 4), ('dx_img_stride', 1), ('N', 0)):
        q = ops._ups9_params(c['dy'], c['up'], c['ldu'], c['Cin'], out, False, 0)
        setattr(q, field, bad)
        assert lib.dp_ups9_dgrad_supported(ctypes.byref(q)) == 0, field
        assert lib.dp_ups9_dgrad(ctypes.byref(q), None) == 1, field                  # hipErrorInvalidValue
        assert not ops.ups9_dgrad_shape_ok(q.N, q.M, q.K, q.H, q.W, q.dy_img_stride, q.dx_img_stride, q.dy_bytes, q.ldu, q.u_bytes,
                                           q.tile, c['up'].data_ptr()), field
    assert lib.dp_launch_count() == before


def _sweep(monkeypatch, mode):
    """4-step Taylor sweep of the tiny UNet (the sweep tests/golden/tiny_unet.npz records) with the nine-product input gradient on every
    upsample convolution ('on'), switched off ('off': DP_UPS9=0), or refused by the gate ('refused')."""
    ops, sweep = pkg('ops'), pkg('sweep')
    calls = [0]
    real = ops.ups9_dgrad

    def counted(*a, **k):
        calls[0] += 1
        return real(*a, **k)
    monkeypatch.setattr(ops, 'ups9_dgrad', counted)
    monkeypatch.setattr(ops, 'UPS9', mode != 'off')
    monkeypatch.setattr(ops, 'ups9_dgrad_gate', (lambda *a: True) if mode == 'on' else (lambda *a: False))
    model = make_model(gc.TINY_CFG, 5)
    clean, noise = torch.from_numpy(gc.det_clean((2, 3, 16, 16), 1)), torch.from_numpy(gc.det_noise((2, 3, 16, 16), 2))
    res = sweep.taylor_sweep(model, pkg('diffusion').DDPMScheduler(), clean.to(DEV), noise.to(DEV), num_steps=4)
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters()}
    pr = sweep.prune_model(model, 0.3)
    return res, grads, [(root, chg, [int(i) for i in pruned]) for root, chg, _, pruned in pr.records], calls[0]


def test_engine_sweep_with_ups9_on_off_and_refused(monkeypatch):
    """The fixture holds the gradients of a FOUR-step sweep, so four steps are run (a two-step sweep has no recorded gradients to hold
    against it).  Its own tolerance: 2e-5 relative per tensor (tests/test_e2e_gpu.py)."""
    g = load_npz('tiny_unet.npz')
    res_on, g_on, masks_on, n_on = _sweep(monkeypatch, 'on')
    res_off, g_off, masks_off, n_off = _sweep(monkeypatch, 'off')
    res_ref, g_ref, masks_ref, n_ref = _sweep(monkeypatch, 'refused')
    assert n_on == 3 * 4 and n_off == 0 and n_ref == 0                       # three upsample convolutions, four steps
    for res in (res_on, res_off):
        assert max(abs(a - b) / b for a, b in zip(res['losses'], g['losses'])) < 1e-5
    worst = {}
    for k in g.files:
        if k.startswith('grad::'):
            for tag, grads in (('on', g_on), ('off', g_off)):
                e = relerr(grads[k[6:]], g[k])
                worst[tag] = max(worst.get(tag, 0.0), e)
                assert e < 2e-5, (tag, k, e)
    print('tiny sweep, worst gradient error against the fixture: DP_UPS9 on %.3e, off %.3e' % (worst['on'], worst['off']))
    assert masks_on == masks_off and len(masks_on) > 0
    # a shape the gate refuses takes the class launches: bit for bit the DP_UPS9=0 run
    assert masks_ref == masks_off and all(torch.equal(g_ref[n], g_off[n]) for n in g_off)
