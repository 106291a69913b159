"""dp_ups9_wgrad + dp_ups9_wgrad_reduce (csrc/ups9_wgrad.hip) against fp64 autograd of conv2d(interpolate(x, 2, 'nearest'), w, padding=1)
on the CPU.  The bound is the project's weight-gradient bound (tests/test_launch_parity_gpu.py TOL_WGRAD): max-abs error below 5e-6 of
the reference's max-abs.  The class path's error on the same inputs (deinterleave2x2 + four conv_wgrad + ups_wfold) is printed beside
it.  Every shape runs with splits = 1, 2 and the launcher's own choice, writing and accumulating onto a non-zero gradient, with the
workspace pre-filled with NaN; two runs are bit-equal; refused launches raise and launch nothing; and the tiny UNet's four-step sweep
with the gates forced open keeps its fixture."""
import ctypes
import functools

import pytest
import torch
import torch.nn.functional as F

import golden_common as gc
from helpers import load_npz, make_model, pkg, relerr
from test_ups9_wgrad_cpu import BRANCHES

pytestmark = pytest.mark.gpu
DEV = 'cuda'
TOL_WGRAD = 5e-6

# N, Cin, Cout, low-resolution H, W
SHAPES = {
    'n2_c64_k64_4x4': (2, 64, 64, 4, 4),        # one tile, borders everywhere, two K tiles
    'n5_c64_k64_2x4': (5, 64, 64, 2, 4),        # a 16-pixel K tile spans two images
    'n3_c80_k96_4x4': (3, 80, 96, 4, 4),        # ragged row and column tiles; P = 48: three K tiles in two splits
    'n2_c64_k64_4x8': (2, 64, 64, 4, 8),        # H != W
    'n2_c128_k72_8x8': (2, 128, 72, 8, 8),      # two column tiles and a ragged second row tile
}


@functools.lru_cache(maxsize=None)
def _case(key):
    N, Cin, Cout, H, W = SHAPES[key]
    g = torch.Generator().manual_seed(977 + len(key) + N)
    x = torch.randn(N, Cin, H, W, dtype=torch.float64, generator=g)
    dy = torch.randn(N, Cout, 2 * H, 2 * W, dtype=torch.float64, generator=g)
    g0 = torch.randn(Cout, Cin, 3, 3, dtype=torch.float64, generator=g)                  # the gradient accumulated onto
    w = torch.zeros(Cout, Cin, 3, 3, dtype=torch.float64, requires_grad=True)
    F.conv2d(F.interpolate(x, scale_factor=2, mode='nearest'), w, padding=1).backward(dy)
    ops = pkg('ops')
    xd = ops.empty_act(tuple(x.shape), DEV).copy_(x.float())
    dyd = ops.empty_act(tuple(dy.shape), DEV).copy_(dy.float())
    return dict(ref=w.grad.detach(), g0=g0.float().double(), g0d=g0.float().to(DEV), x=xd, dy=dyd)


def _class_path(dy, x, gw, accumulate):
    """What the launch pair replaces (engine._ups_conv_bwd on a shape the gate refuses)."""
    ops = pkg('ops')
    dyq = ops.deinterleave2x2(dy)
    gweff = torch.empty((4,) + tuple(gw.shape[:2]) + (2, 2), dtype=torch.float32, device=dy.device)
    for c, spec in enumerate(ops.UPS_CLASS_SPECS):
        ops.conv_wgrad(dyq[c], x, None, gweff[c], spec, accumulate=False)
    return ops.ups_wfold(gweff, gw, accumulate=accumulate)


def _err(got, ref):
    return float((got.double().cpu() - ref).abs().max() / ref.abs().max())


def _poison_workspace():
    ops = pkg('ops')
    ops._workspace(1, torch.device(DEV)).fill_(float('nan'))


def _recent(lib, n):
    arr = (ctypes.c_char_p * 256)()
    k = lib.dp_recent_launches(arr, 256)
    return [arr[i].decode() for i in range(max(0, k - min(n, 256)), k)]


@pytest.mark.parametrize('accumulate', [False, True])
@pytest.mark.parametrize('splits', [1, 2, None])
@pytest.mark.parametrize('key', sorted(SHAPES))
def test_wgrad_matches_fp64(key, splits, accumulate):
    ops = pkg('ops')
    c = _case(key)
    ref = c['ref'] + c['g0'] if accumulate else c['ref']
    lib = ops._lib()
    outs = []
    for _ in range(2):
        gw = c['g0d'].clone()
        _poison_workspace()
        n0 = lib.dp_launch_count()
        ops.ups9_wgrad(c['dy'], c['x'], gw, accumulate=accumulate, splits=splits)
        assert lib.dp_launch_count() == n0 + 2 and _recent(lib, 2) == BRANCHES         # the two new kernels and nothing else
        outs.append(gw)
    cls = _class_path(c['dy'], c['x'], c['g0d'].clone(), accumulate)
    e9, ecls = _err(outs[0], ref), _err(cls, ref)
    print('ups9 wgrad %s splits=%s accumulate=%d: error %.3e of max-abs (class path %.3e)' % (key, splits, accumulate, e9, ecls))
    assert torch.equal(outs[0], outs[1]), 'two runs differ'
    assert e9 < TOL_WGRAD, (key, splits, accumulate, e9, ecls)


def test_channel_slices_of_wider_buffers():
    """x and dy as channel slices of wider buffers (image strides beyond C * H * W) and gw a view inside a larger buffer whose other
    elements stay untouched."""
    ops = pkg('ops')
    key = 'n3_c80_k96_4x4'
    c = _case(key)
    N, Cin, Cout, H, W = SHAPES[key]
    xw = ops.empty_act((N, Cin + 9, H, W), DEV).normal_()
    xs = xw[:, 4:4 + Cin]
    xs.copy_(c['x'])
    dw = ops.empty_act((N, Cout + 6, 2 * H, 2 * W), DEV).normal_()
    ds = dw[:, 3:3 + Cout]
    ds.copy_(c['dy'])
    n = Cout * Cin * 9
    buf = torch.full((n + 64,), 7.0, dtype=torch.float32, device=DEV)
    gw = buf[32:32 + n].view(Cout, Cin, 3, 3)
    ops.ups9_wgrad(ds, xs, gw, accumulate=False)
    plain = torch.empty(Cout, Cin, 3, 3, dtype=torch.float32, device=DEV)
    ops.ups9_wgrad(c['dy'], c['x'], plain, accumulate=False)
    assert torch.equal(gw, plain)
    assert bool((buf[:32] == 7.0).all()) and bool((buf[32 + n:] == 7.0).all())
    assert _err(gw, c['ref']) < TOL_WGRAD


def _params(c, gw, ws, splits, tps):
    ops, L = pkg('ops'), pkg('_lib')
    dy, x = c['dy'], c['x']
    N, Cout, H2, W2 = dy.shape
    Cin = x.shape[1]
    p = L.Ups9WgradParams()
    p.dy, p.x, p.ws, p.gw = dy.data_ptr(), x.data_ptr(), ws.data_ptr(), gw.data_ptr()
    p.dy_img_stride, p.x_img_stride, p.ws_floats = dy.stride(0), x.stride(0), ws.numel()
    p.dy_bytes, p.x_bytes = ops._extent_bytes(dy), ops._extent_bytes(x)
    p.N, p.Co, p.Ci, p.H, p.W = N, Cout, Cin, H2 // 2, W2 // 2
    p.splits, p.tiles_per_split, p.ld, p.accumulate = splits, tps, Cin, 0
    return p


def test_refused_launch_is_an_error_and_launches_nothing():
    ops, L = pkg('ops'), pkg('_lib')
    key = 'n2_c128_k72_8x8'
    c = _case(key)
    N, Cin, Cout, H, W = SHAPES[key]
    lib = L.load()
    gw = torch.empty(Cout, Cin, 3, 3, dtype=torch.float32, device=DEV)
    splits, tps = ops.ups9_wgrad_splits(N, Cin, Cout, H, W)
    ws = torch.empty(splits * 9 * Cout * Cin, dtype=torch.float32, device=DEV)

    def rule(q):
        return ops.ups9_wgrad_shape_ok(q.N, q.Ci, q.Co, q.H, q.W, q.dy_img_stride, q.x_img_stride, q.dy_bytes, q.x_bytes, q.ld, q.splits,
                                       q.tiles_per_split, q.ws_floats, q.dy or 0, q.x or 0, q.ws or 0, q.gw or 0)
    p = _params(c, gw, ws, splits, tps)
    before = lib.dp_launch_count()
    assert rule(p)
    assert lib.dp_ups9_wgrad(ctypes.byref(p), None) == 0 and lib.dp_ups9_wgrad_reduce(ctypes.byref(p), None) == 0     # the block every case below spoils
    torch.cuda.synchronize()
    assert lib.dp_launch_count() == before + 2 and _recent(lib, 2) == BRANCHES
    assert _err(gw, c['ref']) < TOL_WGRAD
    before += 2
    for field, bad in (('dy', c['dy'].data_ptr() + 4), ('dy_img_stride', c['dy'].stride(0) + 1), ('ld', Cin - 1), ('ld', Cin + 1),
                       ('dy_bytes', 1 << 31), ('dy_bytes', 64), ('x_bytes', 1 << 31), ('x_bytes', 64), ('W', 0), ('Ci', -1), ('N', 0),
                       ('x_img_stride', 1), ('dy_img_stride', 2), ('ws_floats', ws.numel() - 1), ('splits', splits + 1), ('splits', 0),
                       ('tiles_per_split', tps - 1), ('gw', 0), ('ws', ws.data_ptr() + 2), ('x', c['x'].data_ptr() + 1)):
        q = _params(c, gw, ws, splits, tps)
        setattr(q, field, bad)
        assert lib.dp_ups9_wgrad(ctypes.byref(q), None) == 1, field                  # hipErrorInvalidValue
        assert lib.dp_ups9_wgrad_reduce(ctypes.byref(q), None) == 1, field
        assert field in ('gw',) or not rule(q), field                                # (a null pointer never reaches the host rule)
    assert lib.dp_launch_count() == before
    # the launcher: a misaligned dy, an odd image stride
    flat = torch.empty(c['dy'].numel() + 8, dtype=torch.float32, device=DEV)
    mis = flat[5:5 + c['dy'].numel()].view_as(c['dy'])                               # 4 bytes off an 8-byte boundary
    assert mis.data_ptr() % 8 == 4
    with pytest.raises(ValueError):
        ops.ups9_wgrad(mis, c['x'], gw)
    per = c['dy'][0].numel() + 1
    odd = torch.empty(N * per + 8, dtype=torch.float32, device=DEV)[4:4 + N * per].view(N, per)[:, :per - 1].view(N, Cout, 2 * H, 2 * W)
    assert odd.stride(0) % 2 == 1 and odd.data_ptr() % 8 == 0
    with pytest.raises(ValueError):
        ops.ups9_wgrad(odd, c['x'], gw)
    assert lib.dp_launch_count() == before


# ---- the engine on the tiny UNet fixture (tiny_unet.npz: 2 x 3 x 16 x 16, four-step sweep), gates forced open
def _open_gates(monkeypatch, on):
    ops = pkg('ops')
    monkeypatch.setattr(ops, 'UPS9', on)
    monkeypatch.setattr(ops, 'UPS9_WGRAD', on)
    monkeypatch.setattr(ops, 'UPS9_FWD_GATE_MIN_BLOCKS', 0)
    monkeypatch.setattr(ops, 'UPS9_GATE_MIN_BLOCKS', 0)
    monkeypatch.setattr(ops, 'UPS9_WGRAD_GATE_MIN_PIX', 0)
    monkeypatch.setattr(ops, 'UPS9_WGRAD_GATE_MIN_CH', 0)


def _sweep(monkeypatch, on):
    ops, sweep = pkg('ops'), pkg('sweep')
    _open_gates(monkeypatch, on)
    calls = [0]
    real = ops.ups9_wgrad

    def counted(*a, **k):
        calls[0] += 1
        return real(*a, **k)
    monkeypatch.setattr(ops, 'ups9_wgrad', counted)
    model = make_model(gc.TINY_CFG, 5)
    clean, noise = torch.from_numpy(gc.det_clean((2, 3, 16, 16), 1)), torch.from_numpy(gc.det_noise((2, 3, 16, 16), 2))
    res = sweep.taylor_sweep(model, pkg('diffusion').DDPMScheduler(), clean.to(DEV), noise.to(DEV), num_steps=4)
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters()}
    pr = sweep.prune_model(model, 0.3)
    monkeypatch.setattr(ops, 'ups9_wgrad', real)
    return res, grads, [(root, chg, [int(i) for i in pruned]) for root, chg, _, pruned in pr.records], calls[0], model


def test_tiny_sweep_with_the_gates_forced_open(monkeypatch):
    """Losses within 1e-5 of the fixture, gradients within 2e-5 per tensor, masks equal to those of the DP_UPS9=0 run."""
    g = load_npz('tiny_unet.npz')
    res_on, g_on, masks_on, n_on, model = _sweep(monkeypatch, True)
    res_off, g_off, masks_off, n_off, _ = _sweep(monkeypatch, False)
    n_up = sum(1 for k in model.state_dict() if 'upsamplers' in k and k.endswith('.weight'))
    assert n_up > 0 and n_on == n_up * 4 and n_off == 0                                 # every upsample convolution, four steps
    for res in (res_on, res_off):
        assert max(abs(a - b) / b for a, b in zip(res['losses'], g['losses'])) < 1e-5
    worst, worst_up = 0.0, 0.0
    for k in g.files:
        if k.startswith('grad::'):
            e = relerr(g_on[k[6:]], g[k])
            worst = max(worst, e)
            if 'upsamplers' in k and k.endswith('.weight'):
                worst_up = max(worst_up, e)
            assert e < 2e-5, (k, e)
    print('tiny sweep with dp_ups9_wgrad: worst gradient error against the fixture %.3e (upsample weights %.3e)' % (worst, worst_up))
    assert masks_on == masks_off and len(masks_on) > 0


def test_one_backward_shows_the_new_kernels_and_no_class_passes(monkeypatch):
    """The ring of one backward pass: the new kernel once per upsample layer, no deinterleave2x2 and no ups_wfold."""
    ops, sweep = pkg('ops'), pkg('sweep')
    _open_gates(monkeypatch, True)
    model = make_model(gc.TINY_CFG, 5)
    clean, noise = torch.from_numpy(gc.det_clean((2, 3, 16, 16), 1)), torch.from_numpy(gc.det_noise((2, 3, 16, 16), 2))
    lib = ops._lib()
    names, real = [], {}

    def spy(fn_name):
        def wrapped(*a, **k):
            n0 = lib.dp_launch_count()
            r = real[fn_name](*a, **k)
            names.extend(_recent(lib, lib.dp_launch_count() - n0))
            return r
        return wrapped
    counts = {'deinterleave2x2': 0, 'ups_wfold': 0}

    def counting(fn_name):
        def wrapped(*a, **k):
            counts[fn_name] += 1
            return real[fn_name](*a, **k)
        return wrapped
    real['ups9_wgrad'] = ops.ups9_wgrad
    monkeypatch.setattr(ops, 'ups9_wgrad', spy('ups9_wgrad'))
    for fn_name in counts:
        real[fn_name] = getattr(ops, fn_name)
        monkeypatch.setattr(ops, fn_name, counting(fn_name))
    sweep.taylor_sweep(model, pkg('diffusion').DDPMScheduler(), clean.to(DEV), noise.to(DEV), num_steps=1)
    torch.cuda.synchronize()
    n_up = sum(1 for k in model.state_dict() if 'upsamplers' in k and k.endswith('.weight'))
    assert n_up > 0 and names == BRANCHES * n_up, names
    assert counts == {'deinterleave2x2': 0, 'ups_wfold': 0}, counts
