"""dp_ups9_fwd (csrc/ups9.hip) against fp64 conv2d(interpolate(x, 2, 'nearest'), w, padding=1) on the CPU, with the error measure and the
bar of tests/test_ups9_gpu.py: max-abs error over the reference's max-abs, below 3e-6; two runs bit-equal.  The class path's error on the
same inputs is held to the same bar, and the two paths may differ by no more than the sum of their errors.  The weight gradient of the
nine-product form is not built: it keeps the class launches, so nothing here covers one."""
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

# N, Cin, Cout, low-resolution H, W
SHAPES = {
    'n5_c20_k36_4x4': (5, 20, 36, 4, 4),        # 80 pixels: one 64-pixel block spans four images, the last block is ragged; K tail, a row tile mostly empty
    'n2_c20_k36_2x6': (2, 20, 36, 2, 6),        # every pixel on a border: every out-of-image patch element
    'n1_c130_k130_4x4': (1, 130, 130, 4, 4),    # crosses two 64-row tiles by two, a K tile by two
    'n2_c64_k64_8x8': (2, 64, 64, 8, 8),        # two full pixel blocks, no tails anywhere
    'n2_c7_k5_5x3': (2, 7, 5, 5, 3),            # odd everything: columns beyond ld, K tail inside the first K tile
}


@functools.lru_cache(maxsize=None)
def _case(key):
    N, Cin, Cout, H, W = SHAPES[key]
    g = torch.Generator().manual_seed(4321 + len(key))
    x = torch.randn(N, Cin, H, W, dtype=torch.float64, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, dtype=torch.float64, generator=g) / (3.0 * Cin ** 0.5)
    b = torch.randn(Cout, dtype=torch.float64, generator=g)
    ref = F.conv2d(F.interpolate(x, scale_factor=2, mode='nearest'), w, padding=1)
    ops = pkg('ops')
    wd, xd = w.float().to(DEV), ops.empty_act(tuple(x.shape), DEV).copy_(x.float())
    up, ldu = ops.pack_weight(ops.ups9_u(wd), 0)
    return dict(ref=ref, ref_b=ref + b[None, :, None, None], w=wd, x=xd, b=b.float().to(DEV), up=up, ldu=ldu, Cout=Cout)


def _class_path(c, x, bias):
    """The four class launches and their interleave pass (engine._ups_conv_fwd on a shape the gate refuses)."""
    ops = pkg('ops')
    N, _, H, W = x.shape
    weff = ops.ups_weff(c['w'])
    q = ops.empty_act((4, N, c['Cout'], H, W), DEV)
    for k, spec in enumerate(ops.UPS_CLASS_SPECS):
        wp, ld = ops.pack_weight(weff[k], 0)
        ops.conv_forward(x, None, wp, ld, c['Cout'], spec, bias=bias, out=q[k])
    return ops.interleave2x2(q)


def _err(got, ref):
    return float((got.double().cpu() - ref).abs().max() / ref.abs().max())


@pytest.mark.parametrize('bias', [False, True])
@pytest.mark.parametrize('key', sorted(SHAPES))
def test_fwd_matches_fp64(key, bias):
    ops = pkg('ops')
    c = _case(key)
    ref = c['ref_b'] if bias else c['ref']
    b = c['b'] if bias else None
    y0 = ops.ups9_fwd(c['x'], c['up'], c['ldu'], c['Cout'], bias=b)
    y1 = ops.ups9_fwd(c['x'], c['up'], c['ldu'], c['Cout'], bias=b)
    cls = _class_path(c, c['x'], b)
    e9, ecls = _err(y0, ref), _err(cls, ref)
    diff = float((y0.double() - cls.double()).abs().max().cpu() / ref.abs().max())
    print('ups9 fwd %s bias=%d: error %.3e of max-abs (class path %.3e), paths differ by %.3e' % (key, bias, e9, ecls, diff))
    assert torch.equal(y0, y1), 'two runs differ'
    assert e9 < TOL and ecls < TOL, (key, e9, ecls)
    assert diff <= e9 + ecls, (key, diff, e9, ecls)


def test_channel_slices_of_wider_buffers():
    """x a channel slice of a wider buffer and y written into one (image strides other than C * H * W); the rest of y stays untouched."""
    ops = pkg('ops')
    c = _case('n5_c20_k36_4x4')
    N, Cin, H, W = c['x'].shape
    wide = ops.empty_act((N, Cin + 9, H, W), DEV).normal_()
    xs = wide[:, 4:4 + Cin]
    xs.copy_(c['x'])
    ywide = ops.empty_act((N, c['Cout'] + 6, 2 * H, 2 * W), DEV).fill_(7.0)
    ys = ywide[:, 2:2 + c['Cout']]
    ops.ups9_fwd(xs, c['up'], c['ldu'], c['Cout'], bias=c['b'], out=ys)
    assert torch.equal(ys, ops.ups9_fwd(c['x'], c['up'], c['ldu'], c['Cout'], bias=c['b']))
    assert bool((ywide[:, :2] == 7.0).all()) and bool((ywide[:, 2 + c['Cout']:] == 7.0).all())
    assert _err(ys, c['ref_b']) < TOL


def test_the_engine_operand():
    ops, engine = pkg('ops'), pkg('engine')
    c = _case('n2_c64_k64_8x8')
    N, Cin, H, W = c['x'].shape
    packs = engine._Packs()
    up, ldu = packs.get('conv', c['w'], ('up9', 0, 0))
    assert ldu == c['ldu'] and torch.equal(up, c['up']) and ('conv', ('up9', 0, 0)) in packs.lazy
    assert torch.equal(ops.ups9_fwd(c['x'], up, ldu, c['Cout']), ops.ups9_fwd(c['x'], c['up'], c['ldu'], c['Cout']))


def test_refused_launch_is_an_error_not_a_silent_fallback():
    ops, L = pkg('ops'), pkg('_lib')
    c = _case('n2_c64_k64_8x8')
    N, Cin, H, W = c['x'].shape
    out = ops.empty_act((N, c['Cout'], 2 * H, 2 * W), DEV)
    lib = L.load()
    p = ops._ups9_fwd_params(c['x'], c['up'], c['ldu'], c['Cout'], None, out)
    before = lib.dp_launch_count()
    assert lib.dp_ups9_fwd(ctypes.byref(p), None) == 0 and lib.dp_launch_count() == before + 1       # the block every case below spoils
    torch.cuda.synchronize()
    before += 1
    for field, bad in (('x_bytes', 1 << 31), ('x_bytes', 64), ('W', 0), ('K', -1), ('ldu', 62), ('ldu', 60), ('u_bytes', 4), ('x_img_stride', 1),
                       ('y_img_stride', 1), ('y_img_stride', 4 * H * W * c['Cout'] + 1), ('N', 0), ('y', out.data_ptr() + 4)):
        q = ops._ups9_fwd_params(c['x'], c['up'], c['ldu'], c['Cout'], None, out)
        setattr(q, field, bad)
        assert lib.dp_ups9_fwd(ctypes.byref(q), None) == 1, field                    # hipErrorInvalidValue
        assert not ops.ups9_fwd_shape_ok(q.N, q.K, q.M, q.H, q.W, q.x_img_stride, q.y_img_stride, q.x_bytes, q.ldu, q.u_bytes,
                                         c['up'].data_ptr(), q.y), field
    assert lib.dp_launch_count() == before
    with pytest.raises(ValueError):
        ops.ups9_fwd(c['x'], c['up'][:-4], c['ldu'], c['Cout'])                      # U is not exactly [9][K][ldu]
    with pytest.raises(ValueError):
        ops.ups9_fwd(c['x'], c['up'], c['ldu'] - 4, c['Cout'])                       # ld narrower than Cout


def _recent(lib, n):
    arr = (ctypes.c_char_p * 256)()
    k = lib.dp_recent_launches(arr, 256)
    return [arr[i].decode() for i in range(max(0, k - min(n, 256)), k)]


def _open_gates(monkeypatch, on):
    ops = pkg('ops')
    monkeypatch.setattr(ops, 'UPS9', on)
    monkeypatch.setattr(ops, 'UPS9_FWD_GATE_MIN_BLOCKS', 0)
    monkeypatch.setattr(ops, 'UPS9_GATE_MIN_BLOCKS', 0)


def test_tiny_forward_with_the_gates_forced_open(monkeypatch):
    """The forward fixture of the tiny UNet (1e-5 absolute, tests/test_e2e_gpu.py) with every upsample convolution on dp_ups9_fwd: the ring
    shows the new kernel once per upsample layer and no interleave pass (nothing else in a forward pass launches one)."""
    ops = pkg('ops')
    _open_gates(monkeypatch, True)
    g = load_npz('tiny_unet.npz')
    model = make_model(gc.TINY_CFG, 5)
    sched = pkg('diffusion').DDPMScheduler()
    clean, noise = torch.from_numpy(gc.det_clean((2, 3, 16, 16), 1)), torch.from_numpy(gc.det_noise((2, 3, 16, 16), 2))
    t = torch.tensor([3, 500])
    noisy = sched.add_noise(clean.to(DEV), noise.to(DEV), t.to(DEV))
    lib = ops._lib()
    with torch.no_grad():
        model(noisy, t.to(DEV))                              # packs and caches
        c0 = lib.dp_launch_count()
        y = model(noisy, t.to(DEV)).sample
        n = lib.dp_launch_count() - c0
    assert 0 < n < 512, n
    names = _recent(lib, n)                                  # the ring holds the last 256: all of the up path, which is the second half
    n_up = sum(1 for k in model.state_dict() if 'upsamplers' in k and k.endswith('.weight'))
    assert n_up > 0 and sum('ups9_fwd_kernel' in s for s in names) == n_up, names
    assert not any('interleave2x2' in s for s in names), names
    assert float((y.cpu() - torch.from_numpy(g['fwd_out'])).abs().max()) < 1e-5


def _sweep(monkeypatch, on):
    ops, sweep = pkg('ops'), pkg('sweep')
    _open_gates(monkeypatch, on)
    calls = [0]
    real = ops.ups9_fwd

    def counted(*a, **k):
        calls[0] += 1
        return real(*a, **k)
    monkeypatch.setattr(ops, 'ups9_fwd', counted)
    model = make_model(gc.TINY_CFG, 5)
    clean, noise = torch.from_numpy(gc.det_clean((2, 3, 16, 16), 1)), torch.from_numpy(gc.det_noise((2, 3, 16, 16), 2))
    res = sweep.taylor_sweep(model, pkg('diffusion').DDPMScheduler(), clean.to(DEV), noise.to(DEV), num_steps=4)
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters()}
    pr = sweep.prune_model(model, 0.3)
    monkeypatch.setattr(ops, 'ups9_fwd', real)
    return res, grads, [(root, chg, [int(i) for i in pruned]) for root, chg, _, pruned in pr.records], calls[0], model


def test_tiny_sweep_and_replay_with_the_gates_forced_open(monkeypatch):
    """The four-step sweep fixture (losses 1e-5, gradients 2e-5 relative per tensor) with the forward and the input gradient of every
    upsample convolution in the nine-product form; the masks equal those of the DP_UPS9=0 run.  Then the pruned model's sampling forward,
    replayed natively with dp_ups9_fwd inside: bit for bit the eager one."""
    g = load_npz('tiny_unet.npz')
    res_on, g_on, masks_on, n_on, model = _sweep(monkeypatch, True)
    res_off, g_off, masks_off, n_off, _ = _sweep(monkeypatch, False)
    assert n_on == 3 * 4 and n_off == 0                      # three upsample convolutions, four steps
    for res in (res_on, res_off):
        assert max(abs(a - b) / b for a, b in zip(res['losses'], g['losses'])) < 1e-5
    worst = 0.0
    for k in g.files:
        if k.startswith('grad::'):
            e = relerr(g_on[k[6:]], g[k])
            worst = max(worst, e)
            assert e < 2e-5, (k, e)
    print('tiny sweep with dp_ups9_fwd and dp_ups9_dgrad: worst gradient error against the fixture %.3e' % worst)
    assert masks_on == masks_off and len(masks_on) > 0

    ops = pkg('ops')
    _open_gates(monkeypatch, True)
    calls = [0]
    real = ops.ups9_fwd

    def counted(*a, **k):
        calls[0] += 1
        return real(*a, **k)
    monkeypatch.setattr(ops, 'ups9_fwd', counted)
    x = torch.from_numpy(gc.det_noise((2, 3, 16, 16), 7)).to(DEV)
    eager = model.sampling_forward(tuple(x.shape), 1, replay=False)
    with torch.no_grad():
        y_eager = eager(x, 500).clone()
    eager.close()
    n_eager = calls[0]
    assert n_eager >= 3
    replayed = model.sampling_forward(tuple(x.shape), 1, replay=True)
    with torch.no_grad():
        replayed(x, 3)
        y_replay = replayed(x, 500).clone()
    nodes = dict(replayed.call.info).get('kernels') if getattr(replayed, 'call', None) is not None else None
    replayed.close()
    assert nodes and calls[0] > n_eager and torch.equal(y_eager, y_replay)
