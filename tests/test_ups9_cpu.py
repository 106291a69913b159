"""The nine-product form of Upsample2D's convolution (csrc/ups9.hip), pinned in fp64 on the CPU.

y = conv3x3(nearest_up2(x), w, pad 1) with U = G w G^T, G = [1 0 0; 1 1 1; 0 0 1]:
  forward          M[a][b] = U[a][b] . V[a][b],  V = B^T d B of the 3x3 low-resolution neighbourhood,  Y = A^T M A
  input gradient   dx = sum_{a,b} U[a][b]^T . T[a][b],  T = R p R^T of the 4x4 high-resolution patch of dy
  weight gradient  dU[a][b] = sum_pixels dM[a][b] (x) V[a][b],  dM = A (2x2 dy block) A^T,  dw = G^T dU G
Each is compared with autograd of conv2d(interpolate(x)).  The input gradient is also restated in the LAYOUT the kernel reads
(dp_pack_weight mode 1 of U: rows [8 - tap][co], columns ci), and the host shape rule is held against a table."""
import pytest
import torch
import torch.nn.functional as F

from helpers import pkg

G = torch.tensor([[1., 0, 0], [1, 1, 1], [0, 0, 1]], dtype=torch.float64)
BT = torch.tensor([[1., -1, 0], [0, 1, 0], [0, -1, 1]], dtype=torch.float64)
AT = torch.tensor([[1., 1, 0], [0, 1, 1]], dtype=torch.float64)
R = torch.tensor([[0., -1, 0, 1], [0, 1, 1, 0], [1, 0, -1, 0]], dtype=torch.float64)

SHAPES = [(3, 5, 7, 4, 4), (2, 6, 4, 8, 8), (1, 3, 2, 5, 3), (2, 4, 4, 1, 1), (1, 2, 3, 2, 6)]      # N, Cin, Cout, H, W


def _case(N, Cin, Cout, H, W, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, Cin, H, W, dtype=torch.float64, generator=g, requires_grad=True)
    w = torch.randn(Cout, Cin, 3, 3, dtype=torch.float64, generator=g, requires_grad=True)
    dy = torch.randn(N, Cout, 2 * H, 2 * W, dtype=torch.float64, generator=g)
    y = F.conv2d(F.interpolate(x, scale_factor=2, mode='nearest'), w, padding=1)
    y.backward(dy)
    return x.detach(), w.detach(), dy, y.detach(), x.grad, w.grad


def _u(w):
    return torch.einsum('ar,oirc,bc->oiab', G, w, G)


def _v(x):
    """V[n, ci, a, b, i, j] = (B^T d B)[a][b] of the 3x3 neighbourhood d of pixel (i, j), zero outside the image."""
    N, Cc, H, W = x.shape
    d = F.unfold(x, 3, padding=1).view(N, Cc, 3, 3, H, W)
    return torch.einsum('ar,ncrsij,bs->ncabij', BT, d, BT)


def _t(dy):
    """T[n, co, a, b, i, j] = (R p R^T)[a][b] of the 4x4 patch p of dy at rows 2i-1 .. 2i+2 / columns 2j-1 .. 2j+2."""
    N, Cc, H2, W2 = dy.shape
    p = F.unfold(dy, 4, padding=1, stride=2).view(N, Cc, 4, 4, H2 // 2, W2 // 2)
    return torch.einsum('ar,ncrsij,bs->ncabij', R, p, R)


def _scale(t):
    return float(t.abs().max()) + 1e-300


@pytest.mark.parametrize('shape', SHAPES)
def test_forward_in_nine_products(shape):
    x, w, dy, y, dx, dw = _case(*shape)
    M = torch.einsum('oiab,niabhw->noabhw', _u(w), _v(x))
    Y = torch.einsum('pa,noabhw,qb->nohpwq', AT, M, AT)                     # (2i + p, 2j + q)
    N, Co, H, _, W, _ = Y.shape
    assert float((Y.reshape(N, Co, 2 * H, 2 * W) - y).abs().max()) < 1e-12 * _scale(y)


@pytest.mark.parametrize('shape', SHAPES)
def test_input_gradient_from_the_high_resolution_patch(shape):
    x, w, dy, y, dx, dw = _case(*shape)
    got = torch.einsum('oiab,noabhw->nihw', _u(w), _t(dy))
    assert float((got - dx).abs().max()) < 1e-12 * _scale(dx)
    # the same sum in the kernel's operand layout: A[tap'][co][ci] = U[co][ci][8 - tap'] (dp_pack_weight mode 1 flips the taps), and the
    # kernel reads row (8 - tap) for T's tap = 3 a + b
    Co, Ci = w.shape[:2]
    A = _u(w).reshape(Co, Ci, 9).flip(2).permute(2, 0, 1)                    # [tap'][co][ci]
    T = _t(dy).reshape(dy.shape[0], Co, 9, *dx.shape[2:])
    got2 = sum(torch.einsum('oi,nohw->nihw', A[8 - tap], T[:, :, tap]) for tap in range(9))
    assert float((got2 - dx).abs().max()) < 1e-12 * _scale(dx)
    # ... and in its other form: the transpose of the forward (dM = A dy-block A^T scattered through B)
    dyb = dy.view(dy.shape[0], Co, dx.shape[2], 2, dx.shape[3], 2)
    dM = torch.einsum('pa,nohpwq,qb->noabhw', AT, dyb, AT)
    dV = torch.einsum('oiab,noabhw->niabhw', _u(w), dM)
    dd = torch.einsum('ar,niabhw,bs->nirshw', BT, dV, BT)                     # gradient of the 3x3 neighbourhoods
    N, _, H, W = dx.shape
    got3 = F.fold(dd.reshape(N, Ci * 9, H * W), (H, W), 3, padding=1)
    assert float((got3 - dx).abs().max()) < 1e-12 * _scale(dx)


@pytest.mark.parametrize('shape', SHAPES)
def test_weight_gradient_folds_through_g(shape):
    x, w, dy, y, dx, dw = _case(*shape)
    N, Co = dy.shape[:2]
    dyb = dy.view(N, Co, x.shape[2], 2, x.shape[3], 2)
    dM = torch.einsum('pa,nohpwq,qb->noabhw', AT, dyb, AT)                  # rows dy[2i], dy[2i] + dy[2i+1], dy[2i+1]
    assert torch.equal(dM[:, :, 0, 0], dyb[:, :, :, 0, :, 0]) and torch.equal(dM[:, :, 2, 2], dyb[:, :, :, 1, :, 1])
    dU = torch.einsum('noabhw,niabhw->oiab', dM, _v(x))
    got = torch.einsum('ar,oiab,bc->oirc', G, dU, G)                        # dw = G^T dU G
    assert float((got - dw).abs().max()) < 1e-12 * _scale(dw)


def test_u_has_integer_coefficients_and_no_halves():
    w = torch.arange(9, dtype=torch.float64).view(1, 1, 3, 3) + 1
    u = _u(w)[0, 0]
    assert u.tolist() == [[1, 6, 3], [12, 45, 18], [7, 24, 9]]


# ---- the host shape rule: one row per accepted / refused launch
def _rule(N, Cin, Cout, H, W, **kw):
    ops = pkg('ops')
    ldu = kw.pop('ldu', (Cin + 3) & ~3)
    a = dict(dy_img_stride=4 * H * W * Cout, dx_img_stride=H * W * Cin, ldu=ldu, u_bytes=9 * Cout * ldu * 4, tile=0, u_ptr=0)
    a['dy_bytes'] = ((N - 1) * a['dy_img_stride'] + 4 * H * W * Cout) * 4
    a.update(kw)
    if 'dy_img_stride' in kw and 'dy_bytes' not in kw:
        a['dy_bytes'] = ((N - 1) * a['dy_img_stride'] + 4 * H * W * Cout) * 4
    return ops.ups9_dgrad_shape_ok(N, Cin, Cout, H, W, a['dy_img_stride'], a['dx_img_stride'], a['dy_bytes'], a['ldu'], a['u_bytes'],
                                   a['tile'], a['u_ptr'])


RULE_TABLE = [
    (dict(N=3, Cin=16, Cout=40, H=4, W=4), True),
    (dict(N=2, Cin=24, Cout=96, H=8, W=8), True),
    (dict(N=1, Cin=8, Cout=16, H=16, W=16), True),
    (dict(N=2, Cin=256, Cout=64, H=16, W=16, tile=2), True),
    (dict(N=256, Cin=256, Cout=256, H=16, W=16, tile=2), True),              # the headline's largest level
    (dict(N=2, Cin=20, Cout=7, H=4, W=8, tile=1), True),                     # odd channel counts, H != W
    (dict(N=1, Cin=3, Cout=5, H=5, W=3), True),
    (dict(N=2, Cin=16, Cout=16, H=4, W=4, dy_img_stride=4 * 16 * 16 + 8), True),      # padded images
    (dict(N=2, Cin=16, Cout=16, H=4, W=4, dy_img_stride=4 * 16 * 16 - 4), False),     # overlapping images
    (dict(N=2, Cin=16, Cout=16, H=4, W=4, dx_img_stride=16 * 16 - 1), False),
    (dict(N=2, Cin=16, Cout=16, H=4, W=4, dy_bytes=4 * (2 * 4 * 16 * 16) - 4), False),   # extent shorter than the images
    (dict(N=2, Cin=18, Cout=16, H=4, W=4, ldu=18), False),                   # ld not a multiple of four
    (dict(N=2, Cin=18, Cout=16, H=4, W=4, ldu=16), False),                   # ld below Cin
    (dict(N=2, Cin=16, Cout=16, H=4, W=4, u_bytes=9 * 16 * 16 * 4 + 4), False),       # not exactly [9][K][ld]
    (dict(N=2, Cin=16, Cout=16, H=4, W=4, u_ptr=8), False),                  # U not 16-byte aligned
    (dict(N=2, Cin=16, Cout=16, H=4, W=4, tile=3), False),
    (dict(N=0, Cin=16, Cout=16, H=4, W=4), False),
    (dict(N=2, Cin=16, Cout=16, H=0, W=4), False),
    (dict(N=512, Cin=256, Cout=256, H=32, W=32), False),                     # dy of 2 GiB: beyond 32-bit byte offsets
    (dict(N=1 << 16, Cin=4, Cout=1, H=128, W=64), False),                    # 2^29 pixels
]


@pytest.mark.parametrize('case', range(len(RULE_TABLE)))
def test_host_shape_rule(case):
    kw, want = RULE_TABLE[case]
    assert _rule(**kw) is want, kw


def test_gate_is_off_with_the_switch_and_never_wants_what_the_rule_cannot_take(monkeypatch):
    ops = pkg('ops')
    monkeypatch.setattr(ops, 'UPS9', False)
    assert not ops.ups9_dgrad_wanted(256, 256, 256, 16, 16)
    monkeypatch.setattr(ops, 'UPS9', True)
    assert not ops.ups9_dgrad_wanted(512, 256, 256, 32, 32)                   # 2 GiB of dy
    assert not ops.ups9_dgrad_wanted(0, 256, 256, 16, 16)
    for t, pix in enumerate(ops.UPS9_TILE_PIX):
        assert pix == (32, 64, 128)[t]
    assert ops.ups9_tile(256, 256, 16, 16) == 2 and ops.ups9_tile(256, 256, 4, 4) == 0
