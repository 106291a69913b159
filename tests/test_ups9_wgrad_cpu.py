"""The nine-product weight gradient of Upsample2D's convolution (csrc/ups9_wgrad.hip) on the host (`-m "not gpu"`): the host shape rule
case by case, the gate and its switches, a numpy stand-in of the split-K partial layout [split][9][Co][Ci] and of the reduce launch
(splits added in ascending order, then dw = G^T dU G) against fp64 autograd, and the launch-site table and plumbing of the new file."""
import os
import re

import numpy as np
import pytest
import torch

from helpers import pkg
from test_ups9_cpu import AT, G, SHAPES, _case, _scale, _v

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- the launch sites of csrc/ups9_wgrad.hip: every kernel expression its U9W_LAUNCH sites can record (tests/test_ups9_wgrad_gpu.py
# asserts the ring shows exactly these two, in this order, for one ops.ups9_wgrad call)
LAUNCH_SITES = {'ups9_wgrad.hip': 2}
BRANCHES = ['ups9_wgrad_kernel', 'ups9_wgrad_reduce_kernel']


# ---- the host shape rule: one row per accepted / refused launch
def _rule(N, Cin, Cout, H, W, **kw):
    ops = pkg('ops')
    want = kw.pop('want_splits', None)
    splits, tps = (kw['splits'], kw['tiles_per_split']) if 'splits' in kw else ops.ups9_wgrad_splits(N, Cin, Cout, H, W, want)
    a = dict(dy_img_stride=4 * H * W * Cout, x_img_stride=H * W * Cin, ld=Cin, splits=splits, tiles_per_split=tps,
             dy_ptr=0, x_ptr=0, ws_ptr=0, gw_ptr=0)
    a.update(kw)
    a.setdefault('dy_bytes', ((N - 1) * a['dy_img_stride'] + 4 * H * W * Cout) * 4)
    a.setdefault('x_bytes', ((N - 1) * a['x_img_stride'] + H * W * Cin) * 4)
    a.setdefault('ws_floats', a['splits'] * 9 * Cout * a['ld'])
    return ops.ups9_wgrad_shape_ok(N, Cin, Cout, H, W, a['dy_img_stride'], a['x_img_stride'], a['dy_bytes'], a['x_bytes'], a['ld'], a['splits'],
                                   a['tiles_per_split'], a['ws_floats'], a['dy_ptr'], a['x_ptr'], a['ws_ptr'], a['gw_ptr'])


RULE_TABLE = [
    (dict(N=2, Cin=64, Cout=64, H=4, W=4), True),
    (dict(N=5, Cin=64, Cout=64, H=2, W=4), True),
    (dict(N=3, Cin=80, Cout=96, H=4, W=4, want_splits=2), True),
    (dict(N=256, Cin=256, Cout=256, H=16, W=16), True),                        # the headline's largest level
    (dict(N=1, Cin=3, Cout=5, H=5, W=3), True),                                # odd everything
    (dict(N=2, Cin=16, Cout=16, H=4, W=4, dy_img_stride=4 * 16 * 16 + 8), True),        # padded images
    (dict(N=2, Cin=16, Cout=16, H=4, W=4, dy_img_stride=4 * 16 * 16 + 7), False),       # odd image stride: 8-byte loads from dy
    (dict(N=2, Cin=16, Cout=16, H=4, W=4, dy_img_stride=4 * 16 * 16 - 4), False),       # overlapping images
    (dict(N=2, Cin=16, Cout=16, H=4, W=4, x_img_stride=16 * 16 - 1), False),
    (dict(N=2, Cin=16, Cout=16, H=4, W=4, x_img_stride=16 * 16 + 3), True),             # x is read four bytes at a time
    (dict(N=2, Cin=16, Cout=16, H=4, W=4, dy_bytes=4 * (2 * 4 * 16 * 16) - 4), False),  # extent shorter than the images
    (dict(N=2, Cin=16, Cout=16, H=4, W=4, x_bytes=4 * (2 * 16 * 16) - 4), False),
    (dict(N=2, Cin=16, Cout=16, H=4, W=4, dy_bytes=1 << 31), False),                    # 2 GiB: bit 31 marks out-of-range offsets
    (dict(N=2, Cin=16, Cout=16, H=4, W=4, x_bytes=1 << 31), False),
    (dict(N=2, Cin=18, Cout=16, H=4, W=4, ld=17), False),                      # ld below Cin
    (dict(N=2, Cin=18, Cout=16, H=4, W=4, ld=19), True),                       # any pitch from Cin on
    (dict(N=2, Cin=16, Cout=16, H=4, W=4, ws_floats=9 * 16 * 16 - 1), False),  # workspace shorter than [splits][9][Co][ld]
    (dict(N=2, Cin=16, Cout=16, H=4, W=4, dy_ptr=4), False),                   # dy not 8-byte aligned
    (dict(N=2, Cin=16, Cout=16, H=4, W=4, dy_ptr=8), True),
    (dict(N=2, Cin=16, Cout=16, H=4, W=4, x_ptr=2), False),
    (dict(N=2, Cin=16, Cout=16, H=4, W=4, ws_ptr=1), False),
    (dict(N=2, Cin=16, Cout=16, H=4, W=4, gw_ptr=6), False),
    (dict(N=2, Cin=16, Cout=16, H=4, W=4, splits=1, tiles_per_split=1), False),         # two K tiles, one covered
    (dict(N=2, Cin=16, Cout=16, H=4, W=4, splits=3, tiles_per_split=1), False),         # an empty split
    (dict(N=2, Cin=16, Cout=16, H=4, W=4, splits=2, tiles_per_split=1), True),
    (dict(N=2, Cin=16, Cout=16, H=4, W=4, splits=0, tiles_per_split=2), False),
    (dict(N=0, Cin=16, Cout=16, H=4, W=4, splits=1, tiles_per_split=1), False),
    (dict(N=2, Cin=16, Cout=0, H=4, W=4, splits=1, tiles_per_split=2), False),
    (dict(N=1 << 21, Cin=1, Cout=1, H=16, W=16, dy_bytes=1024, x_bytes=1024), False),   # 2^29 pixels
]


@pytest.mark.parametrize('i', range(len(RULE_TABLE)))
def test_shape_rule_case_by_case(i):
    kw, want = RULE_TABLE[i]
    assert _rule(**kw) is want, kw


def test_split_choice():
    """As many splits as give UPS9_WGRAD_BLOCKS workgroups, at least four K tiles each, none empty, all K tiles covered."""
    ops = pkg('ops')
    assert ops.UPS9_WGRAD_TILE == (64, 64, 16)
    for shape, splits in [((256, 256, 256, 16, 16), None), ((128, 180, 180, 4, 4), None), ((3, 80, 96, 4, 4), 2), ((2, 64, 64, 4, 4), 7),
                          ((1, 3, 5, 1, 1), None), ((4, 128, 128, 128, 128), None)]:
        N, Cin, Cout, H, W = shape
        s, tps = ops.ups9_wgrad_splits(N, Cin, Cout, H, W, splits)
        nkt = -(-(N * H * W) // 16)
        tiles = -(-Cout // 64) * -(-Cin // 64)
        assert s >= 1 and s * tps >= nkt > (s - 1) * tps, (shape, s, tps)
        if splits is None:
            assert s * tiles <= max(ops.UPS9_WGRAD_BLOCKS, tiles) and (s == 1 or tps >= 4), (shape, s, tps)
        else:
            assert s <= splits
    assert ops.ups9_wgrad_splits(256, 256, 256, 16, 16) == (ops.UPS9_WGRAD_BLOCKS // 16, 4096 * 16 // ops.UPS9_WGRAD_BLOCKS)
    assert ops.ups9_wgrad_splits(3, 80, 96, 4, 4, 2) == (2, 2)                  # three K tiles in two splits


def test_gate_and_switches(monkeypatch):
    ops = pkg('ops')
    shapes = [(256, 256, 256, 4, 4), (256, 256, 256, 8, 8), (256, 256, 256, 16, 16), (128, 180, 180, 4, 4), (128, 180, 180, 16, 16),
              (4, 256, 256, 32, 32), (4, 128, 128, 128, 128), (2, 512, 512, 8, 8), (2, 32, 32, 8, 8), (1, 3, 5, 1, 1)]
    monkeypatch.setattr(ops, 'UPS9', True)
    monkeypatch.setattr(ops, 'UPS9_WGRAD', True)
    # the measured table (profiles/ups9_wgrad_gate.txt): every timed row won; narrower or smaller shapes were not timed and stay off
    measured = [(256, 256, 256, h, h) for h in (4, 8, 16)] + [(128, 180, 180, h, h) for h in (4, 8, 16)] + [
        (128, 179, 179, 16, 16), (256, 128, 128, 16, 16), (4, 512, 512, 8, 8), (4, 512, 512, 16, 16), (4, 256, 256, 32, 32),
        (4, 256, 256, 64, 64), (4, 128, 128, 128, 128), (6, 960, 960, 8, 8), (6, 576, 576, 16, 16), (6, 384, 384, 32, 32)]
    assert all(ops.ups9_wgrad_wanted(*s) for s in measured)
    for s in [(2, 512, 512, 8, 8), (2, 32, 32, 8, 8), (1, 3, 5, 1, 1), (256, 64, 256, 16, 16), (256, 256, 127, 16, 16), (1, 128, 128, 15, 17)]:
        assert not ops.ups9_wgrad_wanted(*s), s
    assert (ops.UPS9_WGRAD_GATE_MIN_PIX, ops.UPS9_WGRAD_GATE_MIN_CH, ops.UPS9_WGRAD_BLOCKS) == (256, 128, 512)
    for s in shapes:
        assert ops.ups9_wgrad_wanted(*s) == ops.ups9_wgrad_gate(*s)
    # never what the rule refuses: no pixels, an extent of 2 GiB or more
    assert not ops.ups9_wgrad_wanted(0, 256, 256, 16, 16) and not ops.ups9_wgrad_wanted(256, 0, 256, 16, 16)
    assert not ops.ups9_wgrad_wanted(2048, 256, 256, 16, 16)                     # dy: 2048 * 256 * 32 * 32 * 4 bytes = 2 GiB
    for N, Cin, Cout, H, W in shapes:
        if ops.ups9_wgrad_wanted(N, Cin, Cout, H, W):
            assert _rule(N, Cin, Cout, H, W), (N, Cin, Cout, H, W)
    for name in ('UPS9', 'UPS9_WGRAD'):
        monkeypatch.setattr(ops, name, False)
        assert not any(ops.ups9_wgrad_wanted(*s) for s in shapes), name
        monkeypatch.setattr(ops, name, True)
    src = open(os.path.join(ROOT, 'diff-pruning_amd', 'ops.py')).read()
    assert "UPS9_WGRAD = os.environ.get('DP_UPS9_WGRAD', '1') not in ('0', '')" in src
    assert "UPS9 = os.environ.get('DP_UPS9', '1') not in ('0', '')" in src


# ---- the partial layout and the reduce launch, in numpy
def _partials(dy, x, splits):
    """ws[split][tap = 3a + b][co][ci] of dp_ups9_wgrad in fp64: K tiles of 16 low-resolution pixels numbered n * H * W + i * W + j over all
    images, split s takes the tiles [s * tps, (s + 1) * tps)."""
    ops = pkg('ops')
    N, Co = dy.shape[:2]
    Ci, H, W = x.shape[1:]
    dyb = dy.view(N, Co, H, 2, W, 2)
    dM = torch.einsum('pa,nohpwq,qb->abonhw', AT, dyb, AT).reshape(9, Co, N * H * W).numpy()
    V = _v(x).permute(2, 3, 1, 0, 4, 5).reshape(9, Ci, N * H * W).numpy()
    s, tps = ops.ups9_wgrad_splits(N, Ci, Co, H, W, splits)
    ws = np.zeros((s, 9, Co, Ci))
    for z in range(s):
        lo, hi = z * tps * 16, min((z + 1) * tps * 16, N * H * W)
        assert lo < hi
        ws[z] = np.einsum('tok,tik->toi', dM[:, :, lo:hi], V[:, :, lo:hi])
    return ws


def _reduce(ws, gw, accumulate):
    """dp_ups9_wgrad_reduce: splits in ascending order, rows (u0 + u1, u1, u1 + u2) of G^T dU, the same on columns, (+)= into gw."""
    u = ws[0].copy()
    for z in range(1, ws.shape[0]):
        u = u + ws[z]
    u = u.reshape(3, 3, *ws.shape[2:])
    g = np.stack([u[0] + u[1], u[1], u[1] + u[2]])
    dw = np.stack([g[:, 0] + g[:, 1], g[:, 1], g[:, 1] + g[:, 2]], axis=1)       # [r][c][co][ci]
    dw = dw.transpose(2, 3, 0, 1)
    return gw + dw if accumulate else dw


@pytest.mark.parametrize('splits', [1, 2, None])
@pytest.mark.parametrize('shape', SHAPES + [(5, 6, 4, 2, 4), (3, 5, 6, 4, 4)])
def test_partial_layout_and_reduce_equal_autograd(shape, splits):
    x, w, dy, y, dx, dw = _case(*shape)
    ws = _partials(dy, x, splits)
    got = _reduce(ws, np.zeros(tuple(w.shape)), False)
    assert float(np.abs(got - dw.numpy()).max()) < 1e-12 * _scale(dw)
    # ... which is G^T dU G of the summed partials
    dU = torch.from_numpy(ws.sum(0)).reshape(3, 3, *ws.shape[2:])
    ref = torch.einsum('ar,aboi,bc->oirc', G, dU, G)
    assert float((torch.from_numpy(got) - ref).abs().max()) < 1e-12 * _scale(dw)
    base = np.full(tuple(w.shape), 0.5)
    assert float(np.abs(_reduce(ws, base, True) - (dw.numpy() + 0.5)).max()) < 1e-12 * (_scale(dw) + 0.5)


# ---- plumbing
def test_every_launch_site_of_ups9_wgrad_hip_is_tabled_and_the_file_is_plumbed():
    """csrc/ups9_wgrad.hip launches through U9W_LAUNCH, a macro of its own with the body of the library's launch macro (the discipline of
    tests/test_stage_study_cpu.py): a new site changes the count, a new kernel is in no table.  The file stays out of the older tables'
    census, which counts the library macro's call text per file; it is in both build lists and declared with its bindings."""
    csrc = os.path.join(ROOT, 'diff-pruning_amd', 'csrc')
    assert list(LAUNCH_SITES) == ['ups9_wgrad.hip']
    src = open(os.path.join(csrc, 'ups9_wgrad.hip')).read()
    body = src.replace('#define U9W_LAUNCH(', '')
    sites = re.findall(r'\bU9W_LAUNCH\(\(?\s*([A-Za-z_]\w*)', body)
    assert len(sites) == LAUNCH_SITES['ups9_wgrad.hip'] == body.count('U9W_LAUNCH('), sites
    assert 'DP_' + 'LAUNCH(' not in src
    assert re.search(r'#define U9W_LAUNCH\(k, \.\.\.\).*dp_launch_names\[dp_launches\+\+ & \(DP_LAUNCH_RING - 1\)\] = #k;.*'
                     r'hipLaunchKernelGGL\(k, __VA_ARGS__\)', src)
    assert sites == BRANCHES and len(set(BRANCHES)) == len(BRANCHES)
    using = {f for f in os.listdir(csrc) if 'U9W_LAUNCH(' in open(os.path.join(csrc, f)).read()}
    assert using == {'ups9_wgrad.hip'}
    assert 'atomicAdd' not in src and 'atomic_' not in src                     # a fixed summation order
    assert 'csrc/ups9_wgrad.hip' in open(os.path.join(ROOT, 'build.sh')).read()
    assert "'csrc/ups9_wgrad.hip'" in open(os.path.join(ROOT, '__graft_entry__.py')).read()
    # header, ctypes table and ops agree
    L, ops = pkg('_lib'), pkg('ops')
    hdr = open(os.path.join(ROOT, 'include', 'dp_hip.h')).read()
    for sym, n in (('dp_ups9_wgrad', 2), ('dp_ups9_wgrad_reduce', 2)):
        assert len(L.SIGNATURES[sym]) == n
        args = 'const dp_ups9_wgrad_params* p, void* stream'
        assert 'int %s(%s);' % (sym, args) in hdr
        assert getattr(L.load(), sym) is not None
    # the native predicate is applied by both launchers and, like dp_ups9_fwd's, not exported
    assert src.count('if (!dp_ups9_wgrad_supported(pp)) return (int)hipErrorInvalidValue;') == 2
    assert 'dp_ups9_wgrad_supported' not in L.SIGNATURES
    fields = re.search(r'typedef struct dp_ups9_wgrad_params \{(.*?)\} dp_ups9_wgrad_params;', hdr, re.S).group(1)
    names = [re.search(r'(\w+)\s*$', part).group(1) for decl in fields.split(';') if decl.strip() for part in decl.split(',')]
    assert names == [f[0] for f in L.Ups9WgradParams._fields_], names
    assert ops._UPS9_WGRAD_NAMES == tuple(BRANCHES)
    bm, bn, kp = ops.UPS9_WGRAD_TILE
    for macro, v in (('U9W_BM', bm), ('U9W_BN', bn), ('U9W_KP', kp)):
        assert re.search(r'#define %s %d\b' % (macro, v), src)
    for name in ('ups9_wgrad', 'ups9_wgrad_wanted', 'ups9_wgrad_gate', 'ups9_wgrad_shape_ok', 'ups9_wgrad_splits'):
        assert callable(getattr(ops, name))
    # the CPU engine tests keep the class path: their stand-in has no such entry
    import mock_ops
    assert not hasattr(mock_ops, 'ups9_wgrad_wanted')
