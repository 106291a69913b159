"""fp64 parity of every buffer-descriptor kernel at the top of its 32-bit reach.

The contraction kernels (csrc/gemm.hip, winograd.hip, winograd2d.hip, winograd43.hip, wgrad2d.hip, ups9.hip) address their inputs through raw
buffer descriptors with 32-bit byte offsets; bit 31 of an offset is the "padding / tail: load 0.0f" marker, which is sound while every
descriptor's num_records stays below 0x80000000.  ops._extent_bytes refuses 2 GiB and more, the shifted descriptors give way a little
earlier (conv_fast_ok / nt_fast_ok: 4 * shift bytes, the F(2, 3) and F(4, 3) rules: 4 * W bytes), and production batches are chosen to end
right below the limit.  tests/test_contraction_dispatch_gpu.py pins every dispatch branch at offsets near zero; this module runs the same
entry points on activations whose extent E is

  2^31 - 4            the top: image stride odd, image 1 ends on the last readable byte
  2^31 - 16           the top with 16-byte aligned image strides (and once more starting one float later: a 4-byte aligned base)
  2^30 + 2^29         mid-reach: offsets with bit 30 set
  the route's rule    its last accepted extent and the first refused one (rounded to 16 bytes as well, and to the route's own alignment
                      where it has one): above the rule the fallback kernel must be the one in the ring, and parity must still hold

THE ARENA.  One module-scoped device buffer: 2^16 guard floats, 2^30 floats, 2^16 guard floats.  Every tensor under test is a two-image view
that starts at the first float behind the front guard with image stride E / 4 - C * H * W, so that its extent is exactly E.  Whatever a
32-bit byte offset can reach from any descriptor base the kernels build (the bases are moved back by at most ~1000 floats) lies inside the
arena: wrong offset arithmetic shows as a parity failure, never as an access outside mapped memory.  The arena is filled with the finite
sentinel 32768.0 before every case (an over-read the kernel zeroes afterwards -- fix_border -- stays harmless; a misread times a weight of
order 1 / sqrt(9 K) is orders of magnitude above every bound), then the two images are written.

Shapes: two images of 16 x 16 to 20 x 17 pixels and 16 to 128 channels, pad 1 -- both images have padded rows and columns, and the top row
of image 0 is where a marker inside a descriptor would show.  The forms that exist only for grids of more than 512 workgroups (F(2x2, 3x3)
with 4-channel K tiles, and its 32-row form) take 514 x 64-pixel images of 8 channels.  Kernel families are reached the way the dispatch
module does: `gates` on the module switches and a pinned ops.pick_tile; never a hand-filled parameter block.  Each case compares EVERY
output element with an fp64 evaluation of the same fp32 inputs on the CPU (helpers.relerr) after a poisoned allocation, under the bounds
of the dispatch module (no new tolerance), and asserts through launched_m which kernel ran.  conv_dgrad has one input, so the second pass
(the arena tensor as x2 of a virtual concat, x1 small) is conv_forward's alone; conv_few_out_kernel takes one source; F(4, 3) has no
input-gradient operand (ops.pack_weight_wino43 is forward only).  conv_wgrad runs
with dy in the arena and x small, the other way round, and (the two direct kernels) with the arena tensor as x2.

Refusals (dp_launch_count unchanged): a view of extent exactly 2^31 through conv_forward / conv_dgrad / conv_wgrad / ups9_fwd / ups9_dgrad,
and bmm_tn / bmm_nn / bmm_nt with a 2^31-byte matrix.  Batch strides past 32 bits: bmm_nn and attention_fwd with a stride of 2^30 + 64 floats.

pytest -s prints one `reach/...` line per launch: profiles/reach_gpu_tests.txt."""
import importlib
import math

import pytest
import torch
import torch.nn.functional as F

import test_contraction_dispatch_gpu as CD
import test_dispatch_parity_gpu as D
from helpers import ref_attention, ref_conv_dgrad, ref_conv_fwd, ref_conv_wgrad, relerr
from test_contraction_dispatch_gpu import B_ATTN, B_BMM, B_DIRECT, B_F43, B_UPS9, B_WINO, B_WINO_WGRAD, gates, guarded_act, launched_m, nan_like
from test_dispatch_parity_gpu import d64, poison, rnd

pytestmark = pytest.mark.gpu

GUARD, BODY, REACH = 1 << 16, 1 << 30, 1 << 31
SENTINEL = 32768.0
TOP, TOP16, MID = REACH - 4, REACH - 16, (1 << 30) + (1 << 29)
CONV_FAST_IMM, NT_FAST_IMM = 3 * 1024, 7 * 65 * 4          # bytes the two fast kernels move their descriptor bases back by (csrc/gemm.hip)


@pytest.fixture(scope='module')
def ops():
    importlib.import_module('diff-pruning_amd')
    o = importlib.import_module('diff-pruning_amd.ops')
    o._lib()
    assert (o._CONV_FAST_IMM_MAX, o._NT_FAST_IMM_MAX, o._MAX_BYTES) == (CONV_FAST_IMM, NT_FAST_IMM, REACH)
    return o


@pytest.fixture(scope='module')
def arena():
    box = [torch.empty(GUARD + BODY + GUARD, dtype=torch.float32, device=D.DEV)]
    yield box[0]
    box.clear()
    torch.cuda.empty_cache()


def view_of(arena, shape, E, off=0):
    """The two-image view of extent E bytes that starts `off` floats behind the front guard (nothing is written)."""
    N, C, H, W = shape
    assert N == 2 and E % 4 == 0 and 0 <= off and GUARD + off + E // 4 <= arena.numel()
    s0 = E // 4 - C * H * W
    assert s0 >= C * H * W
    return arena.as_strided((2, C, H, W), (s0, H * W, W, 1), GUARD + off)


def place(ops, arena, imgs, E, off=0):
    """Sentinel everywhere, then the two images at the two ends of an extent of E bytes."""
    arena.fill_(SENTINEL)
    v = view_of(arena, tuple(imgs.shape), E, off)
    v.copy_(imgs)
    assert ops._extent_bytes(v) == E and v.storage_offset() >= 1
    return v


def extents(rule=0, align=4):
    """{E: label} of a route that accepts E while E + rule < 2^31 (rule = 0: up to the top) and E % align == 0."""
    fl = lambda e, a: e // a * a
    cl = lambda e, a: -(-e // a) * a
    ex = {fl(TOP, align): 'top', TOP16: 'top, 16-byte strides', MID: 'mid-reach'}
    if rule:
        lim = REACH - rule
        for a in sorted({align, 16}):
            ex.setdefault(fl(lim - 4, a), 'last below the rule' + (', %d-byte strides' % a if a > 4 else ''))
            ex.setdefault(cl(lim, a), 'first the rule refuses' + (', %d-byte strides' % a if a > 4 else ''))
    assert all(e % align == 0 and e < REACH for e in ex)
    return ex


def line(report, key, **kv):
    print('reach/%s %s' % (key, ' '.join('%s=%s' % (k, ('%.3e' % v) if isinstance(v, float) else str(v).replace(' ', '')) for k, v in kv.items())))
    report.setdefault('reach/' + key.split(' ')[0], []).append({k: v for k, v in kv.items()})


def check(report, bad, key, err, bound, **kv):
    line(report, key, err=err, bound=bound, **kv)
    if not err <= bound:                                   # NaN is not within
        bad.append((key, err, bound, kv))


# ======================================================================================================================
# conv_forward / conv_dgrad
# ======================================================================================================================
def S(ops, k=3, stride=1, pad=1, ups=0):
    return ops.ConvSpec(k, stride, pad, ups)


_FAST = 'conv_gemm_fast_kernel<%s>'
_GEN = 'conv_gemm_kernel<%s, false, false>'
_NOSPLIT = dict(CONV_SPLITK_BLOCKS=0)
_W1 = dict(WINO_MIN_TILES=0, CONV_SPLITK_BLOCKS=0)
_W2 = dict(WINO_MIN_TILES=0, WINO2D_MIN_TILES=0, CONV_SPLITK_BLOCKS=0)
_W43 = dict(WINO_MIN_TILES=0, WINO43=True, WINO43_MIN_TILES=0, CONV_SPLITK_BLOCKS=0)
# id: (K channels of the arena tensor, M output channels, H, W, stride, pinned pick_tile or None, gates, wino operand, the mirror name while
#      the route accepts, rule: None / 'fast' (4 * shift) / 'row' (4 * W), alignment of E the route needs, bound, kinds, ring names it must hold,
#      predicate on the parameter block)
CONV = {
    'general_128x128':  (24, 40, 16, 16, 2, 0, _NOSPLIT, None, _GEN % '128, 128', None, 4, B_DIRECT, ('fwd', 'dgrad'), (), None),
    'general_64x128':   (24, 40, 16, 16, 1, 1, _NOSPLIT, None, _GEN % '64, 128', None, 4, B_DIRECT, ('fwd', 'dgrad'), (), None),
    'general_64x64':    (24, 40, 16, 16, 1, 2, _NOSPLIT, None, _GEN % '64, 64', None, 4, B_DIRECT, ('fwd', 'dgrad'), (), None),
    'fast_x4':          (32, 100, 16, 16, 1, None, _NOSPLIT, None, _FAST % '128, 128, false, true', 'fast', 4, B_DIRECT, ('fwd', 'dgrad'), (), None),
    'fast_x4_tails':    (24, 100, 16, 16, 1, None, _NOSPLIT, None, _FAST % '128, 128, true, true', 'fast', 4, B_DIRECT, ('fwd', 'dgrad'), (), None),
    'fast_x1':          (32, 100, 16, 18, 1, None, _NOSPLIT, None, _FAST % '128, 128, false, false', 'fast', 4, B_DIRECT, ('fwd', 'dgrad'), (), None),
    'fast_x1_tails':    (24, 100, 16, 18, 1, None, _NOSPLIT, None, _FAST % '128, 128, true, false', 'fast', 4, B_DIRECT, ('fwd', 'dgrad'), (), None),
    'fast_x4_96':       (24, 90, 16, 16, 1, None, _NOSPLIT, None, _FAST % '96, 128, true, true', 'fast', 4, B_DIRECT, ('fwd', 'dgrad'), (), None),
    # 4 tiles and 36 K tiles: 18 slices by ops._conv_ksplit's own rule, more than SPLITK_FOLD_MAX -> the reduction launch
    'fast_x4_splitk':   (64, 100, 16, 16, 1, None, {}, None, _FAST % '128, 128, false, true', 'fast', 4, B_DIRECT, ('fwd', 'dgrad'),
                         ('conv_splitk_epilogue4_kernel',), lambda b: b['ksplit'] > 1),
    'few_out':          (20, 3, 20, 17, 1, None, _NOSPLIT, None, 'conv_few_out_kernel', None, 4, B_DIRECT, ('fwd', 'dgrad'), (), None),
    'wino_16':          (32, 40, 16, 16, 1, None, _W1, '1d', 'conv_wino_kernel<16, 2, 1>', 'row', 4, B_WINO, ('fwd', 'dgrad'), (), None),
    'wino_8':           (24, 80, 16, 16, 1, None, _W1, '1d', 'conv_wino_kernel<8, 1, 1>', 'row', 4, B_WINO, ('fwd', 'dgrad'), (), None),
    # 4 tiles against WINO_MIN_TILES = 16: min(16 // 4, 24 K tiles // 8) = 3 slices
    'wino_16_splitk':   (128, 40, 16, 16, 1, None, dict(WINO_MIN_TILES=16, CONV_SPLITK_BLOCKS=0), '1d', 'conv_wino_kernel<16, 2, 1>', 'row', 4, B_WINO,
                         ('fwd', 'dgrad'), ('conv_splitk_epilogue4_kernel',), lambda b: b['ksplit'] == 3),
    'wino2d':           (24, 40, 16, 16, 1, None, _W2, '2d', 'conv_wino2d_kernel<8, 2, false>', None, 8, B_WINO, ('fwd', 'dgrad'), (), None),
    'wino2d_tail':      (24, 70, 16, 16, 1, None, _W2, '2d', 'conv_wino2d_tail_kernel<8, 2, false>', None, 8, B_WINO, ('fwd', 'dgrad'), (), None),
    # more than 512 workgroups from two images: 514 x 64 pixels = 514 tiles of 128 pixels (x 2 row tiles for 80 rows)
    'wino2d_k4':        (8, 40, 514, 64, 1, None, _W2, '2d', 'conv_wino2d_kernel<4, 3, false>', None, 8, B_WINO, ('fwd', 'dgrad'), (), None),
    'wino2d_m32':       (8, 80, 514, 64, 1, None, _W2, '2d', 'conv_wino2d_m32_kernel<4, 5, false>', None, 8, B_WINO, ('fwd', 'dgrad'), (), None),
    'wino43':           (24, 40, 16, 16, 1, None, _W43, '43', 'conv_wino43_kernel', 'row', 16, B_F43, ('fwd',), (), None),
}
X1_SMALL = 16       # channels of the small first source of the second pass (a whole 16-channel chunk: the TAILS / BK forms are unchanged)


def conv_rule(rule, W):
    return {None: 0, 'fast': 4 * (W + 1) + CONV_FAST_IMM, 'row': 4 * W}[rule]


def run_conv(ops, mp, arena, report, bad, fid, kind, src, E, label, off=0):
    """One launch of family `fid` with the arena tensor as `src` ('x1' / 'x2'; dgrad: 'x1' = dy) at extent E."""
    K, M, H, W, stride, tile, g, wino, want, rule, align, bound, kinds, has, blk = CONV[fid]
    fwd = kind == 'fwd'
    spec = S(ops, 3, stride, 1)
    K1 = X1_SMALL if src == 'x2' else 0
    Kt = K1 + K
    big = place(ops, arena, rnd(2, K, H, W, seed=1), E, off)
    small = guarded_act(ops, rnd(2, K1, H, W, seed=2)) if K1 else None
    x1, x2 = (small, big) if K1 else (big, None)
    w = rnd(*((M, Kt) if fwd else (Kt, M)), 3, 3, seed=3, scale=1.0 / math.sqrt(9 * Kt))
    wp, ld = ops.pack_weight(w, 0 if fwd else 1)
    kw = {}
    if wino == '1d':
        kw['wino'] = ops.pack_weight_wino(w, 0 if fwd else 1)
    elif wino == '2d':
        kw['wino'] = ('2d',) + tuple(ops.pack_weight_wino2d(w, 0 if fwd else 1))
    elif wino == '43':
        kw['wino43'] = ops.pack_weight_wino43(w)
    x64 = d64(x1) if x2 is None else torch.cat([d64(x1), d64(x2)], 1)
    if fwd:
        b = rnd(M, seed=4)
        ref = ref_conv_fwd(x64, d64(w), spec) + d64(b)[None, :, None, None]
        call = lambda: ops.conv_forward(x1, x2, wp, ld, M, spec, bias=b, **kw)
    else:
        in_hw = (H * stride, W * stride)
        ref = ref_conv_dgrad(x64, d64(w), spec, in_hw)
        call = lambda: ops.conv_dgrad(x1, wp, ld, M, spec, in_hw, **kw)
    with mp.context() as m:
        gates(ops, m, **g)
        if tile is not None:
            m.setattr(ops, 'pick_tile', lambda *a, **k: tile)
        poison(ref.numel())
        y, names, seen = launched_m(ops, m, call)
    assert tuple(y.shape) == tuple(ref.shape) and len(seen) == 1, (fid, seen)
    mirror = seen[0][0]
    accepted = E % align == 0 and (off == 0 or align == 4) and E + conv_rule(rule, W) < REACH
    if accepted:
        assert mirror == want and all(h in names for h in has) and (blk is None or blk(seen[0][1])), (fid, kind, src, E, seen, names)
    else:       # above the route's rule (or off its alignment): the direct form, and above the fast kernels' rule its unshifted kernel
        assert rule is not None or align > 4, (fid, E)
        base = 'conv_gemm_kernel<' if E + conv_rule('fast', W) >= REACH else 'conv_gemm'
        assert mirror.startswith(base) and any(n.startswith(base) for n in names), (fid, kind, src, E, seen, names)
    check(report, bad, '%s/%s/%s E=2^31-%d%s' % (fid, kind, src, REACH - E, '+1float' if off else ''), relerr(y, ref), bound,
          kernel=mirror, names=names, route='accepted' if accepted else 'refused', extent=label)


@pytest.mark.parametrize('fid', list(CONV))
def test_conv_at_the_reach(fid, ops, arena, report, monkeypatch):
    K, M, H, W, stride, tile, g, wino, want, rule, align, bound, kinds, has, blk = CONV[fid]
    bad = []
    for kind in kinds:
        for src in (('x1', 'x2') if kind == 'fwd' and fid != 'few_out' else ('x1',)):
            for E, label in sorted(extents(conv_rule(rule, W), align).items()):
                run_conv(ops, monkeypatch, arena, report, bad, fid, kind, src, E, label)
            if align == 4:
                run_conv(ops, monkeypatch, arena, report, bad, fid, kind, src, TOP16, 'top, base one float later', off=1)
    assert not bad, bad


# ======================================================================================================================
# conv_wgrad
# ======================================================================================================================
_WG1 = dict(WGRAD_WINO_MIN_WORK=0, WGRAD_WINO_MIN_FILL=0.0, WGRAD_WINO2D=False)
_WG2 = dict(WGRAD_WINO_MIN_WORK=0, WGRAD_WINO_MIN_FILL=0.0, WGRAD_WINO2D_MIN_FILL=0.0)
# id: (C input channels, Cout, H, W, gates, mirror while accepted, {source in the arena: rule bytes}, bound)
WGRAD = {
    'nt_general':   (40, 100, 18, 18, {}, 'nt_gemm_kernel<128, 128, false, false>', dict(dy=0, x=0), B_DIRECT),
    'nt_general_64': (40, 40, 18, 18, {}, 'nt_gemm_kernel<64, 128, false, false>', dict(dy=0, x=0), B_DIRECT),
    'nt_fast':      (40, 100, 16, 16, {}, 'nt_gemm_fast_kernel<4, false>', dict(dy=NT_FAST_IMM, x=4 * 17 + NT_FAST_IMM), B_DIRECT),
    'nt_fast_96':   (90, 90, 16, 16, {}, 'nt_gemm_fast_kernel<3, false>', dict(dy=NT_FAST_IMM, x=4 * 17 + NT_FAST_IMM), B_DIRECT),
    'wgrad_wino':   (40, 70, 16, 16, _WG1, 'wgrad_wino_kernel<2, 2>', dict(dy=0, x=4 * 16), B_WINO_WGRAD),
    'wgrad_wino2d': (40, 40, 16, 16, _WG2, 'wgrad_wino2d_kernel<4>', dict(dy=0, x=0), B_WINO_WGRAD),
    'wgrad_wino2d_tail': (40, 70, 16, 16, _WG2, 'wgrad_wino2d_tail_kernel<4>', dict(dy=0, x=0), B_WINO_WGRAD),
}


# ... and with the arena tensor as x2: 32 + 40 input channels, the boundary inside a 128-column tile (the general kernel's straddle form)
WGRAD_X1_SMALL = 32
WGRAD_X2 = {'nt_general': 'nt_gemm_kernel<128, 128, true, false>', 'nt_fast': 'nt_gemm_fast_kernel<4, true>'}


def run_wgrad(ops, mp, arena, report, bad, fid, src, E, label, off=0):
    C, Cout, H, W, g, want, rules, bound = WGRAD[fid]
    spec = S(ops)
    x2 = None
    if src == 'dy':
        dy, x = place(ops, arena, rnd(2, Cout, H, W, seed=1), E, off), rnd(2, C, H, W, seed=2)
    elif src == 'x':
        dy, x = rnd(2, Cout, H, W, seed=1), place(ops, arena, rnd(2, C, H, W, seed=2), E, off)
    else:       # the arena tensor as the second source of a virtual concat behind WGRAD_X1_SMALL channels
        dy, x, x2 = rnd(2, Cout, H, W, seed=1), rnd(2, WGRAD_X1_SMALL, H, W, seed=5), place(ops, arena, rnd(2, C, H, W, seed=2), E, off)
        want = WGRAD_X2[fid]
    xs = x if x2 is None else torch.cat([x, x2], 1)
    ref = ref_conv_wgrad(dy, xs, spec, 3, 3)
    gw = nan_like(Cout, xs.shape[1], 3, 3)
    with mp.context() as m:
        gates(ops, m, **g)
        _, names, seen = launched_m(ops, m, lambda: ops.conv_wgrad(dy, x, x2, gw, spec, accumulate=False))
    assert len(seen) == 1, (fid, seen)
    mirror = seen[0][0]
    accepted = E + rules['x' if src == 'x2' else src] < REACH
    if accepted:
        assert mirror == want, (fid, src, E, seen, names)
    else:       # the Winograd rule (4 W) lies inside the fast kernel's (4 shift): above either, the unshifted nt_gemm_kernel
        assert mirror.startswith('nt_gemm_kernel<128, 128') and any(n.startswith('nt_gemm_kernel<') for n in names), (fid, src, E, seen, names)
        assert seen[0][1]['tile'] == 0, (fid, seen)        # no 96 x 96 preference (and its grid / slice sizing) for a launch the fast kernel refuses
    check(report, bad, '%s/%s E=2^31-%d%s' % (fid, src, REACH - E, '+1float' if off else ''), relerr(gw, ref), bound, kernel=mirror, names=names,
          splits=seen[0][1]['splits'], route='accepted' if accepted else 'refused', extent=label)


@pytest.mark.parametrize('fid', list(WGRAD))
def test_wgrad_at_the_reach(fid, ops, arena, report, monkeypatch):
    bad = []
    for src in ('dy', 'x') + (('x2',) if fid in WGRAD_X2 else ()):
        for E, label in sorted(extents(WGRAD[fid][6]['x' if src == 'x2' else src]).items()):
            run_wgrad(ops, monkeypatch, arena, report, bad, fid, src, E, label)
        run_wgrad(ops, monkeypatch, arena, report, bad, fid, src, TOP16, 'top, base one float later', off=1)
    assert not bad, bad


# ======================================================================================================================
# the nine-product kernels: the activation at 2^31 - 16; at 2^31 the host rules refuse, and the convolution that takes over -- the fused
# nearest-x2 upsample of conv_forward on the direct kernel -- gives the same answer from the same view.  That convolution cannot itself
# run AT 2^31: conv_forward raises there like every entry point (test_two_gib_is_refused_without_a_launch), so it runs at the last extent
# both paths accept, 2^31 - 16, and the refusal at 2^31 is held through the host predicates (*_shape_ok with everything else satisfied,
# *_wanted on dense shapes) and through the ValueError of ups9_fwd / ups9_dgrad
# ======================================================================================================================
def _ups9_ref(x64, w64):
    return F.conv2d(F.interpolate(x64, scale_factor=2, mode='nearest'), w64, padding=1)


def test_ups9_at_the_reach(ops, arena, report, monkeypatch):
    bad = []
    N, Cin, Cout, H, W = 2, 20, 36, 16, 16
    w, b = rnd(Cout, Cin, 3, 3, seed=1, scale=1.0 / (3.0 * Cin ** 0.5)), rnd(Cout, seed=2)
    # forward: x in the arena
    x = place(ops, arena, rnd(N, Cin, H, W, seed=3), TOP16)
    up, ldu = ops.pack_weight(ops.ups9_u(w), 0)
    ref = _ups9_ref(d64(x), d64(w)) + d64(b)[None, :, None, None]
    poison(ref.numel())
    y, names, seen = launched_m(ops, monkeypatch, lambda: ops.ups9_fwd(x, up, ldu, Cout, bias=b))
    assert names == [CD._U9F] and [n for n, _ in seen] == [CD._U9F], (names, seen)
    check(report, bad, 'ups9_fwd E=2^31-16', relerr(y, ref), B_UPS9, kernel=names[0])
    wp, ld = ops.pack_weight(w, 0)
    with monkeypatch.context() as m:
        gates(ops, m, CONV_SPLITK_BLOCKS=0)
        poison(ref.numel())
        y, names, seen = launched_m(ops, m, lambda: ops.conv_forward(x, None, wp, ld, Cout, S(ops, 3, 1, 1, 1), bias=b))
    assert len(seen) == 1 and seen[0][0].startswith('conv_gemm_kernel<'), seen
    check(report, bad, 'ups9_fwd/conv_path E=2^31-16', relerr(y, ref), B_DIRECT, kernel=seen[0][0])
    sx, full = x.stride(0), 4 * H * W * Cout
    assert ops.ups9_fwd_shape_ok(N, Cin, Cout, H, W, sx, full, TOP16, ldu, up.numel() * 4, up.data_ptr())
    assert not ops.ups9_fwd_shape_ok(N, Cin, Cout, H, W, sx + 4, full, REACH, ldu, up.numel() * 4, up.data_ptr())
    # input gradient: dy in the arena, every tile
    dy = place(ops, arena, rnd(N, Cout, 2 * H, 2 * W, seed=4), TOP16)
    upd, ldd = ops.pack_weight(ops.ups9_u(w), 1)
    x64 = torch.zeros(N, Cin, H, W, dtype=torch.float64, requires_grad=True)
    ref = torch.autograd.grad(_ups9_ref(x64, d64(w)), x64, d64(dy))[0]
    for tile in (0, 1, 2):
        poison(ref.numel())
        dx, names, seen = launched_m(ops, monkeypatch, lambda: ops.ups9_dgrad(dy, upd, ldd, Cin, tile=tile))
        assert names == [CD._U9D[tile]] and [n for n, _ in seen] == [CD._U9D[tile]], (names, seen)
        check(report, bad, 'ups9_dgrad/tile%d E=2^31-16' % tile, relerr(dx, ref), B_UPS9, kernel=names[0])
    sd = dy.stride(0)
    assert ops.ups9_dgrad_shape_ok(N, Cin, Cout, H, W, sd, H * W * Cin, TOP16, ldd, upd.numel() * 4, 0, upd.data_ptr())
    assert not ops.ups9_dgrad_shape_ok(N, Cin, Cout, H, W, sd + 4, H * W * Cin, REACH, ldd, upd.numel() * 4, 0, upd.data_ptr())
    # dense shapes of 2 GiB: the shape-only gates say no before anything is packed
    assert not ops.ups9_fwd_wanted(1 << 15, 256, 64, 8, 8) and ops.ups9_fwd_wanted((1 << 15) - 1, 256, 64, 8, 8)
    assert not ops.ups9_dgrad_wanted(1 << 15, 64, 64, 8, 8) and ops.ups9_dgrad_wanted((1 << 15) - 1, 64, 64, 8, 8)
    assert not bad, bad


# ======================================================================================================================
# refusals: nothing is launched
# ======================================================================================================================
def test_two_gib_is_refused_without_a_launch(ops, arena):
    lib = ops._lib()
    c0 = lib.dp_launch_count()
    K, M, H, W = 32, 40, 16, 16
    big = view_of(arena, (2, K, H, W), REACH)              # torch.empty memory: nothing is computed
    small_in, small_out = torch.empty(2, K, H, W, device=D.DEV), torch.empty(2, M, H, W, device=D.DEV)
    wp, gw = torch.empty(9 * K * M, device=D.DEV), torch.empty(M, K, 3, 3, device=D.DEV)
    spec = S(ops)
    calls = {
        'conv_forward x1': lambda: ops.conv_forward(big, None, wp, M, M, spec),
        'conv_forward x2': lambda: ops.conv_forward(small_in, big, torch.empty(18 * K * M, device=D.DEV), M, M, spec),
        'conv_dgrad': lambda: ops.conv_dgrad(big, wp, M, M, spec, (H, W)),
        'conv_wgrad x': lambda: ops.conv_wgrad(small_out, big, None, gw, spec),
        'conv_wgrad dy': lambda: ops.conv_wgrad(big, small_out, None, torch.empty(K, M, 3, 3, device=D.DEV), spec),
        'ups9_fwd': lambda: ops.ups9_fwd(big, wp, M, M),
        'ups9_dgrad': lambda: ops.ups9_dgrad(big, wp, M, M),
    }
    # one matrix of 2^15 x 2^14 floats = 2^31 bytes per batch; the other operand is small
    a_tn, a_nn = arena.as_strided((2, 1 << 14, 1 << 15), (1 << 29, 1 << 15, 1), GUARD), arena.as_strided((2, 1 << 15, 1 << 14), (1 << 29, 1 << 14, 1), GUARD)
    b_k4, b_4k = torch.empty(2, 1 << 14, 4, device=D.DEV), torch.empty(2, 4, 1 << 14, device=D.DEV)
    calls.update({
        'bmm_tn a': lambda: ops.bmm_tn(a_tn, b_k4),
        'bmm_tn b': lambda: ops.bmm_tn(b_k4, a_tn),
        'bmm_nn a': lambda: ops.bmm_nn(a_nn, b_k4),
        'bmm_nn b': lambda: ops.bmm_nn(b_4k, a_tn),
        'bmm_nt a': lambda: ops.bmm_nt(a_nn, b_4k),
        'bmm_nt b': lambda: ops.bmm_nt(b_4k, a_nn),
    })
    for name, call in calls.items():
        with pytest.raises(ValueError, match='2 GiB'):
            call()
        assert lib.dp_launch_count() == c0, name
    torch.cuda.synchronize()


# ======================================================================================================================
# batch strides past 32 bits (in bytes): 64-bit base arithmetic in front of the descriptors
# ======================================================================================================================
BS = (1 << 30) + 64


def test_batch_strides_past_32_bits(ops, arena, report, monkeypatch):
    bad = []
    Z, M, K, Nn = 2, 40, 24, 50
    arena.fill_(SENTINEL)
    a = arena.as_strided((Z, M, K), (BS, K, 1), GUARD)
    b = arena.as_strided((Z, K, Nn), (BS, Nn, 1), GUARD + 4096)
    a.copy_(rnd(Z, M, K, seed=1))
    b.copy_(rnd(Z, K, Nn, seed=2))
    ref = 0.25 * torch.bmm(d64(a), d64(b))
    poison(Z * M * Nn)
    o, names, seen = launched_m(ops, monkeypatch, lambda: ops.bmm_nn(a, b, alpha=0.25))
    assert len(seen) == 1 and seen[0][0].startswith('conv_gemm_kernel<') and seen[0][1]['batches'] == Z and seen[0][1]['a_kc'] == 1, seen
    check(report, bad, 'bmm_nn batch_stride=2^30+64', relerr(o, ref), B_BMM, kernel=seen[0][0])

    N, heads, d, dv, H, W = 2, 2, 32, 24, 4, 8
    arena.fill_(SENTINEL)
    q = arena.as_strided((N, heads * d, H, W), (BS, H * W, W, 1), GUARD)
    q.copy_(rnd(N, heads * d, H, W, seed=3))
    k, v = rnd(N, heads * d, H, W, seed=4), rnd(N, heads * dv, H, W, seed=5)
    scale = float(d) ** -0.5
    ref = ref_attention(d64(q), d64(k), d64(v), heads, scale)
    poison(ref.numel())
    o, names, _ = launched_m(ops, monkeypatch, lambda: ops.attention_fwd(q, k, v, heads, scale))
    assert len(names) == 1 and names[0].startswith('attn_fwd_'), names
    check(report, bad, 'attention_fwd q_bs=2^30+64', relerr(o, ref), B_ATTN, kernel=names[0])
    # ... and with k and v behind the same stride (their slabs 4096 floats apart in both halves of the arena)
    kk = arena.as_strided((N, heads * d, H, W), (BS, H * W, W, 1), GUARD + 4096)
    vv = arena.as_strided((N, heads * dv, H, W), (BS, H * W, W, 1), GUARD + 8192)
    kk.copy_(k)
    vv.copy_(v)
    poison(ref.numel())
    o, names, _ = launched_m(ops, monkeypatch, lambda: ops.attention_fwd(q, kk, vv, heads, scale))
    check(report, bad, 'attention_fwd q_bs=k_bs=v_bs=2^30+64', relerr(o, ref), B_ATTN, kernel=names[0])
    assert not bad, bad
