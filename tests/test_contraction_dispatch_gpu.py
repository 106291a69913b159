"""Parity with fp64 on every dispatch branch of the contraction kernels.

The launchers of csrc/gemm.hip, winograd.hip, winograd2d.hip, winograd43.hip, wgrad2d.hip, attention.hip and ups9.hip choose a kernel, a
tile, a tail form or a reduction form from the shape, the alignment and the heuristics of ops.py (pick_tile, _prefer_tile96, _conv_ksplit,
_wino_splits, the gates of conv_wgrad).  Same four tables and the same closing test as tests/test_dispatch_parity_gpu.py:

  BRANCHES      every name the launch sites of the seven files can record, as the ring reports it: the stringised first argument of
                DP_LAUNCH, outer parentheses stripped -- so a launch site inside a launcher template reports the template's parameter
                names (`conv_gemm_kernel<BM, BN, false, true>`), and `name | condition` says which instantiation, or which runtime flag
                of the parameter block, is meant; each with the launcher condition that selects it;
  CASES         entry -> the cases that reach it (@case); an entry without a case FAILS;
  UNREACHED     entries no `ops` entry point can build, each with the ops code that says so; never launched from hand-filled blocks;
  LAUNCH_SITES  DP_LAUNCH( sites per file (tests/test_cpu.py counts them and checks every kernel name against BRANCHES).

Each case calls ONE ops entry point under `launched_m`, which also wraps ops._run: the name ops.py gives the profiler (_cg_name, _nt_name,
_wino_name, _wino2d_name, _wino43_name, _wgrad_wino_name, the wgrad_wino2d name, _UPS9_NAMES, _UPS9_FWD_NAME) must be the contraction name
in the ring after ONE normalisation (mirror_matches): a template parameter name in the ring (BM, BN, TAILS) stands for the mirror's value
-- which is how a case pins the tile -- and the mirror spells defaulted trailing template arguments the way rocprofv3 prints them
(`conv_wino_kernel<16, 2, 1>`, `nt_gemm_kernel<..., false>`).  ops.attention_fwd names its launch 'attn_fwd_fused_kernel' whatever the
schedule (tests/test_launch_parity_gpu.py's FLOOR holds that name); it is not one of the mirrors and is not compared.

Every output is compared with an fp64 evaluation of the same fp32 inputs on the CPU (max-abs error over the reference's max-abs), after a
poisoned allocation; entry points that take `out=` also write a channel slice of a wider buffer whose other elements must stay as they
were; split-K and folded forms run twice and must be bit-equal; forms documented to give the same bits (folded / reduction launch,
epilogue4 / scalar epilogue, taps_mc / taps) are held to that.  Bounds, from the older test of the same kernel:

  direct conv, nt_gemm, linear     2e-5    tests/test_kernels_gpu.py:134 (test_conv_forward_dgrad_wgrad), :155 (test_linear_fwd_dgrad_wgrad)
  bmm_tn / bmm_nn / bmm_nt         1e-5    tests/test_kernels_gpu.py:218 (test_bmm_variants)
  F(2, 3), F(2x2, 3x3) fwd, dgrad  3e-6    tests/test_kernels_gpu.py:1208, :1266
  the two Winograd weight grads    5e-6    tests/test_kernels_gpu.py:1302, :1364
  F(4, 3)                          1e-5    tests/test_kernels_gpu.py:1157
  attention                        1e-5    tests/test_kernels_gpu.py:300
  nine-product kernels             3e-6    tests/test_ups9_gpu.py:16, tests/test_ups9_fwd_wgrad_gpu.py:17 (TOL)
  packers, ups9_u                  0       data movement or a few exact fp32 additions / halvings in a fixed order: the fp32 CPU evaluation
                                           of the same expression.  dp_pack_weight_wino43 multiplies by 1/6, 1/12, 1/24 and adds three
                                           products, which hipcc may fuse: 3 roundings of 2^-24 against fp64, bound 2e-7.

Shapes: the smallest that select the branch and keep its edge -- a last row tile ragged by less than a 32-row block (100, 90, 40, 70 rows), a
K that ends inside a 16- / 8-channel chunk (40, 20, 24 channels), a concat boundary off the chunk for the straddle forms (24 + 16, 13 + 7,
21 + 19) and on it for the others, 72- or 54-pixel images so that the last 128-pixel tile is ragged and tiles span images, Wo % 4 != 0 and
an unguarded input for the non-x4 loaders, Ho * Wo % 4 != 0 for the scalar split-K epilogue.  Branches that need a big grid take the pixels
from many tiny images and very few channels."""
import importlib
import math

import pytest
import torch
import torch.nn.functional as F

import test_dispatch_parity_gpu as D
from helpers import edge_images, edge_tiles, ref_attention, ref_conv_dgrad, ref_conv_fwd, ref_conv_wgrad, relerr
from test_dispatch_parity_gpu import d64, launched, outside_intact, poison, rnd, wide

pytestmark = pytest.mark.gpu

# (attention.hip: the two sites are the two arms of AT_GO, which expands once per tiles-per-wavefront count 1 .. 5: ten names)
LAUNCH_SITES = {'gemm.hip': 22, 'winograd.hip': 7, 'winograd2d.hip': 8, 'winograd43.hip': 2, 'wgrad2d.hip': 6, 'attention.hip': 2,
                'ups9.hip': 5}

B_DIRECT, B_BMM, B_WINO, B_WINO_WGRAD, B_F43, B_ATTN, B_UPS9 = 2e-5, 1e-5, 3e-6, 5e-6, 1e-5, 1e-5, 3e-6

_TILES3 = ('BM = 128, BN = 128', 'BM = 64, BN = 128', 'BM = 64, BN = 64')
_FAST3 = ('BM = 128, TAILS = false', 'BM = 128, TAILS = true', 'BM = 96, TAILS = true')
_CGF_T, _CGF_F = 'conv_gemm_fast_kernel<BM, 128, TAILS, true>', 'conv_gemm_fast_kernel<BM, 128, TAILS, false>'
_CG = 'conv_gemm_kernel<BM, BN, %s, %s>'
_CG_FF, _CG_FT, _CG_TF, _CG_TT = _CG % ('false', 'false'), _CG % ('false', 'true'), _CG % ('true', 'false'), _CG % ('true', 'true')
_NT_F, _NT_T, _NT_M = 'nt_gemm_kernel<BM, BN, false>', 'nt_gemm_kernel<BM, BN, true>', 'nt_gemm_kernel<64, 64, false, true>'
_U9D = ('ups9_dgrad_kernel<128, 32, 8, 4, 1, 2>', 'ups9_dgrad_kernel<128, 64, 4, 2, 2, 3>', 'ups9_dgrad_kernel<128, 128, 4, 2, 2, 2>')
_U9F = 'ups9_fwd_kernel<64, 64, 8, 2>'

BRANCHES = [
    # ---- gemm.hip: dp_conv_gemm.  fast = conv_fast_ok (no a_kc, stride 1, no upsample, <= 32 taps); ops._prefer_tile96 sends every
    # such convolution with more than 64 output rows to tile 0 (128 rows) or 3 (96 rows, when they pad fewer rows)
    'conv_gemm_fast_kernel<128, 64, false, true>',   # tile 4 (ops.CONV_N64_TILES, off by default), fast, no tails, x4
    # TAILS = C % 16 != 0 or (X2 and c_split % 16 != 0); tile 3 is always instantiated with TAILS.  true / false: conv_fast_x4 --
    # (x_guard or pad_l == 0), Wo % 4 == 0, Ws >= 4 (one tap without padding: Ho * Wo % 4 == 0)
] + ['%s | %s' % (k, c) for k in (_CGF_T, _CGF_F) for c in _FAST3] + [
    _CGF_T + ' | ksplit > 1, reduction launch',      # ops._conv_ksplit: more than SPLITK_FOLD_MAX slices (or SPLITK_FOLD off)
    _CGF_T + ' | ksplit > 1, folded (tile_counters)',    # 2 .. SPLITK_FOLD_MAX slices: the last workgroup of a tile adds the slabs
    _CGF_T + ' | batches > 1',                       # bmm_tn on tile 0
    _CGF_T + ' | accumulate',
    # the general kernel: tile 1 / 2 (pick_tile; <= 64 rows), or tile 0 without conv_fast_ok (stride 2, fused upsample, a_kc)
] + ['%s | %s' % (k, c) for k in (_CG_FF, _CG_FT, _CG_TF) for c in _TILES3] + [
    # <.., A_KC, STRADDLE>: a_kc = the k-contiguous A operand of bmm_nn; straddle = X2 and c_split % 16 != 0
    _CG_TT,
    _CG_FF + ' | ksplit > 1, reduction launch',
    _CG_FF + ' | ksplit > 1, folded (tile_counters)',
    _CG_FF + ' | batches > 1',                       # bmm_tn on tile 1 / 2
    _CG_FF + ' | accumulate',
    _CG_TF + ' | batches > 1',                       # bmm_nn
    _CG_TF + ' | ksplit > 1',                        # linear_dgrad (one matrix product may split K)
    _CG_TF + ' | accumulate',
    'conv_splitk_epilogue4_kernel',                  # reduction launch, Ho * Wo % 4 == 0, NPIX % 4 == 0, 16-byte aligned ws / out / res
    'conv_splitk_epilogue_kernel',                   # reduction launch otherwise
    'conv_few_out_kernel',                           # conv_few_out_ok: <= 4 output rows, 3x3 / 1 / 1, one source, bias only
    # ---- gemm.hip: dp_nt_gemm.  fast = nt_fast_ok (not batched / merged / col_bias, stride 1, Wo | 16 or 16 | Wo, Ho * Wo % 16 == 0,
    # P % 16 == 0) on tile 0 (NW = 4: 128 x 128) or 3 (NW = 3: 96 x 96, ops.conv_wgrad when it pads clearly less); TWO = X2
    'nt_gemm_fast_kernel<3, true>', 'nt_gemm_fast_kernel<3, false>', 'nt_gemm_fast_kernel<4, true>', 'nt_gemm_fast_kernel<4, false>',
    # <BM, BN, STRADDLE>: conv_wgrad takes tile 0 (Cout > 64) or 1; tile 2 comes from pick_tile (bmm_nt, linear_forward);
    # straddle = X2 and c_split % BN != 0
] + ['%s | %s' % (k, c) for k in (_NT_F, _NT_T) for c in _TILES3] + [
    _NT_F + ' | batched',                            # bmm_nt
    _NT_F + ' | col_bias',                           # linear_forward with a bias
    _NT_F + ' | splits > 1',                         # pixel slices + a reduction launch
    _NT_M + ' | merge = 1',                          # few input channels (Cin * taps <= 64): taps folded into the columns
    _NT_M + ' | merge = 3',                          # few output channels: the operands swap roles, taps mirrored
    'splitk_reduce_kernel',                          # merged weight gradients and linear_forward's split
    'splitk_reduce_taps_kernel',                     # tap-major partials, ntaps not 9 or 4 (or DP_NO_REDUCE_MC)
    'splitk_reduce_taps_mc_kernel<9>', 'splitk_reduce_taps_mc_kernel<4>',
    'pack_weight_kernel',
    # ---- winograd.hip: dp_conv_wino <BK, WR>.  BK = 16 when C and c_split are multiples of 16, else 8; WR = 1 (32-row tiles, 256
    # pixels) when Wo > 128 or 32-row tiles pad fewer rows than 64-row ones, else 2
    'conv_wino_kernel<16, 1>', 'conv_wino_kernel<8, 1>', 'conv_wino_kernel<16, 2>', 'conv_wino_kernel<8, 2>',
    'conv_wino_kernel<16, 2> | ksplit > 1',          # ops._wino_splits: a grid below WINO_MIN_TILES
    'pack_weight_wino_kernel',
    'wgrad_wino_kernel<3, 3>',                       # tile 3: 96 x 96 covers [Cout x Cin] with < 0.9 of the 64 x 64 padding
    'wgrad_wino_kernel<2, 2>',
    # ---- winograd2d.hip: dp_conv_wino2d.  tail = 1 <= M % 64 <= 32; variant 1 (<4, 3>) = unsplit and more than 512 workgroups
    'conv_wino2d_m32_kernel<4, 5, false>',           # Wo <= 64, unsplit, > 512 workgroups, M <= 96 and tail
    'conv_wino2d_tail_kernel<4, 2, true>', 'conv_wino2d_kernel<4, 2, true>',         # Wo > 64
    'conv_wino2d_tail_kernel<4, 3, false>', 'conv_wino2d_kernel<4, 3, false>',       # Wo <= 64, variant 1
    'conv_wino2d_tail_kernel<8, 2, false>', 'conv_wino2d_kernel<8, 2, false>',       # Wo <= 64, variant 0
    'conv_wino2d_kernel<8, 2, false> | ksplit > 1',
    'pack_weight_wino2d_kernel',
    # ---- winograd43.hip
    'conv_wino43_kernel', 'conv_wino43_kernel | ksplit > 1', 'pack_weight_wino43_kernel',
    # ---- wgrad2d.hip: <LW> = log2(Wo) for Wo = 32 / 16 / 8; tail as above, on Cout
    'wgrad_wino2d_tail_kernel<5>', 'wgrad_wino2d_tail_kernel<4>', 'wgrad_wino2d_tail_kernel<3>',
    'wgrad_wino2d_kernel<5>', 'wgrad_wino2d_kernel<4>', 'wgrad_wino2d_kernel<3>',
    # ---- attention.hip: <NT> = ceil(ceil(max(d, dv) / 32) / 4); pipe = variant 2, or variant 0 and NT <= 2
] + ['attn_fwd_%s_kernel<%d>' % (k, nt) for k in ('pipe', 'fused') for nt in (1, 2, 3, 4, 5)] + [
    # ---- ups9.hip: dp_ups9_params.tile 0 / 1 / 2 (ops.ups9_tile: the widest with UPS9_MIN_BLOCKS workgroups)
] + list(_U9D) + [k + ' | accumulate' for k in _U9D] + [
    _U9F, _U9F + ' | bias', 'ups9_u_kernel',
]

UNREACHED = {
    _CG_TT: 'a_kc is set by ops._bmm_conv_gemm alone (bmm_nn, linear_dgrad), which passes x2 = None to _conv_gemm_params: no second '
            'concat source, so the launcher never computes straddle for a k-contiguous A operand',
    _NT_T + ' | BM = 64, BN = 64': 'ops.conv_wgrad -- the only caller of dp_nt_gemm with a second source -- takes tile 0, 1 or 3 '
                                   '(`tile = 0 if Cout > 64 else 1`); tile 2 comes from pick_tile in bmm_nt / linear_forward, whose '
                                   '_nt_gemm_params get x2 = None, and from the merged form, which dp_nt_gemm refuses with X2',
}

KNOWN = {e.split(' | ')[0] for e in BRANCHES}
CASES = {}


def case(*entries):
    def deco(fn):
        for e in entries:
            assert e in BRANCHES, e
            CASES.setdefault(e, []).append(fn)
        return fn
    return deco


@pytest.fixture(scope='module')
def ops():
    importlib.import_module('diff-pruning_amd')
    o = importlib.import_module('diff-pruning_amd.ops')
    o._lib()
    return o


# ======================================================================================================================
# the comparison and the name mirror
# ======================================================================================================================
def exceeding(res):
    """The figures of a case result (its float values other than `bound`) that are not within the bound; NaN is not within."""
    return {k: v for k, v in res.items() if isinstance(v, float) and k != 'bound' and not v <= res['bound']}


def split_name(s):
    base, _, args = s.partition('<')
    return base, ([a.strip() for a in args[:-1].split(',')] if args else [])


MIRRORED = {'conv_gemm_fast_kernel', 'conv_gemm_kernel', 'conv_few_out_kernel', 'nt_gemm_fast_kernel', 'nt_gemm_kernel', 'conv_wino_kernel',
            'conv_wino2d_kernel', 'conv_wino2d_tail_kernel', 'conv_wino2d_m32_kernel', 'conv_wino43_kernel', 'wgrad_wino_kernel',
            'wgrad_wino2d_kernel', 'wgrad_wino2d_tail_kernel', 'ups9_dgrad_kernel', 'ups9_fwd_kernel'}
_PARAMETER = ('BM', 'BN', 'TAILS')                       # template parameters of the launcher templates of gemm.hip
_DEFAULTED = {('nt_gemm_kernel', 3): ['false'], ('conv_wino_kernel', 2): ['1']}      # MERGE = false, TM = 1


def mirror_matches(ring, mirror):
    """The one normalisation between the launch site's expression and ops._run's name (module docstring)."""
    (rb, ra), (mb, ma) = split_name(ring), split_name(mirror)
    if rb != mb:
        return False
    tail = _DEFAULTED.get((rb, len(ra)), [])
    if len(ma) == len(ra) + len(tail) and tail:
        if ma[len(ra):] != tail:
            return False
        ma = ma[:len(ra)]
    return len(ma) == len(ra) and all(r == m or r in _PARAMETER for r, m in zip(ra, ma))


_BLOCK = ('ksplit', 'tile_counters', 'splits', 'batches', 'batched', 'accumulate', 'merge', 'col_bias', 'tile', 'bias', 'a_kc')


def launched_m(ops, mp, fn):
    """launched(), and what the call gave ops._run: [(name, {field: value} of the parameter block its closure holds)].  The mirror
    names must be the contraction names of the ring, in order."""
    seen = []
    real = ops._run

    def run(call, name, *a, **k):
        blk = {}
        for cell in call.__closure__ or ():
            p = cell.cell_contents
            have = {f[0] for f in getattr(type(p), '_fields_', ())}
            if have:
                blk = {f: getattr(p, f) for f in _BLOCK if f in have}
        seen.append((name, blk))
        return real(call, name, *a, **k)
    with mp.context() as m:
        m.setattr(ops, '_run', run)
        r, names = launched(ops, fn)
    ring = [n for n in names if split_name(n)[0] in MIRRORED]
    mirror = [(n, b) for n, b in seen if split_name(n)[0] in MIRRORED]
    assert len(ring) == len(mirror) and all(mirror_matches(a, b[0]) for a, b in zip(ring, mirror)), \
        ('ops._run names a kernel the library did not launch', ring, [n for n, _ in mirror])
    return r, names, seen


def gates(ops, mp, **kw):
    for k, v in kw.items():
        assert hasattr(ops, k), k
        mp.setattr(ops, k, v)


def guarded_act(ops, t):
    """A contiguous copy with ops.ACT_GUARD readable floats in front of it (what the engines allocate: x_guard = 1)."""
    g = ops.empty_act(tuple(t.shape), t.device).copy_(t)
    assert g.storage_offset() >= 1
    return g


def nan_like(*shape):
    return torch.full(shape, float('nan'), device=D.DEV)


# ======================================================================================================================
# dp_conv_gemm and the Winograd forms through conv_forward / conv_dgrad
# ======================================================================================================================
def run_conv(ops, mp, kind, N, K1, K2, M, H, W, spec, *, want, guarded=True, epi='full', acc=True, blk=None, has=(), wino=None,
             in_hw=None, twice=False, bound=B_DIRECT, keep=None, seed=1):
    """kind 'fwd': conv_forward of cat(x [N, K1, H, W], x2 [N, K2, H, W]) to M output channels; 'dgrad': conv_dgrad of dy [N, K1, H, W]
    (K1 = the convolution's OUTPUT channels) to M input channels of size in_hw.  Two launches: a fresh output with every epilogue
    operand, and a channel slice of a wider buffer (accumulate, alpha = 0.5).  want: the mirror name of both; blk: a predicate on
    the parameter block of the first; has: ring names the first must hold; keep: a dict that receives the two outputs."""
    fwd = kind == 'fwd'
    act = (lambda t: guarded_act(ops, t)) if guarded else (lambda t: t)
    xa = act(rnd(N, K1, H, W, seed=seed))
    xb = act(rnd(N, K2, H, W, seed=seed + 1)) if K2 else None
    assert guarded or xa.storage_offset() == 0
    K = K1 + K2
    w = rnd(*((M, K) if fwd else (K, M)), spec.kh, spec.kw, seed=seed + 2, scale=1.0 / math.sqrt(K * spec.kh * spec.kw))
    wp, ld = ops.pack_weight(w, 0 if fwd else 1)
    kw = {}
    if wino == '1d':
        kw['wino'] = ops.pack_weight_wino(w, 0 if fwd else 1)
    elif wino == '2d':
        kw['wino'] = ('2d',) + tuple(ops.pack_weight_wino2d(w, 0 if fwd else 1))
    elif wino == '43':
        kw['wino43'] = ops.pack_weight_wino43(w)
    x64 = d64(xa) if xb is None else torch.cat([d64(xa), d64(xb)], 1)
    if fwd:
        Ho, Wo = spec.out_hw(H, W)
        plain = ref_conv_fwd(x64, d64(w), spec)
    else:
        Ho, Wo = in_hw or (H, W)
        plain = ref_conv_dgrad(x64, d64(w), spec, (Ho, Wo))
    assert tuple(plain.shape) == (N, M, Ho, Wo)
    b, tadd, res = rnd(M, seed=seed + 3), rnd(N, M, seed=seed + 4), rnd(N, M, Ho, Wo, seed=seed + 5)
    if fwd and epi == 'full':
        ref = (plain + d64(b)[None, :, None, None] + d64(tadd)[:, :, None, None] + d64(res)) * 0.7
        call_a = lambda: ops.conv_forward(xa, xb, wp, ld, M, spec, bias=b, tadd=tadd, res=res, post_scale=0.7, **kw)
    elif fwd:
        ref = plain + d64(b)[None, :, None, None]
        call_a = lambda: ops.conv_forward(xa, xb, wp, ld, M, spec, bias=b, **kw)
    else:
        ref = plain
        call_a = lambda: ops.conv_dgrad(xa, wp, ld, M, spec, (Ho, Wo), **kw)
    poison(N * M * Ho * Wo)
    y, names, seen = launched_m(ops, mp, call_a)
    assert [n for n, _ in seen] == [want], (seen, want)
    assert blk is None or blk(seen[0][1]), seen
    assert all(h in names for h in has), (names, has)
    out = [dict(names=names, shape=(kind, N, K1, K2, M, H, W), mirror=want, out=relerr(y, ref), bound=bound)]
    if twice:
        poison(N * M * Ho * Wo)
        assert torch.equal(call_a(), y), 'two runs of a split-K launch differ'
    view, big = wide(N, M, Ho, Wo, seed + 6)
    before = big.clone()
    if fwd:
        call_b = lambda: ops.conv_forward(xa, xb, wp, ld, M, spec, out=view, accumulate=acc, alpha=0.5, bias=None if acc else b, **kw)
    else:
        call_b = lambda: ops.conv_dgrad(xa, wp, ld, M, spec, (Ho, Wo), out=view, accumulate=acc, alpha=0.5, **kw)
    _, names_b, seen_b = launched_m(ops, mp, call_b)
    assert [n for n, _ in seen_b] == [want] and seen_b[0][1].get('accumulate', 0) == int(acc), (seen_b, want)
    ref_b = 0.5 * plain + (d64(before[:, 2:2 + M]) if acc else (d64(b)[None, :, None, None] if fwd else 0))
    assert outside_intact(big, before, 2, M), 'a launch wrote outside its channel slice'
    out.append(dict(names=names_b, shape=(kind, N, K1, K2, M, H, W), mirror=want, into_slice=True, accumulate=acc,
                    out=relerr(view, ref_b), bound=bound))
    if keep is not None:
        keep['a'], keep['b'] = y.clone(), view.clone()
    return out


def S(ops, k=3, stride=1, pad=1, ups=0):
    return ops.ConvSpec(k, stride, pad, ups)


# 230 images of 9 x 8 pixels: 16560 pixels = 129 tiles of 128 and 48 pixels, every tile spans two or three images; 130 tiles of 128 rows
# and at most 27 K iterations keep ops._conv_ksplit at one slice.  310 images of 9 x 6: Wo % 4 != 0
BIG_N, BIG_H, BIG_W = 230, 9, 8
assert len(edge_images(BIG_N, BIG_H * BIG_W)) == 3 and (BIG_N * BIG_H * BIG_W) % 128 == 48
assert edge_tiles(100, 32)[-4:] == [96, 97, 98, 99] and len(edge_tiles(90, 32)) == 32 + 26       # the ragged last 32-row blocks of 100 and 90 rows


def _reg_conv_fast():
    fast = 'conv_gemm_fast_kernel<%s, %s, %s>'
    shapes = {_FAST3[0]: ('128, 128', 'false', 32, 0, 100),         # 100 rows: the last 32-row block of the tile holds 4
              _FAST3[1]: ('128, 128', 'true', 24, 16, 100),         # 40 channels, boundary inside the second 16-channel chunk
              _FAST3[2]: ('96, 128', 'true', 40, 0, 90)}            # 90 rows on the 96-row tile, K ends inside a chunk
    for cond, (tile, tails, K1, K2, M) in shapes.items():
        @case(_CGF_T + ' | ' + cond, *([_CGF_T + ' | accumulate'] if tails == 'false' else []))
        def x4(ops, mp, tile=tile, tails=tails, K1=K1, K2=K2, M=M):
            yield from run_conv(ops, mp, 'fwd', BIG_N, K1, K2, M, BIG_H, BIG_W, S(ops), want=fast % (tile, tails, 'true'),
                                blk=lambda b: b['ksplit'] <= 1, has=[_CGF_T])
            yield from run_conv(ops, mp, 'dgrad', BIG_N, K1 + K2, 0, M, BIG_H, BIG_W, S(ops),
                                want=fast % (tile, 'true' if (K1 + K2) % 16 else 'false', 'true'), has=[_CGF_T])

        @case(_CGF_F + ' | ' + cond)
        def x1(ops, mp, tile=tile, tails=tails, K1=K1, K2=K2, M=M):
            # an input without a readable float in front of it (pad_l = 1), and Wo = 6
            yield from run_conv(ops, mp, 'fwd', BIG_N, K1, K2, M, BIG_H, BIG_W, S(ops), want=fast % (tile, tails, 'false'), guarded=False,
                                blk=lambda b: b['ksplit'] <= 1, has=[_CGF_F])
            yield from run_conv(ops, mp, 'fwd', 310, K1, K2, M, 9, 6, S(ops), want=fast % (tile, tails, 'false'), has=[_CGF_F])


_reg_conv_fast()


@case('conv_gemm_fast_kernel<128, 64, false, true>')
def conv_fast_n64(ops, mp):
    gates(ops, mp, CONV_N64_TILES=(1, 1 << 30))
    yield from run_conv(ops, mp, 'fwd', BIG_N, 32, 0, 100, BIG_H, BIG_W, S(ops), want='conv_gemm_fast_kernel<128, 64, false, true>')


def _split_pair(ops, mp, N, K, M, H, W, spec, want, ring, folded_first):
    """One split-K shape in both reduction forms: each within the fp64 bound, run twice, and bit-equal to the other."""
    keep = {}
    for fold in ((True, False) if folded_first else (False, True)):
        with mp.context() as m:
            gates(ops, m, SPLITK_FOLD=fold, SPLITK_FOLD_MAX=1 << 30 if fold else ops.SPLITK_FOLD_MAX)
            k = keep.setdefault(fold, {})
            yield from run_conv(ops, m, 'fwd', N, K, 0, M, H, W, spec, want=want, twice=True, keep=k, has=[ring],
                                blk=lambda b, fold=fold: b['ksplit'] > 1 and bool(b['tile_counters']) == fold)
    assert torch.equal(keep[True]['a'], keep[False]['a']) and torch.equal(keep[True]['b'], keep[False]['b']), \
        'the folded split-K reduction and the reduction launch give different bits'


def _epilogue_pair(ops, mp):
    """3 images of 8 x 8: two tiles, 36 K iterations -> 18 slices by ops._conv_ksplit's own rule, more than SPLITK_FOLD_MAX: the
    reduction launch, four pixels a thread; then the scalar epilogue on the same partials (DP_NO_EPI4, read per call): the same bits."""
    assert ops.SPLITK_FOLD and ops.SPLITK_FOLD_MAX == 4
    keep, k2 = {}, {}
    want = 'conv_gemm_fast_kernel<128, 128, false, true>'
    for r in run_conv(ops, mp, 'fwd', 3, 64, 0, 100, 8, 8, S(ops), want=want, twice=True, keep=keep,
                      blk=lambda b: b['ksplit'] == 18 and not b['tile_counters'], has=[_CGF_T, 'conv_splitk_epilogue4_kernel']):
        assert 'conv_splitk_epilogue4_kernel' in r['names'], r
        yield 4, r
    with mp.context() as m:
        m.setenv('DP_NO_EPI4', '1')
        for r in run_conv(ops, m, 'fwd', 3, 64, 0, 100, 8, 8, S(ops), want=want, keep=k2, has=['conv_splitk_epilogue_kernel']):
            assert 'conv_splitk_epilogue_kernel' in r['names'], r
            yield 1, r
    assert torch.equal(keep['a'], k2['a']) and torch.equal(keep['b'], k2['b']), 'epilogue4 and the scalar epilogue give different bits'


@case(_CGF_T + ' | ksplit > 1, reduction launch', 'conv_splitk_epilogue4_kernel')
def conv_fast_splitk_launch(ops, mp):
    yield from (r for form, r in _epilogue_pair(ops, mp) if form == 4)


@case('conv_splitk_epilogue_kernel')
def conv_splitk_scalar_epilogue(ops, mp):
    """5 x 5 images: Ho * Wo % 4 != 0 (and 125 pixels: NPIX % 4 != 0); and the scalar form against epilogue4 on a shape that takes both."""
    res = run_conv(ops, mp, 'fwd', 5, 64, 0, 100, 5, 5, S(ops), want='conv_gemm_fast_kernel<128, 128, false, false>', twice=True,
                   blk=lambda b: b['ksplit'] > 1 and not b['tile_counters'], has=['conv_splitk_epilogue_kernel'])
    assert all('conv_splitk_epilogue_kernel' in r['names'] for r in res)
    yield from res
    yield from (r for form, r in _epilogue_pair(ops, mp) if form == 1)


@case(_CGF_T + ' | ksplit > 1, folded (tile_counters)')
def conv_fast_splitk_folded(ops, mp):
    """71 images of 9 x 8: 40 tiles, 18 K iterations -> 2 slices by the default rule, folded by default."""
    res = run_conv(ops, mp, 'fwd', 71, 32, 0, 100, 9, 8, S(ops), want='conv_gemm_fast_kernel<128, 128, false, true>', twice=True,
                   blk=lambda b: b['ksplit'] == 2 and b['tile_counters'], has=[_CGF_T])
    assert all(not any(n.startswith('conv_splitk') for n in r['names']) for r in res)
    yield from res
    yield from _split_pair(ops, mp, 71, 32, 100, 9, 8, S(ops), 'conv_gemm_fast_kernel<128, 128, false, true>', _CGF_T, True)
    yield from _split_pair(ops, mp, 3, 72, 90, 8, 8, S(ops), 'conv_gemm_fast_kernel<96, 128, true, true>', _CGF_T, True)


# the general kernel.  Tile 0 without the fast loader: a stride-2 convolution whose grid makes pick_tile take it -- 1540 images of
# 8 x 8 -> 4 x 4: 24640 output pixels = 192 tiles and a half
def _reg_conv_general():
    name = 'conv_gemm_kernel<%s, %s, %s>'
    for kernel, straddle, (k1a, k2a), (k1b, k2b), (k1c, k2c) in ((_CG_FF, 'false', (8, 0), (20, 0), (24, 0)),
                                                               (_CG_FT, 'true', (5, 3), (13, 7), (21, 19))):
        @case(kernel + ' | ' + _TILES3[0], *([_CG_FF + ' | accumulate'] if straddle == 'false' else []))
        def t0(ops, mp, kernel=kernel, straddle=straddle, K1=k1a, K2=k2a):
            yield from run_conv(ops, mp, 'fwd', 1540, K1, K2, 100, 8, 8, S(ops, 3, 2, 1), want=name % ('128, 128', 'false', straddle),
                                blk=lambda b: b['ksplit'] <= 1, has=[kernel])

        @case(kernel + ' | ' + _TILES3[1])
        def t1(ops, mp, kernel=kernel, straddle=straddle, K1=k1b, K2=k2b):
            yield from run_conv(ops, mp, 'fwd', BIG_N, K1, K2, 40, BIG_H, BIG_W, S(ops), want=name % ('64, 128', 'false', straddle),
                                has=[kernel])

        @case(kernel + ' | ' + _TILES3[2])
        def t2(ops, mp, kernel=kernel, straddle=straddle, K1=k1c, K2=k2c):
            yield from run_conv(ops, mp, 'fwd', 3, K1, K2, 40, 16, 16, S(ops, 3, 2, 0), want=name % ('64, 64', 'false', straddle),
                                has=[kernel])                       # stride 2, the asymmetric (0, 1, 0, 1) pad
            yield from run_conv(ops, mp, 'fwd', 3, K1, K2, 40, 5, 7, S(ops, 3, 1, 1, 1), want=name % ('64, 64', 'false', straddle),
                                has=[kernel])                       # the fused nearest x2 upsample
            if not K2:
                yield from run_conv(ops, mp, 'dgrad', 3, 40, 0, K1, 8, 8, S(ops, 3, 2, 1), in_hw=(16, 16),
                                    want=name % ('64, 64', 'false', 'false'), has=[kernel])     # sden = 2: the zero-inserted form


_reg_conv_general()


@case(_CG_FF + ' | ksplit > 1, reduction launch')
def conv_general_splitk_launch(ops, mp):
    yield from run_conv(ops, mp, 'fwd', 3, 64, 0, 100, 16, 16, S(ops, 3, 2, 1), want='conv_gemm_kernel<128, 128, false, false>', twice=True,
                        blk=lambda b: b['ksplit'] > ops.SPLITK_FOLD_MAX and not b['tile_counters'],
                        has=[_CG_FF, 'conv_splitk_epilogue4_kernel'])
    # exactly 64 rows: the 64 x 128 tile
    yield from run_conv(ops, mp, 'fwd', 3, 64, 0, 64, 16, 16, S(ops, 3, 2, 1), want='conv_gemm_kernel<64, 128, false, false>', twice=True,
                        blk=lambda b: b['ksplit'] > ops.SPLITK_FOLD_MAX and not b['tile_counters'], has=[_CG_FF])


@case(_CG_FF + ' | ksplit > 1, folded (tile_counters)')
def conv_general_splitk_folded(ops, mp):
    yield from _split_pair(ops, mp, 71, 32, 100, 18, 16, S(ops, 3, 2, 1), 'conv_gemm_kernel<128, 128, false, false>', _CG_FF, True)
    yield from _split_pair(ops, mp, 3, 40, 64, 16, 16, S(ops, 3, 2, 1), 'conv_gemm_kernel<64, 128, false, false>', _CG_FF, False)


@case('conv_few_out_kernel')
def conv_few_out(ops, mp):
    """12 x 12 and 20 x 17 images in 16 x 16 pixel tiles, 20 channels in chunks of 16, 3 and 4 output rows."""
    for N, K, M, H, W in ((3, 20, 3, 12, 12), (2, 37, 4, 20, 17)):
        yield from run_conv(ops, mp, 'fwd', N, K, 0, M, H, W, S(ops), want='conv_few_out_kernel', epi='bias', acc=False,
                            has=['conv_few_out_kernel'])


@case(_CG_FF + ' | ' + _TILES3[2])
def conv_dgrad_s2(ops, mp):
    """conv_dgrad_s2: four stride-1 class convolutions over dy + the interleave pass (pad 0 = the asymmetric pad, and pad 1)."""
    for pad, N, Cout, Cin, Ho, Wo in ((0, 3, 24, 40, 5, 7), (1, 2, 37, 19, 6, 6)):
        spec = S(ops, 3, 2, pad)
        dy, w, add = rnd(N, Cout, Ho, Wo, seed=1), rnd(Cout, Cin, 3, 3, seed=2, scale=1.0 / math.sqrt(9 * Cout)), rnd(N, Cin, 2 * Ho, 2 * Wo, seed=3)
        packs = [ops.pack_weight_s2(w, ph, pw, pad) for ph in (0, 1) for pw in (0, 1)]
        poison(N * Cin * 4 * Ho * Wo)
        dx, names, seen = launched_m(ops, mp, lambda: ops.conv_dgrad_s2(dy, packs, Cin, spec, (2 * Ho, 2 * Wo), add=add))
        assert names == [_CG_FF] * 4 + ['interleave2x2_kernel'] and [n for n, _ in seen] == ['conv_gemm_kernel<64, 64, false, false>'] * 4
        ref = ref_conv_dgrad(d64(dy), d64(w), spec, (2 * Ho, 2 * Wo)) + d64(add)
        yield dict(names=names, shape=(N, Cout, Cin, Ho, Wo), pad=pad, out=relerr(dx, ref), bound=B_DIRECT)


# ======================================================================================================================
# bmm_tn / bmm_nn / bmm_nt, linear
# ======================================================================================================================
def run_bmm(ops, mp, which, Z, M, K, Nn, *, want, blk=None, has=(), col_bias=False, bound=B_BMM):
    """tn: a [Z, K, M]; nn / nt: a [Z, M, K]; b [Z, K, Nn] (nt: [Z, Nn, K]).  A fresh output (alpha = 0.25), then a row slice of a wider
    [Z, M + 5, Nn] buffer (tn / nn: accumulate)."""
    a = rnd(Z, K, M, seed=1) if which == 'tn' else rnd(Z, M, K, seed=1)
    b = rnd(Z, Nn, K, seed=2) if which == 'nt' else rnd(Z, K, Nn, seed=2)
    cb = rnd(Nn, seed=3) if col_bias else None
    a64 = d64(a).transpose(1, 2) if which == 'tn' else d64(a)
    b64 = d64(b).transpose(1, 2) if which == 'nt' else d64(b)
    plain = torch.bmm(a64, b64)
    fn = getattr(ops, 'bmm_' + which)
    extra = dict(col_bias=cb) if which == 'nt' else {}
    poison(Z * M * Nn)
    o, names, seen = launched_m(ops, mp, lambda: fn(a, b, alpha=0.25, **extra))
    assert [n for n, _ in seen] == [want] and (blk is None or blk(seen[0][1])) and all(h in names for h in has), (seen, names, want)
    out = [dict(names=names, shape=(which, Z, M, K, Nn), mirror=want, out=relerr(o, 0.25 * plain + (d64(cb) if col_bias else 0)), bound=bound)]
    big = rnd(Z, M + 5, Nn, seed=4)
    view, before = big[:, 2:2 + M], big.clone()
    acc = which != 'nt'
    _, names_b, seen_b = launched_m(ops, mp, lambda: fn(a, b, alpha=0.5, out=view, **(dict(accumulate=True) if acc else extra)))
    assert [n for n, _ in seen_b] == [want], (seen_b, want)
    assert outside_intact(big, before, 2, M)
    ref_b = 0.5 * plain + (d64(before[:, 2:2 + M]) if acc else (d64(cb) if col_bias else 0))
    out.append(dict(names=names_b, shape=(which, Z, M, K, Nn), mirror=want, into_slice=True, out=relerr(view, ref_b), bound=bound))
    return out


@case(_CGF_T + ' | batches > 1')
def bmm_tn_fast(ops, mp):
    """200 products of 100 x 120 (K = 20): 200 tiles of 128 x 128 are one round, the smaller tiles would need two and four."""
    assert ops.pick_tile(100, 120, 200) == 0
    yield from run_bmm(ops, mp, 'tn', 200, 100, 20, 120, want='conv_gemm_fast_kernel<128, 128, true, true>',
                       blk=lambda b: b['batches'] == 200 and b['ksplit'] <= 1, has=[_CGF_T])


@case(_CG_FF + ' | batches > 1')
def bmm_tn_general(ops, mp):
    assert ops.pick_tile(52, 120, 200) == 1 and ops.pick_tile(52, 37, 3) == 2
    yield from run_bmm(ops, mp, 'tn', 200, 52, 20, 120, want='conv_gemm_kernel<64, 128, false, false>', has=[_CG_FF],
                       blk=lambda b: b['batches'] == 200)
    yield from run_bmm(ops, mp, 'tn', 3, 52, 41, 37, want='conv_gemm_kernel<64, 64, false, false>', has=[_CG_FF])


def _reg_bmm_nn():
    for cond, tile, (Z, M, K, Nn) in zip(_TILES3, ('128, 128', '64, 128', '64, 64'), ((200, 100, 20, 120), (200, 50, 20, 120), (3, 50, 41, 37))):
        @case(_CG_TF + ' | ' + cond, *([_CG_TF + ' | batches > 1', _CG_TF + ' | accumulate'] if Z == 3 else []))
        def c(ops, mp, tile=tile, Z=Z, M=M, K=K, Nn=Nn):
            yield from run_bmm(ops, mp, 'nn', Z, M, K, Nn, want='conv_gemm_kernel<%s, true, false>' % tile, has=[_CG_TF],
                               blk=lambda b: b['batches'] == Z and b['a_kc'] == 1)


_reg_bmm_nn()


@case(_NT_F + ' | batched', _NT_F + ' | ' + _TILES3[2])
def bmm_nt(ops, mp):
    yield from run_bmm(ops, mp, 'nt', 3, 50, 41, 37, want='nt_gemm_kernel<64, 64, false, false>', has=[_NT_F],
                       blk=lambda b: b['batched'] == 1 and b['batches'] == 3)
    yield from run_bmm(ops, mp, 'nt', 200, 100, 20, 120, want='nt_gemm_kernel<128, 128, false, false>', has=[_NT_F])
    yield from run_bmm(ops, mp, 'nt', 200, 50, 20, 120, want='nt_gemm_kernel<64, 128, false, false>', has=[_NT_F])


def run_linear(ops, mp, N, Ci, Co):
    """linear_forward (+ bias), linear_dgrad (fresh, and accumulate into a given buffer), linear_wgrad (accumulate, alpha)."""
    x, w, b, dy = rnd(N, Ci, seed=1), rnd(Co, Ci, seed=2, scale=Ci ** -0.5), rnd(Co, seed=3), rnd(N, Co, seed=4)
    xd, wd, bd, dyd = d64(x), d64(w), d64(b), d64(dy)
    poison(N * Co)
    y, names, seen = launched_m(ops, mp, lambda: ops.linear_forward(x, w, b))
    yield 'fwd', dict(names=names, shape=(N, Ci, Co), out=relerr(y, xd @ wd.t() + bd), bound=B_DIRECT), seen
    poison(N * Ci)
    dx, names, seen = launched_m(ops, mp, lambda: ops.linear_dgrad(dy, w))
    yield 'dgrad', dict(names=names, shape=(N, Ci, Co), out=relerr(dx, dyd @ wd), bound=B_DIRECT), seen
    acc = rnd(N, Ci, seed=5)
    a0 = acc.clone()
    _, names, seen = launched_m(ops, mp, lambda: ops.linear_dgrad(dy, w, out=acc, accumulate=True))
    yield 'dgrad_acc', dict(names=names, shape=(N, Ci, Co), out=relerr(acc, d64(a0) + dyd @ wd), bound=B_DIRECT), seen
    gw = rnd(Co, Ci, seed=6)
    g0 = gw.clone()
    _, names, seen = launched_m(ops, mp, lambda: ops.linear_wgrad(dy, x, gw, alpha=0.5, accumulate=True))
    yield 'wgrad', dict(names=names, shape=(N, Ci, Co), out=relerr(gw, d64(g0) + 0.5 * dyd.t() @ xd), bound=B_DIRECT), seen


def _linear_forward(ops, mp, shapes):
    for N, Ci, Co, split in shapes:
        for what, res, seen in run_linear(ops, mp, N, Ci, Co):
            if what == 'fwd':
                assert seen[0][1]['col_bias'] and (seen[0][1]['splits'] > 1) == split, seen
                assert res['names'] == [_NT_F] + (['splitk_reduce_kernel'] if split else []), res
                if split:
                    x, w, b = rnd(N, Ci, seed=1), rnd(Co, Ci, seed=2, scale=Ci ** -0.5), rnd(Co, seed=3)
                    assert torch.equal(ops.linear_forward(x, w, b), ops.linear_forward(x, w, b)), 'two runs of a split product differ'
                yield res


@case(_NT_F + ' | col_bias')
def linear_forward(ops, mp):
    """K = 100 and 37: one slice (bmm_nt with col_bias); K = 200 with 7 rows: 3 slices of 96 columns + the reduction launch."""
    yield from _linear_forward(ops, mp, ((7, 100, 90, False), (7, 200, 90, True), (33, 37, 92, False)))


@case('splitk_reduce_kernel')
def linear_forward_split(ops, mp):
    yield from _linear_forward(ops, mp, ((7, 200, 90, True), (70, 520, 33, True)))


@case(_CG_TF + ' | ksplit > 1', _CG_TF + ' | accumulate')
def linear_dgrad(ops, mp):
    """70 rows, K = 100 output features: one tile, 7 K iterations -> ops._conv_ksplit splits the single product in 3."""
    for what, res, seen in run_linear(ops, mp, 70, 90, 100):
        if what.startswith('dgrad'):
            assert seen[0][1]['ksplit'] > 1 and seen[0][1]['a_kc'] == 1 and _CG_TF in res['names'], (seen, res)
            assert seen[0][1]['accumulate'] == int(what == 'dgrad_acc')
            yield res


def _linear_wgrad(ops, mp, N, Ci, Co, ring):
    for what, res, seen in run_linear(ops, mp, N, Ci, Co):
        if what == 'wgrad':
            assert ring in res['names'] and seen[0][1]['accumulate'] == 1, (res, seen)
            yield res


@case(_CG_FF + ' | accumulate')
def linear_wgrad_tn(ops, mp):
    """Co % 4 == 0: bmm_tn straight into gw."""
    yield from _linear_wgrad(ops, mp, 33, 37, 92, _CG_FF)


@case(_NT_F + ' | ' + _TILES3[1])
def linear_wgrad_nt(ops, mp):
    """An odd Co has no 16-byte operand rows for the m-contiguous A loader: the 1x1 weight gradient on dp_nt_gemm, one pixel an image."""
    yield from _linear_wgrad(ops, mp, 33, 92, 37, _NT_F)


# ======================================================================================================================
# dp_nt_gemm and the Winograd weight gradients through conv_wgrad
# ======================================================================================================================
def run_wgrad(ops, mp, N, C1, C2, Cout, H, W, spec, *, want, blk=None, has=(), lacks=(), bound=B_DIRECT, twice=False, keep=None):
    """conv_wgrad into a NaN-filled gw (accumulate = False) and into a given one (accumulate, alpha = 0.5)."""
    x, x2 = rnd(N, C1, H, W, seed=1), (rnd(N, C2, H, W, seed=2) if C2 else None)
    Ho, Wo = spec.out_hw(H, W)
    dy = rnd(N, Cout, Ho, Wo, seed=3)
    Cin = C1 + C2
    ref = ref_conv_wgrad(dy, x if x2 is None else torch.cat([x, x2], 1), spec, spec.kh, spec.kw)
    gw = nan_like(Cout, Cin, spec.kh, spec.kw)
    _, names, seen = launched_m(ops, mp, lambda: ops.conv_wgrad(dy, x, x2, gw, spec, accumulate=False))
    assert [n for n, _ in seen] == [want] and (blk is None or blk(seen[0][1])), (seen, want)
    assert all(h in names for h in has) and not any(h in names for h in lacks), (names, has, lacks)
    out = [dict(names=names, shape=(N, C1, C2, Cout, H, W), mirror=want, splits=seen[0][1]['splits'], out=relerr(gw, ref), bound=bound)]
    if twice:
        g2 = nan_like(Cout, Cin, spec.kh, spec.kw)
        ops.conv_wgrad(dy, x, x2, g2, spec, accumulate=False)
        assert torch.equal(gw, g2), 'two runs of a split weight gradient differ'
    ga = rnd(Cout, Cin, spec.kh, spec.kw, seed=4)
    g0 = ga.clone()
    _, names_b, seen_b = launched_m(ops, mp, lambda: ops.conv_wgrad(dy, x, x2, ga, spec, alpha=0.5, accumulate=True))
    assert [n for n, _ in seen_b] == [want], (seen_b, want)
    e = float((d64(ga) - d64(g0) - 0.5 * ref).abs().max() / (0.5 * ref).abs().max())       # the gradient's own scale, as the older tests
    out.append(dict(names=names_b, shape=(N, C1, C2, Cout, H, W), mirror=want, accumulate=True, out=e, bound=bound))
    if keep is not None:
        keep['a'], keep['b'] = gw.clone(), ga.clone()
    return out


def _reg_nt():
    for nw, two, (C1, C2, Cout) in ((4, 'false', (40, 0, 100)), (4, 'true', (24, 16, 100)), (3, 'false', (90, 0, 90)), (3, 'true', (50, 40, 90))):
        @case('nt_gemm_fast_kernel<%d, %s>' % (nw, two))
        def fast(ops, mp, nw=nw, two=two, C1=C1, C2=C2, Cout=Cout):
            want = 'nt_gemm_fast_kernel<%d, %s>' % (nw, two)
            yield from run_wgrad(ops, mp, 3, C1, C2, Cout, 8, 8, S(ops), want=want, blk=lambda b: b['splits'] == 1, lacks=['splitk_reduce_taps_mc_kernel<9>'])
            yield from run_wgrad(ops, mp, 5, C1, C2, Cout, 8, 8, S(ops), want=want, blk=lambda b: b['splits'] == 2, twice=True,
                                 has=['splitk_reduce_taps_mc_kernel<9>'])
            yield from run_wgrad(ops, mp, 6, C1, C2, Cout, 4, 4, S(ops, 1, 1, 0), want=want)       # 16 | Wo ... 16 % 4 == 0: a 1x1 at 4 x 4

    # the general kernel: 6 x 6 images (neither 16 | Wo nor Wo | 16)
    for kernel, straddle, cols in ((_NT_F, 'false', ((40, 0), (128, 12))), (_NT_T, 'true', ((21, 19), (130, 10)))):
        for cond, tile, Cout in zip(_TILES3[:2], ('128, 128', '64, 128'), (100, 40)):
            @case(kernel + ' | ' + cond)
            def gen(ops, mp, kernel=kernel, straddle=straddle, cols=cols, tile=tile, Cout=Cout):
                for C1, C2 in cols:
                    yield from run_wgrad(ops, mp, 3, C1, C2, Cout, 6, 6, S(ops), has=[kernel],
                                         want='nt_gemm_kernel<%s, %s, false>' % (tile, 'true' if C2 and C1 % 128 else 'false'))


_reg_nt()


def _taps_pair(ops, mp, N, C1, Cout, spec, want, mc):
    """A split weight gradient with the all-taps reduction, then with the scalar one (DP_NO_REDUCE_MC, read per call): the same bits."""
    keep, k2 = {}, {}
    for r in run_wgrad(ops, mp, N, C1, 0, Cout, 6, 6, spec, want=want, twice=True, keep=keep, blk=lambda b: b['splits'] == 2, has=[_NT_F, mc]):
        yield 'mc', r
    with mp.context() as m:
        m.setenv('DP_NO_REDUCE_MC', '1')
        for r in run_wgrad(ops, m, N, C1, 0, Cout, 6, 6, spec, want=want, keep=k2, has=['splitk_reduce_taps_kernel'], lacks=[mc]):
            yield 'scalar', r
    assert torch.equal(keep['a'], k2['a']) and torch.equal(keep['b'], k2['b']), 'taps_mc and taps give different bits'


# 8 images of 6 x 6: 288 pixels in two slices of 160 and 128
_TAPS9 = (8, 40, 100, lambda ops: S(ops), 'nt_gemm_kernel<128, 128, false, false>', 'splitk_reduce_taps_mc_kernel<9>')
# the 2 x 2 parity-class kernels of the upsample convolution (ops.UPS_CLASS_SPECS), 20 -> 40 channels
_TAPS4 = [(8, 20, 40, lambda ops, i=i: ops.UPS_CLASS_SPECS[i], 'nt_gemm_kernel<64, 128, false, false>', 'splitk_reduce_taps_mc_kernel<4>')
          for i in (1, 2)]


def _taps(ops, mp, t, form):
    N, C1, Cout, spec, want, mc = t
    yield from (r for f, r in _taps_pair(ops, mp, N, C1, Cout, spec(ops), want, mc) if f == form)


@case(_NT_F + ' | splits > 1', 'splitk_reduce_taps_mc_kernel<9>')
def wgrad_split_taps9(ops, mp):
    yield from _taps(ops, mp, _TAPS9, 'mc')


@case('splitk_reduce_taps_mc_kernel<4>')
def wgrad_split_taps4(ops, mp):
    for t in _TAPS4:
        yield from _taps(ops, mp, t, 'mc')


@case('splitk_reduce_taps_kernel')
def wgrad_split_taps_scalar(ops, mp):
    """One tap (1x1) and 25 (5x5): neither of the all-taps instantiations; and the scalar form on the 9- and 4-tap partials."""
    yield from run_wgrad(ops, mp, 8, 40, 0, 100, 6, 6, S(ops, 1, 1, 0), want='nt_gemm_kernel<128, 128, false, false>', twice=True,
                         blk=lambda b: b['splits'] == 2, has=['splitk_reduce_taps_kernel'])
    yield from run_wgrad(ops, mp, 8, 20, 0, 40, 6, 6, ops.ConvSpec.general(5, 5, 1, 2, 2), want='nt_gemm_kernel<64, 128, false, false>', twice=True,
                         blk=lambda b: b['splits'] == 2, has=['splitk_reduce_taps_kernel'])
    for t in [_TAPS9] + _TAPS4:
        yield from _taps(ops, mp, t, 'scalar')


def _merged_few_in(ops, mp, N, splits):
    return run_wgrad(ops, mp, N, 3, 0, 40, 8, 8, S(ops), want='nt_gemm_kernel<64, 64, false, true>', twice=splits > 1,
                     blk=lambda b: b['merge'] == 1 and b['splits'] == splits, has=[_NT_M] + (['splitk_reduce_kernel'] if splits > 1 else []))


@case(_NT_M + ' | merge = 1')
def wgrad_merged_few_in(ops, mp):
    yield from _merged_few_in(ops, mp, 3, 1)
    yield from _merged_few_in(ops, mp, 5, 2)
    yield from run_wgrad(ops, mp, 3, 4, 0, 70, 16, 16, S(ops, 3, 2, 0), want='nt_gemm_kernel<64, 64, false, true>', blk=lambda b: b['merge'] == 1)


@case('splitk_reduce_kernel')
def wgrad_merged_reduce(ops, mp):
    yield from _merged_few_in(ops, mp, 5, 2)


@case(_NT_M + ' | merge = 3')
def wgrad_merged_few_out(ops, mp):
    for N, splits in ((3, 1), (5, 2)):
        yield from run_wgrad(ops, mp, N, 40, 0, 3, 8, 8, S(ops), want='nt_gemm_kernel<64, 64, false, true>', twice=splits > 1,
                             blk=lambda b: b['merge'] == 3 and b['splits'] == splits, has=[_NT_M])
    yield from run_wgrad(ops, mp, 3, 70, 0, 7, 5, 7, S(ops), want='nt_gemm_kernel<64, 64, false, true>', blk=lambda b: b['merge'] == 3)


def _reg_wgrad_wino():
    for bt, (C1, C2, Cout) in ((2, (40, 0, 70)), (3, (90, 0, 96))):
        @case('wgrad_wino_kernel<%d, %d>' % (bt, bt))
        def c(ops, mp, bt=bt, C1=C1, C2=C2, Cout=Cout):
            gates(ops, mp, WGRAD_WINO_MIN_WORK=0, WGRAD_WINO_MIN_FILL=0.0, WGRAD_WINO2D=False)
            want = 'wgrad_wino_kernel<%d, %d>' % (bt, bt)
            yield from run_wgrad(ops, mp, 2, C1, C2, Cout, 8, 8, S(ops), want=want, bound=B_WINO_WGRAD, blk=lambda b: b['splits'] == 1)
            yield from run_wgrad(ops, mp, 5, C1, C2, Cout, 4, 16, S(ops), want=want, bound=B_WINO_WGRAD, twice=True,
                                 blk=lambda b: b['splits'] > 1, has=['splitk_reduce_taps_mc_kernel<9>'])
            if bt == 2:                                     # two sources, the boundary on a 64-column tile
                yield from run_wgrad(ops, mp, 2, 64, 24, Cout, 8, 8, S(ops), want=want, bound=B_WINO_WGRAD)

    for lw, (H, W) in ((5, (2, 32)), (4, (4, 16)), (3, (8, 8))):
        for tail, Cout in ((True, 70), (False, 40)):
            @case('wgrad_wino2d_%skernel<%d>' % ('tail_' if tail else '', lw))
            def c2(ops, mp, lw=lw, H=H, W=W, tail=tail, Cout=Cout):
                gates(ops, mp, WGRAD_WINO_MIN_WORK=0, WGRAD_WINO_MIN_FILL=0.0, WGRAD_WINO2D_MIN_FILL=0.0)
                want = 'wgrad_wino2d_%skernel<%d>' % ('tail_' if tail else '', lw)
                yield from run_wgrad(ops, mp, 3, 40, 0, Cout, H, W, S(ops), want=want, bound=B_WINO_WGRAD, blk=lambda b: b['splits'] == 1)
                yield from run_wgrad(ops, mp, 9, 32, 24, Cout, H, W, S(ops), want=want, bound=B_WINO_WGRAD, twice=True,
                                     blk=lambda b: b['splits'] > 1, has=['splitk_reduce_taps_mc_kernel<9>'])


_reg_wgrad_wino()


# ======================================================================================================================
# the Winograd forwards / input gradients
# ======================================================================================================================
def _reg_wino():
    for bk, (K1, K2) in ((16, (32, 0)), (8, (16, 8))):
        for wr, M in ((2, 40), (1, 80)):
            @case('conv_wino_kernel<%d, %d>' % (bk, wr))
            def c(ops, mp, bk=bk, wr=wr, K1=K1, K2=K2, M=M):
                """3 images of 8 x 8: 192 pixels, the second 128-pixel tile half empty and spanning two images; then 4 x 16 images."""
                gates(ops, mp, WINO_MIN_TILES=0)
                want = 'conv_wino_kernel<%d, %d, 1>' % (bk, wr)
                yield from run_conv(ops, mp, 'fwd', 3, K1, K2, M, 8, 8, S(ops), want=want, wino='1d', bound=B_WINO, blk=lambda b: b['ksplit'] <= 1)
                yield from run_conv(ops, mp, 'dgrad', 5, K1 + K2, 0, M, 4, 16, S(ops), wino='1d', bound=B_WINO,
                                    want='conv_wino_kernel<%d, %d, 1>' % (16 if (K1 + K2) % 16 == 0 else 8, wr))

    @case('conv_wino_kernel<16, 2> | ksplit > 1')
    def split(ops, mp):
        gates(ops, mp, WINO_MIN_TILES=4 * 1 * 2)                                 # 2 tiles: wants 4 slices, gets min(4, 24 K tiles / 8) = 3
        yield from run_conv(ops, mp, 'fwd', 3, 128, 0, 40, 8, 8, S(ops), want='conv_wino_kernel<16, 2, 1>', wino='1d', bound=B_WINO, twice=True,
                            blk=lambda b: b['ksplit'] == 3, has=['conv_wino_kernel<16, 2>', 'conv_splitk_epilogue4_kernel'])

    @case('conv_wino_kernel<8, 1>')
    def wide_image(ops, mp):
        gates(ops, mp, WINO_MIN_TILES=0)
        yield from run_conv(ops, mp, 'fwd', 1, 24, 0, 40, 2, 256, S(ops), want='conv_wino_kernel<8, 1, 1>', wino='1d', bound=B_WINO)     # Wo > 128


_reg_wino()


def _reg_wino2d():
    small = dict(WINO_MIN_TILES=0, WINO2D_MIN_TILES=0)
    # (entry, gates, [(kind, N, K1, K2, M, H, W)])
    table = (
        ('conv_wino2d_kernel<8, 2, false>', small, [('fwd', 3, 16, 8, 40, 8, 8), ('dgrad', 5, 40, 0, 64, 4, 16), ('fwd', 9, 8, 0, 120, 4, 4)]),
        ('conv_wino2d_tail_kernel<8, 2, false>', small, [('fwd', 3, 16, 8, 70, 8, 8), ('dgrad', 5, 40, 0, 16, 6, 8)]),
        ('conv_wino2d_kernel<4, 2, true>', small, [('fwd', 2, 16, 8, 40, 2, 128), ('dgrad', 1, 40, 0, 48, 4, 256)]),
        ('conv_wino2d_tail_kernel<4, 2, true>', small, [('fwd', 2, 16, 8, 70, 2, 128), ('dgrad', 1, 40, 0, 16, 2, 256)]),
        # more than 512 workgroups from 4 x 4 images and 8 channels
        ('conv_wino2d_kernel<4, 3, false>', {}, [('fwd', 4104, 8, 0, 40, 4, 4), ('dgrad', 4104, 8, 0, 40, 4, 4)]),
        ('conv_wino2d_tail_kernel<4, 3, false>', {}, [('fwd', 1403, 8, 0, 160, 4, 4)]),
        ('conv_wino2d_m32_kernel<4, 5, false>', {}, [('fwd', 2104, 8, 0, 80, 4, 4), ('dgrad', 4104, 8, 0, 24, 4, 4)]),
    )
    for entry, g, shapes in table:
        @case(entry)
        def c(ops, mp, entry=entry, g=g, shapes=shapes):
            gates(ops, mp, **g)
            for kind, N, K1, K2, M, H, W in shapes:
                assert len(edge_images(N, H * W)) >= 3 or H * W > 128            # a 128-pixel block spans images wherever images are smaller
                yield from run_conv(ops, mp, kind, N, K1, K2, M, H, W, S(ops), want=entry, wino='2d', bound=B_WINO, blk=lambda b: b['ksplit'] <= 1)

    @case('conv_wino2d_kernel<8, 2, false> | ksplit > 1')
    def split(ops, mp):
        gates(ops, mp, WINO_MIN_TILES=0, WINO2D_MIN_TILES=4 * 1 * 2)
        yield from run_conv(ops, mp, 'fwd', 3, 128, 0, 40, 8, 8, S(ops), want='conv_wino2d_kernel<8, 2, false>', wino='2d', bound=B_WINO,
                            twice=True, blk=lambda b: b['ksplit'] > 1, has=['conv_splitk_epilogue4_kernel'])


_reg_wino2d()


@case('conv_wino43_kernel')
def wino43(ops, mp):
    gates(ops, mp, WINO_MIN_TILES=0, WINO43=True, WINO43_MIN_TILES=0)
    for N, K1, K2, M, H, W in ((3, 16, 8, 40, 8, 8), (5, 32, 0, 70, 4, 16), (1, 24, 0, 100, 2, 256)):
        yield from run_conv(ops, mp, 'fwd', N, K1, K2, M, H, W, S(ops), want='conv_wino43_kernel', wino='43', bound=B_F43,
                            blk=lambda b: b['ksplit'] <= 1)


@case('conv_wino43_kernel | ksplit > 1')
def wino43_split(ops, mp):
    gates(ops, mp, WINO_MIN_TILES=0, WINO43=True, WINO43_MIN_TILES=4)
    yield from run_conv(ops, mp, 'fwd', 3, 64, 0, 40, 8, 8, S(ops), want='conv_wino43_kernel', wino='43', bound=B_F43, twice=True,
                        blk=lambda b: b['ksplit'] > 1, has=['conv_splitk_epilogue4_kernel'])


# ======================================================================================================================
# attention
# ======================================================================================================================
ATTN_WIDTHS = {1: ((32, 24), (33, 40)), 2: ((160, 130),), 3: ((260, 288),), 4: ((416, 390),), 5: ((544, 520),)}       # (d, dv) per NT


def _reg_attention():
    for kernel, variants in (('pipe', {1: 0, 2: 0, 3: 2, 4: 2, 5: 2}), ('fused', {1: 1, 2: 1, 3: 0, 4: 0, 5: 0})):
        for nt, widths in ATTN_WIDTHS.items():
            @case('attn_fwd_%s_kernel<%d>' % (kernel, nt))
            def c(ops, mp, kernel=kernel, nt=nt, widths=widths, variant=variants[nt]):
                """T = 32 (one key block) and 96; d != dv; two heads at the narrow widths; then into a channel slice of a wider buffer."""
                for d, dv in widths:
                    assert (-(-max(d, dv) // 32) + 3) // 4 == nt
                    for N, heads, H, W in ((2, 2 if nt == 1 else 1, 4, 8), (1, 1, 8, 12)):
                        q, k, v = rnd(N, heads * d, H, W, seed=1), rnd(N, heads * d, H, W, seed=2), rnd(N, heads * dv, H, W, seed=3)
                        scale = float(d) ** -0.5
                        ref = ref_attention(d64(q), d64(k), d64(v), heads, scale)
                        poison(N * heads * dv * H * W)
                        o, names, _ = launched_m(ops, mp, lambda: ops.attention_fwd(q, k, v, heads, scale, variant=variant))
                        assert names == ['attn_fwd_%s_kernel<%d>' % (kernel, nt)], names
                        view, big = wide(N, heads * dv, H, W, 4)
                        before = big.clone()
                        ops.attention_fwd(q, k, v, heads, scale, out=view, variant=variant)
                        assert outside_intact(big, before, 2, heads * dv) and torch.equal(view, o)
                        yield dict(names=names, shape=(N, heads, d, dv, H * W), variant=variant, out=relerr(o, ref), bound=B_ATTN)


_reg_attention()


# ======================================================================================================================
# the nine-product kernels
# ======================================================================================================================
def _ups9_ref(x64, w64):
    return F.conv2d(F.interpolate(x64, scale_factor=2, mode='nearest'), w64, padding=1)


def run_ups9_dgrad(ops, mp, N, Cin, Cout, H, W, tile, default=False):
    w = rnd(Cout, Cin, 3, 3, seed=1, scale=1.0 / (3.0 * Cin ** 0.5))
    dy = guarded_act(ops, rnd(N, Cout, 2 * H, 2 * W, seed=2))
    up, ldu = ops.pack_weight(ops.ups9_u(w), 1)
    x64 = torch.zeros(N, Cin, H, W, dtype=torch.float64, requires_grad=True)
    ref = torch.autograd.grad(_ups9_ref(x64, d64(w)), x64, d64(dy))[0]
    kw = {} if default else dict(tile=tile)
    assert not default or ops.ups9_tile(N, Cin, H, W) == tile
    poison(N * Cin * H * W)
    dx, names, seen = launched_m(ops, mp, lambda: ops.ups9_dgrad(dy, up, ldu, Cin, **kw))
    assert names == [_U9D[tile]] and [n for n, _ in seen] == [_U9D[tile]], (names, seen)
    assert torch.equal(dx, ops.ups9_dgrad(dy, up, ldu, Cin, **kw)), 'two runs differ'
    yield dict(names=names, shape=(N, Cin, Cout, H, W), tile=tile, out=relerr(dx, ref), bound=B_UPS9)
    view, big = wide(N, Cin, H, W, 3)
    before = big.clone()
    _, names, _ = launched_m(ops, mp, lambda: ops.ups9_dgrad(dy, up, ldu, Cin, out=view, accumulate=True, **kw))
    assert names == [_U9D[tile]] and outside_intact(big, before, 2, Cin)
    yield dict(names=names, shape=(N, Cin, Cout, H, W), tile=tile, accumulate=True, out=relerr(view, ref + d64(before[:, 2:2 + Cin])), bound=B_UPS9)


def _reg_ups9():
    for tile in (0, 1, 2):
        @case(_U9D[tile], _U9D[tile] + ' | accumulate')
        def c(ops, mp, tile=tile):
            """3 images of 4 x 4 (a pixel block spans images, the last one is ragged, 40-row K and 16-row M tails), 5 x 3 with odd channel
            counts, 130 rows (two row tiles); tile 2 also as ops.ups9_tile's own choice under the default UPS9_MIN_BLOCKS."""
            for N, Cin, Cout, H, W in ((3, 16, 40, 4, 4), (2, 20, 7, 5, 3), (2, 130, 24, 4, 4)):
                yield from run_ups9_dgrad(ops, mp, N, Cin, Cout, H, W, tile)
            if tile == 2:
                assert ops.UPS9_MIN_BLOCKS == 512
                yield from run_ups9_dgrad(ops, mp, 4090, 8, 8, 4, 4, 2, default=True)


_reg_ups9()


@case(_U9F, _U9F + ' | bias')
def ups9_fwd(ops, mp):
    for N, Cin, Cout, H, W in ((5, 20, 36, 4, 4), (2, 7, 5, 5, 3), (1, 130, 130, 4, 4)):
        w, b = rnd(Cout, Cin, 3, 3, seed=1, scale=1.0 / (3.0 * Cin ** 0.5)), rnd(Cout, seed=2)
        x = guarded_act(ops, rnd(N, Cin, H, W, seed=3))
        up, ldu = ops.pack_weight(ops.ups9_u(w), 0)
        ref = _ups9_ref(d64(x), d64(w))
        for bias in (None, b):
            poison(N * Cout * 4 * H * W)
            y, names, seen = launched_m(ops, mp, lambda: ops.ups9_fwd(x, up, ldu, Cout, bias=bias))
            assert names == [_U9F] and [n for n, _ in seen] == [_U9F] and bool(seen[0][1]['bias']) == (bias is not None), (names, seen)
            assert torch.equal(y, ops.ups9_fwd(x, up, ldu, Cout, bias=bias))
            r = ref + (d64(b)[None, :, None, None] if bias is not None else 0)
            view, big = wide(N, Cout, 2 * H, 2 * W, 4)
            before = big.clone()
            ops.ups9_fwd(x, up, ldu, Cout, bias=bias, out=view)
            assert outside_intact(big, before, 2, Cout) and torch.equal(view, y)
            yield dict(names=names, shape=(N, Cin, Cout, H, W), bias=bias is not None, out=relerr(y, r), bound=B_UPS9)


@case('ups9_u_kernel')
def ups9_u(ops, mp):
    for Cout, Cin in ((7, 5), (130, 70), (4096, 257)):                  # the last: more than 4096 * 256 kernels, the grid-stride loop turns
        w = rnd(Cout, Cin, 3, 3, seed=1)
        poison(w.numel())
        u, names = launched(ops, lambda: ops.ups9_u(w))
        assert names == ['ups9_u_kernel']
        g = w.cpu()
        t = torch.stack([g[:, :, 0], (g[:, :, 0] + g[:, :, 1]) + g[:, :, 2], g[:, :, 2]], 2)
        ref = torch.stack([t[..., 0], (t[..., 0] + t[..., 1]) + t[..., 2], t[..., 2]], 3)
        assert torch.equal(u.cpu(), ref)
        yield dict(names=names, shape=(Cout, Cin), out=relerr(u, ref), bound=0.0)


# ======================================================================================================================
# the weight packers: the fp32 CPU evaluation of the same expression in the same order
# ======================================================================================================================
def _g4(g0, g1, g2):
    return [g0, ((g0 + g1) + g2) * 0.5, ((g0 - g1) + g2) * 0.5, g2]


def _padded(t, ld):
    """[..., K, Mv] -> [..., K, ld] with zero columns."""
    return F.pad(t, (0, ld - t.shape[-1]))


PACK_SHAPES = ((7, 5), (90, 45), (33, 130))


@case('pack_weight_kernel')
def pack_weight(ops, mp):
    for Co, Ci in PACK_SHAPES:
        for tail in ((3, 3), (1, 1), (2, 2), ()):
            w = rnd(Co, Ci, *tail, seed=1)
            taps = max(1, w[0, 0].numel())
            for mode in (0, 1):
                poison(taps * max(Co, Ci) * (max(Co, Ci) + 3))
                (dst, ld), names = launched(ops, lambda: ops.pack_weight(w, mode))
                assert names == ['pack_weight_kernel'] and ld == (((Co if mode == 0 else Ci) + 3) & ~3)
                wc = w.cpu().reshape(Co, Ci, taps)
                ref = wc.permute(2, 1, 0) if mode == 0 else wc.flip(2).permute(2, 0, 1)           # [taps, K, Mv]
                ok = torch.equal(dst.cpu().view(taps, -1, ld), _padded(ref, ld))
                assert ok, (Co, Ci, tail, mode)
                yield dict(names=names, shape=(Co, Ci) + tail, mode=mode, out=0.0 if ok else 1.0, bound=0.0)
    w = rnd(24, 40, 3, 3, seed=2)                                        # the parity-class operands of conv_dgrad_s2
    for ph, pw, pad in ((0, 0, 0), (0, 1, 0), (1, 1, 1)):
        (dst, ld), names = launched(ops, lambda: ops.pack_weight_s2(w, ph, pw, pad))
        kh, kw = ops._s2_taps(ph, pad)[0], ops._s2_taps(pw, pad)[0]
        sub = w.cpu()[:, :, kh][:, :, :, kw].reshape(24, 40, -1)
        ok = torch.equal(dst.cpu().view(len(kh) * len(kw), 24, ld), _padded(sub.flip(2).permute(2, 0, 1), ld))
        assert ok and names == ['pack_weight_kernel']
        yield dict(names=names, shape=(24, 40, len(kh), len(kw)), mode='s2', out=0.0, bound=0.0)


@case('pack_weight_wino_kernel')
def pack_weight_wino(ops, mp):
    for Co, Ci in PACK_SHAPES:
        w = rnd(Co, Ci, 3, 3, seed=1)
        for mode in (0, 1):
            poison(12 * max(Co, Ci) * (max(Co, Ci) + 3))
            (dst, ld), names = launched(ops, lambda: ops.pack_weight_wino(w, mode))
            g = w.cpu() if mode == 0 else w.cpu().flip(2, 3).transpose(0, 1)                      # [Mv, K, ky, kx]
            ref = torch.stack([torch.stack(_g4(g[:, :, ky, 0], g[:, :, ky, 1], g[:, :, ky, 2]), 0) for ky in range(3)], 0)   # [ky, pos, Mv, K]
            ok = torch.equal(dst.cpu().view(3, 4, -1, ld), _padded(ref.transpose(2, 3), ld))
            assert ok and names == ['pack_weight_wino_kernel'], (Co, Ci, mode)
            yield dict(names=names, shape=(Co, Ci), mode=mode, out=0.0, bound=0.0)


@case('pack_weight_wino2d_kernel')
def pack_weight_wino2d(ops, mp):
    for Co, Ci in PACK_SHAPES:
        w = rnd(Co, Ci, 3, 3, seed=1)
        for mode in (0, 1):
            poison(16 * max(Co, Ci) * (max(Co, Ci) + 3))
            (dst, ld), names = launched(ops, lambda: ops.pack_weight_wino2d(w, mode))
            g = w.cpu() if mode == 0 else w.cpu().flip(2, 3).transpose(0, 1)
            t = _g4(g[:, :, 0], g[:, :, 1], g[:, :, 2])                                           # rows i: [Mv, K, b]
            ref = torch.stack([torch.stack(_g4(ti[..., 0], ti[..., 1], ti[..., 2]), 0) for ti in t], 0)      # [i, j, Mv, K]
            ok = torch.equal(dst.cpu().view(4, 4, -1, ld), _padded(ref.transpose(2, 3), ld))
            assert ok and names == ['pack_weight_wino2d_kernel'], (Co, Ci, mode)
            yield dict(names=names, shape=(Co, Ci), mode=mode, out=0.0, bound=0.0)


@case('pack_weight_wino43_kernel')
def pack_weight_wino43(ops, mp):
    for Co, Ci in PACK_SHAPES:
        w = rnd(Co, Ci, 3, 3, seed=1)
        poison(18 * Ci * (Co + 3))
        (dst, ld), names = launched(ops, lambda: ops.pack_weight_wino43(w))
        g = d64(w)
        g0, g1, g2 = g[..., 0], g[..., 1], g[..., 2]                                               # [Co, Ci, ky]
        c6, c12, c24 = (float(torch.tensor(1.0 / k, dtype=torch.float32)) for k in (6, 12, 24))
        ref = torch.stack([g0 * 0.25, (g0 + g1 + g2) * -c6, (g0 - g1 + g2) * -c6, g0 * c24 + g1 * c12 + g2 * c6,
                           g0 * c24 - g1 * c12 + g2 * c6, g2], 0)                                 # [pos, Co, Ci, ky]
        ref = _padded(ref.permute(3, 0, 2, 1), ld)                                                # [ky, pos, Ci, ld]
        assert names == ['pack_weight_wino43_kernel'] and bool((dst.cpu().view(3, 6, Ci, ld)[..., Co:] == 0).all())
        yield dict(names=names, shape=(Co, Ci), out=relerr(dst.view(3, 6, Ci, ld), ref), bound=2e-7)


# ======================================================================================================================
# the closing test: parametrised over the table itself
# ======================================================================================================================
@pytest.mark.parametrize('entry', BRANCHES)
def test_branch(entry, ops, report, monkeypatch):
    assert (entry in CASES) != (entry in UNREACHED), 'every entry has a case or a reason in UNREACHED, never both: %s' % entry
    if entry in UNREACHED:
        return
    name, log, bad = entry.split(' | ')[0], [], []
    known = KNOWN | D.KNOWN
    for fn in CASES[entry]:
        with monkeypatch.context() as mp:
            for res in fn(ops, mp):
                assert name in res['names'], (entry, res['names'])
                assert set(res['names']) <= known, ('a launch name outside the tables', sorted(set(res['names']) - known))
                assert any(isinstance(v, float) and k != 'bound' for k, v in res.items()), res
                res = dict(res, case=fn.__name__)
                print(entry, res)
                log.append({k: (list(v) if isinstance(v, tuple) else v) for k, v in res.items()})
                if exceeding(res):
                    bad.append(res)
                torch.cuda.empty_cache()
    assert log, entry
    report['contraction_dispatch/' + entry] = log
    assert not bad, bad


def test_tables_are_consistent():
    assert len(set(BRANCHES)) == len(BRANCHES) and not set(UNREACHED) - set(BRANCHES)
    assert not set(CASES) - set(BRANCHES) and not KNOWN & D.KNOWN
    assert all(e in CASES or e in UNREACHED for e in BRANCHES), [e for e in BRANCHES if e not in CASES and e not in UNREACHED]
