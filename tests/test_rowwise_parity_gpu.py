"""The contraction kernels against per-row fp64 bounds, on operands whose channels differ in scale by up to 1e8.

The rule (tests/rowwise.py): for every kernel form below and every operand family -- randn (the control), row scales, all scales, all
scales + offsets -- the kernel's output is measured row by row, a row being what the product later reads as one number's worth of
signal (an output channel, an input channel, a (k, c) weight-gradient pair, a bmm row, an attention (image, channel), an importance
score): e_hip = max over rows of the row's largest error over the row's largest cond64, cond64 being the same operation in fp64 on the
absolute values of every operand and epilogue addend.  The bound is 4 x max(e_ref32, e_alg32, 2 x 2^-24), where e_ref32 is torch's fp32
CPU operator and e_alg32 an fp32 CPU restatement of the algorithm the kernel documents with its products added one after another, both
measured the same way against the same fp64 reference: nothing comes from the kernel's output, no row is left out, and the assertion is
e_hip <= bound.  The max-norm figure of the older tests is recorded beside it.  Every case goes through `launched_m` of
tests/test_contraction_dispatch_gpu.py and asserts the kernel that ran; shapes are that table's (the smallest that select the branch and
keep its ragged edges).  The figures of one run on an MI355X, one line per case: profiles/rowwise_gpu_tests.txt."""
import importlib
import os
import time
import zlib

import pytest
import torch

import conftest
import rowwise as R
import test_contraction_dispatch_gpu as C
import test_dispatch_parity_gpu as D
from helpers import spec_pads
from test_contraction_dispatch_gpu import gates, guarded_act, launched_m, nan_like
from test_dispatch_parity_gpu import launched, outside_intact, poison, wide

pytestmark = pytest.mark.gpu

OUT = os.path.join(conftest.OUT, 'rowwise_gpu_tests.txt')           # the suite's output directory, beside test_report.json

# (the reference's geometry, the ops.ConvSpec that must describe the same one)
S3 = (R.SAME3, lambda o: o.ConvSpec(3, 1, 1, 0))
S3_S2P0 = (R.Spec(3, 3, 2, (0, 1, 0, 1), 0), lambda o: o.ConvSpec(3, 2, 0, 0))
S3_S2P1 = (R.Spec(3, 3, 2, (1, 1, 1, 1), 0), lambda o: o.ConvSpec(3, 2, 1, 0))
S3_UPS = (R.UPS3, lambda o: o.ConvSpec(3, 1, 1, 1))
S1 = (R.Spec(1, 1, 1, (0, 0, 0, 0), 0), lambda o: o.ConvSpec(1, 1, 0, 0))
S5 = (R.Spec(5, 5, 1, (2, 2, 2, 2), 0), lambda o: o.ConvSpec.general(5, 5, 1, 2, 2))
S2_CLASS1 = (R.Spec(2, 2, 1, (1, 0, 0, 1), 0), lambda o: o.UPS_CLASS_SPECS[1])

KINDS = ('direct', 'wgrad', 'linear_bmm', 'winograd', 'ups9', 'attention', 'importance')
TABLE = []

# every form the file must see (ring names: the stringised first argument of DP_LAUNCH)
LISTED = [C._CGF_T, C._CGF_F, C._CG_FF, C._CG_FT, C._CG_TF, 'conv_splitk_epilogue4_kernel', 'conv_few_out_kernel', 'interleave2x2_kernel',
          'nt_gemm_fast_kernel<3, false>', 'nt_gemm_fast_kernel<3, true>', 'nt_gemm_fast_kernel<4, false>', 'nt_gemm_fast_kernel<4, true>',
          C._NT_F, C._NT_M, 'splitk_reduce_taps_mc_kernel<9>', 'splitk_reduce_taps_mc_kernel<4>', 'splitk_reduce_taps_kernel', 'splitk_reduce_kernel',
          'conv_wino_kernel<16, 2>', 'wgrad_wino_kernel<3, 3>', 'wgrad_wino_kernel<2, 2>',
          'conv_wino2d_kernel<8, 2, false>', 'conv_wino2d_tail_kernel<8, 2, false>', 'conv_wino2d_m32_kernel<4, 5, false>', 'conv_wino2d_kernel<4, 2, true>',
          'wgrad_wino2d_kernel<5>', 'wgrad_wino2d_kernel<4>', 'wgrad_wino2d_kernel<3>',
          'wgrad_wino2d_tail_kernel<5>', 'wgrad_wino2d_tail_kernel<4>', 'wgrad_wino2d_tail_kernel<3>',
          C._U9F, 'ups9_wgrad_kernel', 'ups9_wgrad_reduce_kernel'] + list(C._U9D) + [
          'attn_fwd_pipe_kernel<1>', 'attn_fwd_fused_kernel<1>', 'attn_fwd_pipe_kernel<2>', 'attn_fwd_fused_kernel<2>',
          'wg_gn_kernel', 'wg_rows_kernel', 'wg_cols_ct_kernel', 'wg_fold_taps_kernel', 'group_score_part_kernel', 'group_score_combine_kernel',
          'pg_score_part_kernel', 'pg_score_combine_kernel']


class Entry:
    def __init__(self, kind, name, build, run, has):
        assert kind in KINDS and name not in [e.name for e in TABLE], name
        self.kind, self.name, self.build, self.run, self.has = kind, name, build, run, tuple(has)
        self.seed = zlib.crc32(name.encode()) % 9973
        TABLE.append(self)


@pytest.fixture(scope='module')
def ops():
    importlib.import_module('diff-pruning_amd')
    o = importlib.import_module('diff-pruning_amd.ops')
    o._lib()
    return o


@pytest.fixture(scope='module', autouse=True)
def record():
    """rowwise_gpu_tests.txt in the suite's output directory: one line per case as the run goes, and the run time on top when the module is done."""
    lines, t0 = [], time.time()
    try:
        os.makedirs(os.path.dirname(OUT), exist_ok=True)
        open(OUT, 'w').close()
    except OSError:
        pass
    yield lines
    try:
        with open(OUT, 'w') as f:
            f.write('# tests/test_rowwise_parity_gpu.py on one MI355X: %d cases in %.0f s (CPU references included)\n' % (len(lines), time.time() - t0))
            f.write('# e_* in units of 2^-24 of the row\'s cond64 maximum; bound = 4 x max(e_ref32, e_alg32, 2); maxnorm = the older figure '
                    '(max error / max |ref64| of the tensor)\n')
            f.write('\n'.join(lines) + '\n')
    except OSError:
        pass


def dev(t):
    return t.to(D.DEV).contiguous()


def the_spec(ops, sp):
    s = sp[1](ops)
    assert (s.kh, s.kw, s.stride, tuple(spec_pads(s)), int(bool(s.ups))) == tuple(sp[0]), (sp[0], spec_pads(s))
    return s


def one_launch(ops, mp, call, want, blk=None, has=()):
    y, names, seen = launched_m(ops, mp, call)
    assert [n for n, _ in seen] == [want], (seen, want)
    assert blk is None or blk(seen[0][1]), seen
    assert all(h in names for h in has), (names, has)
    return y, names, seen[0][1]


# ======================================================================================================================
# conv_forward / conv_dgrad (direct and Winograd)
# ======================================================================================================================
def _wino_kw(ops, w, alg, mode):
    if alg == 'wino1d':
        return dict(wino=ops.pack_weight_wino(w, mode))
    if alg == 'wino2d':
        return dict(wino=('2d',) + tuple(ops.pack_weight_wino2d(w, mode)))
    return {}


def fwd(kind, name, N, K1, K2, M, H, W, sp=S3, *, want, has, epi='full', alg='direct', guarded=True, g=None, blk=None, pair=False):
    """conv_forward of cat(x[:, :K1], x[:, K1:]).  epi 'full' / 'bias' / 'none': a fresh, poisoned output; 'acc': accumulate (alpha = 0.5) into a
    channel slice of a wider buffer holding the case's `prev`, whose neighbours must stay as they were.  pair: the split-K shape in both
    reduction forms (folded, reduction launch), which must give the same bits."""
    def build(fam, e):
        return [R.conv_fwd_case(fam, e.seed, N, K1 + K2, M, H, W, sp[0], alg, epi, alpha=0.5)]

    def once(ops, mp, c, blk, has=has):
        spec, o = the_spec(ops, sp), c.o
        act = (lambda t: guarded_act(ops, dev(t))) if guarded else dev
        xa, xb = act(o['x'][:, :K1]), (act(o['x'][:, K1:]) if K2 else None)
        assert guarded or xa.storage_offset() == 0
        w = dev(o['w'])
        wp, ld = ops.pack_weight(w, 0)
        kw = _wino_kw(ops, w, alg, 0)
        Ho, Wo = spec.out_hw(H, W)
        poison(N * M * Ho * Wo)
        if epi == 'acc':
            view, big = wide(N, M, Ho, Wo, 7)
            view.copy_(dev(o['prev']))
            before = big.clone()
            _, names, b = one_launch(ops, mp, lambda: ops.conv_forward(xa, xb, wp, ld, M, spec, out=view, accumulate=True, alpha=0.5, **kw), want, blk, has)
            assert b.get('accumulate', 0) == 1 and outside_intact(big, before, 2, M), 'a launch wrote outside its channel slice'
            return view.clone(), names
        if epi == 'full':
            call = lambda: ops.conv_forward(xa, xb, wp, ld, M, spec, bias=dev(o['bias'].flatten()), tadd=dev(o['tadd'].reshape(N, M)), res=dev(o['res']),
                                            post_scale=0.7, **kw)
        else:
            call = lambda: ops.conv_forward(xa, xb, wp, ld, M, spec, bias=dev(o['bias'].flatten()) if epi == 'bias' else None, **kw)
        y, names, _ = one_launch(ops, mp, call, want, blk, has)
        return y, names

    def run(ops, mp, cases):
        gates(ops, mp, **(g or {}))
        if not pair:
            y, names = once(ops, mp, cases[0], blk)
            return [(cases[0], y, names, {})]
        outs = {}
        for fold in (True, False):
            with mp.context() as m:
                gates(ops, m, SPLITK_FOLD=fold, SPLITK_FOLD_MAX=1 << 30 if fold else ops.SPLITK_FOLD_MAX)
                outs[fold] = once(ops, m, cases[0], lambda b, fold=fold: b['ksplit'] > 1 and bool(b['tile_counters']) == fold, ())
                assert torch.equal(outs[fold][0], once(ops, m, cases[0], None, ())[0]), 'two runs of a split-K launch differ'
        assert torch.equal(outs[True][0], outs[False][0]), 'the folded split-K reduction and the reduction launch give different bits'
        assert not any(n.startswith('conv_splitk') for n in outs[True][1]) and any(n.startswith('conv_splitk') for n in outs[False][1])
        return [(cases[0], outs[True][0], outs[True][1] + outs[False][1], dict(forms='folded == reduction launch'))]

    Entry(kind, name, build, run, has)


def dgrad(kind, name, N, K, Cin, Ho, Wo, sp=S3, *, want, has, alg='direct', in_hw=None, acc=False, g=None, blk=None):
    """conv_dgrad of dy [N, K, Ho, Wo] to Cin input channels; acc: alpha = 0.5 into a channel slice of a wider buffer."""
    hw = in_hw or (Ho, Wo)

    def build(fam, e):
        return [R.conv_dgrad_case(fam, e.seed, N, K, Cin, Ho, Wo, sp[0], alg, in_hw=hw, acc=acc, alpha=0.5)]

    def run(ops, mp, cases):
        gates(ops, mp, **(g or {}))
        spec, o = the_spec(ops, sp), cases[0].o
        dy, w = guarded_act(ops, dev(o['dy'])), dev(o['w'])
        wp, ld = ops.pack_weight(w, 1)
        kw = _wino_kw(ops, w, alg, 1)
        poison(N * Cin * hw[0] * hw[1])
        if not acc:
            y, names, _ = one_launch(ops, mp, lambda: ops.conv_dgrad(dy, wp, ld, Cin, spec, hw, **kw), want, blk, has)
            return [(cases[0], y, names, {})]
        view, big = wide(N, Cin, hw[0], hw[1], 7)
        view.copy_(dev(o['prev']))
        before = big.clone()
        _, names, b = one_launch(ops, mp, lambda: ops.conv_dgrad(dy, wp, ld, Cin, spec, hw, out=view, accumulate=True, alpha=0.5, **kw), want, blk, has)
        assert b.get('accumulate', 0) == 1 and outside_intact(big, before, 2, Cin), 'a launch wrote outside its channel slice'
        return [(cases[0], view.clone(), names, {})]

    Entry(kind, name, build, run, has)


def dgrad_s2(name, N, Cout, Cin, Ho, Wo, sp, pad):
    """conv_dgrad_s2: four stride-1 class convolutions over dy + the interleave pass, which adds `add`."""
    def build(fam, e):
        return [R.conv_dgrad_case(fam, e.seed, N, Cout, Cin, Ho, Wo, sp[0], in_hw=(2 * Ho, 2 * Wo), acc=True)]

    def run(ops, mp, cases):
        spec, o = the_spec(ops, sp), cases[0].o
        dy, w, add = dev(o['dy']), dev(o['w']), dev(o['prev'])
        packs = [ops.pack_weight_s2(w, ph, pw, pad) for ph in (0, 1) for pw in (0, 1)]
        poison(N * Cin * 4 * Ho * Wo)
        dx, names, seen = launched_m(ops, mp, lambda: ops.conv_dgrad_s2(dy, packs, Cin, spec, (2 * Ho, 2 * Wo), add=add))
        assert names == [C._CG_FF] * 4 + ['interleave2x2_kernel'], names
        return [(cases[0], dx, names, {})]

    Entry('direct', name, build, run, [C._CG_FF, 'interleave2x2_kernel'])


BIG = (C.BIG_N, C.BIG_H, C.BIG_W)
_F = 'conv_gemm_fast_kernel<%s>'
_one = lambda b: b['ksplit'] <= 1

fwd('direct', 'fast x4 128 rows', BIG[0], 32, 0, 100, *BIG[1:], want=_F % '128, 128, false, true', has=[C._CGF_T], blk=_one)
fwd('direct', 'fast x4 128 rows TAILS two sources', BIG[0], 24, 16, 100, *BIG[1:], want=_F % '128, 128, true, true', has=[C._CGF_T], blk=_one)
fwd('direct', 'fast x4 96 rows TAILS', BIG[0], 40, 0, 90, *BIG[1:], want=_F % '96, 128, true, true', has=[C._CGF_T], blk=_one)
fwd('direct', 'fast dword 128 rows unguarded', BIG[0], 32, 0, 100, *BIG[1:], want=_F % '128, 128, false, false', has=[C._CGF_F], guarded=False, blk=_one)
fwd('direct', 'fast dword 128 rows TAILS Wo=6', 310, 24, 16, 100, 9, 6, want=_F % '128, 128, true, false', has=[C._CGF_F])
fwd('direct', 'fast dword 96 rows TAILS Wo=6', 310, 40, 0, 90, 9, 6, want=_F % '96, 128, true, false', has=[C._CGF_F])
fwd('direct', 'fast x4 accumulate into a slice', BIG[0], 32, 0, 100, *BIG[1:], want=_F % '128, 128, false, true', has=[C._CGF_T], epi='acc')
fwd('direct', 'general stride 2', 3, 24, 0, 40, 16, 16, S3_S2P0, want='conv_gemm_kernel<64, 64, false, false>', has=[C._CG_FF])
fwd('direct', 'general stride 2 128 rows', 1540, 8, 0, 100, 8, 8, S3_S2P1, want='conv_gemm_kernel<128, 128, false, false>', has=[C._CG_FF], blk=_one)
fwd('direct', 'general fused upsample', 3, 24, 0, 40, 5, 7, S3_UPS, want='conv_gemm_kernel<64, 64, false, false>', has=[C._CG_FF])
fwd('direct', 'general fused upsample accumulate', 3, 24, 0, 40, 5, 7, S3_UPS, want='conv_gemm_kernel<64, 64, false, false>', has=[C._CG_FF], epi='acc')
fwd('direct', 'general two sources straddle upsample', 3, 21, 19, 40, 5, 7, S3_UPS, want='conv_gemm_kernel<64, 64, false, true>', has=[C._CG_FT])
fwd('direct', 'general two sources straddle 64x128', BIG[0], 13, 7, 40, *BIG[1:], want='conv_gemm_kernel<64, 128, false, true>', has=[C._CG_FT])
fwd('direct', 'general two sources straddle stride 2', 1540, 5, 3, 100, 8, 8, S3_S2P1, want='conv_gemm_kernel<128, 128, false, true>', has=[C._CG_FT])
fwd('direct', 'fast split-K folded == reduction', 71, 32, 0, 100, 9, 8, want=_F % '128, 128, false, true', has=[C._CGF_T, 'conv_splitk_epilogue4_kernel'], pair=True)
fwd('direct', 'fast 96 rows split-K folded == reduction', 3, 72, 0, 90, 8, 8, want=_F % '96, 128, true, true', has=[C._CGF_T], pair=True)
fwd('direct', 'fast split-K accumulate folded == reduction', 71, 32, 0, 100, 9, 8, want=_F % '128, 128, false, true', has=[C._CGF_T], epi='acc', pair=True)
fwd('direct', 'general split-K stride 2 folded == reduction', 71, 32, 0, 100, 18, 16, S3_S2P1, want='conv_gemm_kernel<128, 128, false, false>',
    has=[C._CG_FF], pair=True)
fwd('direct', 'fast split-K 18 slices reduction launch', 3, 64, 0, 100, 8, 8, want=_F % '128, 128, false, true', has=[C._CGF_T, 'conv_splitk_epilogue4_kernel'],
    blk=lambda b: b['ksplit'] == 18 and not b['tile_counters'])
fwd('direct', 'few output rows', 2, 37, 0, 4, 20, 17, want='conv_few_out_kernel', has=['conv_few_out_kernel'], epi='bias')
fwd('direct', 'few output rows 3', 3, 20, 0, 3, 12, 12, want='conv_few_out_kernel', has=['conv_few_out_kernel'], epi='bias')
dgrad('direct', 'dgrad fast 128 rows', BIG[0], 32, 100, *BIG[1:], want=_F % '128, 128, false, true', has=[C._CGF_T])
dgrad('direct', 'dgrad fast 96 rows TAILS accumulate', BIG[0], 40, 90, *BIG[1:], want=_F % '96, 128, true, true', has=[C._CGF_T], acc=True)
dgrad('direct', 'dgrad stride 2 zero-inserted', 3, 40, 24, 8, 8, S3_S2P1, in_hw=(16, 16), want='conv_gemm_kernel<64, 64, false, false>', has=[C._CG_FF])
dgrad('direct', 'dgrad stride 2 zero-inserted accumulate', 3, 40, 24, 8, 8, S3_S2P1, in_hw=(16, 16), want='conv_gemm_kernel<64, 64, false, false>',
      has=[C._CG_FF], acc=True)
dgrad_s2('dgrad stride 2 parity classes pad 0', 3, 24, 40, 5, 7, S3_S2P0, 0)
dgrad_s2('dgrad stride 2 parity classes pad 1', 2, 37, 19, 6, 6, S3_S2P1, 1)

_W0 = dict(WINO_MIN_TILES=0)
_W2 = dict(WINO_MIN_TILES=0, WINO2D_MIN_TILES=0)
fwd('winograd', 'F(2,3) fwd', 3, 32, 0, 40, 8, 8, want='conv_wino_kernel<16, 2, 1>', has=['conv_wino_kernel<16, 2>'], alg='wino1d', g=_W0, blk=_one)
fwd('winograd', 'F(2,3) fwd two sources BK 8', 3, 16, 8, 40, 8, 8, want='conv_wino_kernel<8, 2, 1>', has=['conv_wino_kernel<8, 2>'], alg='wino1d', g=_W0)
fwd('winograd', 'F(2,3) fwd 32-row tiles accumulate', 3, 32, 0, 80, 8, 8, want='conv_wino_kernel<16, 1, 1>', has=['conv_wino_kernel<16, 1>'], alg='wino1d', g=_W0,
    epi='acc')
fwd('winograd', 'F(2,3) fwd ksplit 3', 3, 128, 0, 40, 8, 8, want='conv_wino_kernel<16, 2, 1>', has=['conv_wino_kernel<16, 2>', 'conv_splitk_epilogue4_kernel'],
    alg='wino1d', g=dict(WINO_MIN_TILES=8), blk=lambda b: b['ksplit'] == 3)
dgrad('winograd', 'F(2,3) dgrad', 5, 32, 40, 4, 16, want='conv_wino_kernel<16, 2, 1>', has=['conv_wino_kernel<16, 2>'], alg='wino1d', g=_W0)
dgrad('winograd', 'F(2,3) dgrad accumulate', 5, 24, 40, 4, 16, want='conv_wino_kernel<8, 2, 1>', has=['conv_wino_kernel<8, 2>'], alg='wino1d', g=_W0, acc=True)
_K2 = 'conv_wino2d_kernel<8, 2, false>'
fwd('winograd', 'F(2x2,3x3) fwd two sources', 3, 16, 8, 40, 8, 8, want=_K2, has=[_K2], alg='wino2d', g=_W2, blk=_one)
fwd('winograd', 'F(2x2,3x3) fwd 4x4 images accumulate', 9, 8, 0, 120, 4, 4, want=_K2, has=[_K2], alg='wino2d', g=_W2, epi='acc')
dgrad('winograd', 'F(2x2,3x3) dgrad', 5, 40, 64, 4, 16, want=_K2, has=[_K2], alg='wino2d', g=_W2)
dgrad('winograd', 'F(2x2,3x3) dgrad accumulate', 5, 40, 64, 4, 16, want=_K2, has=[_K2], alg='wino2d', g=_W2, acc=True)
_K2T = 'conv_wino2d_tail_kernel<8, 2, false>'
fwd('winograd', 'F(2x2,3x3) tail fwd', 3, 16, 8, 70, 8, 8, want=_K2T, has=[_K2T], alg='wino2d', g=_W2)
dgrad('winograd', 'F(2x2,3x3) tail dgrad 6x8', 5, 40, 16, 6, 8, want=_K2T, has=[_K2T], alg='wino2d', g=_W2)
_K2M = 'conv_wino2d_m32_kernel<4, 5, false>'
fwd('winograd', 'F(2x2,3x3) m32 fwd', 2104, 8, 0, 80, 4, 4, want=_K2M, has=[_K2M], alg='wino2d')
dgrad('winograd', 'F(2x2,3x3) m32 dgrad', 4104, 8, 24, 4, 4, want=_K2M, has=[_K2M], alg='wino2d')
_K2S, _K2ST = 'conv_wino2d_kernel<4, 2, true>', 'conv_wino2d_tail_kernel<4, 2, true>'
fwd('winograd', 'F(2x2,3x3) segmented Wo 128 fwd', 2, 16, 8, 40, 2, 128, want=_K2S, has=[_K2S], alg='wino2d', g=_W2)
dgrad('winograd', 'F(2x2,3x3) segmented Wo 256 dgrad', 1, 40, 48, 4, 256, want=_K2S, has=[_K2S], alg='wino2d', g=_W2)
fwd('winograd', 'F(2x2,3x3) segmented tail fwd accumulate', 2, 16, 8, 70, 2, 128, want=_K2ST, has=[_K2ST], alg='wino2d', g=_W2, epi='acc')
fwd('winograd', 'F(2x2,3x3) ksplit', 3, 128, 0, 40, 8, 8, want=_K2, has=[_K2, 'conv_splitk_epilogue4_kernel'], alg='wino2d',
    g=dict(WINO_MIN_TILES=0, WINO2D_MIN_TILES=8), blk=lambda b: b['ksplit'] > 1)
dgrad('winograd', 'F(2x2,3x3) ksplit dgrad', 3, 128, 40, 8, 8, want=_K2, has=[_K2, 'conv_splitk_epilogue4_kernel'], alg='wino2d',
      g=dict(WINO_MIN_TILES=0, WINO2D_MIN_TILES=8), blk=lambda b: b['ksplit'] > 1)


# ======================================================================================================================
# conv_wgrad: always a fresh (NaN-filled) target and `+=` (alpha = 0.5) onto a previous gradient scaled like the row
# ======================================================================================================================
def wgrad(kind, name, N, C1, C2, Cout, H, W, sp=S3, *, want, has, lacks=(), alg='direct', g=None, blk=None, blocks=None):
    """blocks = (gate name, value): the same shape again with that many target workgroups; the split counts must differ."""
    def build(fam, e):
        return [R.conv_wgrad_case(fam, e.seed + a, N, C1 + C2, Cout, H, W, sp[0], alg, acc=bool(a), alpha=0.5) for a in (0, 1)]

    def once(ops, mp, c, acc, blk, has=has):
        spec, o = the_spec(ops, sp), c.o
        x, x2, dy = dev(o['x'][:, :C1]), (dev(o['x'][:, C1:]) if C2 else None), dev(o['dy'])
        gw = dev(o['prev']) if acc else nan_like(Cout, C1 + C2, spec.kh, spec.kw)
        call = lambda: ops.conv_wgrad(dy, x, x2, gw, spec, alpha=0.5 if acc else 1.0, accumulate=acc)
        _, names, b = one_launch(ops, mp, call, want, blk, has)
        assert not any(l in names for l in lacks), (names, lacks)
        if b['splits'] > 1:
            g2 = dev(o['prev']) if acc else nan_like(Cout, C1 + C2, spec.kh, spec.kw)
            ops.conv_wgrad(dy, x, x2, g2, spec, alpha=0.5 if acc else 1.0, accumulate=acc)
            assert torch.equal(gw, g2), 'two runs of a split weight gradient differ'
        return gw, names, b['splits']

    def run(ops, mp, cases):
        gates(ops, mp, **(g or {}))
        out = []
        for acc, c in enumerate(cases):
            gw, names, splits = once(ops, mp, c, bool(acc), blk)
            out.append((c, gw, names, dict(accumulate=bool(acc), splits=splits)))
            if blocks:
                with mp.context() as m:
                    gates(ops, m, **{blocks[0]: blocks[1]})
                    gw2, names2, splits2 = once(ops, m, c, bool(acc), None, has[:1])
                assert splits2 != splits, ('the split counts must differ', splits, splits2)
                out.append((c, gw2, names2, dict(accumulate=bool(acc), splits=splits2)))
        return out

    Entry(kind, name, build, run, has)


_MC9, _MC4 = 'splitk_reduce_taps_mc_kernel<9>', 'splitk_reduce_taps_mc_kernel<4>'
_s1, _s2 = (lambda b: b['splits'] == 1), (lambda b: b['splits'] == 2)
for nw, two, (c1, c2, co) in ((4, 'false', (40, 0, 100)), (4, 'true', (24, 16, 100)), (3, 'false', (90, 0, 90)), (3, 'true', (50, 40, 90))):
    k = 'nt_gemm_fast_kernel<%d, %s>' % (nw, two)
    wgrad('wgrad', k + ' one slice', 3, c1, c2, co, 8, 8, want=k, has=[k], lacks=[_MC9], blk=_s1)
    wgrad('wgrad', k + ' two slices', 5, c1, c2, co, 8, 8, want=k, has=[k, _MC9], blk=_s2)
wgrad('wgrad', 'nt_gemm_fast 1x1 at 4x4', 6, 40, 0, 100, 4, 4, S1, want='nt_gemm_fast_kernel<4, false>', has=['nt_gemm_fast_kernel<4, false>'])
wgrad('wgrad', 'nt_gemm 6x6 one slice', 3, 40, 0, 100, 6, 6, want='nt_gemm_kernel<128, 128, false, false>', has=[C._NT_F], blk=_s1)
wgrad('wgrad', 'nt_gemm 6x6 two sources straddle', 3, 21, 19, 40, 6, 6, want='nt_gemm_kernel<64, 128, true, false>', has=[C._NT_T])
wgrad('wgrad', 'nt_gemm splits taps_mc<9>', 8, 40, 0, 100, 6, 6, want='nt_gemm_kernel<128, 128, false, false>', has=[C._NT_F, _MC9], blk=_s2)
wgrad('wgrad', 'nt_gemm splits taps_mc<4>', 8, 20, 0, 40, 6, 6, S2_CLASS1, want='nt_gemm_kernel<64, 128, false, false>', has=[C._NT_F, _MC4], blk=_s2)
wgrad('wgrad', 'nt_gemm splits taps 1x1', 8, 40, 0, 100, 6, 6, S1, want='nt_gemm_kernel<128, 128, false, false>', has=[C._NT_F, 'splitk_reduce_taps_kernel'], blk=_s2)
wgrad('wgrad', 'nt_gemm splits taps 5x5', 8, 20, 0, 40, 6, 6, S5, want='nt_gemm_kernel<64, 128, false, false>', has=[C._NT_F, 'splitk_reduce_taps_kernel'], blk=_s2)
_MG = 'nt_gemm_kernel<64, 64, false, true>'
wgrad('wgrad', 'merge 1 one slice', 3, 3, 0, 40, 8, 8, want=_MG, has=[C._NT_M], blk=lambda b: b['merge'] == 1 and b['splits'] == 1)
wgrad('wgrad', 'merge 1 two slices', 5, 3, 0, 40, 8, 8, want=_MG, has=[C._NT_M, 'splitk_reduce_kernel'], blk=lambda b: b['merge'] == 1 and b['splits'] == 2)
wgrad('wgrad', 'merge 1 stride 2', 3, 4, 0, 70, 16, 16, S3_S2P0, want=_MG, has=[C._NT_M], blk=lambda b: b['merge'] == 1)
wgrad('wgrad', 'merge 3 one slice', 3, 40, 0, 3, 8, 8, want=_MG, has=[C._NT_M], blk=lambda b: b['merge'] == 3 and b['splits'] == 1)
wgrad('wgrad', 'merge 3 two slices', 5, 40, 0, 3, 8, 8, want=_MG, has=[C._NT_M, 'splitk_reduce_kernel'], blk=lambda b: b['merge'] == 3 and b['splits'] == 2)
wgrad('wgrad', 'merge 3 5x7 images', 3, 70, 0, 7, 5, 7, want=_MG, has=[C._NT_M], blk=lambda b: b['merge'] == 3)

_GW = dict(WGRAD_WINO_MIN_WORK=0, WGRAD_WINO_MIN_FILL=0.0, WGRAD_WINO2D=False)
for bt, (c1, c2, co) in ((2, (40, 0, 70)), (3, (90, 0, 96))):
    k = 'wgrad_wino_kernel<%d, %d>' % (bt, bt)
    wgrad('winograd', 'F(3,2) wgrad %d one slice' % bt, 2, c1, c2, co, 8, 8, want=k, has=[k], alg='wino1d', g=_GW, blk=_s1)
    wgrad('winograd', 'F(3,2) wgrad %d slices' % bt, 5, c1, c2, co, 4, 16, want=k, has=[k, _MC9], alg='wino1d', g=_GW, blk=lambda b: b['splits'] > 1)
wgrad('winograd', 'F(3,2) wgrad 2 two sources', 2, 64, 24, 70, 8, 8, want='wgrad_wino_kernel<2, 2>', has=['wgrad_wino_kernel<2, 2>'], alg='wino1d', g=_GW)
_GW2 = dict(WGRAD_WINO_MIN_WORK=0, WGRAD_WINO_MIN_FILL=0.0, WGRAD_WINO2D_MIN_FILL=0.0)
for lw, (h, w_) in ((5, (2, 32)), (4, (4, 16)), (3, (8, 8))):
    for tail, co in ((True, 70), (False, 40)):
        k = 'wgrad_wino2d_%skernel<%d>' % ('tail_' if tail else '', lw)
        wgrad('winograd', 'F(3x3,2x2) %s one source' % k, 3, 40, 0, co, h, w_, want=k, has=[k], alg='wino2d', g=_GW2, blk=_s1)
        # 9 images: 9 K tiles of 64 pixels -> 2 slices with the default 512 target workgroups, one slice with a target of one
        wgrad('winograd', 'F(3x3,2x2) %s two sources, several slices and one' % k, 9, 32, 24, co, h, w_, want=k, has=[k, _MC9], alg='wino2d', g=_GW2,
              blk=lambda b: b['splits'] > 1, blocks=('WGRAD_WINO2D_BLOCKS', 1))


# ======================================================================================================================
# linear and bmm
# ======================================================================================================================
def linear(name, what, N, Ci, Co, *, has, acc=False, blk=None, names_are=None):
    def build(fam, e):
        return [R.linear_case(fam, e.seed, what, N, Ci, Co, alpha=0.5 if what == 'wgrad' else 1.0, acc=acc)]

    def run(ops, mp, cases):
        o = cases[0].o
        if what == 'fwd':
            x, w, b = dev(o['x']), dev(o['w']), dev(o['b'].flatten())
            poison(N * Co)
            y, names, seen = launched_m(ops, mp, lambda: ops.linear_forward(x, w, b))
            assert torch.equal(y, ops.linear_forward(x, w, b)), 'two runs differ'
        elif what == 'dgrad':
            dy, w = dev(o['dy']), dev(o['w'])
            poison(N * Ci)
            if acc:
                y = dev(o['prev'])
                _, names, seen = launched_m(ops, mp, lambda: ops.linear_dgrad(dy, w, out=y, accumulate=True))
            else:
                y, names, seen = launched_m(ops, mp, lambda: ops.linear_dgrad(dy, w))
        else:
            dy, x, y = dev(o['dy']), dev(o['x']), dev(o['prev'])
            _, names, seen = launched_m(ops, mp, lambda: ops.linear_wgrad(dy, x, y, alpha=0.5, accumulate=True))
        assert all(h in names for h in has) and (blk is None or blk(seen[0][1])), (names, seen)
        assert names_are is None or names == names_are, names
        return [(cases[0], y, names, {})]

    Entry('linear_bmm', name, build, run, has)


def bmm(name, which, Z, M, K, Nn, *, want, has, blk=None):
    """A fresh output (alpha = 0.25; nt: + col_bias), then tn / nn: accumulate (alpha = 0.5) into a row slice of a wider buffer."""
    def build(fam, e):
        return [R.bmm_case(fam, e.seed, which, Z, M, K, Nn, 0.25, col_bias=which == 'nt')] + (
            [R.bmm_case(fam, e.seed + 1, which, Z, M, K, Nn, 0.5, acc=True)] if which != 'nt' else [])

    def run(ops, mp, cases):
        fn, out = getattr(ops, 'bmm_' + which), []
        a, b = dev(cases[0].o['a']), dev(cases[0].o['b'])
        extra = dict(col_bias=dev(cases[0].o['cb'].flatten())) if which == 'nt' else {}
        poison(Z * M * Nn)
        y, names, _ = one_launch(ops, mp, lambda: fn(a, b, alpha=0.25, **extra), want, blk, has)
        out.append((cases[0], y, names, {}))
        if which != 'nt':
            a, b = dev(cases[1].o['a']), dev(cases[1].o['b'])
            big = D.rnd(Z, M + 5, Nn, seed=4)
            view = big[:, 2:2 + M]
            view.copy_(dev(cases[1].o['prev']))
            before = big.clone()
            _, names, _ = one_launch(ops, mp, lambda: fn(a, b, alpha=0.5, out=view, accumulate=True), want, None, has)
            assert outside_intact(big, before, 2, M)
            out.append((cases[1], view.clone(), names, dict(accumulate=True)))
        return out

    Entry('linear_bmm', name, build, run, has)


linear('linear_forward one slice', 'fwd', 33, 37, 92, has=[C._NT_F], blk=lambda b: b['col_bias'] and b['splits'] == 1, names_are=[C._NT_F])
linear('linear_forward three slices', 'fwd', 7, 200, 90, has=[C._NT_F, 'splitk_reduce_kernel'], blk=lambda b: b['col_bias'] and b['splits'] > 1)
linear('linear_forward 520 features', 'fwd', 70, 520, 33, has=[C._NT_F, 'splitk_reduce_kernel'], blk=lambda b: b['col_bias'] and b['splits'] > 1)
linear('linear_dgrad split K', 'dgrad', 70, 90, 100, has=[C._CG_TF], blk=lambda b: b['ksplit'] > 1 and b['a_kc'] == 1 and not b['accumulate'])
linear('linear_dgrad split K accumulate', 'dgrad', 70, 90, 100, has=[C._CG_TF], acc=True, blk=lambda b: b['ksplit'] > 1 and b['accumulate'] == 1)
linear('linear_wgrad bmm_tn', 'wgrad', 33, 37, 92, has=[C._CG_FF], blk=lambda b: b['accumulate'] == 1)
linear('linear_wgrad nt_gemm odd Co', 'wgrad', 33, 92, 37, has=[C._NT_F], blk=lambda b: b['accumulate'] == 1)
bmm('bmm_tn fast 200 products', 'tn', 200, 100, 20, 120, want=_F % '128, 128, true, true', has=[C._CGF_T], blk=lambda b: b['batches'] == 200)
bmm('bmm_tn general', 'tn', 3, 52, 41, 37, want='conv_gemm_kernel<64, 64, false, false>', has=[C._CG_FF])
bmm('bmm_nn', 'nn', 3, 50, 41, 37, want='conv_gemm_kernel<64, 64, true, false>', has=[C._CG_TF], blk=lambda b: b['a_kc'] == 1)
bmm('bmm_nn 200 products', 'nn', 200, 100, 20, 120, want='conv_gemm_kernel<128, 128, true, false>', has=[C._CG_TF])
bmm('bmm_nt', 'nt', 3, 50, 41, 37, want='nt_gemm_kernel<64, 64, false, false>', has=[C._NT_F], blk=lambda b: b['batched'] == 1)
bmm('bmm_nt 200 products', 'nt', 200, 100, 20, 120, want='nt_gemm_kernel<128, 128, false, false>', has=[C._NT_F])


# ======================================================================================================================
# the nine-product kernels
# ======================================================================================================================
def ups9_fwd(name, N, Cin, Cout, H, W, bias):
    def build(fam, e):
        return [R.conv_fwd_case(fam, e.seed, N, Cin, Cout, H, W, R.UPS3, 'ups9', 'bias' if bias else 'none')]

    def run(ops, mp, cases):
        o = cases[0].o
        x, w = guarded_act(ops, dev(o['x'])), dev(o['w'])
        up, ldu = ops.pack_weight(ops.ups9_u(w), 0)
        b = dev(o['bias'].flatten()) if bias else None
        poison(N * Cout * 4 * H * W)
        y, names, seen = launched_m(ops, mp, lambda: ops.ups9_fwd(x, up, ldu, Cout, bias=b))
        assert names == [C._U9F] and bool(seen[0][1]['bias']) == bias, (names, seen)
        assert torch.equal(y, ops.ups9_fwd(x, up, ldu, Cout, bias=b))
        return [(cases[0], y, names, dict(bias=bias))]

    Entry('ups9', name, build, run, [C._U9F])


def ups9_dgrad(name, N, Cin, Cout, H, W, tile):
    def build(fam, e):
        return [R.conv_dgrad_case(fam, e.seed + a, N, Cout, Cin, 2 * H, 2 * W, R.UPS3, 'ups9', in_hw=(2 * H, 2 * W), acc=bool(a), lowres=True) for a in (0, 1)]

    def run(ops, mp, cases):
        out = []
        for acc, c in enumerate(cases):
            dy, w = guarded_act(ops, dev(c.o['dy'])), dev(c.o['w'])
            up, ldu = ops.pack_weight(ops.ups9_u(w), 1)
            poison(N * Cin * H * W)
            if acc:
                view, big = wide(N, Cin, H, W, 3)
                view.copy_(dev(c.o['prev']))
                before = big.clone()
                _, names, _ = launched_m(ops, mp, lambda: ops.ups9_dgrad(dy, up, ldu, Cin, out=view, accumulate=True, tile=tile))
                assert outside_intact(big, before, 2, Cin)
                y = view.clone()
            else:
                y, names, _ = launched_m(ops, mp, lambda: ops.ups9_dgrad(dy, up, ldu, Cin, tile=tile))
            assert names == [C._U9D[tile]], names
            out.append((c, y, names, dict(accumulate=bool(acc), tile=tile)))
        return out

    Entry('ups9', name, build, run, [C._U9D[tile]])


def ups9_wgrad(name, N, Cin, Cout, H, W):
    """One slice and several (the caller's count), a fresh target and `+=`."""
    def build(fam, e):
        return [R.conv_wgrad_case(fam, e.seed + a, N, Cin, Cout, H, W, R.UPS3, 'ups9', acc=bool(a)) for a in (0, 1)]

    def run(ops, mp, cases):
        out, counts = [], set()
        for acc, c in enumerate(cases):
            dy, x = guarded_act(ops, dev(c.o['dy'])), guarded_act(ops, dev(c.o['x']))
            for splits in (1, -(-N * H * W // 16)):               # one slice, and one per 16-pixel K tile
                assert ops.ups9_wgrad_splits(N, Cin, Cout, H, W, splits)[0] == splits
                counts.add(splits)
                gw = dev(c.o['prev']) if acc else nan_like(Cout, Cin, 3, 3)
                _, names = launched(ops, lambda: ops.ups9_wgrad(dy, x, gw, accumulate=bool(acc), splits=splits))
                assert names == ['ups9_wgrad_kernel', 'ups9_wgrad_reduce_kernel'], names
                out.append((c, gw, names, dict(accumulate=bool(acc), splits=splits)))
        assert len(counts) == 2
        return out

    Entry('ups9', name, build, run, ['ups9_wgrad_kernel', 'ups9_wgrad_reduce_kernel'])


for _n, _ci, _co, _h, _w in ((5, 20, 36, 4, 4), (2, 7, 5, 5, 3), (1, 130, 130, 4, 4)):
    for _b in (False, True):
        ups9_fwd('ups9_fwd %dx%d->%d %dx%d%s' % (_n, _ci, _co, _h, _w, ' bias' if _b else ''), _n, _ci, _co, _h, _w, _b)
for _t in (0, 1, 2):
    for _n, _ci, _co, _h, _w in ((3, 16, 40, 4, 4), (2, 20, 7, 5, 3), (2, 130, 24, 4, 4)):
        ups9_dgrad('ups9_dgrad tile %d %dx%d<-%d %dx%d' % (_t, _n, _ci, _co, _h, _w), _n, _ci, _co, _h, _w, _t)
for _n, _ci, _co, _h, _w in ((5, 20, 36, 4, 4), (4, 7, 5, 5, 3), (3, 70, 130, 4, 4)):
    ups9_wgrad('ups9_wgrad %dx%d->%d %dx%d' % (_n, _ci, _co, _h, _w), _n, _ci, _co, _h, _w)


# ======================================================================================================================
# attention
# ======================================================================================================================
def attention(name, kernel, nt, variant, N, heads, d, dv, H, W):
    def build(fam, e):
        return [R.attention_case(fam, e.seed, N, heads, d, dv, H, W)]

    def run(ops, mp, cases):
        assert (-(-max(d, dv) // 32) + 3) // 4 == nt
        q, k, v = (dev(cases[0].o[n]) for n in 'qkv')
        poison(N * heads * dv * H * W)
        y, names, _ = launched_m(ops, mp, lambda: ops.attention_fwd(q, k, v, heads, float(d) ** -0.5, variant=variant))
        assert names == ['attn_fwd_%s_kernel<%d>' % (kernel, nt)], names
        return [(cases[0], y, names, dict(variant=variant))]

    Entry('attention', name, build, run, ['attn_fwd_%s_kernel<%d>' % (kernel, nt)])


attention('attention pipe NT 1', 'pipe', 1, 0, 2, 2, 32, 24, 4, 8)
attention('attention pipe NT 1 odd width 96 tokens', 'pipe', 1, 0, 1, 1, 33, 40, 8, 12)
attention('attention fused NT 1', 'fused', 1, 1, 2, 2, 32, 24, 4, 8)
attention('attention fused NT 1 odd width 96 tokens', 'fused', 1, 1, 1, 1, 33, 40, 8, 12)
attention('attention pipe pruned widths 179 / 133', 'pipe', 2, 0, 2, 1, 179, 133, 8, 12)
attention('attention fused pruned widths 179 / 133', 'fused', 2, 1, 2, 1, 179, 133, 8, 12)


# ======================================================================================================================
# importance.hip
# ======================================================================================================================
def wg(name, shape, dim, mode, acc):
    ring = ['wg_gn_kernel'] if mode == 3 else ['wg_rows_kernel'] if dim == 0 else ['wg_cols_ct_kernel', 'wg_fold_taps_kernel']

    def build(fam, e):
        return [R.wg_case(fam, e.seed, shape, dim, mode, acc)]

    def run(ops, mp, cases):
        o = cases[0].o
        w, g = dev(o['w']), dev(o['g'])
        out = dev(o['prev']) if acc else nan_like(shape[0 if mode == 3 else dim])
        _, names = launched(ops, lambda: ops.wg_reduce(w, g, dim, mode, out, acc))
        assert names == ring, names
        return [(cases[0], out, names, dict(mode=mode, dim=dim, accumulate=acc))]

    Entry('importance', name, build, run, ring)


for _mode in (0, 1, 2, 4, 5):
    for _dim in (0, 1):
        wg('wg_reduce mode %d dim %d 3x3' % (_mode, _dim), (70, 37, 3, 3), _dim, _mode, (_mode + _dim) % 2 == 1)
        wg('wg_reduce mode %d dim %d linear' % (_mode, _dim), (50, 64) if _dim == 0 else (3, 300), _dim, _mode, (_mode + _dim) % 2 == 0)
wg('wg_reduce mode 3', (96,), 0, 3, False)
wg('wg_reduce mode 3 accumulate', (1000,), 0, 3, True)


def _lay_out(cases):
    table, out = importlib.import_module('diff-pruning_amd.pruning')._MemberTable(), []
    for c in cases:
        n0 = c.shape[0]
        ms = table.add([(dev(c.o['w%d' % i]), dev(c.o['g%d' % i]), shape[0], shape[1] if len(shape) > 1 else 1,
                         shape[2] * shape[3] if len(shape) > 2 else 1, dim, (mode,), idxs if idxs is not None else list(range(n0)))
                        for i, (shape, dim, mode, idxs) in enumerate(c.members)], n0)
        assert ms is not None and [m['idx_off'] >= 0 for m in ms] == [m[3] is not None for m in c.members]
        out.append((ms, n0))
    return out, table.index_tensor(), table.need


def group(name, sizes, all_groups):
    """ops.group_score on one group, or ops.score_groups on several in one launch pair; 25 and 53 members are two and three chunks of 24."""
    ring = ['pg_score_part_kernel', 'pg_score_combine_kernel'] if all_groups else ['group_score_part_kernel', 'group_score_combine_kernel']

    def build(fam, e):
        return [R.group_case(fam, e.seed + i, n0, n) for i, (n0, n) in enumerate(sizes)]

    def run(ops, mp, cases):
        laid, idx, need = _lay_out(cases)
        scratch = torch.full((max(need, 1),), float('nan'), device=D.DEV)
        total = sum(n0 for _, n0 in laid)
        scores = torch.full((total,), float('nan'), device=D.DEV)
        if all_groups:
            _, names = launched(ops, lambda: ops.score_groups(laid, idx, scratch, scores))
            assert names == ring, names
        else:
            _, names = launched(ops, lambda: ops.group_score(laid[0][0], laid[0][1], idx, scratch, scores))
            assert names == ring * ((len(laid[0][0]) + 23) // 24), names
        out, off = [], 0
        for c, (_, n0) in zip(cases, laid):
            out.append((c, scores[off:off + n0].clone(), names, dict(members=len(c.members))))
            off += n0
        return out

    Entry('importance', name, build, run, ring)


group('group_score 7 members', [(48, 7)], False)
group('group_score 25 members', [(48, 25)], False)
group('group_score 53 members', [(48, 53)], False)
group('score_groups three groups', [(48, 25), (40, 7), (65, 31)], True)


# ======================================================================================================================
# the tests: one per operation kind, over the entries of the kind and the four families
# ======================================================================================================================
def check(entry, family, ops, report, mp, lines):
    cases = entry.build(family, entry)
    bad, seen_names = [], []
    for case, got, names, extra in entry.run(ops, mp, cases):
        torch.cuda.synchronize()
        fig = dict(case.figures(got), names=names, **extra)
        seen_names += names
        line = '%-62s %-20s %-18s e_hip %9.3f  e_ref32 %8.3f  e_alg32 %8.3f  bound %9.3f  maxnorm %.2e  %s %s %s' % (
            entry.name, family, case.kind, fig['e_hip'] / R.EPS, fig['e_ref32'] / R.EPS, fig['e_alg32'] / R.EPS, fig['bound'] / R.EPS, fig['maxnorm'],
            'x'.join(str(s) for s in case.shape[:6]), ' '.join('%s=%s' % kv for kv in sorted(extra.items())), '+'.join(dict.fromkeys(names)))
        print(line)
        lines.append(line)
        try:
            with open(OUT, 'a') as f:
                f.write(line + '\n')
        except OSError:
            pass
        report.setdefault('rowwise/%s/%s' % (entry.name, family), []).append({k: (list(v) if isinstance(v, tuple) else v) for k, v in fig.items()})
        if not fig['e_hip'] <= fig['bound']:
            bad.append(fig)
    assert all(h in seen_names for h in entry.has), (entry.has, seen_names)
    torch.cuda.empty_cache()
    assert not bad, bad


def _make(kind):
    ents = [e for e in TABLE if e.kind == kind]

    @pytest.mark.parametrize('family', R.FAMILIES)
    @pytest.mark.parametrize('entry', ents, ids=[e.name.replace(' ', '_') for e in ents])
    def test(entry, family, ops, report, monkeypatch, record):
        check(entry, family, ops, report, monkeypatch, record)
    test.__name__ = test.__qualname__ = 'test_rowwise_' + kind
    return test


test_rowwise_direct = _make('direct')
test_rowwise_wgrad = _make('wgrad')
test_rowwise_linear_bmm = _make('linear_bmm')
test_rowwise_winograd = _make('winograd')
test_rowwise_ups9 = _make('ups9')
test_rowwise_attention = _make('attention')
test_rowwise_importance = _make('importance')


def test_every_listed_form_has_an_entry():
    """Every entry asserts the ring names of its `has` in the launches it saw; together they hold every form this file is to cover."""
    held = {h for e in TABLE for h in e.has}
    assert not [n for n in LISTED if n not in held], [n for n in LISTED if n not in held]
    assert held <= C.KNOWN | D.KNOWN | {'ups9_wgrad_kernel', 'ups9_wgrad_reduce_kernel', 'pg_score_part_kernel', 'pg_score_combine_kernel'}, \
        sorted(held - C.KNOWN - D.KNOWN)
