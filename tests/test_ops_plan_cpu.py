"""Launch plans of ops.py's contraction dispatch, pinned field by field (no GPU).

With six module-level names of `ops` stubbed (`_lib`, `_stream`, `_chk_act`, `_run`, `_workspace`, `_tile_counters`) the whole host
side of a contraction launch runs on CPU tensors: the entry point fills its parameter block, chooses tiles and split counts, asks
the `*_supported` shape rules (host code of the real library), names the launch and hands the block to the launcher.  The recorder
below writes down every one of these steps; tests/golden/ops_launch_plans.json holds what the case table produced when the
fixture was written (tests/golden/make_ops_plans.py), and the test compares for exact equality.  A change of the dispatch that
moves one field of one parameter block, one split count, one launch name or one flop figure fails here, naming the case.

One `*_supported` answer cannot be produced through the dispatch, because the Python pre-checks mirror the native rule
completely (dp_wgrad_wino2d_supported answering zero) -- the `probe_*` case asks the fake library directly with a hand-made
block, as test_cpu.py::test_winograd_refuses_activations_within_a_row_of_2gib does with the real one."""
import contextlib
import ctypes
import json
import os
import re

import pytest
import torch

from helpers import GOLD, pkg

FIXTURE = os.path.join(GOLD, 'ops_launch_plans.json')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENV = ('DP_WINO2D_VARIANT', 'DP_WINO2D_M32', 'DP_WINO2D_TAIL', 'DP_NO_XCD', 'DP_NO_FAST', 'DP_NO_X4')


# ---------------------------------------------------------------------------------------------------------------------------
# the recorder
# ---------------------------------------------------------------------------------------------------------------------------
class Recorder:
    """Records of one case, in order.  Parameter blocks are stored once each in `blocks` (shared by all cases) and referred to by
    ['B', structure name, index]: the same block goes to `*_supported` and to the launcher."""

    def __init__(self, blocks):
        self.blocks, self.index, self.rec = blocks, {json.dumps(b): i for i, b in enumerate(blocks)}, []

    def struct(self, s):
        """Every _fields_ entry in order: numbers by value, pointers as null (False) / non-null (True), nested structures as lists."""
        out = []
        for name, ctype in s._fields_:
            v = getattr(s, name)
            if isinstance(v, ctypes.Structure):
                out.append(self.struct(v))
            elif ctype is ctypes.c_void_p:
                out.append(bool(v))
            else:
                out.append(v)
        return out

    def arg(self, a):
        obj = getattr(a, '_obj', None)                    # ctypes.byref(structure)
        if isinstance(obj, ctypes.Structure):
            b = self.struct(obj)
            key = json.dumps(b)
            if key not in self.index:
                self.index[key] = len(self.blocks)
                self.blocks.append(b)
            return ['B', type(obj).__name__, self.index[key]]
        if a is None or isinstance(a, ctypes.c_void_p):
            return bool(a)                                # a pointer: null or not
        assert isinstance(a, (int, float)), type(a)
        return a


class FakeLib:
    """Stands in for the loaded library: every symbol is recorded with its arguments and answers 0, except the `*_supported` shape
    rules, which are host code and are forwarded to the real library."""

    def __init__(self, recorder, real):
        self._r, self._real = recorder, real

    def __getattr__(self, name):
        r, real = self._r, self._real

        def call(*args):
            row = ['lib', name, [r.arg(a) for a in args]]
            ret = 0
            if name.endswith('_supported'):
                ret = int(getattr(real, name)(*args))
                row.append(ret)
            r.rec.append(row)
            return ret
        return call


def _chk_act_cpu(x):
    """ops._chk_act without the is_cuda assert."""
    assert x.dtype == torch.float32 and x.dim() == 4, 'activation must be a 4-D fp32 tensor'
    N, Cc, H, W = x.shape
    assert x.stride(3) == 1 or W == 1
    assert (x.stride(2) == W or H == 1) and (x.stride(1) == H * W or Cc == 1), 'inner strides must be contiguous'
    return x.stride(0) if N > 1 else Cc * H * W


@contextlib.contextmanager
def recording(ops, blocks, patch=None, record=True, const_lib=None):
    """Stub the six names on the real `ops` module (plus the constants of `patch`), delete the environment switches the dispatch
    reads at call time, and restore everything afterwards.  record=False / const_lib: the stubs without the bookkeeping, for
    timing the dispatch (tests/golden/make_ops_plans.py --time)."""
    r = Recorder(blocks)
    real_lib, real_run = pkg('_lib').load(), ops._run
    fake = const_lib if const_lib is not None else FakeLib(r, real_lib)
    one = torch.empty(1, dtype=torch.float32)
    null = ctypes.c_void_p(None)

    def run(call, name, flops, abytes=0.0):
        if record:
            held = sorted(type(c.cell_contents).__name__ for c in (call.__closure__ or ())
                          if isinstance(c.cell_contents, ctypes.Structure))
            r.rec.append(['run', name, flops, abytes, held])          # held: the parameter block the launch closure keeps
        return real_run(call, name, flops, abytes)

    def workspace(n, device):
        if record:
            r.rec.append(['ws', n])
        return one

    def tile_counters(n, device):
        if record:
            r.rec.append(['tc', n])
        return one

    stubs = dict(_lib=lambda: fake, _stream=lambda: null, _chk_act=_chk_act_cpu, _run=run, _workspace=workspace,
                 _tile_counters=tile_counters, _prof=None)
    stubs.update(patch or {})
    saved = {k: getattr(ops, k) for k in stubs}
    env = {k: os.environ.pop(k) for k in ENV if k in os.environ}
    try:
        for k, v in stubs.items():
            setattr(ops, k, v)
        yield r
    finally:
        for k, v in saved.items():
            setattr(ops, k, v)
        os.environ.update(env)


# ---------------------------------------------------------------------------------------------------------------------------
# operands (uninitialised CPU memory: nothing reads them, so full-size shapes cost address space only)
# ---------------------------------------------------------------------------------------------------------------------------
def _r4(n):
    return (n + 3) & ~3


def _wino_operand(kind, K, cols):
    """What pack_weight_wino / _wino2d / _wino43 return for K contraction channels and `cols` output rows, as conv_forward's and
    conv_dgrad's `wino` / `wino43` argument."""
    ld = _r4(cols)
    U = torch.empty({'1d': 12, '2d': 16, '43': 18}[kind] * K * ld)
    return ('2d', U, ld) if kind == '2d' else (U, ld)


def _fwd(ops, N, C1, H, W, Cout, spec=None, C2=0, wino=None, wino43=False, guard=True, img_stride=None, opts=(), **kw):
    spec = spec or ops.ConvSpec(3, 1, 1, 0)
    act = (lambda s: ops.empty_act(s, 'cpu')) if guard else (lambda s: torch.empty(s))
    if img_stride is None:
        x = act((N, C1, H, W))
    else:                                                  # images img_stride floats apart (a slice of a wider buffer)
        x = act((N, 1, 1, img_stride)).view(N, img_stride)[:, :C1 * H * W].view(N, C1, H, W)
    x2 = act((N, C2, H, W)) if C2 else None
    Cin, ld = C1 + C2, _r4(Cout)
    wp = torch.empty(spec.kh * spec.kw * Cin * ld)
    Ho, Wo = spec.out_hw(H, W)
    if 'bias' in opts:
        kw['bias'] = torch.empty(Cout)
    if 'tadd' in opts:
        kw['tadd'] = torch.empty(N, Cout)
    if 'res' in opts:
        kw['res'] = ops.empty_act((N, Cout, Ho, Wo), 'cpu')
    if 'accumulate' in opts:
        kw.update(out=ops.empty_act((N, Cout, Ho, Wo), 'cpu'), accumulate=True)
    if wino:
        kw['wino'] = _wino_operand(wino, Cin, Cout)
    if wino43:
        kw['wino43'] = _wino_operand('43', Cin, Cout)
    ops.conv_forward(x, x2, wp, ld, Cout, spec, **kw)


def _dgrad(ops, N, Cout, Ho, Wo, Cin, spec=None, wino=None, **kw):
    spec = spec or ops.ConvSpec(3, 1, 1, 0)
    dy = ops.empty_act((N, Cout, Ho, Wo), 'cpu')
    ldd = _r4(Cin)
    wd = torch.empty(spec.kh * spec.kw * Cout * ldd)
    in_hw = (Ho, Wo) if spec.stride == 1 else (2 * Ho, 2 * Wo)
    if wino:
        kw['wino'] = _wino_operand(wino, Cout, Cin)
    ops.conv_dgrad(dy, wd, ldd, Cin, spec, in_hw, **kw)


def _dgrad_s2(ops, N, Cout, Ho, Wo, Cin, pad, add=False):
    spec = ops.ConvSpec(3, 2, pad, 0)
    dy = ops.empty_act((N, Cout, Ho, Wo), 'cpu')
    ldd = _r4(Cin)
    packs = [(torch.empty(len(ops._s2_taps(ph, pad)[0]) * len(ops._s2_taps(pw, pad)[0]) * Cout * ldd), ldd)
             for ph in (0, 1) for pw in (0, 1)]
    ops.conv_dgrad_s2(dy, packs, Cin, spec, (2 * Ho, 2 * Wo), ops.empty_act((N, Cin, 2 * Ho, 2 * Wo), 'cpu') if add else None)


def _wgrad(ops, N, Cout, H, W, C1, spec=None, C2=0, **kw):
    spec = spec or ops.ConvSpec(3, 1, 1, 0)
    Ho, Wo = spec.out_hw(H, W)
    dy = ops.empty_act((N, Cout, Ho, Wo), 'cpu')
    x = ops.empty_act((N, C1, H, W), 'cpu')
    x2 = ops.empty_act((N, C2, H, W), 'cpu') if C2 else None
    gw = torch.empty(Cout, C1 + C2, spec.kh, spec.kw)
    ops.conv_wgrad(dy, x, x2, gw, spec, **kw)


def _ups9(ops, N, Cout, H, W, Cin, ldu=None):
    ldu = _r4(Cin) if ldu is None else ldu
    dy = ops.empty_act((N, Cout, 2 * H, 2 * W), 'cpu')
    try:
        ops.ups9_dgrad(dy, torch.empty(9 * Cout * max(ldu, 1)), ldu, Cin)
        return 'launched'
    except ValueError as e:
        return 'ValueError: %s' % e


def _probe_wgrad_wino2d(ops, P):
    """dp_wgrad_wino2d_supported on a block the dispatch cannot build (P no multiple of 64: conv_wgrad asks P % 64 first)."""
    L = pkg('_lib')
    p = L.NtGemmParams()
    p.g = ops._geom(16, 16, 16, 16, 16, 16, 3, 1, 1, 1, 1, 0, 64, 64 * 256, 0)
    p.M, p.C, p.NCOLS, p.ntaps, p.P = 64, 64, 64, 9, P
    p.batches, p.splits, p.p_per_split, p.tile = 1, 1, 256, 0
    p.a_bytes, p.x1_bytes = 4 << 20, 4 << 20
    return ops._lib().dp_wgrad_wino2d_supported(ctypes.byref(p))


def _mm(*shape):
    return torch.empty(shape)


def _wanted_grid(ops, fn):
    """One character per (spec, M, C_sources, N, (H, W)) in this order: the grid straddles the shape rules (W < 4, W > 256, W no power
    of two, odd H, odd H * W, H * W % 4, channel multiples of 8 / 16, M < 16), the row-fill rule (M = 40, 44, 45 against 0.7 of a 64-row
    tile; 96 = a tail tile) and the grid rule (>= 512 tiles; split-K with >= 2 slices of 8 K tiles giving >= 256 workgroups), and
    holds every case of test_cpu.py::test_winograd_dispatch_rules."""
    S = ops.ConvSpec
    specs = (S(3, 1, 1, 0), S(1, 1, 0, 0), S(3, 2, 0, 0), S(3, 1, 1, 1), S(3, 1, 0, 0), S.same(2, 2, 1, 1), S.general(3, 3, 1, 1, 1),
             S.general(1, 7, 1, 0, 3))
    Ms = (3, 15, 16, 40, 44, 45, 64, 90, 96, 128, 179, 256, 576)
    Cs = ((3,), (8,), (16,), (24,), (96,), (128,), (179,), (256,), (576,), (256, 128), (72, 56), (64, 3))
    Ns = (1, 4, 12, 128, 256)
    HWs = ((2, 2), (4, 4), (3, 4), (5, 5), (8, 8), (16, 16), (32, 32), (2, 6), (256, 256), (512, 512))
    out = []
    for si, spec in enumerate(specs):
        for M in (Ms if si == 0 else (128,)):
            for Cc in (Cs if si == 0 else ((128,), (256, 128))):
                for N in (Ns if si == 0 else (256,)):
                    out.append(''.join('1' if fn(M, Cc, N, H, W, spec) else '0' for H, W in HWs))
    # the literal cases of test_winograd_dispatch_rules
    S3 = specs[0]
    rules = ((128, (128,), 256, 32, 32, S3), (128, (256, 128), 256, 32, 32, S3), (256, (256,), 256, 4, 4, S3), (128, (128,), 4, 32, 32, S3),
             (128, (3,), 256, 32, 32, S3), (256, (256,), 256, 16, 16, specs[1]), (128, (128,), 256, 32, 32, specs[2]),
             (179, (179,), 128, 16, 16, S3), (90, (96,), 128, 32, 32, S3), (3, (128,), 256, 32, 32, S3), (128, (128,), 4, 256, 256, S3),
             (128, (128,), 4, 512, 512, S3), (576, (576,), 12, 16, 16, S3))
    out.append(''.join('1' if fn(*a) else '0' for a in rules))
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# the case table: name -> (callable(ops) [its return value is recorded unless None or a tensor], constants to patch)
# ---------------------------------------------------------------------------------------------------------------------------
def cases(ops):
    S = ops.ConvSpec
    S1 = S(1, 1, 0, 0)
    W43, W43_SPLIT = dict(WINO43=True, WINO43_MIN_TILES=0), dict(WINO43=True)
    NOWORK = dict(WGRAD_WINO_MIN_WORK=0)
    t = {}
    # ---- conv_forward, direct form
    t['fwd/fast128'] = lambda: _fwd(ops, 256, 128, 32, 32, 128)                     # conv_gemm_fast_kernel<128, 128, false, true>
    t['fwd/fast128_tails'] = lambda: _fwd(ops, 256, 90, 32, 32, 128)                # C % 16 != 0: <128, 128, true, true>
    t['fwd/fast128_unguarded'] = lambda: _fwd(ops, 256, 128, 32, 32, 128, guard=False)         # no x_guard: 4-byte loads
    t['fwd/tile96_m90'] = lambda: _fwd(ops, 64, 96, 32, 32, 90)
    t['fwd/tile96_m179'] = lambda: _fwd(ops, 128, 179, 16, 16, 179)
    t['fwd/tile96_unguarded'] = lambda: _fwd(ops, 64, 96, 32, 32, 90, guard=False)             # <96, 128, true, false>
    t['fwd/tile64x128'] = lambda: _fwd(ops, 256, 64, 32, 32, 64)
    t['fwd/tile64x64'] = lambda: _fwd(ops, 4, 32, 16, 16, 32)
    t['fwd/tile64x128_1x1'] = lambda: _fwd(ops, 256, 128, 16, 16, 64, S1)
    t['fwd/1x1'] = lambda: _fwd(ops, 256, 256, 16, 16, 256, S1)
    t['fwd/1x1_small'] = lambda: _fwd(ops, 256, 256, 8, 8, 256, S1)                 # 16 K tiles on 128 tiles: not split
    t['fwd/concat'] = lambda: _fwd(ops, 256, 128, 32, 32, 128, C2=128)
    t['fwd/concat_straddle'] = lambda: _fwd(ops, 256, 72, 32, 32, 128, C2=56)       # c_split % 16 != 0
    t['fwd/concat_straddle_general_tile'] = lambda: _fwd(ops, 256, 72, 32, 32, 64, C2=56)
    t['fwd/image_stride'] = lambda: _fwd(ops, 256, 128, 32, 32, 128, img_stride=192 * 1024)
    for o in ('bias', 'tadd', 'res', 'accumulate'):
        t['fwd/opt_' + o] = (lambda o=o: _fwd(ops, 64, 128, 16, 16, 128, opts=(o,)))
    t['fwd/opt_relu'] = lambda: _fwd(ops, 64, 128, 16, 16, 128, relu=True)
    t['fwd/opt_alpha'] = lambda: _fwd(ops, 64, 128, 16, 16, 128, alpha=0.5)
    t['fwd/opt_post_scale'] = lambda: _fwd(ops, 64, 128, 16, 16, 128, post_scale=0.7071067811865476)
    t['fwd/opt_all'] = lambda: _fwd(ops, 64, 128, 16, 16, 128, opts=('bias', 'tadd', 'res', 'accumulate'), relu=True, alpha=0.5,
                                    post_scale=0.7071067811865476, wino='2d')
    t['fwd/upsample'] = lambda: _fwd(ops, 64, 128, 16, 16, 128, S(3, 1, 1, 1))
    t['fwd/stride2_pad0'] = lambda: _fwd(ops, 256, 128, 32, 32, 128, S(3, 2, 0, 0))
    t['fwd/stride2_pad1'] = lambda: _fwd(ops, 256, 128, 32, 32, 128, S(3, 2, 1, 0))
    t['fwd/general_1x7'] = lambda: _fwd(ops, 32, 128, 17, 17, 192, S.general(1, 7, 1, 0, 3))
    t['fwd/general_3x3_s2_valid'] = lambda: _fwd(ops, 32, 32, 149, 149, 32, S.general(3, 3, 2, 0, 0))
    t['fwd/class_2x2'] = lambda: _fwd(ops, 64, 128, 16, 16, 128, S.same(2, 2, 1, 0))
    t['fwd/conv_in'] = lambda: _fwd(ops, 256, 3, 32, 32, 128)
    t['fwd/conv_out'] = lambda: _fwd(ops, 256, 128, 32, 32, 3)
    t['fwd/splitk_folded'] = lambda: _fwd(ops, 16, 128, 32, 32, 128)                # 128 tiles, 4 slices (<= SPLITK_FOLD_MAX)
    t['fwd/splitk_reduce_launch'] = lambda: _fwd(ops, 8, 128, 32, 32, 128)          # 64 tiles, 8 slices
    t['fwd/splitk_mid_grid'] = lambda: _fwd(ops, 12, 384, 32, 32, 384)              # 288 tiles: 256 < tiles < 512
    t['fwd/splitk_tile96'] = lambda: _fwd(ops, 16, 192, 16, 16, 180)
    t['fwd/splitk_m64'] = lambda: _fwd(ops, 16, 128, 16, 16, 64)
    t['fwd/splitk_tiny'] = lambda: _fwd(ops, 4, 256, 4, 4, 256)
    t['fwd/splitk_fold_off'] = (lambda: _fwd(ops, 16, 128, 32, 32, 128), dict(SPLITK_FOLD=False))
    t['fwd/splitk_off'] = (lambda: _fwd(ops, 16, 128, 32, 32, 128), dict(CONV_SPLITK_BLOCKS=0))
    # ---- conv_forward, F(2, 3)
    t['fwd/wino_full'] = lambda: _fwd(ops, 64, 128, 32, 32, 128, wino='1d')
    t['fwd/wino_bk8_rows32'] = lambda: _fwd(ops, 128, 72, 32, 32, 90, wino='1d')
    t['fwd/wino_concat_mixed16'] = lambda: _fwd(ops, 16, 264, 8, 8, 256, C2=248, wino='1d')   # C % 16 == 0, its sources are not
    t['fwd/wino_splitk'] = lambda: _fwd(ops, 256, 256, 4, 4, 256, wino='1d')
    t['fwd/wino_split_refused_odd_npix'] = lambda: _fwd(ops, 9, 1024, 7, 7, 2048, wino='1d')
    t['fwd/wino_grid_refused'] = lambda: _fwd(ops, 4, 128, 32, 32, 128, wino='1d')
    t['fwd/wino_unsupported_split'] = lambda: _fwd(ops, 1024, 256, 2, 2, 256, wino='1d')      # W < 4: fields restored, direct form
    t['fwd/wino_image_stride'] = lambda: _fwd(ops, 64, 128, 32, 32, 128, wino='1d', img_stride=128 * 1024 + 1)
    t['fwd/wino_unsupported_w512'] = lambda: _fwd(ops, 1, 128, 512, 512, 128, wino='1d')
    t['fwd/wino_off'] = (lambda: _fwd(ops, 64, 128, 32, 32, 128, wino='1d'), dict(WINO=False))
    t['fwd/wino_min_tiles_0'] = (lambda: _fwd(ops, 4, 128, 32, 32, 128, wino='1d'), dict(WINO_MIN_TILES=0))
    # ---- conv_forward, F(2x2, 3x3)
    t['fwd/wino2d_4_3'] = lambda: _fwd(ops, 64, 128, 32, 32, 128, wino='2d')
    t['fwd/wino2d_8_2_splitk'] = lambda: _fwd(ops, 256, 256, 4, 4, 256, wino='2d')
    t['fwd/wino2d_8_2_one_round'] = lambda: _fwd(ops, 16, 128, 32, 32, 256, wino='2d')       # exactly 512 workgroups
    t['fwd/wino2d_w128'] = lambda: _fwd(ops, 4, 128, 128, 128, 128, wino='2d')
    t['fwd/wino2d_m32'] = lambda: _fwd(ops, 128, 96, 32, 32, 96, wino='2d')
    t['fwd/wino2d_tail_4_3'] = lambda: _fwd(ops, 64, 160, 32, 32, 160, wino='2d')
    t['fwd/wino2d_tail_8_2'] = lambda: _fwd(ops, 16, 224, 32, 32, 224, wino='2d')
    t['fwd/wino2d_concat'] = lambda: _fwd(ops, 64, 256, 32, 32, 128, C2=128, wino='2d')
    t['fwd/wino2d_grid_refused'] = lambda: _fwd(ops, 4, 128, 32, 32, 128, wino='2d')
    t['fwd/wino2d_unsupported_odd_h'] = lambda: _fwd(ops, 64, 128, 31, 32, 128, wino='2d')    # the DIRECT form follows, not F(2, 3)
    t['fwd/wino2d_unsupported_odd_stride'] = lambda: _fwd(ops, 64, 128, 32, 32, 128, wino='2d', img_stride=128 * 1024 + 1)
    t['fwd/wino2d_unsupported_split'] = lambda: _fwd(ops, 1024, 256, 2, 2, 256, wino='2d')
    t['fwd/wino2d_off'] = (lambda: _fwd(ops, 64, 128, 32, 32, 128, wino='2d'), dict(WINO2D=False))
    # ---- conv_forward, F(4, 3)
    t['fwd/wino43_full'] = (lambda: _fwd(ops, 64, 128, 32, 32, 128, wino43=True, wino='1d'), W43)
    t['fwd/wino43_concat_opts'] = (lambda: _fwd(ops, 8, 64, 16, 16, 96, C2=64, wino43=True, opts=('bias', 'tadd', 'res')), W43)
    t['fwd/wino43_splitk'] = (lambda: _fwd(ops, 256, 256, 4, 4, 256, wino43=True, wino='1d'), W43_SPLIT)
    t['fwd/wino43_grid_refused'] = (lambda: _fwd(ops, 4, 128, 32, 32, 128, wino43=True, wino='2d'), W43_SPLIT)
    t['fwd/wino43_unsupported'] = (lambda: _fwd(ops, 1024, 256, 2, 2, 256, wino43=True), W43)
    t['fwd/wino43_off'] = lambda: _fwd(ops, 64, 128, 32, 32, 128, wino43=True, wino='1d')
    # ---- conv_dgrad
    t['dgrad/direct'] = lambda: _dgrad(ops, 256, 128, 32, 32, 128)
    t['dgrad/direct_splitk'] = lambda: _dgrad(ops, 16, 256, 16, 16, 128, alpha=2.0)
    t['dgrad/wino'] = lambda: _dgrad(ops, 64, 128, 32, 32, 96, wino='1d')
    t['dgrad/wino2d'] = lambda: _dgrad(ops, 64, 128, 32, 32, 256, wino='2d')
    t['dgrad/wino2d_accumulate'] = lambda: _dgrad(ops, 256, 256, 4, 4, 256, wino='2d', accumulate=True,
                                                  out=ops.empty_act((256, 256, 4, 4), 'cpu'))
    t['dgrad/stride2'] = lambda: _dgrad(ops, 256, 128, 16, 16, 128, S(3, 2, 1, 0))
    t['dgrad/1x1'] = lambda: _dgrad(ops, 256, 256, 16, 16, 128, S1)
    t['dgrad/class_2x2'] = lambda: _dgrad(ops, 64, 128, 16, 16, 128, S.same(2, 2, 0, 1))
    t['dgrad_s2/pad0'] = lambda: _dgrad_s2(ops, 256, 128, 16, 16, 128, 0)
    t['dgrad_s2/pad1_add'] = lambda: _dgrad_s2(ops, 16, 256, 8, 8, 256, 1, add=True)
    # ---- conv_wgrad
    t['wgrad/merged_few_in'] = lambda: _wgrad(ops, 256, 128, 32, 32, 3)
    t['wgrad/merged_few_out'] = lambda: _wgrad(ops, 256, 3, 32, 32, 128)
    t['wgrad/merged_one_split'] = lambda: _wgrad(ops, 1, 128, 8, 8, 3, accumulate=False)
    for W, N in ((8, 1024), (16, 256), (32, 64)):
        t['wgrad/wino2d_w%d' % W] = (lambda W=W, N=N: _wgrad(ops, N, 128, W, W, 128))
    t['wgrad/wino2d_one_split_p64'] = (lambda: _wgrad(ops, 1, 128, 8, 8, 128, alpha=0.5, accumulate=False), NOWORK)
    t['wgrad/wino2d_tail'] = lambda: _wgrad(ops, 128, 96, 32, 32, 96)
    t['wgrad/wino2d_concat'] = lambda: _wgrad(ops, 64, 128, 32, 32, 256, C2=128)
    t['wgrad/wino2d_blocks_patched'] = (lambda: _wgrad(ops, 64, 128, 32, 32, 128), dict(WGRAD_WINO2D_BLOCKS=64, WGRAD_BLOCKS=2048))
    t['wgrad/wino2d_refused_w64'] = lambda: _wgrad(ops, 32, 128, 64, 64, 128)       # F(2, 3) follows, 64 x 64 tiles
    t['wgrad/wino2d_concat_on_32'] = lambda: _wgrad(ops, 64, 128, 32, 32, 96, C2=32)          # boundary on 32, not on 64
    t['wgrad/wino2d_refused_concat48'] = lambda: _wgrad(ops, 64, 128, 32, 32, 48, C2=80)      # concat boundary off 32 (and 64): direct
    t['wgrad/wino2d_off'] = (lambda: _wgrad(ops, 64, 128, 32, 32, 128), dict(WGRAD_WINO2D=False))
    t['wgrad/wino_tile96'] = lambda: _wgrad(ops, 32, 96, 64, 64, 96)
    t['wgrad/wino_tile96_concat'] = lambda: _wgrad(ops, 32, 96, 64, 64, 96, C2=96)
    t['wgrad/wino_one_split'] = (lambda: _wgrad(ops, 1, 128, 8, 8, 128), dict(WGRAD_WINO_MIN_WORK=0, WGRAD_WINO2D=False))
    t['wgrad/wino_blocks_patched'] = (lambda: _wgrad(ops, 32, 128, 64, 64, 128), dict(WGRAD_BLOCKS=256))
    t['wgrad/wino_unsupported_w4'] = lambda: _wgrad(ops, 4096, 128, 4, 4, 128)      # both Winograd forms refuse: direct
    t['wgrad/wino_off'] = (lambda: _wgrad(ops, 64, 128, 32, 32, 128), dict(WGRAD_WINO=False))
    t['wgrad/direct128'] = lambda: _wgrad(ops, 4, 128, 32, 32, 128)
    t['wgrad/direct128_concat'] = lambda: _wgrad(ops, 4, 128, 32, 32, 128, C2=128)
    t['wgrad/direct96'] = lambda: _wgrad(ops, 4, 96, 32, 32, 90)
    t['wgrad/direct96_concat'] = lambda: _wgrad(ops, 4, 90, 32, 32, 96, C2=96)
    t['wgrad/direct_cout64'] = lambda: _wgrad(ops, 4, 64, 32, 32, 128)
    t['wgrad/direct_straddle'] = lambda: _wgrad(ops, 4, 64, 32, 32, 72, C2=56)
    t['wgrad/direct_stride2'] = lambda: _wgrad(ops, 256, 128, 32, 32, 128, S(3, 2, 0, 0))
    t['wgrad/direct_upsample'] = lambda: _wgrad(ops, 64, 128, 16, 16, 128, S(3, 1, 1, 1))
    t['wgrad/direct_class_2x2'] = lambda: _wgrad(ops, 64, 128, 16, 16, 128, S.same(2, 2, 1, 0))
    t['wgrad/1x1'] = lambda: _wgrad(ops, 256, 256, 16, 16, 256, S1)                  # half the block target
    t['wgrad/one_split'] = lambda: _wgrad(ops, 1, 128, 8, 8, 128, accumulate=False)
    t['wgrad/max_splits'] = lambda: _wgrad(ops, 64, 128, 32, 32, 128, max_splits=4)
    t['wgrad/max_splits_1'] = lambda: _wgrad(ops, 64, 128, 32, 32, 128, max_splits=1)
    t['wgrad/min_pix_patched'] = (lambda: _wgrad(ops, 4, 128, 32, 32, 128), dict(WGRAD_MIN_PIX=1024))
    # ---- batched products and Linear layers
    t['bmm_tn'] = lambda: ops.bmm_tn(_mm(1024, 64, 256), _mm(1024, 64, 256), alpha=0.125)
    t['bmm_tn/z1_splitk'] = lambda: ops.bmm_tn(_mm(1, 4096, 128), _mm(1, 4096, 256))
    t['bmm_nn'] = lambda: ops.bmm_nn(_mm(1024, 64, 256), _mm(1024, 256, 256))         # conv_gemm_kernel<64, 128, true, false>
    t['bmm_nn/small'] = lambda: ops.bmm_nn(_mm(8, 48, 64), _mm(8, 64, 64), accumulate=True, out=_mm(8, 48, 64))
    t['bmm_nn/m128'] = lambda: ops.bmm_nn(_mm(256, 128, 256), _mm(256, 256, 256))
    t['bmm_nt'] = lambda: ops.bmm_nt(_mm(1024, 64, 256), _mm(1024, 256, 256), alpha=2.0)
    t['bmm_nt/col_bias'] = lambda: ops.bmm_nt(_mm(1, 256, 512), _mm(1, 512, 512), col_bias=_mm(512))
    t['linear_forward'] = lambda: ops.linear_forward(_mm(256, 512), _mm(512, 512), _mm(512))   # split-K over the features
    t['linear_forward/bmm'] = lambda: ops.linear_forward(_mm(256, 32), _mm(128, 32))
    t['linear_dgrad'] = lambda: ops.linear_dgrad(_mm(256, 512), _mm(512, 128))
    t['linear_dgrad/rows32'] = lambda: ops.linear_dgrad(_mm(32, 512), _mm(512, 9984))
    t['linear_wgrad'] = lambda: ops.linear_wgrad(_mm(256, 512), _mm(256, 128), _mm(512, 128))
    t['linear_wgrad/odd_width'] = lambda: ops.linear_wgrad(_mm(256, 179), _mm(256, 128), _mm(179, 128), alpha=0.5, accumulate=False)
    # ---- the shape rules the dispatch reads outside the convolution paths
    t['ups9_dgrad'] = lambda: _ups9(ops, 256, 128, 8, 8, 128)
    t['ups9_dgrad/refused'] = lambda: _ups9(ops, 256, 128, 8, 8, 128, ldu=64)
    t['attention_fused_ok'] = lambda: [ops.attention_fused_ok(T, d, d) for T, d in ((256, 64), (250, 64), (256, 512), (1024, 384))]
    t['probe_wgrad_wino2d_supported'] = lambda: [_probe_wgrad_wino2d(ops, 256), _probe_wgrad_wino2d(ops, 224)]
    # ---- the host mirrors
    t['wanted/wino'] = lambda: _wanted_grid(ops, ops.wino_wanted)
    t['wanted/wino2d'] = lambda: _wanted_grid(ops, ops.wino2d_wanted)
    t['wanted/wino43_off'] = lambda: _wanted_grid(ops, ops.wino43_wanted)
    t['wanted/wino43'] = (lambda: _wanted_grid(ops, ops.wino43_wanted), W43_SPLIT)
    t['wanted/wino_min_tiles_0'] = (lambda: _wanted_grid(ops, ops.wino_wanted), dict(WINO_MIN_TILES=0))
    t['wanted/wino2d_fill_0'] = (lambda: _wanted_grid(ops, ops.wino2d_wanted), dict(WINO2D_MIN_FILL=0.0, WINO2D_MIN_TILES=128))
    t['wanted/wino2d_off'] = (lambda: _wanted_grid(ops, ops.wino2d_wanted), dict(WINO2D=False))
    return {k: (v if isinstance(v, tuple) else (v, None)) for k, v in t.items()}


def record_plans():
    """{'blocks': [parameter blocks], 'cases': {name: [records]}} of the case table against the `ops` module as it is."""
    ops = pkg('ops')
    blocks, out = [], {}
    for name, (fn, patch) in cases(ops).items():
        with recording(ops, blocks, patch) as r:
            ret = fn()
        if ret is not None and not isinstance(ret, torch.Tensor):
            r.rec.append(['ret', ret])
        out[name] = r.rec
    return json.loads(json.dumps({'blocks': blocks, 'cases': out}))          # the JSON round trip (exact for doubles)


# ---------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def plans():
    return record_plans()


def _expand(doc, rec):
    """A case's records with the block references replaced by the blocks (indices depend on the order of the case table)."""
    return [[r[0], r[1], [(a[:2] + [doc['blocks'][a[2]]]) if isinstance(a, list) and a and a[0] == 'B' else a for a in r[2]]] + r[3:]
            if r[0] == 'lib' else r for r in rec]


def test_launch_plans_equal_the_recorded_fixture(plans):
    """Every case of the table yields, record by record, what the fixture holds: library calls with every field of every parameter
    block, `*_supported` answers, launch names with flops and bytes, workspace and tile-counter sizes, return values."""
    with open(FIXTURE) as f:
        want = json.load(f)
    assert sorted(plans['cases']) == sorted(want['cases'])
    bad = []
    for name in want['cases']:
        got, exp = _expand(plans, plans['cases'][name]), _expand(want, want['cases'][name])
        if got != exp:
            first = next((i for i, (a, b) in enumerate(zip(got, exp)) if a != b), min(len(got), len(exp)))
            bad.append((name, first, got[first] if first < len(got) else None, exp[first] if first < len(exp) else None))
    assert not bad, bad[:3]


def test_case_table_reaches_every_floor_launch_name_and_both_answers_of_every_shape_rule(plans):
    """The two conditions that keep the table from being thin: every contraction launch name of the launch-parity floor
    (tests/test_launch_parity_gpu.py FLOOR) is among the recorded _run names, and every `*_supported` symbol of include/dp_hip.h is
    recorded answering zero and non-zero."""
    src = open(os.path.join(ROOT, 'tests', 'test_launch_parity_gpu.py')).read()
    floor_src = src[src.index('FLOOR = {'):src.index('NOT_IN_STEP')]
    floor = {n for n in re.findall(r"'([^']+)'", floor_src) if n.startswith(('conv_gemm', 'conv_wino', 'nt_gemm', 'wgrad_wino'))}
    assert len(floor) >= 25, floor
    recs = [r for rec in plans['cases'].values() for r in rec]
    ran = {r[1] for r in recs if r[0] == 'run'}
    assert not floor - ran, sorted(floor - ran)
    hdr = open(os.path.join(ROOT, 'include', 'dp_hip.h')).read()
    rules = set(re.findall(r'^int (dp_\w+_supported)\(', hdr, re.M))
    assert len(rules) >= 7, rules
    for sym in sorted(rules):
        answers = {bool(r[3]) for r in recs if r[0] == 'lib' and r[1] == sym}
        assert answers == {False, True}, (sym, answers)
    # every launch closure holds its parameter block directly (launch_name of the launch-parity test reads ksplit / splits there)
    assert all(len(r[4]) == 1 for r in recs if r[0] == 'run'), [r for r in recs if r[0] == 'run' and len(r[4]) != 1][:3]
