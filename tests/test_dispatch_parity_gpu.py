"""Parity with fp64 on every dispatch branch of the non-contraction kernels.

The launchers of csrc/norm.hip, transformer.hip, elementwise.hip, importance.hip, optim.hip, vq.hip, sampler.hip, ldm_sampler.hip and
ema.hip choose a kernel, a template instantiation or a vector path from the shape, the alignment and the optional operands (the
contraction kernels have the same tables in tests/test_contraction_dispatch_gpu.py).  Every launch records the kernel expression
of its launch site (DP_LAUNCH in csrc/dp_common.h, read back through dp_recent_launches), so a case can state which branch it took:

  BRANCHES    every name (or `name | condition` where a runtime flag rather than the name selects the path) the tabled launch
              sites can record, written out by hand, each with the launcher condition that selects it;
  CASES       entry -> the cases that reach it (registered with @case below); an entry without a case FAILS;
  UNREACHED   entries that cannot be reached through `ops` without changing process state, each with its reason;
  LAUNCH_SITES  DP_LAUNCH( sites per file: tests/test_cpu.py counts them and checks every kernel name they launch against BRANCHES.

test_branch is parametrised over BRANCHES itself.  Each case calls ONE ops entry point under `launched`, asserts that the entry's
name is among the names of that call and that every name is a known one, and compares every output (for strided outputs also every
element outside the written view) with an fp64 evaluation of the same operation on the CPU.  Bounds are the ones the older tests
of the same kernels use: 2e-5 GroupNorm, 1e-5 everything else (relative to the largest reference magnitude), 0 for pure data
movement.  The ill-conditioned input families (test_*_ill_conditioned) use max(4 e_ref32, floor) with e_ref32 = the error of torch's
fp32 CPU operator against fp64 on the same input and floor = that same older bound."""
import ctypes
import importlib
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import ref_groupnorm, relerr

pytestmark = pytest.mark.gpu
DEV = 'cuda'
CAP = 8192 * 256                     # dp_grid / tf_grid: at most 8192 workgroups of 256 threads; past it the grid-stride loop turns
BIG = 3 * CAP + 77                   # "just past a multiple of the cap, with a ragged end"

LAUNCH_SITES = {'norm.hip': 19, 'transformer.hip': 8, 'elementwise.hip': 35, 'importance.hip': 8, 'optim.hip': 8, 'vq.hip': 2,
                'sampler.hip': 4, 'ldm_sampler.hip': 2, 'ema.hip': 2}

_GN_ADDS = ('false, false', 'true, false', 'false, true', 'true, true')       # <.., A1, A2>: add1 / add2 present
BRANCHES = [
    # ---- transformer.hip
    'ln_fwd_kernel<64>',                         # N*T >= 65536
    'ln_fwd_kernel<16>',                         # N*T <  65536
    'ln_bwd_kernel<64>',                         # N*T >= 65536
    'ln_bwd_kernel<16>',                         # N*T <  65536
    'ln_param_kernel',                           # second launch of every dp_layernorm_bwd
    'geglu_fwd_kernel', 'geglu_bwd_kernel', 'add_rowvec_kernel',               # grid-stride, tf_grid
    # ---- norm.hip: GroupNorm forward.  vec4 = HW % 4 == 0, image strides % 4 == 0, 16-byte aligned pointers; cnt4 = (C / G) * HW / 4
    'gn_fwd_wave_kernel<1>',                     # vec4, N*G >= 1024, (C/G) * HW <= 2048, cnt4 <= 64
    'gn_fwd_wave_kernel<2>',                     # ... 64 < cnt4 <= 128
    'gn_fwd_wave_kernel<4>',                     # ... 128 < cnt4 <= 256
    'gn_fwd_wave_kernel<8>',                     # ... 256 < cnt4 <= 512
    'gn_fwd_vec4_kernel<1>',                     # vec4, not the wave form, cnt4 <= 256
    'gn_fwd_vec4_kernel<2>',                     # ... 256 < cnt4 <= 512
    'gn_fwd_vec4_kernel<4>',                     # ... 512 < cnt4 <= 1024
    'gn_fwd_vec4_kernel<8>',                     # ... 1024 < cnt4 <= 2048
    'gn_fwd_vec4_kernel<0>',                     # ... cnt4 > 2048 (streaming form)
    'gn_fwd_kernel | cached',                    # not vec4, (C/G) * HW <= 8192: the group is kept in registers
    'gn_fwd_kernel | streaming',                 # not vec4, (C/G) * HW > 8192: three passes over memory
    # split GroupNorm (ops._gn_slices: N*G < 1024, HW >= 1024, vec4): slices = 1 while HW < 8192, else 2 .. 32
    'gn_split_part_fwd_kernel | slices == 1', 'gn_split_part_fwd_kernel | slices > 1',
    'gn_split_combine_fwd_kernel | slices == 1', 'gn_split_combine_fwd_kernel | slices > 1',
    'gn_split_apply_fwd_kernel | slices == 1', 'gn_split_apply_fwd_kernel | slices > 1',
    # ---- GroupNorm backward.  HW4 = HW / 4
    # wave: vec4, HW4 a power of two <= 64, (C/G) * HW <= 2048, N*G >= 1024; NV from cnt4 as in the forward
] + ['gn_bwd_wave_kernel<%d, %s>' % (nv, a) for nv in (1, 2, 4, 8) for a in _GN_ADDS] + [
    # vec4c: vec4, not wave, HW4 <= 256, C/G <= 8; NCH = 1 for C/G <= 4, else 2
] + ['gn_bwd_vec4c_kernel<%d, %s>' % (nch, a) for nch in (1, 2) for a in _GN_ADDS] + [
    'gn_bwd_vec4_kernel',                        # vec4 and (HW4 > 256 or C/G > 8)
    'gn_bwd_kernel',                             # not vec4
    'gn_split_part_bwd_kernel | slices == 1', 'gn_split_part_bwd_kernel | slices > 1',
    'gn_split_combine_bwd_kernel | slices == 1', 'gn_split_combine_bwd_kernel | slices > 1',
] + ['gn_split_apply_bwd_kernel<%s>' % a for a in _GN_ADDS] + [
    # ---- norm.hip: column / row sums
    'colsum_kernel',
    'colsum_batch_kernel',                       # one launch per <= 80 items; a repeated destination closes the launch
    'rowsum_kernel<true>',                       # HW < 4096, vec4 (HW % 4 == 0, image stride % 4 == 0, 16-byte aligned)
    'rowsum_kernel<false>',                      # HW < 4096, not vec4
    'rowsum_plane_kernel<true>',                 # HW >= 4096, vec4
    'rowsum_plane_kernel<false>',                # HW >= 4096, not vec4
    # ---- elementwise.hip: grid-stride kernels (dp_grid) and softmax
    'silu_fwd_kernel', 'silu_bwd_kernel', 'axpby_kernel', 'copy_strided_kernel', 'add_noise_kernel', 'q_sample_kernel',
    'cfg_combine_kernel', 'ddim_step_kernel', 'ddpm_step_kernel', 'dropout_apply_kernel', 'scale_if_stopped_kernel',
    'downsum_kernel', 'ups_weff_kernel', 'ups_wfold_kernel',
    # vec: even width, even class / image strides of the low-resolution side, image strides % 4 and 16-byte alignment of the other
    'upsample2x_kernel | vec', 'upsample2x_kernel | scalar',
    'interleave2x2_kernel | vec', 'interleave2x2_kernel | scalar',
    'deinterleave2x2_kernel | vec', 'deinterleave2x2_kernel | scalar',
    'softmax_fwd_kernel | cols <= 1024',         # the row is kept in registers
    'softmax_fwd_kernel | cols > 1024',          # three passes over memory
    'softmax_bwd_kernel',
    # ---- importance.hip
    'wg_gn_kernel',                              # mode 3
    'wg_rows_kernel',                            # dim 0
    'wg_cols_ct_kernel', 'wg_fold_taps_kernel',  # dim 1: two launches
    'gather_add_kernel',
    'group_score_part_kernel', 'group_score_combine_kernel',                   # one pair per <= 24 members, accumulate from the second on
    'slice_batch_kernel',                        # one launch per <= 48 items
    # ---- elementwise.hip: one launch site each, no template argument, no path flag
    'temb_kernel', 'mse_kernel', 'sum_partials_kernel', 'kd_kernel', 'kd_terms_kernel', 'early_exit_update_kernel',
    'early_exit_update_ratio_kernel', 'dropout_mask_kernel', 'randn_philox_kernel', 'u8_to_float_kernel', 'pool2d_kernel',
    'resize_bilinear_kernel', 'ssim_tile_kernel', 'ssim_finish_kernel', 'mse_per_image_kernel', 'pack_weight_batch_kernel',
    # ---- optim.hip
    'sumsq_kernel', 'clip_coef_kernel', 'adam_ema_kernel', 'set_step_scalars_kernel', 'adam_ema_dev_kernel',
    'adamw_ema_kernel<true>',                    # every buffer 16-byte aligned and n >= 4: 16-byte accesses + a scalar tail
    'adamw_ema_kernel<false>',                   # otherwise
    'embedding_bwd_kernel',
    # ---- vq.hip: one instantiation per embedding width D = 1 .. 16
] + ['vq_quantize_kernel<%d>' % d for d in range(1, 17)] + [
    'vq_loss_kernel',
    # ---- sampler.hip.  16-byte accesses between a scalar head and tail when every pointer has the same 16-byte phase, else 4-byte ones
    'denoise_step_kernel<0>',                    # mode 0: generalized_steps
    'denoise_step_kernel<1>',                    # mode 1: ddpm_steps
    'image_to_u8_kernel<true>',                  # C <= 4, HW % 4 == 0, image stride % 4 == 0, x 16-byte and out 4-byte aligned
    'image_to_u8_kernel<false>',                 # otherwise
    # ---- ldm_sampler.hip: <ORDER, GUIDED> (the two sites of CFG_DENOISE_CASE, once per order 0 .. 4); GUIDED = e holds both halves
] + ['cfg_denoise_step_kernel<%d, %s>' % (o, g) for o in range(5) for g in ('true', 'false')] + [
    # ---- ema.hip
    'ema_update_kernel<true>',                   # both buffers 16-byte aligned and n >= 4: 16-byte accesses + a scalar tail
    'ema_update_kernel<false>',                  # otherwise
]

UNREACHED = {}

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


def launched(ops, fn):
    """(fn(), the kernel names of the launches fn issued, oldest first)."""
    lib = ops._lib()
    c0 = lib.dp_launch_count()
    r = fn()
    n = lib.dp_launch_count() - c0
    assert 0 < n <= 256, n
    arr = (ctypes.c_char_p * 256)()
    k = lib.dp_recent_launches(arr, 256)
    assert k >= n
    names = [arr[i].decode() for i in range(k - n, k)]
    return r, [s[1:-1] if s.startswith('(') else s for s in names]


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed + sum(shape))
    return (torch.randn(*shape, generator=g) * scale).to(DEV)


def d64(t):
    return t.detach().double().cpu()


def poison(n):
    """Fills the block the caching allocator hands to the next allocation of n floats with NaN: an output the kernel does not
    write completely cannot inherit the right values from an earlier call."""
    t = torch.full((n + 8,), float('nan'), device=DEV)
    del t


def wide(N, C, H, W, seed, lead=2, extra=5, fill=None):
    """An [N, C, H, W] channel slice of a wider buffer (free image stride, 16-byte aligned when H * W % 4 == 0) and the buffer."""
    big = rnd(N, C + extra, H, W, seed=seed) if fill is None else torch.full((N, C + extra, H, W), float(fill), device=DEV)
    return big[:, lead:lead + C], big


def outside_intact(big, before, lead, C):
    return torch.equal(big[:, :lead], before[:, :lead]) and torch.equal(big[:, lead + C:], before[:, lead + C:])


# ======================================================================================================================
# LayerNorm (channel-major tokens)
# ======================================================================================================================
def ref_layernorm(x, gamma, beta, eps, dy=None, add=None):
    """fp64: y, stats [N, T, 2] = (mean, rstd) and, with dy, dx (+ add) and pws [N, C, 2] = (sum_t dy, sum_t dy * xhat)."""
    N, C = x.shape[:2]
    mean = x.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(x.var(1, unbiased=False, keepdim=True) + eps)
    xh = (x - mean) * rstd
    g = gamma.view(1, C, 1, 1)
    y = xh * g + beta.view(1, C, 1, 1)
    stats = torch.stack([mean.reshape(N, -1), rstd.reshape(N, -1)], -1)
    if dy is None:
        return y, stats
    gd = dy * g
    dx = rstd * (gd - gd.mean(1, keepdim=True) - xh * (gd * xh).mean(1, keepdim=True))
    if add is not None:
        dx = dx + add
    pws = torch.stack([dy.sum((2, 3)), (dy * xh).sum((2, 3))], -1)
    return y, stats, dx, pws


def ln_forms(ntok):
    return ('ln_fwd_kernel<64>', 'ln_bwd_kernel<64>') if ntok >= 65536 else ('ln_fwd_kernel<16>', 'ln_bwd_kernel<16>')


def run_ln_fwd(ops, N, C, H, W, strided=True, x=None, seed=1, check=True):
    ntok = N * H * W
    if x is None:
        x = (wide(N, C, H, W, seed)[0] if strided else rnd(N, C, H, W, seed=seed)) + 0.2
    gamma, beta = 1 + 0.2 * rnd(C, seed=2), 0.1 * rnd(C, seed=3)
    if strided:
        out, big = wide(N, C, H, W, 0, fill=777.0)
        before = big.clone()
    else:
        poison(N * C * H * W)
        out = None
    (y, st), names = launched(ops, lambda: ops.layernorm_fwd(x, gamma, beta, out=out))
    assert names == [ln_forms(ntok)[0]], names
    e_y = e_st = 0.0
    for n in range(N if check else 0):                        # image by image: the fp64 reference of 63 M elements stays small
        yr, sr = ref_layernorm(d64(x[n:n + 1]), d64(gamma), d64(beta), 1e-5)
        e_y, e_st = max(e_y, relerr(y[n:n + 1], yr)), max(e_st, relerr(st[n:n + 1], sr))
    assert not strided or outside_intact(big, before, 2, C)
    return dict(names=names, shape=(N, C, H, W), y=e_y, stats=e_st, bound=1e-5), (x, gamma, beta, st)


def run_ln_bwd(ops, N, C, H, W, with_add, strided=True):
    ntok = N * H * W
    _, (x, gamma, beta, st) = run_ln_fwd(ops, N, C, H, W, strided=strided, check=False)
    dy = wide(N, C, H, W, 4)[0] if strided else rnd(N, C, H, W, seed=4)
    add = (wide(N, C, H, W, 5)[0] if strided else rnd(N, C, H, W, seed=5)) if with_add else None
    if strided:
        out, big = wide(N, C, H, W, 0, fill=777.0)
        before = big.clone()
    else:
        poison(N * C * H * W)
        out = None
    (dx, pws), names = launched(ops, lambda: ops.layernorm_bwd(x, gamma, st, dy, add=add, out=out))
    assert names == [ln_forms(ntok)[1], 'ln_param_kernel'], names
    e_dx = e_p = 0.0
    for n in range(N):
        _, _, dxr, pr = ref_layernorm(d64(x[n:n + 1]), d64(gamma), d64(beta), 1e-5, d64(dy[n:n + 1]),
                                      None if add is None else d64(add[n:n + 1]))
        e_dx, e_p = max(e_dx, relerr(dx[n:n + 1], dxr)), max(e_p, relerr(pws[n:n + 1], pr))
    assert not strided or outside_intact(big, before, 2, C)
    return dict(names=names, shape=(N, C, H, W), add=with_add, dx=e_dx, pws=e_p, bound=1e-5)


# N*T = 65536 exactly / 66049 (ragged last 64-token workgroup) / 65535 (the 16-token form, ragged); C = 50 and 77 are no multiples
# of 8 or 32 (tail channel of the two-stream loop in both forms); C = 960 is the widest LDM layer
LN_64 = [(4, 50, 128, 128), (1, 77, 257, 257)]
LN_16 = [(1, 50, 257, 255), (3, 77, 5, 7), (2, 960, 16, 16)]


@case('ln_fwd_kernel<64>')
def ln_fwd64(ops):
    for N, C, H, W in LN_64:
        assert N * H * W >= 65536
        yield run_ln_fwd(ops, N, C, H, W)[0]
    assert (257 * 257) % 64 != 0
    yield run_ln_fwd(ops, 4, 960, 128, 128, strided=False)[0]


@case('ln_fwd_kernel<16>')
def ln_fwd16(ops):
    for N, C, H, W in LN_16:
        assert N * H * W < 65536
        yield run_ln_fwd(ops, N, C, H, W)[0]
    assert 257 * 255 == 65535


@case('ln_bwd_kernel<64>')
def ln_bwd64(ops):
    for i, (N, C, H, W) in enumerate(LN_64):
        yield run_ln_bwd(ops, N, C, H, W, with_add=bool(i))
    yield run_ln_bwd(ops, 4, 960, 128, 128, with_add=True, strided=False)


@case('ln_bwd_kernel<16>')
def ln_bwd16(ops):
    for i, (N, C, H, W) in enumerate(LN_16):
        yield run_ln_bwd(ops, N, C, H, W, with_add=bool(i % 2))


@case('ln_param_kernel')
def ln_param(ops):                                           # T = 35 (< one wavefront), N*C = 231 rows (ragged last workgroup of 4 rows)
    yield run_ln_bwd(ops, 3, 77, 5, 7, with_add=False)


# ======================================================================================================================
# GroupNorm
# ======================================================================================================================
def gn_fwd_name(N, C, HW, G, vec4=True):
    """dp_groupnorm_silu_fwd's choice, restated from the launcher (ops._gn_slices decides the split form first)."""
    cpg = C // G
    if not vec4 or HW % 4:
        return 'gn_fwd_kernel'
    cnt4 = cpg * (HW // 4)
    if cpg * HW <= 2048 and N * G >= 1024:
        return 'gn_fwd_wave_kernel<%d>' % (1 if cnt4 <= 64 else 2 if cnt4 <= 128 else 4 if cnt4 <= 256 else 8)
    return 'gn_fwd_vec4_kernel<%d>' % (1 if cnt4 <= 256 else 2 if cnt4 <= 512 else 4 if cnt4 <= 1024 else 8 if cnt4 <= 2048 else 0)


def gn_bwd_name(N, C, HW, G, a1, a2):
    cpg, HW4 = C // G, HW // 4
    a = '%s, %s' % ('true' if a1 else 'false', 'true' if a2 else 'false')
    if HW % 4:
        return 'gn_bwd_kernel'
    cnt4 = cpg * HW4
    if 1 <= HW4 <= 64 and HW4 & (HW4 - 1) == 0 and cpg * HW <= 2048 and N * G >= 1024:
        return 'gn_bwd_wave_kernel<%d, %s>' % (1 if cnt4 <= 64 else 2 if cnt4 <= 128 else 4 if cnt4 <= 256 else 8, a)
    if HW4 <= 256 and cpg <= 8:
        return 'gn_bwd_vec4c_kernel<%d, %s>' % (1 if cpg <= 4 else 2, a)
    return 'gn_bwd_vec4_kernel'


def gn_inputs(N, C1, C2, H, W, seed=1, x=None):
    C = C1 + C2
    if x is None:
        x = rnd(N, C, H, W, seed=seed) + 0.3
    xa, xb = (x[:, :C1].contiguous(), x[:, C1:].contiguous()) if C2 else (x, None)
    return x, xa, xb, 1 + 0.2 * rnd(C, seed=3), 0.1 * rnd(C, seed=4)


def run_gn_fwd(ops, N, C1, C2, H, W, G, silu, expect, slices=None, x=None):
    C, HW = C1 + C2, H * W
    x, xa, xb, gamma, beta = gn_inputs(N, C1, C2, H, W, x=x)
    out, big = wide(N, C, H, W, 0, fill=777.0)
    before = big.clone()
    sl = ops._gn_slices(N, G, HW, (xa, xb, out), ())
    assert sl == (slices or 0) or (slices == '>1' and sl > 1), (sl, slices)
    (y, stats), names = launched(ops, lambda: ops.groupnorm_fwd(xa, xb, gamma, beta, G, 1e-6, silu, out=out))
    assert names == expect, (names, expect)
    xr = d64(x)
    e_y = relerr(y, ref_groupnorm(xr, d64(gamma), d64(beta), G, 1e-6, silu))
    xg = xr.reshape(N * G, -1)
    sr = torch.stack([xg.mean(1), 1.0 / torch.sqrt(xg.var(1, unbiased=False) + 1e-6)], -1)
    e_st = relerr(stats, sr)
    assert outside_intact(big, before, 2, C)
    return dict(names=names, shape=(N, C1, C2, H, W, G), silu=silu, y=e_y, stats=e_st, bound=2e-5)


def run_gn_bwd(ops, N, C1, C2, H, W, G, silu, a1, a2, want_rows, expect, x=None):
    C = C1 + C2
    x, xa, xb, gamma, beta = gn_inputs(N, C1, C2, H, W, x=x)
    _, stats = ops.groupnorm_fwd(xa, xb, gamma, beta, G, 1e-6, silu)
    dz = rnd(N, C, H, W, seed=5)
    add1 = wide(N, C, H, W, 6)[0] if a1 else None
    add2 = wide(N, C, H, W, 7, lead=4, extra=4)[0] if a2 else None
    out, big = wide(N, C, H, W, 0, fill=777.0)
    before = big.clone()
    r, names = launched(ops, lambda: ops.groupnorm_bwd(xa, xb, gamma, beta, stats, dz, G, silu, add1=add1, add2=add2, out=out,
                                                       want_rows=want_rows))
    assert names == expect, (names, expect)
    dx, pws = r[0], r[1]
    xr = d64(x).requires_grad_(True)
    gr = d64(gamma).expand(N, C).clone().requires_grad_(True)      # per-image parameters: their gradients are the rows of pws
    br = d64(beta).expand(N, C).clone().requires_grad_(True)
    ref_groupnorm(xr, gr, br, G, 1e-6, silu).backward(d64(dz))
    dxr = xr.grad + (d64(add1) if a1 else 0) + (d64(add2) if a2 else 0)
    res = dict(names=names, shape=(N, C1, C2, H, W, G), silu=silu, adds=(a1, a2), dx=relerr(dx, dxr),
               pws=relerr(pws, torch.stack([br.grad, gr.grad], -1)), bound=2e-5)
    if want_rows:
        if r[2] is None:
            assert expect[0].startswith('gn_split')
        else:
            res['rows'] = relerr(r[2], dxr.sum((2, 3)))
    assert outside_intact(big, before, 2, C)
    return res


# (N, C1, C2, H, W, G) per kernel; the concat boundary C1 lies inside a group wherever C2 != 0
GN_WAVE = {1: (32, 256, 0, 4, 4, 32), 2: (32, 100, 156, 8, 8, 32), 4: (32, 128, 0, 16, 16, 32), 8: (32, 100, 156, 16, 16, 32)}
GN_VEC4 = {1: (2, 64, 0, 16, 16, 32), 2: (2, 100, 156, 16, 16, 32), 4: (2, 128, 0, 24, 24, 32), 8: (2, 100, 156, 24, 24, 32),
           0: (2, 128, 0, 24, 24, 8)}
GN_VEC4C = {1: (2, 50, 78, 16, 16, 32), 2: (2, 100, 156, 16, 16, 32)}
GN_VEC4_BWD = [(2, 100, 28, 8, 8, 8), (32, 64, 0, 36, 36, 32)]           # C/G = 16 > 8;  HW4 = 324 > 256 with N*G = 1024 (no split form)
GN_SCALAR = [(2, 20, 12, 3, 3, 8), (2, 128, 0, 23, 23, 8)]               # HW % 4 != 0: cached (36 per group) / streaming (8464 per group)
GN_SPLIT = {1: (2, 20, 44, 32, 32, 8), '>1': (1, 32, 0, 128, 128, 8)}


def _reg_gn_fwd():
    for nv, shp in GN_WAVE.items():
        @case('gn_fwd_wave_kernel<%d>' % nv)
        def c(ops, shp=shp, nv=nv):
            name = gn_fwd_name(shp[0], shp[1] + shp[2], shp[3] * shp[4], shp[5])
            assert name == 'gn_fwd_wave_kernel<%d>' % nv
            yield run_gn_fwd(ops, *shp, True, [name])
    for ni, shp in GN_VEC4.items():
        @case('gn_fwd_vec4_kernel<%d>' % ni)
        def c(ops, shp=shp, ni=ni):
            name = gn_fwd_name(shp[0], shp[1] + shp[2], shp[3] * shp[4], shp[5])
            assert name == 'gn_fwd_vec4_kernel<%d>' % ni
            yield run_gn_fwd(ops, *shp, ni != 4, [name])
    for key, shp in zip(('cached', 'streaming'), GN_SCALAR):
        @case('gn_fwd_kernel | ' + key)
        def c(ops, shp=shp, key=key):
            per = (shp[1] + shp[2]) // shp[5] * shp[3] * shp[4]
            assert (shp[3] * shp[4]) % 4 and (per <= 8192) == (key == 'cached')
            yield run_gn_fwd(ops, *shp, True, ['gn_fwd_kernel'])
    for sl, shp in GN_SPLIT.items():
        key = 'slices == 1' if sl == 1 else 'slices > 1'

        @case(*['gn_split_%s_fwd_kernel | %s' % (k, key) for k in ('part', 'combine', 'apply')])
        def c(ops, shp=shp, sl=sl):
            yield run_gn_fwd(ops, *shp, True, ['gn_split_part_fwd_kernel', 'gn_split_combine_fwd_kernel', 'gn_split_apply_fwd_kernel'],
                             slices=sl)


_reg_gn_fwd()
_ADDS = ((False, False), (True, False), (False, True), (True, True))


def _reg_gn_bwd():
    for fam, table in (('wave', GN_WAVE), ('vec4c', GN_VEC4C)):
        for nv, shp in table.items():
            for i, (a1, a2) in enumerate(_ADDS):
                @case('gn_bwd_%s_kernel<%d, %s>' % (fam, nv, _GN_ADDS[i]))
                def c(ops, shp=shp, a1=a1, a2=a2, i=i):
                    name = gn_bwd_name(shp[0], shp[1] + shp[2], shp[3] * shp[4], shp[5], a1, a2)
                    yield run_gn_bwd(ops, *shp, True, a1, a2, i % 2 == 0, [name])
                    yield run_gn_bwd(ops, *shp, False, a1, a2, i % 2 == 1, [name])

    @case('gn_bwd_vec4_kernel')
    def c4(ops):
        for shp in GN_VEC4_BWD:
            for i, (a1, a2) in enumerate(_ADDS):
                assert gn_bwd_name(shp[0], shp[1] + shp[2], shp[3] * shp[4], shp[5], a1, a2) == 'gn_bwd_vec4_kernel'
                yield run_gn_bwd(ops, *shp, True, a1, a2, i % 2 == 0, ['gn_bwd_vec4_kernel'])

    @case('gn_bwd_kernel')
    def cs(ops):
        for shp in GN_SCALAR:
            for i, (a1, a2) in enumerate(_ADDS):
                yield run_gn_bwd(ops, *shp, True, a1, a2, i % 2 == 1, ['gn_bwd_kernel'])

    for i, (a1, a2) in enumerate(_ADDS):
        @case('gn_split_apply_bwd_kernel<%s>' % _GN_ADDS[i])
        def c(ops, a1=a1, a2=a2, i=i):
            for shp in GN_SPLIT.values():
                yield run_gn_bwd(ops, *shp, True, a1, a2, i == 3, ['gn_split_part_bwd_kernel', 'gn_split_combine_bwd_kernel',
                                                                    'gn_split_apply_bwd_kernel<%s>' % _GN_ADDS[i]])
    for sl, shp in GN_SPLIT.items():
        key = 'slices == 1' if sl == 1 else 'slices > 1'

        @case('gn_split_part_bwd_kernel | ' + key, 'gn_split_combine_bwd_kernel | ' + key)
        def c(ops, shp=shp, sl=sl):
            N, C1, C2, H, W, G = shp
            got = ops._gn_slices(N, G, H * W, (), ())
            assert got == 1 if sl == 1 else got > 1
            yield run_gn_bwd(ops, *shp, False, True, False, False, ['gn_split_part_bwd_kernel', 'gn_split_combine_bwd_kernel',
                                                                     'gn_split_apply_bwd_kernel<true, false>'])


_reg_gn_bwd()


# ======================================================================================================================
# column / row sums
# ======================================================================================================================
@case('colsum_kernel')
def colsum(ops):
    for N, C, ws, wo, acc in ((256, 256, 2, 1, True), (7, 90, 1, 0, False), (128, 513, 1, 0, True), (3, 64, 2, 0, False), (37, 70, 3, 2, True)):
        src, dst = rnd(N, C, ws, seed=N), rnd(C, seed=C)
        d0 = dst.clone()
        _, names = launched(ops, lambda: ops.colsum_accum(src, N, C, ws, wo, dst, acc))
        assert names == ['colsum_kernel']
        ref = d64(src)[:, :, wo].sum(0) + (d64(d0) if acc else 0)
        yield dict(names=names, shape=(N, C, ws, wo, acc), out=relerr(dst, ref), bound=1e-5)


@case('colsum_batch_kernel')
def colsum_batch(ops):
    """A repeated destination inside one flush closes the launch: 3 launches for [a, b, a, c, a], each sum complete and in order;
    and 170 distinct items: ceil(170 / 80) = 3 launches."""
    q = ops.ColsumQueue()
    a, b, c = rnd(90, seed=1), rnd(64, seed=2), rnd(513, seed=3)
    a0, c0 = a.clone(), c.clone()
    s = [rnd(7, 90, 2, seed=4), rnd(33, 64, 1, seed=5), rnd(19, 90, 1, seed=6), rnd(128, 513, 1, seed=7), rnd(5, 90, 3, seed=8)]
    q.add(s[0], 7, 90, 2, 1, a, True)
    q.add(s[1], 33, 64, 1, 0, b, False)
    q.add(s[2], 19, 90, 1, 0, a, True)
    q.add(s[3], 128, 513, 1, 0, c, True)
    q.add(s[4], 5, 90, 3, 2, a, True)
    _, names = launched(ops, q.flush)
    assert names == ['colsum_batch_kernel'] * 3, names
    ra = d64(a0) + d64(s[0])[:, :, 1].sum(0) + d64(s[2])[:, :, 0].sum(0) + d64(s[4])[:, :, 2].sum(0)
    yield dict(names=names, a=relerr(a, ra), b=relerr(b, d64(s[1])[:, :, 0].sum(0)), c=relerr(c, d64(c0) + d64(s[3])[:, :, 0].sum(0)),
               bound=1e-5)
    srcs = [rnd(5 + i % 9, 30 + i, 2, seed=i) for i in range(170)]
    dsts = [torch.zeros(30 + i, device=DEV) for i in range(170)]
    for i in range(170):
        q.add(srcs[i], 5 + i % 9, 30 + i, 2, i % 2, dsts[i], False)
    _, names = launched(ops, q.flush)
    assert names == ['colsum_batch_kernel'] * 3, names
    yield dict(names=names, items=170, out=max(relerr(dsts[i], d64(srcs[i])[:, :, i % 2].sum(0)) for i in range(170)), bound=1e-5)


def _rowsum(ops, name, shape, lead):
    big = rnd(*shape, seed=17)
    v = big[:, lead:lead + 3]
    HW = shape[2] * shape[3]
    vec4 = HW % 4 == 0 and (shape[1] * HW) % 4 == 0 and v.data_ptr() % 16 == 0
    assert name == ('rowsum_plane_kernel' if HW >= 4096 else 'rowsum_kernel') + ('<true>' if vec4 else '<false>'), (shape, lead, vec4)
    poison(shape[0] * 3)
    rows, names = launched(ops, lambda: ops.rowsum_nc(v))
    assert names == [name], names
    return dict(names=names, shape=shape, HW=HW, out=relerr(rows, d64(v).sum((2, 3))), bound=1e-5)


@case('rowsum_kernel<true>')
def rowsum_t(ops):                                            # HW = 4092 (just below the plane form), 64, 4
    for shape in ((3, 5, 62, 66), (4, 6, 8, 8), (130, 7, 2, 2)):
        yield _rowsum(ops, 'rowsum_kernel<true>', shape, 1)


@case('rowsum_kernel<false>')
def rowsum_f(ops):                                            # HW = 4095 / 4092 behind an unaligned image stride / 15
    for shape in ((2, 4, 63, 65), (2, 4, 5, 3)):
        yield _rowsum(ops, 'rowsum_kernel<false>', shape, 1)
    x = rnd(2 * 5 * 4092 + 3, seed=3)[3:].view(2, 5, 62, 66)         # 16-byte alignment broken by the view's offset
    rows, names = launched(ops, lambda: ops.rowsum_nc(x[:, 1:4]))
    assert names == ['rowsum_kernel<false>'] and x.data_ptr() % 16
    yield dict(names=names, shape=(2, 3, 62, 66), out=relerr(rows, d64(x[:, 1:4]).sum((2, 3))), bound=1e-5)


@case('rowsum_plane_kernel<true>')
def rowsum_pt(ops):                                           # HW = 4096 exactly, and 16384
    for shape in ((3, 5, 64, 64), (2, 4, 128, 128)):
        yield _rowsum(ops, 'rowsum_plane_kernel<true>', shape, 1)


@case('rowsum_plane_kernel<false>')
def rowsum_pf(ops):                                           # HW = 4097 / 4489
    for shape in ((2, 4, 17, 241), (2, 3, 67, 67)):
        yield _rowsum(ops, 'rowsum_plane_kernel<false>', shape, 0)


# ======================================================================================================================
# grid-stride kernels: n below one workgroup and n = 3 * cap + 77 (fourth trip of the loop, ragged end); the 4-D entry points on
# channel slices of wider buffers with more than 2 * cap elements
# ======================================================================================================================
def trips(total):
    assert total > 2 * CAP and total % 256, total
    return total


SHAPE4 = (3, 87, 128, 127)            # 4 242 816 elements: third trip, ragged
assert 3 * 87 * 128 * 127 > 2 * CAP and (3 * 87 * 128 * 127) % 256


def _flat(ops, name, call, ref, n_in, exact=False, sizes=(77, BIG)):
    for n in sizes:
        xs = [rnd(n, seed=10 * i + n % 7, scale=2.0) for i in range(n_in)]
        poison(n)
        out, names = launched(ops, lambda: call(*xs))
        assert names == [name], names
        r = ref(*[d64(t) for t in xs])
        if exact:
            assert torch.equal(out.cpu().double(), r)
        yield dict(names=names, n=n, out=relerr(out, r), bound=0.0 if exact else 1e-5)


@case('silu_fwd_kernel')
def silu_fwd(ops):
    yield from _flat(ops, 'silu_fwd_kernel', ops.silu_fwd, F.silu, 1)


@case('silu_bwd_kernel')
def silu_bwd(ops):
    def ref(x, dy):
        s = torch.sigmoid(x)
        return dy * s * (1 + x * (1 - s))
    yield from _flat(ops, 'silu_bwd_kernel', ops.silu_bwd, ref, 2)
    for n in (77, BIG):
        x, dy, acc = rnd(n, seed=1, scale=2.0), rnd(n, seed=2), rnd(n, seed=3)
        a0 = acc.clone()
        _, names = launched(ops, lambda: ops.silu_bwd(x, dy, out=acc, accumulate=True))
        assert names == ['silu_bwd_kernel']
        yield dict(names=names, n=n, accumulate=True, out=relerr(acc, d64(a0) + ref(d64(x), d64(dy))), bound=1e-5)


@case('axpby_kernel')
def axpby(ops):
    for n in (77, BIG):
        for b in (-0.5, 0.0):
            x, y = rnd(n, seed=1), rnd(n, seed=2)
            y0 = y.clone()
            if b == 0.0:
                y.fill_(float('nan'))                         # b == 0 overwrites: y is not read
            _, names = launched(ops, lambda: ops.axpby(x, 2.0, y, b))
            assert names == ['axpby_kernel']
            yield dict(names=names, n=n, b=str(b), out=relerr(y, 2.0 * d64(x) + (b * d64(y0) if b else 0)), bound=1e-5)


@case('cfg_combine_kernel')
def cfg_combine(ops):
    yield from _flat(ops, 'cfg_combine_kernel', lambda u, c: ops.cfg_combine(u, c, 3.0), lambda u, c: u + 3.0 * (c - u), 2)


@case('ddim_step_kernel')
def ddim_step(ops):
    a_t, a_prev, std = 0.37, 0.52, 0.11

    def ref(x, e, vn=None, clip=None):
        x0 = (x - (1 - a_t) ** 0.5 * e) / a_t ** 0.5
        if clip:
            x0 = x0.clamp(-clip, clip)
        s = std if vn is not None else 0.0
        return a_prev ** 0.5 * x0 + (1 - a_prev - s * s) ** 0.5 * e + (s * vn if vn is not None else 0)
    yield from _flat(ops, 'ddim_step_kernel', lambda x, e: ops.ddim_step(x, e, a_t, a_prev, clip=True, clip_range=0.8),
                     lambda x, e: ref(x, e, None, 0.8), 2)
    yield from _flat(ops, 'ddim_step_kernel', lambda x, e, vn: ops.ddim_step(x, e, a_t, a_prev, std=std, vnoise=vn, clip=False),
                     lambda x, e, vn: ref(x, e, vn, None), 3)


@case('ddpm_step_kernel')
def ddpm_step(ops):
    sa, sb, c0, c1, sig = 0.61, 0.79, 0.013, 0.985, 0.07
    yield from _flat(ops, 'ddpm_step_kernel', lambda x, e, vn: ops.ddpm_step(x, e, sa, sb, c0, c1, sig, vn, clip=True, clip_range=0.8),
                     lambda x, e, vn: c0 * ((x - sb * e) / sa).clamp(-0.8, 0.8) + c1 * x + sig * vn, 3)
    yield from _flat(ops, 'ddpm_step_kernel', lambda x, e: ops.ddpm_step(x, e, sa, sb, c0, c1, clip=False),
                     lambda x, e: c0 * ((x - sb * e) / sa) + c1 * x, 2)


@case('scale_if_stopped_kernel')
def zero_if_stopped(ops):
    for n in (77, BIG):
        for stopped in (0.0, 1.0):
            x = rnd(n, seed=1)
            x0 = x.clone()
            state = torch.tensor([1.0, stopped, 3.0], device=DEV)
            _, names = launched(ops, lambda: ops.zero_if_stopped(x, state))
            assert names == ['scale_if_stopped_kernel']
            assert torch.equal(x, torch.zeros_like(x) if stopped else x0)
            yield dict(names=names, n=n, stopped=bool(stopped), out=0.0, bound=0.0)


def _per_image(ops, name, call, ref, shapes=((3, 5, 3, 5), (3, 87, 128, 127))):
    """x0 / noise [B, ...] contiguous with a per-image coefficient looked up through a timestep vector."""
    for shp in shapes:
        B = shp[0]
        if shp[1] > 5:
            trips(B * shp[1] * shp[2] * shp[3])
        x0, nz = rnd(*shp, seed=1), rnd(*shp, seed=2)
        t = torch.tensor([999, 0, 417][:B], dtype=torch.long, device=DEV)
        tab = torch.linspace(0.9999, 0.00004, 1000, device=DEV)
        tab2 = (1 - tab * tab).sqrt()
        poison(x0.numel())
        out, names = launched(ops, lambda: call(x0, nz, tab, tab2, t))
        assert names == [name], names
        a, b = (d64(v)[t.cpu()].view(B, 1, 1, 1) for v in (tab, tab2))
        yield dict(names=names, shape=shp, out=relerr(out, ref(d64(x0), d64(nz), a, b)), bound=1e-5)


@case('add_noise_kernel')
def add_noise(ops):
    yield from _per_image(ops, 'add_noise_kernel', lambda x, nz, acp, _, t: ops.add_noise(x, nz, acp, t),
                          lambda x, nz, a, _: a.sqrt() * x + (1 - a).sqrt() * nz)


@case('q_sample_kernel')
def q_sample(ops):
    yield from _per_image(ops, 'q_sample_kernel', ops.q_sample, lambda x, nz, a, b: a * x + b * nz)


@case('copy_strided_kernel')
def copy_strided(ops):
    for shp in ((3, 4, 4, 4), SHAPE4):
        for acc in (False, True):
            N, C, H, W = shp
            src = wide(N, C, H, W, 1)[0]
            dst, big = wide(N, C, H, W, 2, lead=3, extra=4)
            before = big.clone()
            _, names = launched(ops, lambda: ops.copy_strided(src, dst, accumulate=acc))
            assert names == ['copy_strided_kernel']
            ref = d64(src) + (d64(before[:, 3:3 + C]) if acc else 0)
            assert outside_intact(big, before, 3, C) and (acc or torch.equal(dst, src))
            yield dict(names=names, shape=shp, accumulate=acc, out=relerr(dst, ref), bound=1e-5 if acc else 0.0)


@case('dropout_apply_kernel')
def dropout_apply(ops):
    from oracle import philox_ref as PH
    for shp in ((3, 5, 6, 6), SHAPE4):
        N, C, H, W = shp
        x = wide(N, C, H, W, 1)[0]
        out, big = wide(N, C, H, W, 0, fill=777.0)
        before = big.clone()
        d = ops.dropout_desc(0.25, 11, 'a.dropout', 2, n_off=5)
        y, names = launched(ops, lambda: ops.dropout_apply(x, d, out=out))
        assert names == ['dropout_apply_kernel']
        m = torch.from_numpy(PH.dropout_multipliers(x.numel(), 0.25, 11, 'a.dropout', 2, 5 * x[0].numel())).view(shp)
        assert outside_intact(big, before, 2, C)
        bad = int((y.cpu() != x.cpu() * m).sum())
        assert bad == 0, bad
        yield dict(names=names, shape=shp, mismatches=bad, out=0.0, bound=0.0)


@case('geglu_fwd_kernel')
def geglu_fwd(ops):
    for N, C, H, W in ((2, 3, 3, 5), SHAPE4):
        z = rnd(N, 2 * C, H, W, seed=6)
        poison(N * C * H * W)
        o, names = launched(ops, lambda: ops.geglu_fwd(z))
        assert names == ['geglu_fwd_kernel']
        a, g = d64(z).chunk(2, dim=1)
        yield dict(names=names, shape=(N, 2 * C, H, W), out=relerr(o, a * F.gelu(g)), bound=1e-5)


@case('geglu_bwd_kernel')
def geglu_bwd(ops):
    for N, C, H, W in ((2, 3, 3, 5), SHAPE4):
        z, do = rnd(N, 2 * C, H, W, seed=6), rnd(N, C, H, W, seed=7)
        poison(N * 2 * C * H * W)
        dz, names = launched(ops, lambda: ops.geglu_bwd(z, do))
        assert names == ['geglu_bwd_kernel']
        a, g = d64(z).chunk(2, dim=1)
        dgelu = 0.5 * (1 + torch.erf(g / math.sqrt(2))) + g * torch.exp(-0.5 * g * g) / math.sqrt(2 * math.pi)
        ref = torch.cat([d64(do) * F.gelu(g), d64(do) * a * dgelu], 1)
        yield dict(names=names, shape=(N, 2 * C, H, W), out=relerr(dz, ref), bound=1e-5)


@case('add_rowvec_kernel')
def add_rowvec(ops):
    for shp in ((2, 3, 3, 5), SHAPE4):
        N, C, H, W = shp
        x, v = wide(N, C, H, W, 1)[0], rnd(N, C, seed=8)
        out, big = wide(N, C, H, W, 0, fill=777.0)
        before = big.clone()
        o, names = launched(ops, lambda: ops.add_rowvec(x, v, out=out))
        assert names == ['add_rowvec_kernel'] and outside_intact(big, before, 2, C)
        yield dict(names=names, shape=shp, out=relerr(o, d64(x) + d64(v)[:, :, None, None]), bound=1e-5)


@case('downsum_kernel')
def downsum(ops):
    for shp in ((2, 3, 4, 5), (3, 87, 128, 127)):             # output shape; dy is twice as high and wide
        N, C, H, W = shp
        dy = wide(N, C, 2 * H, 2 * W, 1)[0]
        out, big = wide(N, C, H, W, 0, fill=777.0)
        before = big.clone()
        o, names = launched(ops, lambda: ops.downsum2x2(dy, out=out))
        assert names == ['downsum_kernel'] and outside_intact(big, before, 2, C)
        yield dict(names=names, shape=shp, out=relerr(o, F.avg_pool2d(d64(dy), 2) * 4), bound=1e-5)


def _upsample(ops, key, shapes, misalign=False):
    for N, C, H, W in shapes:
        x = wide(N, C, H, W, 1)[0]
        if misalign:                                          # an odd image stride breaks the 8-byte loads
            x = rnd(N, C * H * W + 1, seed=1)[:, :C * H * W].view(N, C, H, W)
        vec = W % 2 == 0 and x.stride(0) % 2 == 0 and x.data_ptr() % 8 == 0
        assert vec == (key == 'vec')
        threads = N * C * 2 * H * (W // 2 if vec else 2 * W)
        if C > 8:
            trips(threads)
        poison(N * C * 4 * H * W)
        y, names = launched(ops, lambda: ops.upsample2x(x))
        assert names == ['upsample2x_kernel']
        assert torch.equal(y, x.repeat_interleave(2, 2).repeat_interleave(2, 3))
        yield dict(names=names, shape=(N, C, H, W), path=key, threads=threads, out=0.0, bound=0.0)


@case('upsample2x_kernel | vec')
def upsample_vec(ops):
    yield from _upsample(ops, 'vec', ((2, 3, 3, 4), (3, 89, 127, 126)))


@case('upsample2x_kernel | scalar')
def upsample_scalar(ops):
    yield from _upsample(ops, 'scalar', ((2, 3, 3, 5), (3, 45, 127, 63)))
    yield from _upsample(ops, 'scalar', ((2, 3, 3, 4),), misalign=True)


def _ref_interleave(q):
    _, N, C, Ho, Wo = q.shape
    y = torch.empty(N, C, 2 * Ho, 2 * Wo, dtype=q.dtype, device=q.device)
    for ph in (0, 1):
        for pw in (0, 1):
            y[:, :, ph::2, pw::2] = q[2 * ph + pw]
    return y


def _interleave(ops, key, shapes):
    for N, C, Ho, Wo in shapes:
        vec = Wo % 2 == 0 and (N * C * Ho * Wo) % 2 == 0 and (C * Ho * Wo) % 2 == 0
        assert vec == (key == 'vec')
        threads = N * C * 2 * Ho * (Wo // 2 if vec else 2 * Wo)
        if C > 8:
            trips(threads)
        for with_add in (False, True):
            q = rnd(4, N, C, Ho, Wo, seed=1)
            add = wide(N, C, 2 * Ho, 2 * Wo, 2)[0] if with_add else None
            poison(N * C * 4 * Ho * Wo)
            y, names = launched(ops, lambda: ops.interleave2x2(q, add=add))
            assert names == ['interleave2x2_kernel']
            ref = _ref_interleave(q)
            if with_add:
                ref = ref + add                               # one fp32 addition: exact in both
            assert torch.equal(y, ref)
            yield dict(names=names, shape=(N, C, Ho, Wo), path=key, add=with_add, threads=threads, out=0.0, bound=0.0)


@case('interleave2x2_kernel | vec')
def interleave_vec(ops):
    yield from _interleave(ops, 'vec', ((2, 3, 3, 4), (3, 89, 127, 126)))


@case('interleave2x2_kernel | scalar')
def interleave_scalar(ops):
    yield from _interleave(ops, 'scalar', ((2, 3, 3, 5), (3, 45, 127, 63)))


def _deinterleave(ops, key, shapes):
    for N, C, Ho, Wo in shapes:
        y = wide(N, C, 2 * Ho, 2 * Wo, 1)[0]
        vec = Wo % 2 == 0 and (N * C * Ho * Wo) % 2 == 0 and (C * Ho * Wo) % 2 == 0
        assert vec == (key == 'vec')
        threads = N * C * 2 * Ho * (Wo // 2 if vec else 2 * Wo)
        if C > 8:
            trips(threads)
        poison(N * C * 4 * Ho * Wo)
        q, names = launched(ops, lambda: ops.deinterleave2x2(y))
        assert names == ['deinterleave2x2_kernel']
        assert torch.equal(_ref_interleave(q), y)
        yield dict(names=names, shape=(N, C, Ho, Wo), path=key, threads=threads, out=0.0, bound=0.0)


@case('deinterleave2x2_kernel | vec')
def deinterleave_vec(ops):
    yield from _deinterleave(ops, 'vec', ((2, 3, 3, 4), (3, 89, 127, 126)))


@case('deinterleave2x2_kernel | scalar')
def deinterleave_scalar(ops):
    yield from _deinterleave(ops, 'scalar', ((2, 3, 3, 5), (3, 45, 127, 63)))


def _ups_t(parity, k):
    return (0 if k == 0 else 1) if parity == 0 else (1 if k == 2 else 0)


@case('ups_weff_kernel')
def ups_weff(ops):
    for M in (77, CAP + 77):                                  # one thread per (Cout, Cin) pair
        w = rnd(1, M, 3, 3, seed=1)
        poison(16 * M)
        weff, names = launched(ops, lambda: ops.ups_weff(w))
        assert names == ['ups_weff_kernel']
        wr, ref = d64(w), torch.zeros(4, 1, M, 2, 2, dtype=torch.float64)
        for cls in range(4):
            for ky in range(3):
                for kx in range(3):
                    ref[cls, :, :, _ups_t(cls >> 1, ky), _ups_t(cls & 1, kx)] += wr[:, :, ky, kx]
        yield dict(names=names, M=M, out=relerr(weff, ref), bound=1e-5)


@case('ups_wfold_kernel')
def ups_wfold(ops):
    for M in (77, CAP + 77):
        for acc in (False, True):
            gweff, gw = rnd(4, 1, M, 2, 2, seed=1), rnd(1, M, 3, 3, seed=2)
            g0 = gw.clone()
            if not acc:
                gw.fill_(float('nan'))
            _, names = launched(ops, lambda: ops.ups_wfold(gweff, gw, accumulate=acc))
            assert names == ['ups_wfold_kernel']
            ge, ref = d64(gweff), (d64(g0) if acc else torch.zeros(1, M, 3, 3, dtype=torch.float64))
            for cls in range(4):
                for ky in range(3):
                    for kx in range(3):
                        ref[:, :, ky, kx] += ge[cls, :, :, _ups_t(cls >> 1, ky), _ups_t(cls & 1, kx)]
            yield dict(names=names, M=M, accumulate=acc, out=relerr(gw, ref), bound=1e-5)


# ======================================================================================================================
# softmax
# ======================================================================================================================
def run_softmax(ops, s, scale=0.125):
    cols = s.shape[-1]
    poison(s.numel())
    p, names = launched(ops, lambda: ops.softmax_fwd(s))
    assert names == ['softmax_fwd_kernel']
    res = dict(names=names, shape=tuple(s.shape), fwd=relerr(p, d64(s).softmax(-1)))
    dp_ = rnd(*s.shape, seed=2)
    p2 = ops.softmax_fwd(s * scale)
    poison(s.numel())
    ds, names2 = launched(ops, lambda: ops.softmax_bwd(p2, dp_, scale))
    assert names2 == ['softmax_bwd_kernel']
    sr = d64(s * scale).requires_grad_(True)                  # the kernel's input is the fp32 product s * scale
    sr.softmax(-1).backward(d64(dp_))
    res.update(names_bwd=names2, bwd=relerr(ds, sr.grad * scale), cols=cols)
    return res


@case('softmax_fwd_kernel | cols <= 1024')
def softmax_cached(ops):
    for shape in ((6, 256, 256), (5, 16, 16), (3, 7, 1024), (2, 3, 1), (1, 5, 65)):       # 5, 21, 6 rows: ragged last workgroup of 4 rows
        assert shape[-1] <= 1024
        r = run_softmax(ops, rnd(*shape, seed=1, scale=3.0))
        yield dict(names=r['names'], shape=shape, out=r['fwd'], bound=1e-5)


@case('softmax_fwd_kernel | cols > 1024')
def softmax_streaming(ops):
    for shape in ((3, 4, 1025), (3, 5, 1500), (1, 2, 4099)):
        assert shape[-1] > 1024
        r = run_softmax(ops, rnd(*shape, seed=1, scale=3.0))
        yield dict(names=r['names'], shape=shape, out=r['fwd'], bound=1e-5)


@case('softmax_bwd_kernel')
def softmax_bwd(ops):
    for shape in ((6, 256, 256), (5, 16, 16), (3, 5, 1500), (2, 3, 1), (1, 5, 65)):
        r = run_softmax(ops, rnd(*shape, seed=1, scale=3.0))
        yield dict(names=r['names_bwd'], shape=shape, out=r['bwd'], bound=1e-5)


# ======================================================================================================================
# importance
# ======================================================================================================================
_WG_F = {0: lambda t: t.abs().pow(2), 1: lambda t: t.abs(), 2: lambda t: t, 4: None, 5: lambda t: t}


def ref_wg(w, g, dim, mode):
    """fp64 Taylor / Fisher channel reduction of one member ([R, C, T...] weight and gradient)."""
    if mode == 3:
        return (w * g).abs()
    t = g * g if mode == 4 else _WG_F[mode](w * g)
    s = (t if dim == 0 else t.transpose(0, 1)).flatten(1).sum(1)
    return s.abs() if mode == 2 else s


@case('wg_gn_kernel')
def wg_gn(ops):
    for R in (96, 1000):
        for acc in (False, True):
            w, g, o = rnd(R, seed=7), rnd(R, seed=8), rnd(R, seed=9)
            o0 = o.clone()
            _, names = launched(ops, lambda: ops.wg_reduce(w, g, 0, 3, o, acc))
            assert names == ['wg_gn_kernel']
            yield dict(names=names, R=R, out=relerr(o, ref_wg(d64(w), d64(g), 0, 3) + (d64(o0) if acc else 0)), bound=1e-5)


@case('wg_rows_kernel')
def wg_rows(ops):
    for shape in ((70, 37, 3, 3), (50, 64), (3, 5, 1, 1)):
        for mode in (0, 1, 2, 4, 5):
            w, g, o = rnd(*shape, seed=3), rnd(*shape, seed=4), rnd(shape[0], seed=5)
            o0, acc = o.clone(), mode % 2 == 1
            _, names = launched(ops, lambda: ops.wg_reduce(w, g, 0, mode, o, acc))
            assert names == ['wg_rows_kernel']
            yield dict(names=names, shape=shape, mode=mode, out=relerr(o, ref_wg(d64(w), d64(g), 0, mode) + (d64(o0) if acc else 0)),
                       bound=1e-5)


@case('wg_cols_ct_kernel', 'wg_fold_taps_kernel')
def wg_cols(ops):
    for shape in ((70, 37, 3, 3), (50, 64), (3, 300, 1, 1), (9, 5, 2, 2)):
        for mode in (0, 1, 2, 4, 5):
            w, g, o = rnd(*shape, seed=3), rnd(*shape, seed=4), rnd(shape[1], seed=5)
            o0, acc = o.clone(), mode % 2 == 0
            _, names = launched(ops, lambda: ops.wg_reduce(w, g, 1, mode, o, acc))
            assert names == ['wg_cols_ct_kernel', 'wg_fold_taps_kernel']
            yield dict(names=names, shape=shape, mode=mode, out=relerr(o, ref_wg(d64(w), d64(g), 1, mode) + (d64(o0) if acc else 0)),
                       bound=1e-5)


@case('gather_add_kernel')
def gather_add(ops):
    for n, m in ((37, 90), (1000, 1000)):
        src, dst = rnd(m, seed=1), rnd(n, seed=2)
        idx = torch.randperm(m, generator=torch.Generator().manual_seed(n))[:n].to(DEV)
        d0 = dst.clone()
        _, names = launched(ops, lambda: ops.gather_add(src, idx, dst))
        assert names == ['gather_add_kernel'] and torch.equal(dst, d0 + src[idx])
        yield dict(names=names, n=n, out=0.0, bound=0.0)


@case('group_score_part_kernel', 'group_score_combine_kernel')
def group_score(ops):
    """7, 24, 25 and 53 members (1, 1, 2 and 3 chunks of <= 24; the later chunks accumulate) against the member-by-member fp64 sum."""
    n0 = 48
    for n_members in (7, 24, 25, 53):
        members, idx_host, need, ref = [], [], 0, torch.zeros(n0, dtype=torch.float64)
        for i in range(n_members):
            kind, mode = i % 4, (0, 1, 2, 0, 4, 5)[i % 6]
            gen = torch.Generator().manual_seed(100 + i)
            if kind == 0:                                     # GroupNorm weight
                shape, m = (n0,), dict(R=n0, C=1, T=1, dim=0, mode=3)
            elif kind == 1:                                   # out-channel member
                shape, m = (n0, 5 + i, 3, 3), dict(R=n0, C=5 + i, T=9, dim=0, mode=mode)
            elif kind == 2:                                   # in-channel member, 3 x 3 taps
                shape, m = (7 + i, n0, 3, 3), dict(R=7 + i, C=n0, T=9, dim=1, mode=mode)
            else:                                             # in-channel member of a wider layer: an index list picks its channels
                shape, m = (11, n0 + 16, 1, 1), dict(R=11, C=n0 + 16, T=1, dim=1, mode=mode)
            w, g = torch.randn(*shape, generator=gen).to(DEV), torch.randn(*shape, generator=gen).to(DEV)
            m.update(w=w, g=g, full_off=0, col_off=0, idx_off=-1)
            full = ref_wg(d64(w), d64(g), m['dim'], m['mode'])
            if m['mode'] != 3 and m['dim'] == 1:
                m['col_off'] = need
                need += m['C'] * m['T']
            else:
                m['full_off'] = need
                need += m['R']
            if kind == 3:
                idxs = [(3 * j + i) % (n0 + 16) for j in range(n0)]
                m['idx_off'] = len(idx_host)
                idx_host.extend(idxs)
                full = full[idxs]
            ref += full
            members.append(m)
        scratch = torch.full((need,), float('nan'), device=DEV)
        idx_dev = torch.tensor(idx_host, dtype=torch.long, device=DEV) if idx_host else None
        score = torch.full((n0,), float('nan'), device=DEV)
        _, names = launched(ops, lambda: ops.group_score(members, n0, idx_dev, scratch, score))
        assert names == ['group_score_part_kernel', 'group_score_combine_kernel'] * ((n_members + 23) // 24), names
        yield dict(names=names, members=n_members, out=relerr(score, ref), bound=1e-5)


@case('slice_batch_kernel')
def slice_batch(ops):
    """5, 48, 49 and 101 items (1, 1, 2 and 3 launches), both dims, one item large enough for a second trip of its 256-workgroup loop."""
    for n_items in (5, 48, 49, 101):
        items, keep_host, want = [], [], []
        for i in range(n_items):
            dim = i % 2
            R, C, T = (600, 500, 9) if i == 2 else (5 + i % 7, 6 + i % 5, (1, 9, 4)[i % 3])
            src = torch.randn(R, C, T, generator=torch.Generator().manual_seed(i)).to(DEV)
            full = R if dim == 0 else C
            keep = sorted(torch.randperm(full, generator=torch.Generator().manual_seed(1000 + i))[:max(1, full - 2)].tolist())
            dst = torch.full((len(keep), C, T) if dim == 0 else (R, len(keep), T), float('nan'), device=DEV)
            items.append((src, dst, R, C, T, dim, len(keep), len(keep_host)))
            keep_host.extend(keep)
            want.append(src.index_select(dim, torch.tensor(keep, device=DEV)))
        keep_dev = torch.tensor(keep_host, dtype=torch.long, device=DEV)
        _, names = launched(ops, lambda: ops.slice_batch(items, keep_dev))
        assert names == ['slice_batch_kernel'] * ((n_items + 47) // 48), names
        bad = sum(0 if torch.equal(it[1], w) else 1 for it, w in zip(items, want))
        assert bad == 0 and 598 * 500 * 9 > 256 * 1024
        yield dict(names=names, items=n_items, mismatching=bad, out=0.0, bound=0.0)


# ======================================================================================================================
# the remaining kernels of elementwise.hip
# ======================================================================================================================
@case('temb_kernel')
def temb(ops):
    """sin / cos of t * f in fp32.  The frequency f = expf(e) is within 2 ulp and the product is rounded once, so the ARGUMENT is off by up
    to 3 * 2^-24 * t f (1.8e-4 rad at t = 999) before sinf / cosf add their own ulp: the error is bounded per element, as
    |got - ref| <= 2e-7 * (1 + t), against sin / cos of the fp64 argument."""
    for B, dim, flip, shift in ((3, 128, False, 1.0), (5, 33, True, 0.0), (8200, 257, True, 1.0)):
        if B > 100:
            assert B * dim > CAP and (B * dim) % 256
        t = (torch.rand(B, generator=_gen(B)) * 999).to(DEV)
        poison(B * dim)
        emb, names = launched(ops, lambda: ops.timestep_embedding(t, dim, flip, shift))
        assert names == ['temb_kernel']
        half = dim // 2
        arg = d64(t)[:, None] * torch.exp(-math.log(10000.0) * torch.arange(half, dtype=torch.float64) / (half - shift))[None]
        first, second = (arg.cos(), arg.sin()) if flip else (arg.sin(), arg.cos())
        ref = torch.cat([first, second, torch.zeros(B, dim - 2 * half, dtype=torch.float64)], 1)
        yield dict(names=names, shape=(B, dim), flip=flip, scaled_err=float(((d64(emb) - ref).abs() / (1 + d64(t))[:, None]).max()),
                   bound=2e-7)


@case('mse_kernel', 'sum_partials_kernel')
def mse(ops):
    for n in (77, 24576, BIG):
        o, nz = rnd(n, seed=1), rnd(n, seed=2)
        poison(n)
        (loss, dout), names = launched(ops, lambda: ops.mse_fwd_bwd(o, nz, 2.0 / n, 1.0 / n))
        assert names == ['mse_kernel', 'sum_partials_kernel']
        d = d64(o) - d64(nz)
        yield dict(names=names, n=n, loss=relerr(loss, (d * d).sum().view(1) / n), dout=relerr(dout, 2.0 / n * d), bound=1e-5)
        state = torch.tensor([1.0, 1.0, 2.0], device=DEV)                      # stopped: the gradient of an overshoot step is an exact zero
        (loss2, dout2), names = launched(ops, lambda: ops.mse_fwd_bwd(o, nz, 2.0 / n, 1.0 / n, stop_state=state))
        assert torch.equal(loss2, loss) and float(dout2.abs().max()) == 0.0
        (loss3, none), names = launched(ops, lambda: ops.mse_fwd_bwd(o, nz, 2.0 / n, 1.0 / n, want_grad=False))
        assert none is None and torch.equal(loss3, loss)
        yield dict(names=names, n=n, variants='stopped, no gradient', out=0.0, bound=0.0)


@case('kd_kernel', 'kd_terms_kernel')
def kd(ops):
    for n in (77, 5000, BIG):
        S, T, E = rnd(n, seed=1), rnd(n, seed=2), rnd(n, seed=3)
        w_kd, w_eps, gs, ls = 0.7, 0.3, 2.0 / 64, 1.0 / 64
        poison(n)
        (terms, dout), names = launched(ops, lambda: ops.kd_fwd_bwd(S, T, E, w_kd, w_eps, gs, ls))
        assert names == ['kd_kernel', 'kd_terms_kernel']
        dk, de = d64(S) - d64(T), d64(S) - d64(E)
        kdv, epsv = ls * (dk * dk).sum(), ls * (de * de).sum()
        ref = torch.stack([w_kd * kdv + w_eps * epsv, kdv, epsv])
        yield dict(names=names, n=n, terms=float(((d64(terms) - ref).abs() / ref.abs()).max()), dout=relerr(dout, gs * (w_kd * dk + w_eps * de)),
                   bound=1e-5)


def _early_exit(ops, call, name, ratio):
    seq = [0.5, 0.8, 0.3, 0.081, 0.0799999, 0.5, 0.01]
    for thr in (0.1, -1.0, 0.5):
        state = torch.tensor([-1.0 if ratio else 0.0, 0.0, 0.0], device=DEV)
        rec, names = torch.zeros(16, device=DEV), []
        for l in seq:
            names += launched(ops, lambda: call(torch.tensor([l], device=DEV), thr, state, rec))[1]
        assert names == [name] * len(seq)
        mx, want = torch.tensor(-1.0 if ratio else 0.0), []
        for l in seq:                                          # the reference's lines on fp32 0-d tensors
            lt = torch.tensor(l, dtype=torch.float32)
            want.append(float(lt))
            if lt > mx:
                mx = lt
            if bool(lt / mx < thr) if ratio else bool(lt < mx * torch.tensor(thr, dtype=torch.float32)):
                break
        st = state.cpu().tolist()
        assert int(st[2]) == len(want) and rec[:len(want)].cpu().tolist() == want and float(mx) == st[0], (st, want)
        assert st[1] == (1.0 if len(want) < len(seq) else 0.0)
        yield dict(names=names[:1], thr=str(thr), steps=len(want), out=0.0, bound=0.0)


@case('early_exit_update_kernel')
def early_exit(ops):
    yield from _early_exit(ops, ops.early_exit_update, 'early_exit_update_kernel', False)


@case('early_exit_update_ratio_kernel')
def early_exit_ratio(ops):
    yield from _early_exit(ops, ops.early_exit_update_ratio, 'early_exit_update_ratio_kernel', True)


@case('dropout_mask_kernel')
def dropout_mask(ops):
    from oracle import philox_ref as PH
    for p, seed, site, step, idx0, n in ((0.1, 7, 'mid_block.resnets.0.dropout', 3, 0, 77), (0.5, (1 << 63) + 12345, 'x.to_out.1', 4000000000, (1 << 34) - 777, CAP + 77)):
        d = ops.dropout_desc(p, seed, site, step)
        poison(n)
        got, names = launched(ops, lambda: ops.dropout_mask(n, d, DEV, idx0))
        assert names == ['dropout_mask_kernel']
        bad = int((got.cpu().numpy() != PH.dropout_multipliers(n, p, seed, site, step, idx0)).sum())
        assert bad == 0, bad
        yield dict(names=names, n=n, mismatches=bad, out=0.0, bound=0.0)


@case('randn_philox_kernel')
def randn_philox(ops):
    """One thread per 4 draws: 4 * cap + 311 draws take a second trip.  Device logf / cosf / sinf against numpy: 5e-6 absolute on draws of
    at most 6.8 (tests/test_kernels_gpu.py::test_randn_philox_matches_oracle_and_is_shard_invariant)."""
    from oracle import philox_ref as PH
    for seed, sid, step, idx0, n in ((0, 0, 0, 2, 7), ((1 << 62) + 5, 3, 999, (1 << 34) + 3, 4 * CAP + 311)):
        poison(n)
        got, names = launched(ops, lambda: ops.randn_philox((n,), seed, sid, step, idx0=idx0, device=DEV))
        assert names == ['randn_philox_kernel']
        yield dict(names=names, n=n, abs_err=float(np.abs(got.cpu().numpy() - PH.randn(n, seed, sid, step, idx0)).max()), bound=5e-6)


@case('u8_to_float_kernel')
def u8_to_float(ops):
    from oracle import data_ref
    data = importlib.import_module('diff-pruning_amd.data')
    rng = np.random.default_rng(3)
    for hwc, shape in ((True, (2, 17, 23, 3)), (False, (5, 3, 32, 32)), (True, (75, 171, 171, 3))):
        if shape[0] > 50:
            assert np.prod(shape) > CAP and np.prod(shape) % 256
        u8 = rng.integers(0, 256, shape, dtype=np.uint8)
        for mode, flip, dq, n_off in ((1, 0.5, False, 0), (2, 0.5, True, 11), (0, 0.0, False, 3)):
            poison(int(np.prod(shape)))
            got, names = launched(ops, lambda: data.to_device_batch(u8, hwc, torch.device(DEV), mode, flip, seed=77, epoch=4, n_off=n_off, dequant=dq))
            assert names == ['u8_to_float_kernel']
            want = data_ref.transform_batch(u8, hwc, mode, flip, 77, 4, n_off, dq)
            assert torch.equal(got.cpu(), want), (hwc, shape, mode)
            yield dict(names=names, shape=shape, mode=mode, out=0.0, bound=0.0)


@case('pool2d_kernel')
def pool2d(ops):
    metrics = importlib.import_module('diff-pruning_amd.metrics')
    for shp, lead in (((3, 20, 35, 35), 0), ((2, 30, 17, 17), 4), ((3, 600, 35, 35), 2)):
        x = rnd(*shp, seed=1)[:, lead:shp[1] - lead] if lead else rnd(*shp, seed=1)
        for k, st, pad, mode, ref in ((3, 1, 1, 'avg', lambda t: F.avg_pool2d(t, 3, 1, 1, count_include_pad=False)),
                                      (3, 1, 1, 'max', lambda t: F.max_pool2d(t, 3, 1, 1)), (3, 2, 0, 'max', lambda t: F.max_pool2d(t, 3, 2))):
            y, names = launched(ops, lambda: metrics.pool2d(x, k, st, pad, mode))
            assert names == ['pool2d_kernel']
            if shp[1] == 600 and st == 1:
                assert y.numel() > CAP
            yield dict(names=names, shape=tuple(x.shape), pool=(k, st, pad, mode), out=relerr(y, ref(d64(x))), bound=2e-5)


@case('resize_bilinear_kernel')
def resize_bilinear(ops):
    """The kernel restates ATen's fp32 arithmetic: the source coordinate scale * (dst + 0.5) - 0.5 is rounded to fp32, which moves the
    interpolation weights by up to 300 * 2^-24 (measured: ATen fp32 is 3.7e-5 from fp64 on 300 x 280 -> 299 x 299).  So the fp64
    comparison follows max(4 e_ref32, 2e-6) with e_ref32 = ATen fp32 against fp64 on the same input, and the kernel stays within the older
    test's 2e-6 of ATen fp32 itself (values in [-1, 1])."""
    metrics = importlib.import_module('diff-pruning_amd.metrics')
    g = _gen(5)
    for shape, size, a, b in (((4, 3, 32, 32), (299, 299), 2.0, -1.0), ((2, 3, 300, 280), (299, 299), 1.0, 0.0), ((9, 3, 32, 32), (299, 299), 1.0, 0.0)):
        img = torch.rand(*shape, generator=g).to(DEV)
        if shape[0] == 9:
            assert 9 * 3 * 299 * 299 > CAP
        got, names = launched(ops, lambda: metrics.resize_bilinear(img, size, a, b))
        assert names == ['resize_bilinear_kernel']
        want = a * F.interpolate(d64(img), size=size, mode='bilinear', align_corners=False) + b
        want32 = a * F.interpolate(img.cpu(), size=size, mode='bilinear', align_corners=False) + b
        e_ref32 = float((want32.double() - want).abs().max())
        vs_aten = float((got.cpu() - want32).abs().max())
        assert vs_aten < 2e-6, vs_aten
        yield dict(names=names, shape=shape, abs_err=float((d64(got) - want).abs().max()), ref32=dict(e_ref32=e_ref32, vs_aten_fp32=vs_aten),
                   bound=max(4 * e_ref32, 2e-6))


@case('ssim_tile_kernel', 'ssim_finish_kernel')
def ssim(ops):
    from oracle import metrics_ref as M
    metrics = importlib.import_module('diff-pruning_amd.metrics')
    g = _gen(6)
    for shape in ((5, 3, 32, 32), (2, 3, 70, 45), (70, 1, 16, 19)):
        a = torch.rand(*shape, generator=g)
        b = (a + 0.1 * torch.randn(*shape, generator=g)).clamp(0, 1)
        got, names = launched(ops, lambda: metrics.ssim(a.to(DEV), b.to(DEV)))
        assert names == ['ssim_tile_kernel', 'ssim_finish_kernel']
        yield dict(names=names, shape=shape, out=relerr(got, M.ssim(a.double(), b.double())), bound=2e-5)


@case('mse_per_image_kernel')
def mse_per_image(ops):
    metrics = importlib.import_module('diff-pruning_amd.metrics')
    for shape in ((5, 3, 32, 32), (3, 1, 1, 7), (2, 3, 300, 280)):
        a, b = rnd(*shape, seed=1), rnd(*shape, seed=2)
        got, names = launched(ops, lambda: metrics.mse_per_image(a, b))
        assert names == ['mse_per_image_kernel']
        yield dict(names=names, shape=shape, out=relerr(got, ((d64(a) - d64(b)) ** 2).mean(dim=(1, 2, 3))), bound=2e-5)


@case('pack_weight_batch_kernel')
def pack_weight_batch(ops):
    """Pure data movement (and the Winograd weight transforms): element for element equal to the per-layer packers."""
    ws = [rnd(90, 45, 3, 3, seed=1), rnd(128, 256, 1, 1, seed=2), rnd(33, 70, seed=3), rnd(3, 96, 3, 3, seed=5)]
    items = [(w, m) for w in ws for m in (0, 1)] * 9                       # 72 items: more than one launch
    items += [(w, (kind, m)) for kind in ('wino', 'wino2d') for w in ws if w.dim() == 4 and w.shape[2] == 3 for m in (0, 1)]
    got, names = launched(ops, lambda: ops.pack_weight_batch(items))
    assert set(names) == {'pack_weight_batch_kernel'} and len(names) > 1, names
    for (w, m), (buf, ld) in zip(items, got):
        ref, ld0 = ({'wino': ops.pack_weight_wino, 'wino2d': ops.pack_weight_wino2d}[m[0]](w, m[1]) if isinstance(m, tuple)
                    else ops.pack_weight(w, m))
        assert ld == ld0 and torch.equal(buf, ref), (tuple(w.shape), m)
    yield dict(names=names, items=len(items), out=0.0, bound=0.0)


# ======================================================================================================================
# optim.hip, vq.hip
# ======================================================================================================================
@case('sumsq_kernel')
def sumsq(ops):
    for n in (77, 10000, BIG):
        x = rnd(n, seed=1)
        poison(512)
        partial, names = launched(ops, lambda: ops.sumsq_partials(x))
        assert names == ['sumsq_kernel']
        per = (n + 511) // 512
        ref = torch.stack([(d64(x)[b * per:(b + 1) * per] ** 2).sum() for b in range(512)])
        yield dict(names=names, n=n, partial=relerr(partial, ref), bound=1e-5)


@case('clip_coef_kernel')
def clip_coef(ops):
    for n, max_norm in ((512, 1.0), (512, 1e4), (7, 2.0), (300, 0.5)):
        partial = rnd(n, seed=2).abs()
        nc, names = launched(ops, lambda: ops.clip_coef(partial, max_norm))
        assert names == ['clip_coef_kernel']
        nrm = d64(partial).sum().sqrt()
        ref = torch.stack([nrm, torch.clamp(max_norm / (nrm + 1e-6), max=1.0)])
        yield dict(names=names, n=n, max_norm=str(max_norm), out=float(((d64(nc) - ref).abs() / ref).max()), bound=1e-5)


def _ref_adam(p, g, m, v, ema, coef, lr, b1, b2, eps, step, decay):
    g = g * coef
    m = b1 * m + (1 - b1) * g
    v = b2 * v + (1 - b2) * g * g
    p = p - (lr / (1 - b1 ** step)) * m / (v.sqrt() / math.sqrt(1 - b2 ** step) + eps)
    return p, m, v, (None if ema is None else (1 - decay) * p + decay * ema)


def _adam(ops, name, dev):
    lr, b1, b2, eps, step, decay = 2e-4, 0.9, 0.999, 1e-8, 3, 0.9999
    for n, with_ema, with_coef in ((77, True, True), (10000, False, False), (10001, True, False)):
        p, g, m, v = rnd(n, seed=9), rnd(n, seed=10), 0.1 * rnd(n, seed=11), (0.1 * rnd(n, seed=12)).abs()
        ema = rnd(n, seed=13) if with_ema else None
        coef = torch.tensor([0.37], device=DEV) if with_coef else None
        ref = _ref_adam(d64(p), d64(g), d64(m), d64(v), None if ema is None else d64(ema), 0.37 if with_coef else 1.0, lr, b1, b2, eps, step, decay)
        if dev:
            hyper = torch.zeros(4, device=DEV)
            ops.set_step_scalars(hyper, lr, b1, b2, step)
            _, names = launched(ops, lambda: ops.adam_ema_dev(p, g, m, v, ema, coef, hyper, b1, b2, eps, decay))
        else:
            _, names = launched(ops, lambda: ops.adam_ema(p, g, m, v, ema, coef, lr, b1, b2, eps, step, decay))
        assert names == [name]
        res = dict(names=names, n=n, ema=with_ema, clip=with_coef, p=relerr(p, ref[0]), m=relerr(m, ref[1]), v=relerr(v, ref[2]), bound=1e-5)
        if with_ema:
            res['ema_err'] = relerr(ema, ref[3])
        yield res


@case('adam_ema_kernel')
def adam_ema(ops):
    yield from _adam(ops, 'adam_ema_kernel', False)


@case('adam_ema_dev_kernel')
def adam_ema_dev(ops):
    yield from _adam(ops, 'adam_ema_dev_kernel', True)


@case('set_step_scalars_kernel')
def set_step_scalars(ops):
    for lr, b1, b2, step in ((2e-4, 0.9, 0.999, 3), (1e-3, 0.5, 0.99, 4000000000)):
        hyper = torch.full((4,), float('nan'), device=DEV)
        _, names = launched(ops, lambda: ops.set_step_scalars(hyper, lr, b1, b2, step))
        assert names == ['set_step_scalars_kernel']
        want = np.array([lr, 1.0 - b1 ** step, 1.0 - b2 ** step], dtype=np.float32)
        got = hyper.cpu().numpy()
        assert (got[:3] == want).all() and int(got[3:4].view(np.uint32)[0]) == step & 0xFFFFFFFF, (got, want)
        yield dict(names=names, step=step, out=0.0, bound=0.0)


def _adamw(ops, name, n, offset, with_ema, with_coef):
    lr, b1, b2, eps, wd, step, decay = 1e-3, 0.9, 0.999, 1e-8, 0.01, 3, 0.999
    def buf(seed, f=lambda t: t):                             # a view `offset` floats into its allocation
        base = torch.empty(n + offset, device=DEV)
        base[offset:] = f(rnd(n, seed=seed))
        return base[offset:]
    p, g, m, v = buf(9), buf(10), buf(11, lambda t: 0.1 * t), buf(12, lambda t: (0.1 * t).abs())
    ema = buf(13) if with_ema else None
    coef = torch.tensor([0.37], device=DEV) if with_coef else None
    vec = n >= 4 and all(t is None or t.data_ptr() % 16 == 0 for t in (p, g, m, v, ema))
    assert name == 'adamw_ema_kernel<%s>' % ('true' if vec else 'false'), (n, offset, vec)
    pr, gr, mr, vr = d64(p), d64(g) * (0.37 if with_coef else 1.0), d64(m), d64(v)
    er = None if ema is None else d64(ema)
    _, names = launched(ops, lambda: ops.adamw_ema(p, g, m, v, ema, lr, b1, b2, eps, wd, step, ema_decay=decay, coef=coef))
    assert names == [name], names
    pr = pr * (1 - lr * wd)
    mr = mr + (gr - mr) * (1 - b1)
    vr = vr * b2 + (1 - b2) * gr * gr
    pr = pr - (lr / (1 - b1 ** step)) * mr / (vr.sqrt() / math.sqrt(1 - b2 ** step) + eps)
    res = dict(names=names, n=n, offset=offset, ema=with_ema, clip=with_coef, p=relerr(p, pr), m=relerr(m, mr), v=relerr(v, vr), bound=1e-5)
    if with_ema:
        res['ema_err'] = relerr(ema, er - (1 - decay) * (er - pr))
    return res


@case('adamw_ema_kernel<true>')
def adamw_vec(ops):
    for n, e, c in ((4, True, False), (1003, True, True), (4096 * 256 * 4 + 1027, False, False)):        # the last: second trip + scalar tail
        yield _adamw(ops, 'adamw_ema_kernel<true>', n, 0, e, c)


@case('adamw_ema_kernel<false>')
def adamw_scalar(ops):
    for n, off, e, c in ((3, 0, True, False), (1003, 1, True, True), (4096 * 256 + 77, 3, False, False)):
        yield _adamw(ops, 'adamw_ema_kernel<false>', n, off, e, c)


@case('embedding_bwd_kernel')
def embedding_bwd(ops):
    for B, D, rows in ((4, 7, 3), (70, 100, 10), (300, 512, 1000)):                                    # 1, 2 and 5 words of row mask
        ids = torch.randint(0, rows, (B,), generator=_gen(B))
        ids[-1] = ids[0]                                                                                # a repeated id across mask words
        dctx, dW = rnd(B, D, seed=1), rnd(rows, D, seed=2)
        ref = d64(dW).index_add(0, ids, d64(dctx))
        _, names = launched(ops, lambda: ops.embedding_bwd(ids.to(DEV), dctx, dW))
        assert names == ['embedding_bwd_kernel']
        yield dict(names=names, shape=(B, D, rows), out=relerr(dW, ref), bound=1e-5)


def _reg_vq():
    for D in range(1, 17):
        @case('vq_quantize_kernel<%d>' % D, *(['vq_loss_kernel'] if D in (1, 4, 16) else []))
        def c(ops, D=D):
            """A strided latent, 600 codes (two LDS chunks of 512), 70 and 1030 pixels (ragged last workgroup).  The index is the fp64
            argmin unless two codes are closer than fp32 resolves (then its fp64 distance is within 1e-6 of the minimum)."""
            for N, H, W in ((2, 5, 7), (2, 5, 103)):
                z = wide(N, D, H, W, 3)[0]
                E = rnd(600, D, seed=4)
                poison(N * D * H * W)
                (zq, loss, idx), names = launched(ops, lambda: ops.vq_quantize(z, E))
                assert names == ['vq_quantize_kernel<%d>' % D, 'vq_loss_kernel'], names
                zr = d64(z).permute(0, 2, 3, 1).reshape(-1, D)
                dist = ((zr[:, None, :] - d64(E)[None]) ** 2).sum(-1)
                chosen = dist.gather(1, idx.cpu()[:, None])[:, 0]
                best = dist.min(1).values
                near_tie = int((idx.cpu() != dist.argmin(1)).sum())
                assert bool((chosen <= best * (1 + 1e-6)).all())
                e_sel = d64(E)[idx.cpu()]
                zq_ref = e_sel.view(N, H, W, D).permute(0, 3, 1, 2)
                loss_ref = 1.25 * ((e_sel - zr) ** 2).mean()
                yield dict(names=names, shape=(N, D, H, W), index_near_ties=near_tie, zq=relerr(zq, zq_ref),
                           loss=abs(float(loss) - float(loss_ref)) / float(loss_ref), bound=1e-5)


_reg_vq()


# ======================================================================================================================
# the sampler updates and the EMA (sampler.hip, ldm_sampler.hip, ema.hip): flat buffers at every alignment the launchers tell apart
# ======================================================================================================================
NAN = float('nan')


def _at(n, off, seed=None, scale=1.0):
    """n floats that start `off` floats behind a 16-byte boundary (random, or NaN for an output) and the buffer they lie in."""
    buf = torch.full((n + 8,), NAN, device=DEV) if seed is None else rnd(n + 8, seed=seed, scale=scale)
    return buf[4 + off:4 + off + n], buf


def _rest_is_nan(buf, off, n):
    return bool(buf[:4 + off].isnan().all()) and bool(buf[4 + off + n:].isnan().all())


# (n, the offset of every pointer, the offset of eps alone).  16-byte path with a 1-element tail / below one float4 / three trips of
# the grid-stride loop + a tail / a shared phase of 4 bytes: a 3-element head / eps on another phase: 4-byte accesses throughout
FLAT_ALIGN = ((77, 0, 0), (3, 0, 0), (BIG, 0, 0), (1003, 1, 1), (1003, 0, 2), (4 * 4096 * 256 + 4099, 3, 0))


def _reg_denoise():
    for mode in (0, 1):
        @case('denoise_step_kernel<%d>' % mode)
        def c(ops, mode=mode):
            coef = (0.79, 0.61, 0.72, 0.11, 0.68) if mode == 0 else (1.64, 1.30, 0.013, 0.985, 1.02, 0.07)
            for i, (n, off, off_e) in enumerate(FLAT_ALIGN):
                with_z, with_x0, in_place = i % 3 != 1, i % 2 == 0, i == 3
                x, e = _at(n, off, 1)[0], _at(n, off_e, 2)[0]
                z = _at(n, off, 3)[0] if with_z else None
                (out, obuf), (x0, xbuf) = ((x, None) if in_place else _at(n, off)), (_at(n, off) if with_x0 else (None, None))
                xr, er, zr = d64(x), d64(e), (d64(z) if with_z else 0.0)
                _, names = launched(ops, lambda: ops.denoise_step(x, e, mode, coef, z=z, out=out, x0_out=x0))
                assert names == ['denoise_step_kernel<%d>' % mode], names
                if mode == 0:
                    s1, s2, s3, c1, c2 = coef
                    x0r = (xr - er * s1) / s2
                    nr = s3 * x0r + c1 * zr + c2 * er
                else:
                    r1, r2, k0, kx, dd, sig = coef
                    x0r = (r1 * xr - r2 * er).clamp(-1, 1)
                    nr = (k0 * x0r + kx * xr) / dd + sig * zr
                assert (in_place or _rest_is_nan(obuf, off, n)) and (not with_x0 or _rest_is_nan(xbuf, off, n))
                res = dict(names=names, n=n, offsets=(off, off_e), z=with_z, in_place=in_place, next=relerr(out, nr), bound=1e-5)
                if with_x0:
                    res['x0'] = relerr(x0, x0r)
                yield res


_reg_denoise()


def _image_bytes(x, rescaled):
    """The torch fp32 expression the kernel restates, operation by operation."""
    v = ((x + 1.0) / 2.0 if rescaled else x).clamp(0.0, 1.0)
    return (v * 255.0 + 0.5).clamp(0.0, 255.0).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def _image_to_u8(ops, name, x, rescaled):
    N, C, H, W = x.shape
    vec = C <= 4 and (H * W) % 4 == 0 and (x.stride(0) if N > 1 else 0) % 4 == 0 and x.data_ptr() % 16 == 0
    assert name == 'image_to_u8_kernel<%s>' % ('true' if vec else 'false'), (tuple(x.shape), x.stride(), vec)
    out = torch.full((N * H * W * C + 8,), 77, dtype=torch.uint8, device=DEV)
    view = out[4:4 + N * H * W * C].view(N, H, W, C)
    _, names = launched(ops, lambda: ops.image_to_u8(x, rescaled=rescaled, out=view))
    assert names == [name], names
    ref = _image_bytes(x.cpu(), rescaled)
    bad = int((view.cpu() != ref).sum())
    assert bool((out[:4] == 77).all()) and bool((out[4 + N * H * W * C:] == 77).all())
    far = int((view.cpu().int() - _image_bytes(d64(x), rescaled).int()).abs().max())          # fp64: at most the next byte
    assert bad == 0 and far <= 1, (bad, far)
    return dict(names=names, shape=(N, C, H, W), rescaled=rescaled, mismatches=bad, out=float(bad), bound=0.0)


def _beyond(x):
    """The view itself, scaled in place so that values lie beyond both clamps."""
    return x.mul_(1.5)


@case('image_to_u8_kernel<true>')
def image_to_u8_vec(ops):
    """Channel slices of wider buffers, 1 .. 4 channels, values beyond both clamps; 66 planes of 256 x 256: the grid-stride loop turns."""
    for i, (N, C, H, W) in enumerate(((3, 3, 8, 8), (2, 4, 6, 10), (2, 1, 2, 2), (2, 2, 4, 9), (66, 1, 256, 256))):
        big = N * H * W > CAP
        x = _beyond(wide(N, C, H, W, 1, lead=1 if big else 2, extra=1 if big else 6)[0])
        assert not big or N * (H * W // 4) > 4096 * 256
        yield _image_to_u8(ops, 'image_to_u8_kernel<true>', x, i % 2 == 0)


@case('image_to_u8_kernel<false>')
def image_to_u8_scalar(ops):
    """5 channels / HW % 4 != 0 / an image stride that is no multiple of 4 / a view 4 bytes behind a 16-byte boundary / 1.35 M bytes:
    the grid-stride loop turns."""
    yield _image_to_u8(ops, 'image_to_u8_kernel<false>', _beyond(wide(2, 5, 8, 8, 1)[0]), True)
    yield _image_to_u8(ops, 'image_to_u8_kernel<false>', _beyond(wide(3, 3, 5, 3, 1)[0]), False)
    yield _image_to_u8(ops, 'image_to_u8_kernel<false>', _beyond(rnd(2, 3 * 64 + 1, seed=1)[:, :3 * 64].view(2, 3, 8, 8)), True)
    yield _image_to_u8(ops, 'image_to_u8_kernel<false>', _beyond(rnd(2 * 3 * 64 + 1, seed=1)[1:].view(2, 3, 8, 8)), True)
    yield _image_to_u8(ops, 'image_to_u8_kernel<false>', _beyond(wide(5, 3, 299, 301, 1, lead=1, extra=0)[0]), True)


def _reg_cfg_denoise():
    need = (0, 1, 2, 3, 1)
    for order in range(5):
        for guided in (True, False):
            @case('cfg_denoise_step_kernel<%d, %s>' % (order, 'true' if guided else 'false'))
            def c(ops, order=order, guided=guided):
                """The guided form reads its conditional half n floats behind the unconditional one: n % 4 != 0 puts it on another phase."""
                name = 'cfg_denoise_step_kernel<%d, %s>' % (order, 'true' if guided else 'false')
                coef, scale, temp = (0.63, 0.78, 0.81, 0.52, 0.27), 3.0, 0.9
                for i, (n, off, off_e) in enumerate(((77, 0, 0), (80, 0, 0), (3, 0, 0), (BIG + 3, 0, 0), (1004, 1, 1), (1003, 0, 2))):
                    with_z, with_x0, with_eg, in_place = i % 3 != 1, i % 2 == 0, i % 2 == 1 or i == 3, i == 4
                    x, e = _at(n, off, 1)[0], _at(2 * n if guided else n, off_e, 2)[0]
                    hist = [_at(n, off, 10 + k)[0] for k in range(need[order])]
                    z = _at(n, off, 3)[0] if with_z else None
                    out, obuf = (x, None) if in_place else _at(n, off)
                    x0, xbuf = _at(n, off) if with_x0 else (None, None)
                    eg, gbuf = _at(n, off) if with_eg else (None, None)
                    xr, er, zr = d64(x), d64(e), (d64(z) if with_z else 0.0)
                    h = [d64(t) for t in hist]
                    _, names = launched(ops, lambda: ops.cfg_denoise_step(x, e, coef, scale=scale if guided else None, order=order, hist=hist, z=z,
                                                                          temperature=temp, out=out, x0_out=x0, eg_out=eg))
                    assert names == [name], names
                    egr = er[:n] + scale * (er[n:] - er[:n]) if guided else er
                    epr = (egr, (3 * egr - h[0]) / 2 if order == 1 else None, (23 * egr - 16 * h[0] + 5 * h[1]) / 12 if order == 2 else None,
                           (55 * egr - 59 * h[0] + 37 * h[1] - 9 * h[2]) / 24 if order == 3 else None, (h[0] + egr) / 2 if order == 4 else None)[order]
                    s1m, sat, sap, cdir, sigma = coef
                    x0r = (xr - s1m * epr) / sat
                    nr = sap * x0r + cdir * epr + sigma * zr * temp
                    assert (in_place or _rest_is_nan(obuf, off, n)) and (not with_x0 or _rest_is_nan(xbuf, off, n))
                    assert not with_eg or _rest_is_nan(gbuf, off, n)
                    res = dict(names=names, n=n, offsets=(off, off_e), z=with_z, in_place=in_place, next=relerr(out, nr), bound=1e-5)
                    if with_x0:
                        res['x0'] = relerr(x0, x0r)
                    if with_eg:
                        res['eg'] = relerr(eg, egr)
                    yield res


_reg_cfg_denoise()


def _ema(ops, name, n, off_s, off_p, decay):
    (s, sbuf), p = _at(n, off_s, 1), _at(n, off_p, 2)[0]
    vec = s.data_ptr() % 16 == 0 and p.data_ptr() % 16 == 0 and n >= 4
    assert name == 'ema_update_kernel<%s>' % ('true' if vec else 'false'), (n, off_s, off_p)
    sr, pr, before = d64(s), d64(p), sbuf.clone()
    omd = float(np.float32(1) - np.float32(decay))
    _, names = launched(ops, lambda: ops.ema_update(s, p, decay))
    assert names == [name], names
    assert torch.equal(sbuf[:4 + off_s], before[:4 + off_s]) and torch.equal(sbuf[4 + off_s + n:], before[4 + off_s + n:])
    return dict(names=names, n=n, offsets=(off_s, off_p), decay=str(decay), out=relerr(s, sr - omd * (sr - pr)), bound=1e-5)


@case('ema_update_kernel<true>')
def ema_vec(ops):
    for n, decay in ((4, 0.5), (1003, 0.9999), (4096 * 256 * 4 + 1027, 0.5)):                          # the last: second trip + scalar tail
        yield _ema(ops, 'ema_update_kernel<true>', n, 0, 0, decay)


@case('ema_update_kernel<false>')
def ema_scalar(ops):
    for n, off_s, off_p, decay in ((3, 0, 0, 0.5), (1003, 1, 1, 0.9999), (1003, 0, 2, 0.5), (4096 * 256 + 77, 3, 0, 0.5)):
        yield _ema(ops, 'ema_update_kernel<false>', n, off_s, off_p, decay)


# ======================================================================================================================
# the closing test: parametrised over the table itself
# ======================================================================================================================
@pytest.mark.parametrize('entry', BRANCHES)
def test_branch(entry, ops, report):
    assert (entry in CASES) != (entry in UNREACHED), 'every entry has a case or a reason in UNREACHED, never both: %s' % entry
    if entry in UNREACHED:
        return
    name, log, bad = entry.split(' | ')[0], [], []
    for fn in CASES[entry]:
        for res in fn(ops):
            names = res['names'] + res.get('names_bwd', [])
            assert name in names, (entry, names)
            assert set(names) <= KNOWN, ('a launch name outside the tables', sorted(set(names) - KNOWN))
            errs = {k: v for k, v in res.items() if isinstance(v, float) and k != 'bound'}
            assert errs, res
            res = dict(res, case=fn.__name__)
            log.append({k: (list(v) if isinstance(v, tuple) else v) for k, v in res.items()})
            if any(not v <= res['bound'] for v in errs.values()):
                bad.append(res)
            torch.cuda.empty_cache()
    assert log, entry
    report['dispatch/' + entry] = log
    assert not bad, bad


def test_tables_are_consistent():
    assert len(set(BRANCHES)) == len(BRANCHES) and not set(UNREACHED) - set(BRANCHES)
    assert not set(CASES) - set(BRANCHES)


# ======================================================================================================================
# ill-conditioned inputs: max(4 e_ref32, floor)
# ======================================================================================================================
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def gn_family(name, N, C, H, W, G):
    x = torch.randn(N, C, H, W, generator=_gen(11))
    cpg = C // G
    if name == 'randn+10':
        x += 10
    elif name == 'randn+30':
        x += 30
    elif name == 'channel offsets N(0, 10^2)':
        x += 10 * torch.randn(1, C, 1, 1, generator=_gen(12))
    elif name == 'one element 1e3':
        x[0, 0, 0, 0] = 1e3
        x[-1, -1, -1, -1] = 1e3
        x[0, cpg + 1, H // 2, 1] = -1e3
    elif name == "a group's first channel +-100":
        x[:, 0::2 * cpg] += 100
        x[:, cpg::2 * cpg] -= 100
    elif name == '1e-3 randn':
        x *= 1e-3
    else:
        raise KeyError(name)
    return x


GN_FAMILIES = ('randn+10', 'randn+30', 'channel offsets N(0, 10^2)', 'one element 1e3', "a group's first channel +-100", '1e-3 randn')
GN_ILL_SHAPES = [(32, 256, 16, 16, 32), (2, 256, 16, 16, 32), (1, 32, 128, 128, 8), (2, 32, 3, 3, 8)]      # wave<8> / vec4 + vec4c / split, 4 slices / scalar


@pytest.mark.parametrize('shape', GN_ILL_SHAPES, ids=str)
@pytest.mark.parametrize('family', GN_FAMILIES)
def test_groupnorm_ill_conditioned(ops, report, family, shape):
    """GroupNorm + SiLU forward and dx on offsets, per-channel means, outliers and tiny scales: within max(4 e_ref32, 2e-5) of fp64."""
    N, C, H, W, G = shape
    xc = gn_family(family, N, C, H, W, G)
    x = xc.to(DEV)
    gamma, beta, dz = 1 + 0.2 * rnd(C, seed=3), 0.1 * rnd(C, seed=4), rnd(N, C, H, W, seed=5)
    (y, stats), names = launched(ops, lambda: ops.groupnorm_fwd(x, None, gamma, beta, G, 1e-6, True))
    (dx, _), names_b = launched(ops, lambda: ops.groupnorm_bwd(x, None, gamma, beta, stats, dz, G, True))
    assert set(names + names_b) <= KNOWN

    def ref(dt):
        xr = xc.to(dt).requires_grad_(True)
        yr = F.silu(F.group_norm(xr, G, gamma.cpu().to(dt), beta.cpu().to(dt), 1e-6))
        yr.backward(dz.cpu().to(dt))
        return yr.detach(), xr.grad
    y64, dx64 = ref(torch.float64)
    y32, dx32 = ref(torch.float32)
    rec = dict(names=names + names_b)
    for k, got, r64, r32 in (('fwd', y, y64, y32), ('dx', dx, dx64, dx32)):
        e_hip, e_ref32 = relerr(got, r64), relerr(r32, r64)
        rec[k] = dict(e_hip=e_hip, e_ref32=e_ref32, bound=max(4 * e_ref32, 2e-5))
    report['ill/gn/%s/%s' % (family, shape)] = rec
    print(family, shape, rec)
    assert all(v['e_hip'] <= v['bound'] for k, v in rec.items() if k != 'names'), rec


def ln_family(name, N, C, H, W):
    x = torch.randn(N, C, H, W, generator=_gen(21))
    if name == 'randn+10':
        x += 10
    elif name == 'randn+30':
        x += 30
    elif name == 'channel offsets N(0, 10^2)':
        x += 10 * torch.randn(1, C, 1, 1, generator=_gen(22))
    elif name == 'one element 1e3':
        x[0, C // 2, 0, 1] = 1e3
        x[-1, -1, -1, -1] = -1e3
    elif name == 'channel 0 = +100':
        x[:, 0] = 100
    elif name == 'channel 0 = -100':
        x[:, 0] = -100
    elif name == 'last channel = +100':
        x[:, -1] = 100
    elif name == 'last channel = -100':
        x[:, -1] = -100
    elif name == 'channels 0 and 5 = +100 / -100':
        x[:, 0] = 100
        x[:, 5] = -100
    elif name == '1e-3 randn':
        x *= 1e-3
    else:
        raise KeyError(name)
    return x


LN_FAMILIES = ('randn+10', 'randn+30', 'channel offsets N(0, 10^2)', 'one element 1e3', 'channel 0 = +100', 'channel 0 = -100',
               'last channel = +100', 'last channel = -100', 'channels 0 and 5 = +100 / -100', '1e-3 randn')
LN_ILL_SHAPES = [(2, 50, 16, 16), (2, 320, 16, 16), (2, 960, 16, 16), (4, 50, 128, 128)]         # the 16-token form x 3 widths, the 64-token form


@pytest.mark.parametrize('shape', LN_ILL_SHAPES, ids=str)
@pytest.mark.parametrize('family', LN_FAMILIES)
def test_layernorm_ill_conditioned(ops, report, family, shape):
    """LayerNorm forward and dx (its rstd comes from the forward) on offsets, per-channel means, outliers in the first / last channel
    and tiny scales: within max(4 e_ref32, 1e-5) of fp64."""
    N, C, H, W = shape
    xc = ln_family(family, N, C, H, W)
    x = xc.to(DEV)
    gamma, beta, dy = 1 + 0.2 * rnd(C, seed=2), 0.1 * rnd(C, seed=3), rnd(N, C, H, W, seed=4)
    (y, st), names = launched(ops, lambda: ops.layernorm_fwd(x, gamma, beta))
    (dx, _), names_b = launched(ops, lambda: ops.layernorm_bwd(x, gamma, st, dy))
    assert names + names_b == list(ln_forms(N * H * W)) + ['ln_param_kernel']

    def ref(dt):
        xr = xc.to(dt).requires_grad_(True)
        yr = F.layer_norm(xr.permute(0, 2, 3, 1), (C,), gamma.cpu().to(dt), beta.cpu().to(dt), 1e-5).permute(0, 3, 1, 2)
        yr.backward(dy.cpu().to(dt))
        return yr.detach(), xr.grad
    y64, dx64 = ref(torch.float64)
    y32, dx32 = ref(torch.float32)
    rec = dict(names=names + names_b)
    for k, got, r64, r32 in (('fwd', y, y64, y32), ('dx', dx, dx64, dx32)):
        e_hip, e_ref32 = relerr(got, r64), relerr(r32, r64)
        rec[k] = dict(e_hip=e_hip, e_ref32=e_ref32, bound=max(4 * e_ref32, 1e-5))
    report['ill/ln/%s/%s' % (family, shape)] = rec
    print(family, shape, rec)
    assert all(v['e_hip'] <= v['bound'] for k, v in rec.items() if k != 'names'), rec


def softmax_family(name, rows, cols):
    s = torch.randn(rows, cols, generator=_gen(31))
    if name == 'one logit 80 above the rest':
        s[torch.arange(rows), torch.arange(rows) % cols] += 80
    elif name == 'rows shifted by -1e4':
        s -= 1e4
    elif name == 'constant rows':
        s = s[:, :1].expand(rows, cols).contiguous()
    elif name == 'every second logit -1e9':
        s[:, 1::2] = -1e9
    elif name == '30 randn':
        s *= 30
    else:
        raise KeyError(name)
    return s


SM_FAMILIES = ('one logit 80 above the rest', 'rows shifted by -1e4', 'constant rows', 'every second logit -1e9', '30 randn')


@pytest.mark.parametrize('shape', [(37, 256), (10, 1500), (6, 16)], ids=str)
@pytest.mark.parametrize('family', SM_FAMILIES)
def test_softmax_ill_conditioned(ops, report, family, shape):
    """Softmax forward, and backward at scale 0.125, on peaked / shifted / constant / masked rows: within max(4 e_ref32, 1e-5) of fp64."""
    sc = softmax_family(family, *shape)
    s, scale = sc.to(DEV), 0.125
    dp_ = rnd(*shape, seed=2)
    p, names = launched(ops, lambda: ops.softmax_fwd(s))
    p2 = ops.softmax_fwd(s * scale)
    ds, names_b = launched(ops, lambda: ops.softmax_bwd(p2, dp_, scale))
    assert names + names_b == ['softmax_fwd_kernel', 'softmax_bwd_kernel']

    def ref(dt):
        sr = (sc * scale).to(dt).requires_grad_(True)         # fp32 product first: what the kernels are given
        sr.softmax(-1).backward(dp_.cpu().to(dt))
        return sc.to(dt).softmax(-1), sr.grad * scale
    p64, ds64 = ref(torch.float64)
    p32, ds32 = ref(torch.float32)
    rec = dict(names=names + names_b)
    for k, got, r64, r32 in (('fwd', p, p64, p32), ('bwd', ds, ds64, ds32)):
        e_hip, e_ref32 = relerr(got, r64), relerr(r32, r64)
        rec[k] = dict(e_hip=e_hip, e_ref32=e_ref32, bound=max(4 * e_ref32, 1e-5))
    report['ill/softmax/%s/%s' % (family, shape)] = rec
    print(family, shape, rec)
    assert all(v['e_hip'] <= v['bound'] for k, v in rec.items() if k != 'names'), rec
