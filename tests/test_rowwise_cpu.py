"""tests/rowwise.py on the CPU: the restatements are the operations they restate, the row figure has the power it claims, and the bounds
of tests/test_rowwise_parity_gpu.py stay small on every family at every shape that file uses.

  exactness  every restatement (the direct chains, F(2, 3), F(2x2, 3x3), F(3, 2), F(3x3, 2x2) and the three nine-product forms, the
             bmm / linear / attention / importance chains) evaluated in fp64 equals ref64 to 1e-12 of cond64: the matrices were copied
             correctly from the kernels' header comments;
  power      on `row scales`, the wrong result ref64 + 1e-6 x (the largest row, added to every row) -- what a stale split-K slab or a
             workspace tile added to the wrong output tile looks like -- passes the max-norm bound the kernel's older tests use (the B_*
             constants of tests/test_contraction_dispatch_gpu.py; 1e-5 for the importance kernels, tests/test_dispatch_parity_gpu.py) and
             is at least 1000 x the bound of the row figure;
  cap        e_ref32 and e_alg32 are finite and the bound is below 1e-3 for every case of the GPU table."""
import math

import pytest
import torch

import rowwise as R
import test_contraction_dispatch_gpu as C
import test_rowwise_parity_gpu as G
from helpers import ref_attention, ref_conv_dgrad, ref_conv_fwd, ref_conv_wgrad

S2P0, S2P1 = G.S3_S2P0[0], G.S3_S2P1[0]

# (builder, its arguments after (family, seed), the older max-norm bound of the kernel): one of every operation kind and algorithm
KINDS = {
    'conv_fwd direct': (R.conv_fwd_case, (3, 24, 40, 8, 8), {}, C.B_DIRECT),
    'conv_fwd direct stride 2 accumulate': (R.conv_fwd_case, (3, 24, 40, 16, 16, S2P0), dict(epi='acc', alpha=0.5), C.B_DIRECT),
    'conv_fwd direct upsample': (R.conv_fwd_case, (3, 21, 40, 5, 7, R.UPS3), dict(epi='bias'), C.B_DIRECT),
    'conv_fwd F(2,3)': (R.conv_fwd_case, (3, 24, 40, 8, 8), dict(alg='wino1d'), C.B_WINO),
    'conv_fwd F(2x2,3x3)': (R.conv_fwd_case, (3, 24, 40, 4, 16), dict(alg='wino2d'), C.B_WINO),
    'ups9_fwd': (R.conv_fwd_case, (5, 20, 36, 4, 4, R.UPS3), dict(alg='ups9', epi='bias'), C.B_UPS9),
    'conv_dgrad direct': (R.conv_dgrad_case, (3, 40, 24, 8, 8), {}, C.B_DIRECT),
    'conv_dgrad stride 2 pad 1': (R.conv_dgrad_case, (3, 40, 24, 8, 8, S2P1), dict(in_hw=(16, 16), acc=True, alpha=0.5), C.B_DIRECT),
    'conv_dgrad stride 2 pad 0': (R.conv_dgrad_case, (3, 24, 40, 5, 7, S2P0), dict(in_hw=(10, 14), acc=True), C.B_DIRECT),
    'conv_dgrad F(2,3)': (R.conv_dgrad_case, (5, 32, 40, 4, 16), dict(alg='wino1d'), C.B_WINO),
    'conv_dgrad F(2x2,3x3)': (R.conv_dgrad_case, (5, 40, 64, 4, 16), dict(alg='wino2d', acc=True, alpha=0.5), C.B_WINO),
    'ups9_dgrad': (R.conv_dgrad_case, (3, 40, 16, 8, 8, R.UPS3), dict(alg='ups9', in_hw=(8, 8), lowres=True, acc=True), C.B_UPS9),
    'conv_wgrad direct': (R.conv_wgrad_case, (4, 48, 40, 16, 16), {}, C.B_DIRECT),
    'conv_wgrad direct accumulate': (R.conv_wgrad_case, (3, 40, 100, 6, 6), dict(acc=True, alpha=0.5), C.B_DIRECT),
    'conv_wgrad 1x1': (R.conv_wgrad_case, (8, 40, 100, 6, 6, G.S1[0]), dict(acc=True, alpha=0.5), C.B_DIRECT),
    'conv_wgrad F(3,2)': (R.conv_wgrad_case, (2, 40, 70, 8, 8), dict(alg='wino1d'), C.B_WINO_WGRAD),
    'conv_wgrad F(3x3,2x2)': (R.conv_wgrad_case, (3, 40, 70, 4, 16), dict(alg='wino2d', acc=True, alpha=0.5), C.B_WINO_WGRAD),
    'ups9_wgrad': (R.conv_wgrad_case, (5, 20, 36, 4, 4, R.UPS3), dict(alg='ups9', acc=True), C.B_UPS9),
    'bmm_tn': (R.bmm_case, ('tn', 3, 52, 41, 37, 0.25), {}, C.B_BMM),
    'bmm_nn accumulate': (R.bmm_case, ('nn', 3, 50, 41, 37, 0.5), dict(acc=True), C.B_BMM),
    'bmm_nt col_bias': (R.bmm_case, ('nt', 3, 50, 41, 37, 0.25), dict(col_bias=True), C.B_BMM),
    'linear_forward': (R.linear_case, ('fwd', 7, 200, 90), {}, C.B_DIRECT),
    'linear_dgrad': (R.linear_case, ('dgrad', 70, 90, 100), dict(acc=True), C.B_DIRECT),
    'linear_wgrad': (R.linear_case, ('wgrad', 33, 37, 92, 0.5), {}, C.B_DIRECT),
    'attention': (R.attention_case, (2, 2, 32, 24, 4, 8), {}, C.B_ATTN),
    'attention pruned widths': (R.attention_case, (2, 1, 179, 133, 8, 12), {}, C.B_ATTN),
    'group_score': (R.group_case, (48, 25), {}, 1e-5),
}
for _mode in (0, 1, 2, 4, 5):
    for _dim in (0, 1):
        KINDS['wg_reduce mode %d dim %d' % (_mode, _dim)] = (R.wg_case, ((70, 37, 3, 3), _dim, _mode, bool((_mode + _dim) % 2)), {}, 1e-5)
KINDS['wg_reduce mode 3'] = (R.wg_case, ((96,), 0, 3, True), {}, 1e-5)


def make(kind, family, seed=3):
    f, args, kw, b_old = KINDS[kind]
    return f(family, seed, *args, **kw), b_old


def test_rowwise_figure():
    ref = torch.tensor([[1.0, -2.0], [1e-6, 3e-6]], dtype=torch.float64)
    cond = ref.abs() * 2
    got = ref + torch.tensor([[1e-3, 0.0], [0.0, 3e-9]], dtype=torch.float64)
    assert R.rowwise(got, ref, cond, (0,)) == pytest.approx(max(1e-3 / 4.0, 3e-9 / 6e-6))
    assert R.rowwise(got, ref, cond, (1,)) == pytest.approx(max(1e-3 / 2.0, 3e-9 / 4.0))
    assert R.rowwise(got, ref, cond, (0, 1)) == pytest.approx(1e-3 / 2.0)
    assert math.isnan(R.rowwise(got * float('nan'), ref, cond, (0,)))
    with pytest.raises(AssertionError):                                     # a row whose cond64 maximum is 0 is an error of the test
        R.rowwise(got, ref, cond * torch.tensor([[1.0], [0.0]], dtype=torch.float64), (0,))
    assert R.pick_rows(torch.arange(100.0)) == [0, 1, 21, 40, 59, 78, 98, 99] and R.pick_rows(torch.tensor([3.0, 1.0, 2.0])) == [0, 1, 2]
    t = torch.arange(24.0).reshape(2, 3, 4)
    assert torch.equal(R.to_rows(t, (1,))[2], t[:, 2].reshape(-1)) and torch.equal(R.to_rows(t, (0, 1))[4], t[1, 1])


def test_families():
    specs = dict(x=((4, 6, 5, 5), 1.0, {1: 'con:x'}, 1), w=((7, 6, 3, 3), 0.1, {0: 'row:k', 1: 'con:w'}, None), b=((1, 7, 1, 1), 1.0, {1: 'row:k'}, None))
    for fam in R.FAMILIES:
        assert all(torch.equal(a, b) for a, b in zip(R.draw(fam, 5, specs).values(), R.draw(fam, 5, specs).values()))       # seeded
    rn, rs, al, of = (R.draw(f, 5, specs) for f in R.FAMILIES)
    spread = lambda t, ax: float(torch.log10(t.abs().amax([d for d in range(t.dim()) if d != ax])).std())
    assert spread(rn['w'], 0) < 0.3 and spread(rs['w'], 0) > 1.0 and spread(rs['w'], 1) < 0.3 and spread(rs['x'], 1) < 0.3
    assert spread(al['w'], 1) > 1.0 and spread(al['x'], 1) > 1.0 and bool((al['x'] < 0).any())
    # the bias carries the scale of its weight row
    ratio = (rs['b'].flatten().abs() / rs['w'].abs().amax((1, 2, 3))).log10()
    assert float(ratio.std()) < 0.7 < float(rs['b'].flatten().abs().log10().std())
    assert bool((of['x'] > 0).all()) and bool((of['x'].amin((0, 2, 3)) >= 1.9 * (of['x'].amax((0, 2, 3)) - of['x'].amin((0, 2, 3))) / 2).all())


@pytest.mark.parametrize('family', R.FAMILIES)
@pytest.mark.parametrize('kind', sorted(KINDS))
def test_restatement_is_exact_in_fp64(kind, family):
    c, _ = make(kind, family)
    ev = c.evaluate()
    o64 = {n: t.double() for n, t in c.o.items()}
    rows = list(range(to_n(c))) if to_n(c) <= 16 else sorted(set(ev['rows']) | {0, to_n(c) - 1})
    e = R.rowwise(c.alg_out(o64, rows), *c.at_rows(rows, ev['ref64'], ev['cond64']), (0,))
    assert e <= 1e-12, (kind, family, e)
    assert math.isfinite(ev['e_ref32']) and math.isfinite(ev['e_alg32']) and 8 * R.EPS <= ev['bound'] < 1e-3, ev


def to_n(c):
    return R.to_rows(c.evaluate()['ref64'], c.row_dims).shape[0]


def test_plain_forms_are_the_suites_references():
    """ref64 of the cases is what tests/helpers.py computes for the same operands (the references the older parity tests use)."""
    class Sp:                                                               # the attributes helpers.spec_pads reads of an ops.ConvSpec
        keep, sym, stride, pad, pad_h, pad_w, kh, kw, ups = False, False, 2, 0, 0, 0, 3, 3, 0
    for kind in ('conv_fwd direct stride 2 accumulate', 'conv_dgrad stride 2 pad 0', 'conv_dgrad stride 2 pad 1'):
        c, _ = make(kind, 'all scales')
        o = {n: t.double() for n, t in c.o.items()}
        sp = Sp()
        sp.pad = sp.pad_h = sp.pad_w = int(kind.endswith('pad 1'))
        if 'fwd' in kind:
            assert torch.allclose(c.plain(o), ref_conv_fwd(o['x'], o['w'], sp), rtol=1e-13, atol=0)
        else:
            ref = ref_conv_dgrad(o['dy'], o['w'], sp, c.plain_shape[2:])
            assert float((c.plain(o) - ref).abs().max()) <= 1e-13 * float(ref.abs().max())
    c, _ = make('conv_wgrad direct', 'row scales')
    o = {n: t.double() for n, t in c.o.items()}
    sp = Sp()
    sp.stride, sp.pad, sp.pad_h, sp.pad_w = 1, 1, 1, 1
    ref = ref_conv_wgrad(o['dy'], o['x'], sp, 3, 3)
    assert float(((c.plain(o) - ref).abs() / c.evaluate()['cond64']).max()) <= 1e-13
    c, _ = make('attention', 'row scales')
    o = {n: t.double() for n, t in c.o.items()}
    assert torch.allclose(c.plain(o), ref_attention(o['q'], o['k'], o['v'], 2, 32 ** -0.5), rtol=1e-12, atol=0)


@pytest.mark.parametrize('kind', sorted(KINDS))
def test_row_figure_sees_a_1e6_leak_the_max_norm_accepts(kind):
    c, b_old = make(kind, 'row scales')
    ev = c.evaluate()
    wrong = R.leak(c, 1e-6)
    old, new = R.relerr(wrong, ev['ref64']), R.rowwise(wrong, ev['ref64'], ev['cond64'], c.row_dims)
    print(kind, 'max-norm %.2e (bound %.0e)  row figure %.2e (bound %.2e)' % (old, b_old, new, ev['bound']))
    assert old <= b_old, (kind, old, b_old)
    assert new >= 1000 * ev['bound'], (kind, new, ev['bound'])


def test_issue_example_leak():
    """The weight gradient of the issue: N = 4, 48 -> 40 channels, 16 x 16 images, scales 1e-4 .. 1e4 on the dy and x channels.  The leak scores
    1e-6 under the max-norm figure and is wrong in every digit of the small rows; torch's fp32 operator stays within a few units per row."""
    c, _ = make('conv_wgrad direct', 'row scales')
    ev = c.evaluate()
    wrong = R.leak(c, 1e-6)
    assert R.relerr(wrong, ev['ref64']) <= 1.01e-6
    assert R.rowwise(wrong, ev['ref64'], ev['cond64'], c.row_dims) > 1e6 * R.EPS and ev['e_ref32'] < 16 * R.EPS and ev['e_alg32'] < 16 * R.EPS


@pytest.mark.parametrize('family', R.FAMILIES)
@pytest.mark.parametrize('entry', G.TABLE, ids=[e.name.replace(' ', '_') for e in G.TABLE])
def test_gpu_table_bounds_stay_under_the_cap(entry, family):
    for c in entry.build(family, entry):
        ev = c.evaluate()
        assert math.isfinite(ev['e_ref32']) and math.isfinite(ev['e_alg32']), (entry.name, family, ev['e_ref32'], ev['e_alg32'])
        assert 8 * R.EPS <= ev['bound'] < 1e-3, (entry.name, family, ev['bound'])
        assert bool(torch.isfinite(ev['ref64']).all()) and all(bool(torch.isfinite(t).all()) for t in c.o.values())


def test_gpu_table_covers_the_listed_forms():
    held = {h for e in G.TABLE for h in e.has}
    assert not [n for n in G.LISTED if n not in held]
    assert {e.kind for e in G.TABLE} == set(G.KINDS)
