"""The data-free magnitude criteria on the host (`-m "not gpu"`): pruning.MagnitudeImportance (any p, five reductions, six normalisers) and
pruning.LAMPImportance over the torch stand-ins of tests/mock_ops_magnitude.py, against tests/golden/magnitude_family.json / .npz, which
make_golden_magnitude.py recorded from the reference's own classes (ddpm_exp/torch_pruning/importance.py:18-126, 154-219) and its own
MagnitudePruner.

Bound of a score vector: max(4 e_ref32, 1e-5) on helpers.relerr (max-abs error over the group's max-abs score) -- e_ref32 = the
reference's own fp32-against-fp64 error of that configuration, stored per case; 1e-5 = the floor tests/test_prune_global_gpu.py holds
scores to.  The fixture keeps, per group, the fp64 reference at magnitude_ref.sample_positions and the vector's max-abs (the
generator's docstring says why), so the error is the largest over those channels, over the stored max-abs."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import golden_common as gc
import magnitude_ref as MR
from helpers import load_json, load_npz, pkg
from test_cpu import _cpu_engine, _cpu_model, _cpu_step_init, _ldm_inputs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = ('tiny', 'heads', 'ldm')
FLOOR = 1e-5


def load_fixture():
    fx = load_json('magnitude_family.json')
    fx['arrays'] = {m: load_npz('magnitude_family_%s.npz' % m) for m in MODELS}
    return fx


FX = load_fixture()


def config_of(key):
    cls, p, red, norm = key.split('/')
    return cls, (float(p) if '.' in p else int(p)), red, (None if norm == 'None' else norm)


def build_model(name, device=None):
    """-> (model, pruner arguments) of a fixture model, weights as the generator's."""
    if name == 'ldm':
        ldm = pkg('ldm')
        model = ldm.UNetModel(**gc.LDM_TINY_CFG)
        gc.det_init_(model, 9)
        chg = {}
        for m in model.modules():
            if isinstance(m, ldm.CrossAttention):
                chg[m.to_q] = chg[m.to_k] = chg[m.to_v] = m.heads
        model = model.eval() if device is None else model.to(device).eval()
        return model, dict(channel_groups=chg, ignored_layers=[model.out])
    cfg, seed = (gc.TINY_CFG, 5) if name == 'tiny' else (load_json('groups_more.json')['heads8_4lvl']['cfg'], 4)
    model = _cpu_model(cfg, seed)
    if device is not None:
        model = model.to(device)
    chg = {}
    if name == 'heads':
        for m in model.modules():
            if hasattr(m, 'to_q') and hasattr(m, 'heads'):
                chg[m.to_q] = chg[m.to_k] = chg[m.to_v] = m.heads
        assert chg
    return model, dict(channel_groups=chg, ignored_layers=[model.conv_out])


def all_groups(model, kw):
    pruning = pkg('pruning')
    pr = pruning.MagnitudePruner(model, None, importance=pruning.MagnitudeImportance(), ch_sparsity=0.3, **kw)
    groups = list(pr.DG.get_all_groups(pr.ignored_layers, pr.root_module_types))
    return groups, [pr.get_channel_groups(g) for g in groups]


def make_criterion(key, **kw):
    cls, p, red, norm = config_of(key)
    return getattr(pkg('pruning'), cls)(p=p, group_reduction=red, normalizer=norm, **kw)


def score_errors(model_name, key, scores):
    """-> the largest sampled relerr of `scores` (one vector per group) against the fixture's reference of configuration `key`."""
    ref, off, worst = FX['arrays'][model_name]['scores/%s/ref' % key], 0, 0.0
    widths = FX['models'][model_name]['groups']
    assert len(scores) == len(widths)
    for s, (root, n) in zip(scores, widths):
        assert s is not None and s.dtype == torch.float32 and tuple(s.shape) == (n,), root
        pos = MR.sample_positions(n)
        want, top = ref[off:off + len(pos)].astype(np.float64), float(ref[off + len(pos)])
        off += len(pos) + 1
        got = s.detach().cpu().double().numpy()[pos]
        assert np.isfinite(got).all(), (key, root)
        worst = max(worst, float(np.max(np.abs(got - want)) / max(top, 1e-30)))
    assert off == len(ref)
    return worst


@pytest.fixture()
def mocked(monkeypatch):
    import mock_ops_magnitude as mock
    for sub in ('engine', 'sweep', 'train', 'diffusion', 'pruning'):
        monkeypatch.setattr(pkg(sub), 'ops', mock)
    monkeypatch.setattr(pkg('unet').UNet2DModel, 'engine', _cpu_engine)
    monkeypatch.setattr(pkg('sweep').HipSweepStep, '__init__', _cpu_step_init)
    del mock.calls[:]
    return mock


@pytest.fixture(scope='module')
def models():
    """The three fixture models with their groups, built once and never pruned (shared by the score tests)."""
    out = {}
    for name in MODELS:
        model, kw = build_model(name)
        out[name] = (model,) + all_groups(model, kw)
    return out


# ---------------------------------------------------------------------------------------------- the fixture itself
def test_fixture_conditions():
    """What the issue asks of the committed data: every configuration for every model, the gap of every mask case at least 100 times the
    reference's own fp32-against-fp64 error, and a global case whose mask needs the normaliser."""
    for m in MODELS:
        keys = set(FX['models'][m]['scores'])
        want = {'MagnitudeImportance/%s/%s/%s' % (p, r, n) for p in (1, 2, 3, 0.5) for r in MR.REDUCTIONS for n in MR.NORMALIZERS}
        if m != 'ldm':
            want |= {'LAMPImportance/%s/mean/mean' % p for p in (1, 2)}
        assert keys == want, (m, keys ^ want)
        assert all(0 <= v['e_ref32'] < 1e-3 for v in FX['models'][m]['scores'].values())
    assert [len(FX['models'][m]['groups']) for m in MODELS] == [50, 57, 109]
    for name, case in FX['masks'].items():
        assert case['gap'] >= 100 * case['err64'] > 0, name
    crit = {(c['model'], tuple(c['criterion']), c['global_pruning']) for c in FX['masks'].values()}
    for m in ('tiny', 'heads'):
        assert {(m, ('MagnitudeImportance', 1, 'mean', 'mean'), False), (m, ('MagnitudeImportance', 2, 'max', 'standarization'), False),
                (m, ('MagnitudeImportance', 1, 'sum', 'max'), True), (m, ('MagnitudeImportance', 2, 'mean', 'sum'), True),
                (m, ('LAMPImportance', 2, 'mean', 'mean'), True)} <= crit
    assert FX['masks']['ldm_global_p1_sum_max_round2']['round_to'] == 2
    assert any(c.get('differs_without_normalizer') for c in FX['masks'].values())
    assert FX['masks']['tiny_global_p1_sum_max']['differs_without_normalizer']
    for f in ['magnitude_family.json'] + ['magnitude_family_%s.npz' % m for m in MODELS]:
        assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', f)) < (1 << 20), f


# ---------------------------------------------------------------------------------------------- scores
@pytest.mark.parametrize('model_name', MODELS)
def test_every_configuration_scores_like_the_reference(mocked, models, model_name):
    """Every configuration of the fixture through score_all on the stand-ins: one magnitude_rows and one magnitude_finish call for all
    groups (the default configuration: the present score_groups path), each group's vector within its bound."""
    model, groups, chg = models[model_name]
    lines = []
    for key, meta in FX['models'][model_name]['scores'].items():
        imp = make_criterion(key)
        del mocked.calls[:]
        got = imp.score_all(groups, chg)
        names = [c[0] for c in mocked.calls]
        assert names == (['score_groups'] if key == 'MagnitudeImportance/2/mean/mean' else ['magnitude_rows', 'magnitude_finish']), (key, names)
        err, bound = score_errors(model_name, key, got), max(4 * meta['e_ref32'], FLOOR)
        lines.append((err / bound, key, err, bound))
        assert err <= bound, (model_name, key, err, bound)
    print('worst of %s: %s err %.3g bound %.3g' % ((model_name,) + max(lines)[1:]))


@pytest.mark.parametrize('key', ['MagnitudeImportance/1/sum/max', 'MagnitudeImportance/0.5/prod/gaussian',
                                 'MagnitudeImportance/3/max/standarization', 'MagnitudeImportance/2/first/None', 'LAMPImportance/2/mean/mean'])
def test_score_all_equals_group_by_group_calls_and_the_torch_path(mocked, monkeypatch, models, key):
    """score_all == [criterion(group)] bit for bit on the stand-ins; with PRUNE_BATCH off (and for a callable normaliser) the torch
    expressions run group by group, no stand-in is called, and the scores agree within the bound of the configuration."""
    model, groups, chg = models['tiny']
    imp = make_criterion(key)
    got = imp.score_all(groups, chg)
    one = [imp(g, ch_groups=c) for g, c in zip(groups, chg)]
    assert len(got) == len(one) == 50 and all(torch.equal(a, b) for a, b in zip(got, one))
    assert [c[0] for c in mocked.calls] == ['magnitude_rows', 'magnitude_finish'] * 51
    del mocked.calls[:]
    monkeypatch.setattr(pkg('pruning'), 'PRUNE_BATCH', False)
    plain = imp.score_all(groups, chg)
    assert not mocked.calls
    bound = max(4 * FX['models']['tiny']['scores'][key]['e_ref32'], FLOOR)
    assert score_errors('tiny', key, plain) <= bound
    from helpers import relerr
    assert max(relerr(a, b) for a, b in zip(got, plain)) <= 2 * bound


def test_callable_normalizer_and_wide_group_take_the_torch_path(mocked, monkeypatch, models):
    model, groups, chg = models['tiny']
    pruning = pkg('pruning')
    seen = []

    def norm(x):
        seen.append(x)
        return x / x.max()
    got = pruning.MagnitudeImportance(p=1, group_reduction='sum', normalizer=norm).score_all(groups, chg)
    assert not mocked.calls and len(seen) == 50 and all(t.dim() == 1 for t in seen)
    want = pruning.MagnitudeImportance(p=1, group_reduction='sum', normalizer='max').score_all(groups, chg)
    assert score_errors('tiny', 'MagnitudeImportance/1/sum/max', got) <= max(4 * FX['models']['tiny']['scores']['MagnitudeImportance/1/sum/max']['e_ref32'], FLOOR)
    assert len(want) == len(got)
    del mocked.calls[:]
    monkeypatch.setattr(mocked, 'MAGNITUDE_MAX_WIDTH', 127)              # the widest group of the tiny UNet no longer fits
    wide = pruning.MagnitudeImportance(p=1, group_reduction='sum', normalizer='max').score_all(groups, chg)
    n_wide = sum(1 for _, n in FX['models']['tiny']['groups'] if n > 127)
    assert 0 < n_wide < 50 and [c[:2] for c in mocked.calls] == [('magnitude_rows', mocked.calls[0][1]), ('magnitude_finish', 50 - n_wide)]
    assert score_errors('tiny', 'MagnitudeImportance/1/sum/max', wide) <= FLOOR      # the wide groups by torch, each in its place


def test_default_configuration_keeps_the_bits_of_the_parent_commit(mocked, models):
    """MagnitudeImportance(2, 'mean', 'mean') stays on the code path it had: `parent_default/<model>` holds the scores the commit before
    csrc/magnitude.hip gave over tests/mock_ops.py (recorded from a checkout of that commit, not from the code under test)."""
    pruning = pkg('pruning')
    for name in ('tiny', 'heads'):
        model, groups, chg = models[name]
        want = FX['arrays'][name]['parent_default/' + name]
        for imp in (pruning.MagnitudeImportance(), pruning.MagnitudeImportance(2, 'mean', 'mean'), pruning.importance.MagnitudeImportance(p=2)):
            assert not imp.scores_stay_on_device
            got = torch.cat(imp.score_all(groups, chg)).numpy()
            assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), name
            one = torch.cat([imp(g, ch_groups=c) for g, c in zip(groups, chg)]).numpy()
            assert np.array_equal(one.view(np.uint32), want.view(np.uint32)), name
    assert 'magnitude_rows' not in {c[0] for c in mocked.calls}


# ---------------------------------------------------------------------------------------------- masks
def oracle_forward_after(name, model):
    P = {n: p.detach() for n, p in model.named_parameters()}
    with torch.no_grad():
        if name == 'ldm':
            from oracle import ldm_ref as L
            x, ctx, _, t = _ldm_inputs()
            return L.ldm_unet_forward(P, gc.LDM_TINY_CFG, x, t, ctx)
        from oracle import diffusion_ref as D, unet_ref as U
        cfg, cs, ns, t = (gc.TINY_CFG, 1, 2, [3, 500]) if name == 'tiny' else (load_json('groups_more.json')['heads8_4lvl']['cfg'], 81, 82, [5, 700])
        H = cfg['sample_size']
        clean, noise, t = torch.from_numpy(gc.det_clean((2, 3, H, H), cs)), torch.from_numpy(gc.det_noise((2, 3, H, H), ns)), torch.tensor(t)
        return U.unet_forward(P, cfg, D.add_noise(D.alphas_cumprod(), clean, noise, t), t)


def run_mask_case(name, device=None, **kw):
    case = FX['masks'][name]
    cls, p, red, norm = case['criterion']
    imp = getattr(pkg('pruning'), cls)(p=p, group_reduction=red, normalizer=norm)
    model, _ = build_model(case['model'], device)
    if case['model'] == 'ldm':
        pr = pkg('ldm_sweep').prune_ldm_model(model, case['ratio'], importance=imp, global_pruning=case['global_pruning'], round_to=case['round_to'])
    else:
        _, pkw = build_model(case['model'])
        chg = {}
        if case['model'] == 'heads':
            for m in model.modules():
                if hasattr(m, 'to_q') and hasattr(m, 'heads'):
                    chg[m.to_q] = chg[m.to_k] = chg[m.to_v] = m.heads
        pr = pkg('sweep').prune_model(model, case['ratio'], importance=imp, channel_groups=chg, global_pruning=case['global_pruning'])
    return model, pr


def check_mask_case(name, model, pr):
    case = FX['masks'][name]
    assert [(r[0], r[1]) for r in pr.records] == [(g[0], g[1]) for g in case['groups']]
    mism = [g[0] for r, g in zip(pr.records, case['groups']) if r[3] != sorted(gc.expand(g[2]))]
    assert not mism, (name, mism)
    assert [list(p.shape) for _, p in model.named_parameters()] == case['shapes_after']
    assert sum(p.numel() for p in model.parameters()) == case['params_after']
    if case['global_pruning']:
        assert pr.initial_total_channels == case['initial_total_channels']
        assert abs(pr.global_threshold - case['threshold']) <= 1e-5 * abs(case['threshold'])


@pytest.mark.parametrize('name', sorted(FX['masks']))
def test_masks_match_the_reference(mocked, name):
    """The reference's own MagnitudePruner with each criterion: the same yielded groups in the same order, the same indices, shapes
    after, the global threshold; the oracle's forward on the pruned weights gives the reference's fwd_after."""
    model, pr = run_mask_case(name)
    check_mask_case(name, model, pr)
    case = FX['masks'][name]
    names = [c[0] for c in mocked.calls]
    if case['global_pruning']:
        assert names == ['magnitude_rows', 'magnitude_finish', 'select_smallest'], names
    else:
        assert set(names) == {'magnitude_rows', 'magnitude_finish'} and len(names) == 2 * len(pr.records)
    y = oracle_forward_after(case['model'], model)
    e = float((y - torch.from_numpy(FX['arrays'][case['model']]['masks/%s/fwd_after' % name])).abs().max())
    assert e < 1e-5, (name, e)


def test_the_normaliser_decides_the_global_mask(mocked):
    """(p = 1, 'sum', 'max') globally: the fixture's mask differs from the mask of the un-normalised member sum (what a criterion that
    ignores `normalizer` yields), so reproducing the fixture needs the normaliser."""
    model, pr = run_mask_case('tiny_global_p1_sum_max')
    pruning = pkg('pruning')
    bare_model, _ = build_model('tiny')
    bare = pkg('sweep').prune_model(bare_model, FX['masks']['tiny_global_p1_sum_max']['ratio'],
                                    importance=pruning.MagnitudeImportance(p=1, group_reduction='sum', normalizer=None), global_pruning=True)
    assert [(r[0], r[3]) for r in bare.records] != [(r[0], r[3]) for r in pr.records]


# ---------------------------------------------------------------------------------------------- arguments
def test_argument_errors():
    pruning = pkg('pruning')
    M, L = pruning.importance.MagnitudeImportance, pruning.importance.LAMPImportance
    for cls in (M, L):
        with pytest.raises(NotImplementedError):
            cls(group_reduction='median')
        with pytest.raises(NotImplementedError):
            cls(normalizer='standardization')                           # the reference's spelling is 'standarization'
        with pytest.raises(ValueError):
            cls(group_reduction=None)
        for p in (0, -1, None, 'two'):
            with pytest.raises(ValueError):
                cls(p=p)
        for p in (1, 2, 3, 0.5, 2.0):
            assert cls(p=p).p == p
        assert cls(normalizer=None).normalizer is None and callable(cls(normalizer=lambda x: x).normalizer)
    assert L().lamp == 'vendored' and L(paper_order=True).lamp == 'paper' and M().lamp is None
    assert 'honours only' in pruning.TaylorImportance.__doc__


def test_lamp_refuses_members_of_different_length_and_keeps_index_order(mocked):
    """A group whose members differ in length: MagnitudeImportance drops the odd member (importance.py:118-122), LAMPImportance raises
    RuntimeError naming the root.  LAMP leaves the index lists as they are; MagnitudeImportance sorts them in place."""
    pruning = pkg('pruning')
    a, b = torch.nn.Conv2d(3, 6, 3), torch.nn.Conv2d(6, 4, 1)
    idx = [5, 0, 3, 1, 2, 4]
    group = pruning.Group([(pruning.Dependency(a, 'conv_a', 'out'), list(idx)), (pruning.Dependency(b, 'conv_b', 'in'), list(idx))])
    lamp = pruning.LAMPImportance(p=2)
    got = lamp(group)
    assert [ix for _, ix in group] == [idx, idx]
    rows = MR.member_rows([(a.weight, 6, 3, 9, 0, idx), (b.weight, 4, 6, 1, 1, idx)], 2, root=True)
    from helpers import relerr
    assert relerr(got, MR.finish(rows, 'mean', 'mean', 'vendored')) < FLOOR
    # an in-channel member with the group's channels twice over (both halves of a concatenation): importance.py:188-195 views it as
    # [n0, 2, .] -- two consecutive entries of its list to a channel; here and in the torch path
    c = torch.nn.Conv2d(12, 5, 3)
    twice = [7, 1, 0, 11, 4, 5, 2, 3, 10, 9, 8, 6]
    folded = pruning.Group([(pruning.Dependency(a, 'conv_a', 'out'), list(idx)), (pruning.Dependency(c, 'conv_c', 'in'), list(twice))])
    rows = MR.member_rows([(a.weight, 6, 3, 9, 0, idx), (c.weight, 5, 12, 9, 1, twice)], 2, root=True)
    pair = c.weight.detach().double()[:, [7, 1]].reshape(-1)
    assert abs(float(rows[1, 0]) - float(pair.square().sum().sqrt())) < 1e-12
    got = lamp(folded)
    assert mocked.calls[-2:] == [('magnitude_rows', 2), ('magnitude_finish', 1, 'mean', 'mean', 'vendored')]
    assert relerr(got, MR.finish(rows, 'mean', 'mean', 'vendored')) < FLOOR
    assert relerr(lamp._torch_score(*lamp._mag_members(folded)), MR.finish(rows, 'mean', 'mean', 'vendored')) < FLOOR
    odd = pruning.Group([(pruning.Dependency(a, 'conv_a', 'out'), list(idx)), (pruning.Dependency(b, 'conv_b', 'in'), [0, 1, 2])])
    with pytest.raises(RuntimeError, match='conv_a'):
        lamp(odd)
    with pytest.raises(RuntimeError, match='conv_a'):                    # an out-channel member of another length: torch.stack fails there
        lamp(pruning.Group([(pruning.Dependency(a, 'conv_a', 'out'), [0, 1, 2]), (pruning.Dependency(a, 'conv_a2', 'out'), list(idx))]))
    mag = pruning.MagnitudeImportance(p=1, group_reduction='sum', normalizer=None)
    got = mag(odd)
    assert odd[0][1] == sorted(idx)
    assert relerr(got, MR.member_rows([(a.weight, 6, 3, 9, 0, sorted(idx))], 1)[0]) < FLOOR
    with pytest.raises(IndexError):
        mag(pruning.Group([(pruning.Dependency(a, 'conv_a', 'out'), [0, 6])]))


@pytest.mark.parametrize('p', [1, 2])
def test_paper_order_matches_the_fp64_restatement(mocked, models, p):
    """paper_order=True: each channel gets its own LAMP score (the scatter with the true inverse permutation), against the fp64
    restatement of tests/magnitude_ref.py on every group of the tiny UNet; the vendored order differs from it on the same groups."""
    from helpers import relerr
    model, groups, chg = models['tiny']
    pruning = pkg('pruning')
    got = pruning.LAMPImportance(p=p, paper_order=True).score_all(groups, chg)
    vend = pruning.LAMPImportance(p=p).score_all(groups, chg)
    bound = max(4 * FX['models']['tiny']['scores']['LAMPImportance/%d/mean/mean' % p]['e_ref32'], FLOOR)
    differs = 0
    for g, s, v in zip(groups, got, vend):
        members = pruning.LAMPImportance(p=p)._mag_members(g)[1]
        rows = MR.member_rows(members, p, root=True)
        want = MR.finish(rows, 'mean', 'mean', 'paper')
        assert relerr(s, want) <= bound
        assert relerr(v, MR.finish(rows, 'mean', 'mean', 'vendored')) <= bound
        # the paper's score: the largest channel scores 1, and ascending scores follow ascending magnitudes
        assert float(s.max()) == 1.0 and torch.equal(torch.argsort(s), torch.argsort(MR.finish(rows, 'mean', 'mean').float(), stable=True)) \
            or len(s) < 3
        differs += int(not torch.equal(s, v))
    assert differs > 40


# ---------------------------------------------------------------------------------------------- the library surface
def test_header_signatures_build_and_launch_sites_agree():
    """include/dp_hip.h, _lib.SIGNATURES, ops and build.sh agree on csrc/magnitude.hip; its launches go through MG_LAUNCH, a macro of its own
    with the body of the library's launch macro, and its sites are tabled in tests/test_magnitude_family_gpu.py."""
    import test_magnitude_family_gpu as T
    L, ops = pkg('_lib'), pkg('ops')
    hdr = open(os.path.join(ROOT, 'include', 'dp_hip.h')).read()
    for name in ('dp_magnitude_rows', 'dp_magnitude_finish', 'dp_magnitude_max_width'):
        assert re.search(r'^int %s\(' % name, hdr, re.M) and name in L.SIGNATURES
    assert ctypes.sizeof(L.MagMember) == 56 and ctypes.sizeof(L.MagGroup) == 24
    assert re.search(r'typedef struct dp_mag_member \{\s*const float\* w;\s*int R, C, T, dim, n0, blk0, fold, _pad;\s*long long idx_off, row_off;\s*\}', hdr)
    assert [f[0] for f in L.MagMember._fields_] == ['w', 'R', 'C', 'T', 'dim', 'n0', 'blk0', 'fold', '_pad', 'idx_off', 'row_off']
    assert re.search(r'typedef struct dp_mag_group \{\s*long long row_off, score_off;\s*int n0, members;\s*\}', hdr)
    lib = L.load()
    assert lib.dp_magnitude_max_width() == ops.MAGNITUDE_MAX_WIDTH >= 4096
    import mock_ops_magnitude as mock
    assert mock.MAGNITUDE_MAX_WIDTH == ops.MAGNITUDE_MAX_WIDTH
    for tab in ('MAGNITUDE_REDUCTIONS', 'MAGNITUDE_NORMALIZERS', 'MAGNITUDE_LAMP'):
        assert getattr(mock, tab) == getattr(ops, tab)
    assert list(ops.MAGNITUDE_REDUCTIONS) == MR.REDUCTIONS and list(ops.MAGNITUDE_NORMALIZERS) == MR.NORMALIZERS
    assert 'csrc/magnitude.hip' in open(os.path.join(ROOT, 'build.sh')).read()
    csrc = os.path.join(ROOT, 'diff-pruning_amd', 'csrc')
    src = open(os.path.join(csrc, 'magnitude.hip')).read()
    assert '#define MG_MAX_WIDTH %d' % ops.MAGNITUDE_MAX_WIDTH in src
    body = src.replace('#define MG_LAUNCH(', '')
    sites = re.findall(r'\bMG_LAUNCH\(\(?\s*([A-Za-z_]\w*(?:<\d>)?)', body)
    assert list(T.LAUNCH_SITES) == ['magnitude.hip'] and len(sites) == T.LAUNCH_SITES['magnitude.hip'] == body.count('MG_LAUNCH('), sites
    assert 'DP_' + 'LAUNCH(' not in src.replace('DP_LAUNCH_CHECK(', '') and 'atomicAdd' not in src and 'atomicCAS' not in src
    assert re.search(r'#define MG_LAUNCH\(k, \.\.\.\).*dp_launch_names\[dp_launches\+\+ & \(DP_LAUNCH_RING - 1\)\] = #k;.*'
                     r'hipLaunchKernelGGL\(k, __VA_ARGS__\)', src)
    assert set(sites) == set(T.BRANCHES) and len(set(T.BRANCHES)) == len(T.BRANCHES)
    assert all(e in T.CASES for e in T.BRANCHES), sorted(set(T.BRANCHES) - set(T.CASES))
    using = {f for f in os.listdir(csrc) if 'MG_LAUNCH(' in open(os.path.join(csrc, f)).read()}
    assert using == {'magnitude.hip'}
    assert set(vars(pkg('pruning').importance)) >= {'MagnitudeImportance', 'LAMPImportance'}
