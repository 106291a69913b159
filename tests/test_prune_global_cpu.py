"""Global pruning on the host (`-m "not gpu"`): MetaPruner(global_pruning=True) over the CPU stand-ins of tests/mock_ops_prune_global.py
against tests/golden/global_prune.json, which make_golden_global.py recorded from the reference's own
`MagnitudePruner(global_pruning=True)` (metapruner.py:126-133, 256-297).  The gradients are the oracle's (torch autograd on the host, as
the reference's are); every committed case decides its mask with a relative gap between the k-th and (k+1)-th smallest score of at least
100 times the fp32-against-fp64 error of the reference's own scores (asserted by the generator, re-checked here)."""
import numpy as np
import pytest
import torch

import golden_common as gc
from helpers import load_json, load_npz, oracle_params, pkg, relerr
from test_cpu import _cpu_engine, _cpu_model, _cpu_step_init, _ldm_grads_oracle


def load_fixture():
    """global_prune.json with the arrays of global_prune.npz put back: every group row becomes dict(root, ch_groups, score, score64,
    yielded, pruned) with its slice of the step's concatenated ranked scores; `fwd_after` per case."""
    fx, arr = load_json('global_prune.json'), load_npz('global_prune.npz')
    for name, case in fx.items():
        case['fwd_after'] = arr[name + '/fwd_after']
        for i, st in enumerate(case['steps']):
            s32, s64, off, groups = arr['%s/%d/score32' % (name, i)], arr['%s/%d/score64' % (name, i)], 0, []
            assert s32.dtype == np.float32 and s64.dtype == np.float64 and len(s32) == len(s64) == st['n_ranked']
            for root, chg, n, yielded, pruned in st['groups']:
                groups.append(dict(root=root, ch_groups=chg, score=s32[off:off + n], score64=s64[off:off + n], yielded=bool(yielded),
                                   pruned=pruned))
                off += n
            assert off == st['n_ranked']
            st['groups'] = groups
    return fx


FX = load_fixture()
TINY_CASES = ['tiny_taylor_0.1', 'tiny_taylor_0.3', 'tiny_taylor_0.5', 'tiny_magnitude_0.3', 'tiny_taylor_0.3_two_steps']
ALL_CASES = TINY_CASES + ['tiny_heads_taylor_0.3', 'ldm_tiny_taylor_0.3']
SCORE_BOUND = 2e-5          # the bound tests/test_cpu.py holds the mocked criteria's scores to against the reference's


@pytest.fixture()
def mocked(monkeypatch):
    import mock_ops_prune_global as mock
    for sub in ('engine', 'sweep', 'train', 'diffusion', 'pruning'):
        monkeypatch.setattr(pkg(sub), 'ops', mock)
    monkeypatch.setattr(pkg('unet').UNet2DModel, 'engine', _cpu_engine)
    monkeypatch.setattr(pkg('sweep').HipSweepStep, '__init__', _cpu_step_init)
    del mock.calls[:]
    return mock


def test_fixture_conditions():
    """What the issue asks of every committed case, from the stored numbers: the cases, both steps of the iterative one, empty index
    lists present, and gap >= 100 x the largest relative fp32-vs-fp64 difference of the ranked scores (recomputed from both)."""
    assert sorted(FX) == sorted(ALL_CASES)
    assert [len(FX[c]['steps']) for c in ALL_CASES] == [1, 1, 1, 1, 2, 1, 1]
    assert all(FX[c]['initial_total_channels'] == 1048 for c in TINY_CASES)
    for name, case in FX.items():
        for st in case['steps']:
            s32 = np.concatenate([g['score'] for g in st['groups']])
            s64 = np.concatenate([g['score64'] for g in st['groups']])
            k = st['n_pruned']
            assert len(s32) == st['n_ranked'] and 0 < k < len(s32)
            srt = np.sort(s32).astype(np.float64)
            gap = (srt[k] - srt[k - 1]) / srt[k]
            err = float(np.max(np.abs(s32.astype(np.float64) - s64) / np.abs(s64)))
            assert st['threshold'] == float(np.float32(srt[k - 1]))
            assert abs(gap - st['gap']) <= 1e-12 and abs(err - st['err64']) <= 1e-12
            assert gap >= 100 * err, (name, gap, err)
            assert any(not g['pruned'] for g in st['groups']), name          # groups that lose no channel are recorded (and yielded)


def test_every_launch_site_of_prune_global_is_in_its_branch_table():
    """csrc/prune_global.hip launches through PG_LAUNCH, a macro of its own with the body of the library's launch macro, and its sites
    are tabled in tests/test_prune_global_gpu.py (the discipline of tests/test_eval_metrics_cpu.py): a new site changes the count, a new
    kernel is in no table, an entry without a case fails -- before a GPU is needed.  The file stays out of the older tables' census,
    which counts the library macro's call text per file; dp_score_groups uses no atomics at all."""
    import os
    import re
    import test_prune_global_gpu as T
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'diff-pruning_amd', 'csrc')
    assert list(T.LAUNCH_SITES) == ['prune_global.hip']
    src = open(os.path.join(csrc, 'prune_global.hip')).read()
    body = src.replace('#define PG_LAUNCH(', '')
    sites = re.findall(r'\bPG_LAUNCH\(\(?\s*([A-Za-z_]\w*)', body)
    assert len(sites) == T.LAUNCH_SITES['prune_global.hip'] == body.count('PG_LAUNCH('), sites
    assert 'DP_' + 'LAUNCH(' not in src
    assert re.search(r'#define PG_LAUNCH\(k, \.\.\.\).*dp_launch_names\[dp_launches\+\+ & \(DP_LAUNCH_RING - 1\)\] = #k;.*'
                     r'hipLaunchKernelGGL\(k, __VA_ARGS__\)', src)
    assert set(sites) == set(T.BRANCHES) and len(set(T.BRANCHES)) == len(T.BRANCHES)
    assert all(e in T.CASES for e in T.BRANCHES), sorted(set(T.BRANCHES) - set(T.CASES))
    using = {f for f in os.listdir(csrc) if 'PG_LAUNCH(' in open(os.path.join(csrc, f)).read()}
    assert using == {'prune_global.hip'}
    score_part = src[:src.index('#define PG_HIST_BLOCKS')]                      # dp_score_groups: no atomics of any kind
    assert 'atomicAdd' not in score_part and src.count('atomicAdd(') == src.count('atomicAdd(&h[') == 2        # LDS counters only


def tiny_model_with_oracle_grads(name):
    """The model of a fixture case with the oracle's accumulated gradients (the reference's sweep, on the host in fp32)."""
    from oracle import diffusion_ref as D
    if name.startswith('tiny_heads'):
        cfg, seed, steps, cs, ns = load_json('groups_more.json')['heads8_4lvl']['cfg'], 4, 2, 81, 82
    else:
        cfg, seed, steps, cs, ns = gc.TINY_CFG, 5, 4, 1, 2
    H = cfg['sample_size']
    clean = torch.from_numpy(gc.det_clean((2, 3, H, H), cs))
    noise = torch.from_numpy(gc.det_noise((2, 3, H, H), ns))
    P = oracle_params(cfg, seed)
    D.taylor_sweep(P, cfg, clean, noise, steps)
    model = _cpu_model(cfg, seed)
    for n, p in model.named_parameters():
        p.grad = P[n].grad.clone()
    return model


def run_case(name, **kw):
    """-> (model, pruner) after every step of the case, through the package's own entry points."""
    case = FX[name]
    if name.startswith('ldm'):
        ldm = pkg('ldm')
        cfg, P = _ldm_grads_oracle()
        model = ldm.UNetModel(**cfg)
        gc.det_init_(model, 9)
        for n, p in model.named_parameters():
            p.grad = P[n].grad.clone()
        pr = pkg('ldm_sweep').prune_ldm_model(model, case['ratio'], global_pruning=True, **kw)
        return model, pr
    pruning = pkg('pruning')
    model = tiny_model_with_oracle_grads(name)
    imp = pruning.MagnitudeImportance() if 'magnitude' in name else pruning.TaylorImportance()
    chg = {}
    if name.startswith('tiny_heads'):
        for m in model.modules():
            if hasattr(m, 'to_q') and hasattr(m, 'heads'):
                chg[m.to_q] = chg[m.to_k] = chg[m.to_v] = m.heads
        assert chg
    pr = pkg('sweep').prune_model(model, case['ratio'], importance=imp, channel_groups=chg, global_pruning=True,
                                  iterative_steps=case['iterative_steps'], **kw)
    return model, pr


def check_against_fixture(name, model, pr, score_bound=SCORE_BOUND):
    case = FX[name]
    assert pr.initial_total_channels == case['initial_total_channels']
    want = [g for st in case['steps'] for g in st['groups'] if g['yielded']]
    assert [(r[0], r[1]) for r in pr.records] == [(g['root'], g['ch_groups']) for g in want]         # the same groups, the same order
    worst = 0.0
    for r, g in zip(pr.records, want):
        assert r[3] == sorted(gc.expand(g['pruned'])), (name, g['root'])
        worst = max(worst, relerr(r[2], g['score']))
    assert worst < score_bound, (name, worst)
    thr = case['steps'][-1]['threshold']
    assert abs(pr.global_threshold - thr) <= score_bound * abs(thr), (pr.global_threshold, thr)
    assert [list(p.shape) for _, p in model.named_parameters()] == case['shapes_after']
    assert sum(p.numel() for p in model.parameters()) == case['params_after']
    return worst


@pytest.mark.parametrize('name', ALL_CASES)
def test_global_prune_matches_the_reference(mocked, name):
    """The same yielded groups in the same order, the same indices (empty lists included), the threshold, initial_total_channels,
    shapes_after -- both steps of the iterative case -- with every group scored in one call and selected in one call per step."""
    model, pr = run_case(name)
    check_against_fixture(name, model, pr)
    steps = FX[name]['iterative_steps']
    assert [c[0] for c in mocked.calls] == ['score_groups', 'select_smallest'] * steps, mocked.calls
    assert [c[3] for c in mocked.calls if c[0] == 'select_smallest'] == [st['n_pruned'] for st in FX[name]['steps']]
    assert any(not r[3] for r in pr.records)                            # a group that loses nothing is yielded, as the reference does
    hist = pr.pruning_history()
    assert len(hist) == len(pr.records) and [h[0] for h in hist] == [r[0] for r in pr.records]


@pytest.mark.parametrize('name', ['tiny_taylor_0.3', 'tiny_magnitude_0.3', 'tiny_taylor_0.3_two_steps', 'ldm_tiny_taylor_0.3'])
def test_group_by_group_path_gives_the_same_indices(mocked, monkeypatch, name):
    """PRUNE_BATCH off: the criterion is called group by group and the selection is torch.topk on the host -- the same records."""
    _, batched = run_case(name)
    assert mocked.calls
    del mocked.calls[:]
    monkeypatch.setattr(pkg('pruning'), 'PRUNE_BATCH', False)
    model, plain = run_case(name)
    assert not mocked.calls
    assert [(r[0], r[1], r[3]) for r in plain.records] == [(r[0], r[1], r[3]) for r in batched.records]
    assert plain.global_threshold == batched.global_threshold
    check_against_fixture(name, model, plain)


@pytest.mark.parametrize('crit', ['full1', 'full2', 'abs', 'fisher', 'taylor_mv'])
def test_every_criterion_scores_all_groups_like_its_call(mocked, crit):
    """score_all(groups) == [criterion(group)] bit for bit on the stand-ins (same member reductions, same member order, the criterion's
    own finish); FullTaylorImportance(order=2) adds two reductions per member before the member sum and is scored group by group."""
    pruning = pkg('pruning')
    model = tiny_model_with_oracle_grads('tiny_taylor_0.3')
    imp = dict(full1=lambda: pruning.FullTaylorImportance(order=1), full2=lambda: pruning.FullTaylorImportance(order=2),
               abs=pruning.AbsTaylorImportance, fisher=pruning.FisherImportance,
               taylor_mv=lambda: pruning.TaylorImportance(multivariable=True))[crit]()
    pr = pruning.MagnitudePruner(model, None, importance=imp, global_pruning=True, ch_sparsity=0.3, ignored_layers=[model.conv_out])
    groups = list(pr.DG.get_all_groups(pr.ignored_layers, pr.root_module_types))
    got = imp.score_all(groups, [pr.get_channel_groups(g) for g in groups])
    assert bool(mocked.calls) == (crit != 'full2')
    want = [imp(g) for g in groups]
    assert len(got) == len(want) == 50
    assert all((a is None) == (b is None) and (a is None or torch.equal(a, b)) for a, b in zip(got, want))
    for g in pr.step(interactive=True):
        g.prune()
    assert pr.records and sum(p.numel() for p in model.parameters()) < 2257283


def test_stand_in_select_equals_topk():
    """The stand-in (integer image of the floats, integer selection) against torch.topk + `<=` on random vectors with ties, both
    zeros, negative values and a denormal; a NaN is refused; k = 1 and k = n."""
    import mock_ops_prune_global as mock
    g = torch.Generator().manual_seed(11)
    for n in (1, 2, 63, 64, 65, 1000):
        x = torch.randn(n, generator=g)
        if n >= 63:
            x[torch.randint(0, n, (n // 3,), generator=g)] = float(x[5])                  # a tie block
            x[7], x[8], x[9], x[10] = 0.0, -0.0, 1e-41, -1e-41
        cuts = sorted(set([0, n] + [int(v) for v in torch.randint(0, n + 1, (4,), generator=g)]))
        for k in sorted({1, max(1, n // 2), n}):
            thres, idx = mock.select_smallest(x, cuts, k)
            want = torch.topk(x, k=k, largest=False)[0][-1]
            assert thres == float(want), (n, k)
            for a, b, ix in zip(cuts, cuts[1:], idx):
                assert ix.tolist() == (x[a:b] <= want).nonzero().view(-1).tolist()
    keys = mock.float_keys(np.array([-np.inf, -1.0, -1e-41, -0.0, 0.0, 1e-41, 1.0, np.inf], dtype=np.float32))
    assert keys[3] == keys[4] and all(a < b for a, b in zip(np.delete(keys, 3), np.delete(keys, 3)[1:]))
    with pytest.raises(RuntimeError):
        mock.select_smallest(torch.tensor([1.0, float('nan'), 2.0]), [0, 3], 1)
    with pytest.raises(ValueError):
        mock.select_smallest(torch.tensor([1.0, 2.0]), [0, 2], 3)


def test_local_path_is_unchanged(mocked):
    """global_pruning=False over the new stand-in module still produces tiny_prune.json's indices, without a global call."""
    fx = load_json('tiny_prune.json')
    model = _cpu_model(gc.TINY_CFG, 5)
    clean = torch.from_numpy(gc.det_clean((2, 3, 16, 16), 1))
    noise = torch.from_numpy(gc.det_noise((2, 3, 16, 16), 2))
    sweep = pkg('sweep')
    sweep.taylor_sweep(model, pkg('diffusion').DDPMScheduler(), clean, noise, num_steps=4)
    pr = sweep.prune_model(model, 0.3)
    assert not pr.global_pruning and pr.global_threshold is None and not mocked.calls
    assert [r[3] for r in pr.records] == [r['pruned'] for r in fx['prune']]
    assert {n: list(p.shape) for n, p in model.named_parameters()} == fx['shapes_after']


@pytest.mark.parametrize('name', ['tiny_taylor_0.5', 'ldm_tiny_taylor_0.3'])
def test_history_and_checkpoint_round_trip(mocked, tmp_path, name):
    """pruning_history() of a globally pruned model (empty index lists included) replays on a fresh model, and checkpoint.save_pruned /
    load_pruned reproduce every tensor; the pruned tiny UNet still runs a sweep step on the (stand-in) engine."""
    ckpt, pruning = pkg('checkpoint'), pkg('pruning')
    model, pr = run_case(name)
    hist = pr.pruning_history()
    if name.startswith('ldm'):
        fresh = pkg('ldm').UNetModel(**gc.LDM_TINY_CFG)
    else:
        fresh = _cpu_model(gc.TINY_CFG, 5)
    pruning.DependencyGraph(fresh).load_pruning_history(hist)
    assert [list(p.shape) for _, p in fresh.named_parameters()] == FX[name]['shapes_after']
    ckpt.save_pruned(model, str(tmp_path), hist)
    back = ckpt.load_pruned(str(tmp_path))
    sd = model.state_dict()
    assert len(back.state_dict()) == len(sd) and all(torch.equal(v, sd[k]) for k, v in back.state_dict().items())
    if not name.startswith('ldm'):
        clean = torch.from_numpy(gc.det_clean((2, 3, 16, 16), 1))
        noise = torch.from_numpy(gc.det_noise((2, 3, 16, 16), 2))
        res = pkg('sweep').taylor_sweep(model, pkg('diffusion').DDPMScheduler(), clean, noise, num_steps=1)
        assert np.isfinite(res['losses'][0])
