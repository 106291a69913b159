"""Global pruning on the device (`-m gpu`): the two launchers of csrc/prune_global.hip and MetaPruner(global_pruning=True) end to end.

  dp_score_groups     bit-equal to dp_group_score called group by group on the same tensors (modes 0-5, a table of more than 24
                      members, a dim-1 member with T = 9, GroupNorm members, index-mapped members, R / C in {1, 3, 63, 64, 65, 257});
                      against fp64 by max(4 e_ref32, 1e-5) on max-abs error over the reference's max-abs -- e_ref32 = the same sums in
                      torch fp32 on the host, 1e-5 = the bound tests/test_kernels_gpu.py holds dp_wg_reduce to.
  dp_select_smallest  EXACT against a host sort of the same values (fp32 -> fp64 is exact, so is the comparison): threshold, per-group
                      ascending positions with score <= threshold, counts; two calls give identical bytes; a NaN is refused.
  end to end          every case of tests/golden/global_prune.json / .npz (the reference's own MagnitudePruner(global_pruning=True)) on the HIP
                      models: indices, shapes, fwd_after < 1e-5 (the bound of tests/test_e2e_gpu.py for tiny_prune.json's fwd_after),
                      gradients of the ratio-0.5 model against the oracle at that file's pruned-sweep bound (2e-5, loss 1e-5), one
                      FinetuneEngine step, save / load / history replay.

Launch-site tables of csrc/prune_global.hip (the discipline of tests/test_eval_metrics_gpu.py, for the file's own PG_LAUNCH macro):
  BRANCHES every kernel expression the file's launch sites can record; LAUNCH_SITES PG_LAUNCH( sites per file
  (tests/test_prune_global_cpu.py counts them); CASES entry -> the cases that reach it and assert the ring names.
Every measured value is printed beside its bound (pytest -s); profiles/prune_global_gpu_tests.txt holds them."""
import ctypes

import numpy as np
import pytest
import torch

import golden_common as gc
from helpers import load_json, make_model, pkg, relerr

pytestmark = pytest.mark.gpu
DEV = 'cuda'

LAUNCH_SITES = {'prune_global.hip': 9}
BRANCHES = ['pg_score_part_kernel', 'pg_score_combine_kernel', 'pg_sel_init_kernel', 'pg_sel_hist_kernel', 'pg_sel_pick_kernel',
            'pg_sel_count_kernel', 'pg_sel_scan_kernel', 'pg_sel_compact_kernel', 'pg_sel_scatter_kernel']
SCORE_NAMES = BRANCHES[:2]
SELECT_NAMES = BRANCHES[2:3] + BRANCHES[3:5] * 4 + BRANCHES[5:]
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
    o = pkg('ops')
    o.L.load()
    return o


def launched(ops, fn):
    """(fn(), the kernel expressions of the launches fn issued, oldest first)."""
    lib = ops.L.load()
    c0 = lib.dp_launch_count()
    r = fn()
    n = lib.dp_launch_count() - c0
    assert 0 < n <= 256, n
    arr = (ctypes.c_char_p * 256)()
    k = lib.dp_recent_launches(arr, 256)
    assert k >= n
    return r, [arr[i].decode() for i in range(k - n, k)]


def _line(report, key, **kw):
    report['prune_global/' + key] = kw
    print('prune_global/%s %s' % (key, ' '.join('%s=%.3e' % (k, v) if isinstance(v, float) else '%s=%s' % (k, v) for k, v in kw.items())))


def rnd(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


# ====================================================================================================================== dp_score_groups
SIZES = (1, 3, 63, 64, 65, 257)


def build_table(mode):
    """Groups of host tensors: [(members, n0, idx lists)], members = dict(w, g, R, C, T, dim, mode, idx) in dp_group_score's terms.
    Per n0 in SIZES: an out-channel conv member, an in-channel conv member with T = 9, an in-channel linear member, a GroupNorm member,
    an index-mapped in-channel member and an index-mapped out-channel member; R / C walk SIZES.  The n0 = 65 group has 31 members."""
    groups, seed = [], 100 * mode
    for gi, n0 in enumerate(SIZES):
        other = SIZES[(gi + 2) % len(SIZES)]
        other2 = SIZES[(gi + 4) % len(SIZES)]
        specs = [(n0, other, 9, 0, None), (other2, n0, 9, 1, None), (other, n0, 1, 1, None), ('gn', n0),
                 (other2, n0 + 5, 1, 1, 'map'), (n0 + 7, other, 1, 0, 'map')]
        if n0 == 65:
            specs += [(n0, 1 + (j % 5), 1 + 8 * (j % 2), 0, None) if j % 3 else (2 + j, n0, 1 + 8 * (j % 2), 1, None) for j in range(25)]
        members = []
        for sp in specs:
            seed += 2
            if sp[0] == 'gn':
                members.append(dict(w=rnd(n0, seed=seed), g=rnd(n0, seed=seed + 1), R=n0, C=1, T=1, dim=0, mode=3, idx=None))
                continue
            R, C, T, dim, mapped = sp
            n_full = R if dim == 0 else C
            idx = None
            if mapped:
                idx = sorted(torch.randperm(n_full, generator=torch.Generator().manual_seed(seed))[:n0].tolist())
            members.append(dict(w=rnd(R, C, T, seed=seed), g=rnd(R, C, T, seed=seed + 1), R=R, C=C, T=T, dim=dim, mode=mode, idx=idx))
        groups.append((members, n0))
    assert max(len(m) for m, _ in groups) > 24
    return groups


def lay_out(groups, device):
    """Offsets as pruning's own member table assigns them: (groups for ops.score_groups, idx tensor, scratch length).  A member
    without an index list takes all n0 channels of its layer in order."""
    table, out = pkg('pruning')._MemberTable(), []
    for members, n0 in groups:
        ms = table.add([(m['w'].to(device).contiguous(), m['g'].to(device).contiguous(), m['R'], m['C'], m['T'], m['dim'], (m['mode'],),
                         m['idx'] if m['idx'] is not None else list(range(n0))) for m in members], n0)
        assert [d['idx_off'] >= 0 for d in ms] == [m['idx'] is not None for m in members]
        out.append((ms, n0))
    return out, torch.tensor(table.idx, dtype=torch.int64, device=device), table.need


def host_scores(groups, dtype):
    """The member sums of every group in `dtype` on the host, members added in order."""
    res = []
    for members, n0 in groups:
        acc = torch.zeros(n0, dtype=dtype)
        for m in members:
            w, g = m['w'].to(dtype), m['g'].to(dtype)
            p = w * g
            if m['mode'] == 3:
                v = p.abs()
            else:
                f = {0: p.abs() ** 2, 1: p.abs(), 2: p, 4: g * g, 5: p}[m['mode']]
                v = f.sum(dim=(1, 2)) if m['dim'] == 0 else f.sum(dim=(0, 2))
                if m['mode'] == 2:
                    v = v.abs()
            acc = acc + (v[m['idx']] if m['idx'] is not None else v)
        res.append(acc)
    return res


@case('pg_score_part_kernel', 'pg_score_combine_kernel')
def score_case(ops, report, mode=0):
    groups = build_table(mode)
    laid, idx, need = lay_out(groups, DEV)
    total = sum(n0 for _, n0 in groups)
    scratch = torch.empty(need, device=DEV)
    scores = torch.full((total,), float('nan'), device=DEV)
    _, names = launched(ops, lambda: ops.score_groups(laid, idx, scratch, scores))
    again = torch.full((total,), float('nan'), device=DEV)
    ops.score_groups(laid, idx, torch.empty(need, device=DEV), again)
    assert torch.equal(scores, again), 'two calls differ'
    off, worst_bits = 0, 0
    ref64, ref32 = host_scores(groups, torch.float64), host_scores(groups, torch.float32)
    for gi, (members, n0) in enumerate(laid):
        # dp_group_score on this group alone, with offsets of its own
        own, oidx, oneed = lay_out([groups[gi]], DEV)
        one = torch.full((n0,), float('nan'), device=DEV)
        ops.group_score(own[0][0], n0, oidx if oidx.numel() else None, torch.empty(max(oneed, 1), device=DEV), one)
        got = scores[off:off + n0]
        assert torch.equal(got, one), ('mode %d group %d (n0 = %d, %d members): bits differ from dp_group_score' % (mode, gi, n0, len(members)),
                                       float((got - one).abs().max()))
        err, e32 = relerr(got, ref64[gi]), relerr(ref32[gi], ref64[gi])
        bound = max(4 * e32, 1e-5)
        _line(report, 'score_groups/mode%d/n0_%d' % (mode, n0), members=len(members), err=err, bound=bound, e_ref32=e32)
        assert err <= bound, (mode, n0, err, bound)
        off += n0
    return names


@pytest.mark.parametrize('mode', [0, 1, 2, 4, 5])
def test_score_groups_equals_group_score_and_fp64(ops, report, mode):
    """Modes 0, 1, 2, 4, 5 on the conv / linear members; mode 3 is the GroupNorm member of every group."""
    assert score_case(ops, report, mode) == SCORE_NAMES


def test_score_groups_refuses_bad_tables(ops):
    """Offsets outside the scratch / index / score vectors and a table that does not tile the scores are refused before any launch."""
    groups = build_table(0)[:2]
    laid, idx, need = lay_out(groups, DEV)
    total = sum(n0 for _, n0 in groups)
    scores = torch.zeros(total, device=DEV)
    lib = ops.L.load()
    c0 = lib.dp_launch_count()
    with pytest.raises(ops.L.DpHipError):
        ops.score_groups(laid, idx, torch.empty(need - 1, device=DEV), scores)                  # scratch one float short
    with pytest.raises(ops.L.DpHipError):
        ops.score_groups(laid, idx[:-1].contiguous(), torch.empty(need, device=DEV), scores)    # index list one entry short
    bad = [(laid[0][0], laid[0][1] + 1), laid[1]]
    with pytest.raises((ops.L.DpHipError, AssertionError)):
        ops.score_groups(bad, idx, torch.empty(need, device=DEV), torch.zeros(total + 1, device=DEV))      # n0 larger than a member
    assert lib.dp_launch_count() == c0


# ====================================================================================================================== dp_select_smallest
def select_input(n, seed):
    x = rnd(n, seed=seed)
    if n >= 63:
        g = torch.Generator().manual_seed(seed + 1)
        x[torch.randint(0, n, (n // 3,), generator=g)] = float(x[5])             # a block of ties
        x[7], x[8], x[9], x[10] = 0.0, -0.0, 1e-41, -1e-41                          # both zeros, denormals of both signs
    return x


def cuts_for(n, seed):
    g = torch.Generator().manual_seed(seed)
    return sorted(set([0, n] + [int(v) for v in torch.randint(0, n + 1, (5,), generator=g)]))


def check_select(ops, report, key, x, cuts, k):
    """Exact: threshold == the k-th smallest by a host sort, every group's positions == `x <= threshold` ascending; the call twice."""
    xd = x.to(DEV)
    (thres, idx, raw), names = launched(ops, lambda: ops.select_smallest(xd, cuts, k, raw=True))
    assert names == SELECT_NAMES, names
    thres2, idx2, raw2 = ops.select_smallest(xd, cuts, k, raw=True)
    assert raw.numpy().tobytes() == raw2.numpy().tobytes(), 'two calls differ'
    x64 = x.double().numpy()
    want = np.sort(x64)[k - 1]
    assert thres == want, (key, thres, want)                                    # 0.0 == -0.0, as torch compares them
    n_sel = 0
    for a, b, ix in zip(cuts, cuts[1:], idx):
        assert ix.dtype == np.int64 and ix.tolist() == np.nonzero(x64[a:b] <= want)[0].tolist(), (key, a, b)
        n_sel += len(ix)
    assert n_sel >= k
    _line(report, 'select/' + key, n=len(x64), k=k, groups=len(cuts) - 1, selected=n_sel, threshold=float(thres), exact=True)


@case(*BRANCHES[2:])
def select_case(ops, report, n=1000):
    for k in sorted({1, max(1, n // 2), n}):
        check_select(ops, report, 'n%d_k%d' % (n, k), select_input(n, 7 + n), cuts_for(n, n), k)


@pytest.mark.parametrize('n', [1, 63, 64, 65, 1000, 70001])
def test_select_smallest_sizes(ops, report, n):
    select_case(ops, report, n)


def test_select_smallest_edge_values(ops, report):
    """All-equal input (every k selects everything); a tie block straddling k (every tie goes); k-th value zero with both zeros present;
    a vector of negative values; one NaN anywhere is refused with a RuntimeError, and so is an inf-free vector around it not."""
    same = torch.full((1000,), 0.37)
    for k in (1, 500, 1000):
        check_select(ops, report, 'all_equal_k%d' % k, same, [0, 10, 1000], k)
    g = torch.Generator().manual_seed(3)
    x = torch.cat([-1.0 - torch.rand(300, generator=g), torch.full((200,), 0.25), 1.0 + torch.rand(500, generator=g)])
    x = x[torch.randperm(1000, generator=g)]
    thres, idx = ops.select_smallest(x.to(DEV), [0, 333, 1000], 400)
    assert thres == 0.25 and sum(len(i) for i in idx) == 500                       # k = 400 falls inside the 200 ties: all are taken
    check_select(ops, report, 'tie_block_k400', x, [0, 333, 1000], 400)
    z = torch.cat([-torch.rand(10, generator=g) - 0.5, torch.tensor([0.0, -0.0, 0.0, -0.0]), torch.rand(10, generator=g) + 0.5])
    check_select(ops, report, 'zeros_k12', z, [0, 11, 24], 12)
    thres, idx = ops.select_smallest(z.to(DEV), [0, 11, 24], 12)
    assert thres == 0.0 and sum(len(i) for i in idx) == 14
    check_select(ops, report, 'negative_k7', -torch.rand(65, generator=g) - 1e-3, [0, 65], 7)
    check_select(ops, report, 'with_inf_k3', torch.tensor([float('inf'), 1.0, -float('inf'), 2.0, 1e-45, -1e-45]), [0, 2, 6], 3)
    for pos in (0, 40, 999):
        bad = select_input(1000, 5)
        bad[pos] = float('nan')
        with pytest.raises(RuntimeError, match='NaN'):
            ops.select_smallest(bad.to(DEV), [0, 1000], 10)
    with pytest.raises(ValueError):
        ops.select_smallest(same.to(DEV), [0, 1000], 1001)


def test_select_smallest_one_million(ops, report):
    """n = 2^20 + 3: more chunks than one scan strip (513 > 256), the histogram grid at its cap, k in the middle."""
    n = (1 << 20) + 3
    x = rnd(n, seed=9)
    x[::7] = x[3]
    check_select(ops, report, 'n%d' % n, x, [0, 5, 70000, 70001, n], n // 2)


@pytest.mark.parametrize('entry', BRANCHES)
def test_branch(ops, report, entry):
    """Every PG_LAUNCH site is reached by a case whose launches name it in the ring (the cases assert the whole name sequence)."""
    assert entry in CASES, 'no case reaches %s' % entry
    for fn in CASES[entry]:
        _, names = launched(ops, lambda: fn(ops, report))
        assert entry in names and set(names) <= set(BRANCHES) | {'group_score_part_kernel', 'group_score_combine_kernel'}, (entry, names)


# ====================================================================================================================== end to end
from test_prune_global_cpu import FX                   # noqa: E402  (global_prune.json + global_prune.npz, put together)
ALL_CASES = ['tiny_taylor_0.1', 'tiny_taylor_0.3', 'tiny_taylor_0.5', 'tiny_magnitude_0.3', 'tiny_taylor_0.3_two_steps',
             'tiny_heads_taylor_0.3', 'ldm_tiny_taylor_0.3']


def hip_case(name):
    """The HIP model of a fixture case after its sweep (gradients from the HIP engine) and the case's stored forward input."""
    from test_e2e_gpu import _inputs, _ldm_model_with_grads, _run_sweep
    if name.startswith('ldm'):
        model, (x, ctx, noise, t) = _ldm_model_with_grads()
        return model, lambda m: m(x, t, context=ctx)
    if name.startswith('tiny_heads'):
        cfg, seed, steps, cs, ns, t = load_json('groups_more.json')['heads8_4lvl']['cfg'], 4, 2, 81, 82, [5, 700]
    else:
        cfg, seed, steps, cs, ns, t = gc.TINY_CFG, 5, 4, 1, 2, [3, 500]
    model = make_model(cfg, seed)
    clean, noise = _inputs(2, cfg['sample_size'], cs, ns)
    _run_sweep(model, clean, noise, steps)
    sched = pkg('diffusion').DDPMScheduler()
    tt = torch.tensor(t, device=DEV)
    return model, lambda m: m(sched.add_noise(clean.to(DEV), noise.to(DEV), tt), tt).sample


def hip_prune(name, model):
    case_ = FX[name]
    if name.startswith('ldm'):
        return pkg('ldm_sweep').prune_ldm_model(model, case_['ratio'], global_pruning=True)
    pruning = pkg('pruning')
    imp = pruning.MagnitudeImportance() if 'magnitude' in name else pruning.TaylorImportance()
    chg = {}
    if name.startswith('tiny_heads'):
        for m in model.modules():
            if hasattr(m, 'to_q') and hasattr(m, 'heads'):
                chg[m.to_q] = chg[m.to_k] = chg[m.to_v] = m.heads
    return pkg('sweep').prune_model(model, case_['ratio'], importance=imp, channel_groups=chg, global_pruning=True,
                                    iterative_steps=case_['iterative_steps'])


def check_records(name, model, pr, report):
    case_ = FX[name]
    want = [g for st in case_['steps'] for g in st['groups'] if g['yielded']]
    assert pr.initial_total_channels == case_['initial_total_channels']
    assert [(r[0], r[1]) for r in pr.records] == [(g['root'], g['ch_groups']) for g in want]
    mism = [g['root'] for r, g in zip(pr.records, want) if r[3] != sorted(gc.expand(g['pruned']))]
    worst = max(relerr(r[2], g['score']) for r, g in zip(pr.records, want))
    thr = case_['steps'][-1]['threshold']
    e_thr = abs(pr.global_threshold - thr) / abs(thr)
    _line(report, 'e2e/' + name, groups=len(pr.records), empty=sum(1 for r in pr.records if not r[3]), mask_mismatches=len(mism),
          score_rel_worst=worst, score_bound=1e-4, threshold_rel=e_thr, gap=min(st['gap'] for st in case_['steps']))
    assert not mism, mism
    assert worst < 1e-4 and e_thr < 1e-4                 # tests/test_e2e_gpu.py's bound for the scores of tiny_prune.json
    assert [list(p.shape) for _, p in model.named_parameters()] == case_['shapes_after']
    assert sum(p.numel() for p in model.parameters()) == case_['params_after']


@pytest.mark.parametrize('name', ALL_CASES)
def test_global_prune_matches_the_reference_on_the_device(ops, report, name):
    """Sweep on the HIP engine, one dp_score_groups + one dp_select_smallest per step, the reference's indices and shapes, and the
    pruned model's forward on the stored input within 1e-5 of the reference's pruned model."""
    model, forward = hip_case(name)
    lib = ops.L.load()
    c0 = lib.dp_launch_count()
    pr = hip_prune(name, model)
    check_records(name, model, pr, report)
    with torch.no_grad():
        y = forward(model)
    e = float((y.cpu() - torch.from_numpy(FX[name]['fwd_after'])).abs().max())
    _line(report, 'e2e/%s/fwd_after' % name, err_abs=e, bound=1e-5, launches=int(lib.dp_launch_count() - c0))
    assert e < 1e-5


def test_group_by_group_path_gives_the_same_indices_on_the_device(ops, report, monkeypatch):
    """PRUNE_BATCH off: dp_wg_reduce member by member, torch.topk on the host -- the same records, bit-equal scores."""
    name = 'tiny_taylor_0.3'
    model, _ = hip_case(name)
    pr = hip_prune(name, model)
    monkeypatch.setattr(pkg('pruning'), 'PRUNE_BATCH', False)
    model2, _ = hip_case(name)
    pr2 = hip_prune(name, model2)
    check_records(name, model2, pr2, report)
    assert [(r[0], r[1], r[3]) for r in pr.records] == [(r[0], r[1], r[3]) for r in pr2.records]
    assert all(torch.equal(a[2], b[2]) for a, b in zip(pr.records, pr2.records)) and pr.global_threshold == pr2.global_threshold


def test_pruned_half_model_trains_and_round_trips(ops, report, tmp_path):
    """The ratio-0.5 model (widths such as 51 and 83): a 2-step sweep against the oracle on the same weights at the bounds of
    tests/test_e2e_gpu.py::test_pruned_model_sweep_matches_oracle (loss 1e-5, gradients 2e-5), one FinetuneEngine step, and
    save_pruned / load_pruned / history replay reproducing the model."""
    from oracle import diffusion_ref as D
    from test_e2e_gpu import _inputs, _run_sweep
    ckpt, pruning, train = pkg('checkpoint'), pkg('pruning'), pkg('train')
    name = 'tiny_taylor_0.5'
    cfg = gc.TINY_CFG
    model, forward = hip_case(name)
    pr = hip_prune(name, model)
    widths = sorted({int(p.shape[0]) for p in model.parameters()})
    clean, noise = _inputs(2, 16)
    P = {n: p.detach().cpu().clone().requires_grad_(True) for n, p in model.named_parameters()}
    res = _run_sweep(model, clean, noise, 2)
    ref = D.taylor_sweep(P, cfg, clean, noise, 2)
    worst = max(relerr(p.grad, P[n].grad) for n, p in model.named_parameters() if float(P[n].grad.abs().max()) > 1e-7)
    loss_rel = max(abs(a - b) / b for a, b in zip(res['losses'], ref))
    _line(report, 'e2e/half_model_sweep', loss_rel=loss_rel, loss_bound=1e-5, grad_rel_worst=worst, grad_bound=2e-5, widths=widths)
    assert loss_rel < 1e-5 and worst < 2e-5
    # history replay + checkpoint round trip (before the finetune step moves the weights)
    hist = pr.pruning_history()
    fresh = make_model(cfg, 5, device='cpu')
    pruning.DependencyGraph(fresh).load_pruning_history(hist)
    assert [list(p.shape) for _, p in fresh.named_parameters()] == FX[name]['shapes_after']
    ckpt.save_pruned(model, str(tmp_path), hist)
    back = ckpt.load_pruned(str(tmp_path)).to(DEV).eval()
    sd = model.state_dict()
    assert len(back.state_dict()) == len(sd) and all(torch.equal(v, sd[k]) for k, v in back.state_dict().items())
    with torch.no_grad():
        assert torch.equal(forward(back), forward(model))
    # one finetune step on the odd widths
    eng = train.FinetuneEngine(model, pkg('diffusion').DDPMScheduler(), lr=2e-4, ema_decay=0.9999)
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    loss = eng.step(clean.to(DEV), noise.to(DEV), torch.tensor([3, 500], device=DEV))
    moved = sum(1 for n, p in model.named_parameters() if not torch.equal(p, before[n]))
    _line(report, 'e2e/half_model_finetune', loss=float(loss), tensors_moved=moved, tensors=len(before))
    assert np.isfinite(float(loss)) and moved > 0.9 * len(before)
