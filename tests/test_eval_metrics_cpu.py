"""CPU tests of the evaluation metrics (diff-pruning_amd/metrics.py: inception_score, kernel_inception_distance, precision_recall,
knn_radii2, inside_manifold): the launch-site tables of csrc/evalmetrics.hip against its source, and the Python orchestration --
permutation, subset draws, split boundaries, block loops -- over CPU stand-ins of the kernels (tests/mock_ops_eval_metrics.py)
against the fp64 restatement of the definitions (tests/eval_metrics_ref.py).

Where equality is asserted the inputs are small integers: every fp32 Gram element and every squared distance is then exact, so the
stand-in path and the fp64 restatement see the same numbers and no comparison hangs on a rounding.  The double sums differ in order
only: 1e-12 relative."""
import os
import re

import numpy as np
import pytest
import torch

import eval_metrics_ref as R
from helpers import pkg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = 1e-12


@pytest.fixture
def M(monkeypatch):
    import mock_ops_eval_metrics as mock
    mod = pkg('metrics')
    monkeypatch.setattr(mod, 'ops', mock)
    monkeypatch.setattr(mod, '_em_dev', lambda *ts: None)          # the stand-ins take host tensors
    for name in mock.KERNELS:
        assert callable(getattr(mod, name)), name
        monkeypatch.setattr(mod, name, getattr(mock, name))
    del mock.calls[:]
    mod.mock = mock
    return mod


def ints(n, d, seed, lo=-3, hi=4, shift=0):
    g = torch.Generator().manual_seed(seed)
    return (torch.randint(lo, hi, (n, d), generator=g) + shift).float()


# ---------------------------------------------------------------------------------------------- tables against the source
def test_every_launch_site_of_evalmetrics_is_in_its_branch_table():
    """csrc/evalmetrics.hip launches through EM_LAUNCH, a macro of its own with the body of the library's launch macro (ring store,
    count, launch), and its sites are tabled in tests/test_eval_metrics_gpu.py: a new site changes the count, a new kernel is in no
    table, an entry without a case fails -- all before a GPU is needed.  The file must stay out of the two older tables' census, which
    counts the library macro's call text per file."""
    import test_eval_metrics_gpu as T
    csrc = os.path.join(ROOT, 'diff-pruning_amd', 'csrc')
    tabled = {e.split(' | ')[0].split('<')[0] for e in T.BRANCHES}
    seen = set()
    for fname, want in T.LAUNCH_SITES.items():
        src = open(os.path.join(csrc, fname)).read()
        body = src.replace('#define EM_LAUNCH(', '')
        sites = re.findall(r'\bEM_LAUNCH\(\(?\s*([A-Za-z_]\w*)', body)
        assert len(sites) == want == body.count('EM_LAUNCH('), (fname, len(sites), want)
        assert 'DP_' + 'LAUNCH(' not in src, fname
        assert re.search(r'#define EM_LAUNCH\(k, \.\.\.\).*dp_launch_names\[dp_launches\+\+ & \(DP_LAUNCH_RING - 1\)\] = #k;.*'
                         r'hipLaunchKernelGGL\(k, __VA_ARGS__\)', src)
        assert 'atomic' not in src.lower().replace('no atomics', ''), 'the evaluation reductions use no atomics'
        seen.update(sites)
    assert seen == tabled, (sorted(seen - tabled), sorted(tabled - seen))
    assert list(T.LAUNCH_SITES) == ['evalmetrics.hip']
    using = {f for f in os.listdir(csrc) if 'EM_LAUNCH(' in open(os.path.join(csrc, f)).read()}
    assert using == set(T.LAUNCH_SITES), using
    assert all(e in T.CASES for e in T.BRANCHES), sorted(set(T.BRANCHES) - set(T.CASES))
    assert len(set(T.BRANCHES)) == len(T.BRANCHES)
    # the k instantiations of the merge kernel: 1 .. DP_EM_MAX_K, the header's value and metrics.KNN_MAX_K + 1
    hdr = open(os.path.join(ROOT, 'include', 'dp_hip.h')).read()
    kmax = int(re.search(r'#define DP_EM_MAX_K (\d+)', hdr).group(1))
    assert kmax == pkg('metrics').KNN_MAX_K + 1
    assert [e for e in T.BRANCHES if e.startswith('em_knn_merge_kernel')] == ['em_knn_merge_kernel<%d>' % k for k in range(1, kmax + 1)]
    assert len(re.findall(r'EM_KNN_CASE\((\d)\)', src)) == kmax
    # build lists
    assert 'csrc/evalmetrics.hip' in open(os.path.join(ROOT, 'build.sh')).read()
    assert "'csrc/evalmetrics.hip'" in open(os.path.join(ROOT, '__graft_entry__.py')).read()


def test_cpu_tensors_raise():
    mod = pkg('metrics')
    x = torch.zeros(4, 3)
    for call in (lambda: mod.row_norms2(x), lambda: mod.knn_radii2(x, 1), lambda: mod.inside_manifold(x, x, torch.zeros(4)),
                 lambda: mod.precision_recall(x, x, 1), lambda: mod.kernel_inception_distance(x, x, 1, 2),
                 lambda: mod.inception_score(x, 2), lambda: mod.isc_rows(x), lambda: mod.poly_sums(x, 1.0, 1.0, 3),
                 lambda: mod.calculate_metrics('a', 'b', device='cpu')):
        with pytest.raises(RuntimeError):
            call()


# ---------------------------------------------------------------------------------------------- Inception Score
@pytest.mark.parametrize('n,c,splits', [(103, 7, 10), (10, 5, 10), (37, 1008, 4), (12, 1, 3)])
def test_inception_score_orchestration(M, n, c, splits):
    logits = torch.randn(n, c, generator=torch.Generator().manual_seed(n + c)) * 3
    got = M.inception_score(logits, splits=splits)
    mean, std, scores = R.inception_score(logits, splits)
    assert abs(got['inception_score_mean'] - mean) <= EPS * mean and abs(got['inception_score_std'] - std) <= EPS * mean
    # the split boundaries (N not divisible by splits) and the permutation
    col = [c_ for c_ in M.mock.calls if c_[0] == 'isc_colmeans']
    assert [(lo, hi) for _, lo, hi in col] == [(i * n // splits, (i + 1) * n // splits) for i in range(splits)]
    unshuffled = M.inception_score(logits, splits=splits, shuffle=False)
    mean_u, std_u, _ = R.inception_score(logits, splits, shuffle=False)
    assert abs(unshuffled['inception_score_mean'] - mean_u) <= EPS * mean_u and abs(unshuffled['inception_score_std'] - std_u) <= EPS * mean_u
    if c > 1 and n > splits:
        assert unshuffled['inception_score_mean'] != got['inception_score_mean']


def test_inception_score_permutation_is_randomstate_2020(M, monkeypatch):
    n = 23
    logits = torch.arange(n, dtype=torch.float32)[:, None] * torch.ones(1, 3)
    seen = []
    real = M.isc_rows
    monkeypatch.setattr(M, 'isc_rows', lambda l: (seen.append(l[:, 0].clone()), real(l))[1])
    M.inception_score(logits, splits=2)
    assert np.array_equal(seen[0].numpy().astype(np.int64), np.random.RandomState(2020).permutation(n))


def test_inception_score_known_answers(M):
    u = M.inception_score(torch.full((40, 9), 0.25), splits=4)
    assert abs(u['inception_score_mean'] - 1.0) <= 1e-12 and u['inception_score_std'] <= 1e-12
    for c in (4, 10):
        n = 20 * c                                   # every split of the shuffled rows is not balanced, the unshuffled ones are
        logits = torch.zeros(n, c)
        logits[torch.arange(n), torch.arange(n) % c] = 60.0
        s = M.inception_score(logits, splits=4, shuffle=False)
        assert abs(s['inception_score_mean'] - c) <= 1e-9 * c and s['inception_score_std'] <= 1e-9 * c
    with pytest.raises(ValueError):
        M.inception_score(torch.zeros(3, 4), splits=10)


# ---------------------------------------------------------------------------------------------- KID
def test_kid_orchestration_and_subset_draws(M):
    f1, f2 = ints(40, 8, 1), ints(33, 8, 2, shift=1)
    got = M.kernel_inception_distance(f1, f2, subsets=5, subset_size=12)
    mean, std, vals = R.kernel_inception_distance(f1, f2, subsets=5, subset_size=12)
    scale = max(abs(v) for v in vals)
    assert abs(got['kernel_inception_distance_mean'] - mean) <= EPS * scale * 100
    assert abs(got['kernel_inception_distance_std'] - std) <= EPS * scale * 100
    for (a1, a2), (b1, b2) in zip(M.kid_subset_indices(40, 33, 5, 12), R.kid_subsets(40, 33, 5, 12)):
        assert np.array_equal(a1, b1) and np.array_equal(a2, b2)
    rng = np.random.RandomState(2020)
    assert np.array_equal(M.kid_subset_indices(40, 33, 1, 12)[0][0], rng.choice(40, 12, replace=False))
    assert [c for c in M.mock.calls if c[0] == 'bmm_nt'][:3] == [('bmm_nt', 12, 12, 8)] * 3
    # other kernel parameters reach the kernel
    got = M.kernel_inception_distance(f1, f2, subsets=2, subset_size=7, degree=2, gamma=0.5, coef0=0.25)
    mean, std, _ = R.kernel_inception_distance(f1, f2, subsets=2, subset_size=7, degree=2, gamma=0.5, coef0=0.25)
    assert abs(got['kernel_inception_distance_mean'] - mean) <= 1e-12 * abs(mean) * 100


def test_kid_feature_slices(M):
    """d > KID_SLAB: every Gram matrix is ceil(d / 128) batched products over 128-column slices (the last zero-padded), handed to the
    sum kernel as [S, m, m]; the value is the restatement's."""
    f1, f2 = ints(30, 300, 3, -1, 2), ints(25, 300, 4, -1, 2, shift=1)
    got = M.kernel_inception_distance(f1, f2, subsets=3, subset_size=9)
    mean, std, vals = R.kernel_inception_distance(f1, f2, subsets=3, subset_size=9)
    scale = max(abs(v) for v in vals)
    assert abs(got['kernel_inception_distance_mean'] - mean) <= EPS * scale * 100
    assert abs(got['kernel_inception_distance_std'] - std) <= EPS * scale * 100
    assert [c for c in M.mock.calls if c[0] == 'bmm_nt'] == [('bmm_nt', 9, 9, 128)] * 9
    assert [c for c in M.mock.calls if c[0] == 'poly_sums'] == [('poly_sums', 3, 9, 9)] * 9
    x = torch.arange(2 * 5, dtype=torch.float32).view(2, 5)
    sl = M._k_slabs(x, 2)
    assert sl.shape == (3, 2, 2) and sl.is_contiguous() and torch.equal(sl[2], torch.tensor([[4.0, 0.0], [9.0, 0.0]]))
    assert torch.equal(torch.cat([sl[0], sl[1], sl[2]], 1)[:, :5], x) and M._k_slabs(x, 5).shape == (1, 2, 5)


def test_kid_subset_larger_than_a_set_raises(M):
    f1, f2 = ints(10, 4, 1), ints(6, 4, 2)
    for f in (lambda: M.kernel_inception_distance(f1, f2, subsets=2, subset_size=7),
              lambda: M.kernel_inception_distance(f2, f1, subsets=2, subset_size=7), lambda: M.kid_subset_indices(5, 9, 1, 6)):
        with pytest.raises(ValueError):
            f()
    assert np.isfinite(M.kernel_inception_distance(f1, f2, subsets=2, subset_size=6)['kernel_inception_distance_mean'])


def test_kid_of_a_set_against_itself_under_identical_draws_is_not_positive(M, monkeypatch):
    """With X = Y (the same rows drawn on both sides) mmd^2 = 2 (sum K - tr K) / (m (m - 1)) - 2 sum K / m^2
    = 2 (sum K - m tr K) / (m^2 (m - 1)), which is <= 0 for the Gram matrix of a positive-definite kernel: K_ij <= (K_ii + K_jj) / 2,
    so sum K <= m tr K."""
    f = torch.randn(50, 16, generator=torch.Generator().manual_seed(5))
    draws = M.kid_subset_indices(50, 50, 6, 20)
    monkeypatch.setattr(M, 'kid_subset_indices', lambda *a, **k: [(i1, i1) for i1, _ in draws])
    got = M.kernel_inception_distance(f, f, subsets=6, subset_size=20)
    assert got['kernel_inception_distance_mean'] <= 1e-12


# ---------------------------------------------------------------------------------------------- precision / recall
@pytest.mark.parametrize('row_block,col_block', [(4096, 65536), (5, 7), (1, 64), (13, 3)])
def test_knn_and_inside_block_loops(M, row_block, col_block):
    a, b = ints(41, 6, 3), ints(29, 6, 4, shift=1)
    for k in (1, 3, 8):
        r2 = M.knn_radii2(a, k, row_block, col_block)
        assert torch.equal(r2.double(), R.radii2(a, k))
        hit = M.inside_manifold(b, a, r2, row_block, col_block)
        assert torch.equal(hit.bool(), R.inside(b, a, r2))
    merges = [c for c in M.mock.calls if c[0] == 'knn_merge']
    rb, cb = min(row_block, 41), min(col_block, 41)
    per_k = -(-41 // rb) * -(-41 // cb)
    assert len(merges) == 3 * per_k and sum(c[4] for c in merges) == 3 * -(-41 // rb)        # `first` once per row block
    assert {c[1] for c in merges} <= {rb, 41 % rb or rb} and {c[2] for c in merges} <= {cb, 41 % cb or cb}


def test_precision_recall_orchestration_and_known_answers(M):
    f1, f2 = ints(60, 5, 7, -2, 3), ints(45, 5, 8, -2, 3, shift=1)
    got = M.precision_recall(f1, f2, k=3, row_block=16, col_block=11)
    p, r, f = R.precision_recall(f1, f2, 3)
    assert (got['precision'], got['recall']) == (p, r) and abs(got['f_score'] - f) <= 1e-15 and 0 < p < 1 and 0 < r < 1
    same = M.precision_recall(f1, f1.clone(), k=3)
    assert same == {'precision': 1.0, 'recall': 1.0, 'f_score': 1.0}
    far = M.precision_recall(f1, f1 + 1000.0, k=3)
    assert far == {'precision': 0.0, 'recall': 0.0, 'f_score': 0.0}


def test_knn_argument_checks(M):
    a = ints(5, 3, 1)
    with pytest.raises(ValueError):
        M.knn_radii2(a, 9)
    with pytest.raises(ValueError):
        M.knn_radii2(a, 0)
    with pytest.raises(ValueError):
        M.knn_radii2(a, 5)                       # 5 rows have no 6th-smallest distance
    assert M.knn_radii2(a, 4).shape == (5,)


def test_gram_blocks_stay_below_the_32_bit_reach(M):
    reach = 1 << 31
    for n, d in ((50000, 2048), (3000000, 2048), (50000, 1), (3000000, 100000)):
        rb, cb = M._em_blocks(n, n, d, 4096, 65536)
        assert rb * d * 4 < reach and cb * d * 4 < reach and rb * cb * 4 < reach and rb >= 1 and cb >= 1
    assert M._em_blocks(50000, 50000, 2048, 4096, 65536) == (4096, 50000)
    assert M._em_blocks(10 ** 6, 10 ** 6, 2048, 10 ** 6, 10 ** 6)[0] * 2048 * 4 < reach
