"""The ddpm_exp sampler's host side (diff-pruning_amd/ddpm_exp_sampler.py) without a GPU: the timestep lists and alpha tables against
the fixtures the reference wrote (tests/golden/make_golden_ddpm_exp_sampler.py), the Python loops over a CPU stand-in of the two
kernels (tests/mock_ops_sampler.py) against the reference's own chains and single steps, and the file bookkeeping of the jobs."""
import os

import numpy as np
import pytest
import torch

import ddpm_exp_sampler_ref as R
from helpers import pkg


@pytest.fixture
def S(monkeypatch):
    import mock_ops_sampler
    mod = pkg('ddpm_exp_sampler')
    monkeypatch.setattr(mod, 'ops', mock_ops_sampler)
    del mock_ops_sampler.calls[:]
    return mod


def _betas():
    return pkg('ddpm_exp_sampler').linear_betas()


# ---------------------------------------------------------------------------------------------- (a) sequences, alpha tables
def test_timestep_sequences_and_alpha_tables_equal_the_reference():
    S, g = pkg('ddpm_exp_sampler'), R.load(R.SEQ_FILE)
    table = S.alpha_table(_betas())
    assert table.dtype == torch.float32 and table.shape == (1001,) and float(table[0]) == 1.0
    for k, (T, n, skip) in enumerate(R.SEQ_CASES):
        seq = S.timestep_sequence(T, n, skip)
        assert seq == [int(v) for v in g['%d:seq' % k]] and all(type(v) is int for v in seq), (T, n, skip)
        assert np.array_equal(table[torch.tensor(seq) + 1].numpy(), g['%d:alpha' % k]), (T, n, skip)
        assert np.array_equal(table[:1].numpy(), g['%d:alpha_m1' % k])
    assert len(S.timestep_sequence(1000, 7, 'uniform')) == 8 and S.timestep_sequence(1000, 7, 'uniform')[-1] == 994
    q = S.timestep_sequence(1000, 100, 'quad')
    assert q[:6] == [0, 0, 0, 0, 1, 2] and q[-1] == 800 and len(q) == 100


def test_unknown_skip_type_or_sample_type_raises():
    S = pkg('ddpm_exp_sampler')
    with pytest.raises(NotImplementedError):
        S.timestep_sequence(1000, 10, 'linear')
    with pytest.raises(NotImplementedError):
        S.Sampler(R.toy_model, _betas(), (3, 8, 8), skip_type='cosine', device='cpu')
    with pytest.raises(NotImplementedError):
        S.Sampler(R.toy_model, _betas(), (3, 8, 8), sample_type='ddim', device='cpu')
    for kw in (dict(logit_transform=True), dict(image_mean=True)):
        with pytest.raises(NotImplementedError):
            S.Sampler(R.toy_model, _betas(), (3, 8, 8), device='cpu', **kw)


# ---------------------------------------------------------------------------------------------- (b) the reference's fp32 single steps
@pytest.mark.parametrize('name', R.step_case_names())
def test_python_loop_reproduces_the_reference_fp32_single_step(S, name):
    """The host scalars (0-d fp32 torch ops in the reference's order) and the stand-in's elementwise order give the reference's own
    fp32 result bit for bit: seq = [j, i], xs[1] and x0_preds[0], exactly as the fixture was drawn."""
    g = R.load(R.STEPS_FILE)
    i, j = [int(v) for v in g[name + ':ij']]
    scale, eta = float(g[name + ':scale']), float(g[name + ':eta'])
    x, e, z = (torch.from_numpy(g[k]) for k in ('x', 'e', 'z'))
    x, e = x * scale, e * scale
    if name.startswith('gen'):
        xs, x0s = S.generalized_steps(x, [j, i], lambda xx, t: e, _betas(), eta=eta, noise_fn=lambda k, shape: z)
    else:
        xs, x0s = S.ddpm_steps(x, [j, i], lambda xx, t: e, _betas(), noise_fn=lambda k, shape: z)
    assert xs[0] is x and len(xs) == 3 and len(x0s) == 2
    assert np.array_equal(xs[1].numpy(), g[name + ':next32']), float(np.abs(xs[1].numpy() - g[name + ':next32']).max())
    assert np.array_equal(x0s[0].numpy(), g[name + ':x0_32']), float(np.abs(x0s[0].numpy() - g[name + ':x0_32']).max())
    for got, key, err in ((xs[1], ':next64', ':e_ref32_next'), (x0s[0], ':x0_64', ':e_ref32_x0')):
        assert float(np.abs(got.double().numpy() - g[name + key]).max()) <= R.single_step_bound(g[name + err], g[name + key])
    if name.startswith('ddpm_clamp'):
        share = float((x0s[0].abs() == 1.0).double().mean())
        assert 0.1 <= float(g[name + ':clamp_share']) <= 0.9 and abs(share - float(g[name + ':clamp_share'])) < 0.01


# ---------------------------------------------------------------------------------------------- (c) chains over the toy model
@pytest.mark.parametrize('skip', ['uniform', 'quad'])
@pytest.mark.parametrize('kind,eta', R.CHAIN_KINDS)
def test_python_loops_reproduce_the_reference_chains_on_the_toy_model(S, skip, kind, eta):
    import mock_ops_sampler
    g = R.load(R.TOY_FILE)
    pre = skip + ':'
    name = pre + R.chain_name(kind, eta)
    seq = S.timestep_sequence(1000, R.CHAIN_N, skip)
    assert seq == [int(v) for v in g[pre + 'seq']]
    x_T, noise = torch.from_numpy(g[pre + 'x_T']), torch.from_numpy(g[pre + 'noise'])
    asked = []

    def noise_fn(k, shape):
        asked.append(k)
        assert tuple(shape) == tuple(x_T.shape)
        return noise[k]
    ts = []

    def model(x, t):
        ts.append(t.clone())
        return R.toy_model(x, t)
    if kind == 'generalized':
        xs, x0s = S.generalized_steps(x_T, seq, model, _betas(), eta=eta, noise_fn=noise_fn)
    else:
        xs, x0s = S.ddpm_steps(x_T, seq, model, _betas(), noise_fn=noise_fn)
    assert xs[0] is x_T and len(xs) == len(seq) + 1 and len(x0s) == len(seq)
    # the timestep reaches the model as the reference passes it: i for every image, walking seq backwards
    assert [t.tolist() for t in ts] == [[float(i)] * x_T.shape[0] for i in reversed(seq)]
    # eta = 0 draws nothing; ddpm_steps draws at every step but t = 0
    assert asked == ([] if (kind, eta) == ('generalized', 0.0) else list(range(len(seq))) if kind == 'generalized'
                     else [k for k, i in enumerate(reversed(seq)) if i != 0])
    # ... bit for bit the reference's own fp32 chain, every state and every x0 prediction
    assert np.array_equal(torch.stack(xs).numpy(), g[name + ':xs32'])
    assert np.array_equal(torch.stack(x0s).numpy(), g[name + ':x0s32'])
    # keep='last': the same final state, nothing else held, the input untouched, later steps in place
    del mock_ops_sampler.calls[:]
    keep = x_T.clone()
    f = S.generalized_steps if kind == 'generalized' else S.ddpm_steps
    kw = dict(eta=eta) if kind == 'generalized' else {}
    last, none = f(x_T, seq, R.toy_model, _betas(), keep='last', noise_fn=noise_fn, **kw)
    assert len(last) == 1 and none == [] and torch.equal(last[0], xs[-1]) and torch.equal(x_T, keep)
    assert [c[3] for c in mock_ops_sampler.calls] == [False] + [True] * (len(seq) - 1) and not any(c[2] for c in mock_ops_sampler.calls)


def test_generator_noise_and_sampler_sample_image(S):
    """Without noise_fn the noise is torch.randn(shape, generator=...) in step order; Sampler.sample_image returns the last state or
    the (xs, x0_preds) pair."""
    betas = _betas()
    smp = S.Sampler(R.toy_model, betas, R.TOY_SHAPE[1:], timesteps=10, sample_type='generalized', skip_type='quad', eta=1.0, device='cpu')
    x = torch.randn(R.TOY_SHAPE, generator=torch.Generator().manual_seed(1))
    gen = torch.Generator().manual_seed(2)
    drawn = [torch.randn(R.TOY_SHAPE, generator=gen) for _ in range(10)]
    want = S.generalized_steps(x, smp.seq, R.toy_model, betas, eta=1.0, noise_fn=lambda k, shape: drawn[k])
    xs, x0s = smp.sample_image(x, last=False, generator=torch.Generator().manual_seed(2))
    assert all(torch.equal(a, b) for a, b in zip(xs, want[0])) and all(torch.equal(a, b) for a, b in zip(x0s, want[1]))
    assert torch.equal(smp.sample_image(x, generator=torch.Generator().manual_seed(2)), want[0][-1])
    d = S.Sampler(R.toy_model, betas, R.TOY_SHAPE[1:], timesteps=10, sample_type='ddpm_noisy', device='cpu')
    want = S.ddpm_steps(x, d.seq, R.toy_model, betas, generator=torch.Generator().manual_seed(3))
    assert torch.equal(d.sample_image(x, generator=torch.Generator().manual_seed(3)), want[0][-1])


# ---------------------------------------------------------------------------------------------- the jobs' bookkeeping
class _Stub:
    """eps = 0.1 x: records every x_T (the first call of each round: t is the largest timestep)."""

    def __init__(self, t_first):
        self.t_first, self.x_T = t_first, []

    def __call__(self, x, t):
        if float(t[0]) == self.t_first:
            self.x_T.append(x.clone())
        return 0.1 * x


def test_sample_fid_file_names_rounds_seed_and_resume(S, tmp_path):
    from PIL import Image
    import mock_ops_sampler
    stub = _Stub(900.0)
    smp = S.Sampler(stub, _betas(), (3, 4, 4), timesteps=10, device='cpu')
    folder = str(tmp_path / 'fid')
    n = smp.sample_fid(folder, total_n_samples=11, batch_size=4, seed=7, rank=2, world=4)
    assert n == 8 and len(stub.x_T) == 2                                    # n_rounds = (11 - 0) // 4
    assert sorted(os.listdir(folder), key=lambda f: int(f.split('.')[0])) == ['%d.png' % i for i in range(8)]
    gen = torch.Generator().manual_seed(7 + 2)                              # seed + rank; eta = 0 draws nothing in between
    for got in stub.x_T:
        assert torch.equal(got, torch.randn((4, 3, 4, 4), generator=gen))
    # the bytes of the files are image_to_u8 of the final states
    want = torch.cat([mock_ops_sampler.image_to_u8(smp.sample_image(x)) for x in list(stub.x_T)]).numpy()
    got = np.stack([np.asarray(Image.open(os.path.join(folder, '%d.png' % i))) for i in range(8)])
    assert got.dtype == np.uint8 and np.array_equal(got, want) and want.min() != want.max()
    # continue from the existing folder: img_id = 8 files, n_rounds = (17 - 8) // 4 = 2
    stub.x_T = []
    assert smp.sample_fid(folder, total_n_samples=17, batch_size=4, seed=7, rank=0, world=1) == 8 and len(stub.x_T) == 2
    assert sorted(os.listdir(folder), key=lambda f: int(f.split('.')[0])) == ['%d.png' % i for i in range(16)]
    assert torch.equal(stub.x_T[0], torch.randn((4, 3, 4, 4), generator=torch.Generator().manual_seed(7)))
    assert smp.sample_fid(folder, total_n_samples=17, batch_size=4, seed=7, rank=0, world=1) == 0      # (17 - 16) // 4
    assert smp.sample_fid(str(tmp_path / 'dry'), total_n_samples=4, batch_size=4, seed=1, rank=0, world=1, save=False) == 4
    assert os.listdir(str(tmp_path / 'dry')) == []


def test_sample_sequence_and_interpolation_files(S, tmp_path):
    from PIL import Image
    import mock_ops_sampler
    stub = _Stub(994.0)
    smp = S.Sampler(stub, _betas(), (3, 4, 4), timesteps=7, device='cpu')                 # 8 steps
    seq_dir, int_dir = str(tmp_path / 'seq'), str(tmp_path / 'interp')
    assert smp.sample_sequence(seq_dir, generator=torch.Generator().manual_seed(4)) == 64
    assert sorted(os.listdir(seq_dir)) == sorted('%d_%d.png' % (j, i) for j in range(8) for i in range(8))
    _, x0s = smp.sample_image(stub.x_T[0], last=False)                                     # the files hold the x0 PREDICTIONS
    for i in (0, 7):
        want = mock_ops_sampler.image_to_u8(x0s[i]).numpy()
        for j in (0, 5):
            assert np.array_equal(np.asarray(Image.open(os.path.join(seq_dir, '%d_%d.png' % (j, i)))), want[j])
    stub.x_T = []
    assert smp.sample_interpolation(int_dir, generator=torch.Generator().manual_seed(5)) == 11
    assert sorted(os.listdir(int_dir), key=lambda f: int(f.split('.')[0])) == ['%d.png' % i for i in range(11)]
    assert [tuple(x.shape) for x in stub.x_T] == [(8, 3, 4, 4), (3, 3, 4, 4)]              # 11 slerp points in batches of 8
    gen = torch.Generator().manual_seed(5)
    z1, z2 = torch.randn((1, 3, 4, 4), generator=gen), torch.randn((1, 3, 4, 4), generator=gen)
    assert torch.allclose(stub.x_T[0][0:1], z1, atol=1e-5) and torch.allclose(stub.x_T[1][2:3], z2, atol=1e-5)
