"""The ldm_exp samplers' host side (diff-pruning_amd/ldm_sampler.py) without a GPU: the timestep lists and the per-step scalars
against the tables the reference wrote (tests/golden/make_golden_ldm_sampler.py), the Python loops over a CPU stand-in of the
kernel (tests/mock_ops_ldm_sampler.py) against the reference's own single steps and chains -- for equality: every operation of
the stand-in and of the toy model is a correctly rounded fp32 operation -- and the bookkeeping of sample_classes."""
import os
import types

import numpy as np
import pytest
import torch

import ldm_sampler_ref as R
from helpers import pkg


@pytest.fixture
def S(monkeypatch):
    import mock_ops_ldm_sampler as mock
    mod = pkg('ldm_sampler')
    monkeypatch.setattr(mod, 'ops', mock)
    del mock.calls[:]
    return mod


# ---------------------------------------------------------------------------------------------- (a) timestep lists, tables
@pytest.mark.parametrize('discr', R.TABLE_DISCR)
@pytest.mark.parametrize('eta', R.TABLE_ETAS)
@pytest.mark.parametrize('n_steps', R.TABLE_S)
def test_timesteps_and_tables_equal_the_reference(n_steps, eta, discr):
    """Every table entry whose flag is clean (the reference's own fp32 square roots on the generating host were the correctly
    rounded ones) equals the reference's bit for bit; a flagged entry is within one ulp; at most 5 % of a table is flagged."""
    S, g = pkg('ldm_sampler'), R.load(R.TABLES_FILE)
    key = R.table_key(n_steps, eta, discr)
    steps = S.ddim_timesteps(discr, n_steps, 1000)
    assert np.array_equal(steps, g[key + ':timesteps'])
    got = S.sampling_tables(R.alphas_cumprod32(), steps, eta)
    assert got.dtype == torch.float32 and tuple(got.shape) == (len(steps), 5)
    got, want, flag = got.numpy(), g[key + ':table'], g[key + ':flag'].astype(bool)
    assert flag.mean() <= 0.05, (key, flag.mean())
    assert np.array_equal(got[~flag], want[~flag]), (key, np.argwhere(got[~flag] != want[~flag])[:4])
    assert (R.ulp_distance(got[flag], want[flag]) <= 1).all(), key
    assert np.array_equal(got[:, 4], want[:, 4])                      # sigma takes no fp32 square root: never off
    if eta == 0:
        assert not got[:, 4].any()


def test_timestep_lists():
    S = pkg('ldm_sampler')
    assert list(S.ddim_timesteps('uniform', 20, 1000)[:3]) == [1, 51, 101] and len(S.ddim_timesteps('uniform', 250, 1000)) == 250
    assert len(S.ddim_timesteps('uniform', 7, 1000)) == 8                  # 1000 // 7 = 142: range(0, 1000, 142) has 8 entries
    q = S.ddim_timesteps('quad', 20, 1000)
    assert q[0] == 1 and q[-1] == 801 and len(q) == 20                     # int(0.8 * 1000) + the reference's 1
    with pytest.raises(NotImplementedError):
        S.ddim_timesteps('linear', 20, 1000)


# ---------------------------------------------------------------------------------------------- (b) single steps
@pytest.mark.parametrize('name', list(R.STEP_CASES))
def test_stand_in_reproduces_the_reference_fp32_single_step(S, name):
    import mock_ops_ldm_sampler as mock
    g = R.load(R.STEPS_FILE)
    nxt, x0, eg = R.run_step(mock, S, g, name)
    assert np.array_equal(nxt.numpy(), g[name + ':next_32']), float(np.abs(nxt.numpy() - g[name + ':next_32']).max())
    assert np.array_equal(x0.numpy(), g[name + ':x0_32']), float(np.abs(x0.numpy() - g[name + ':x0_32']).max())
    if eg is not None:
        assert np.array_equal(eg.numpy(), g[name + ':eg32'])
    for got, what in ((nxt, 'next'), (x0, 'x0')):
        err = float(np.abs(got.double().numpy() - g['%s:%s_64' % (name, what)]).max())
        assert err <= R.single_step_bound(g['%s:e_ref32_%s' % (name, what)], g['%s:%s_64' % (name, what)])


# ---------------------------------------------------------------------------------------------- (c) chains over the toy model
def _toy_inputs(g):
    return tuple(torch.from_numpy(g[k]) for k in ('x_T', 'cond', 'uncond'))


@pytest.mark.parametrize('name', list(R.TOY_CHAINS))
def test_chains_over_the_toy_model_equal_the_reference(S, name):
    import mock_ops_ldm_sampler as mock
    kind, discr, n_steps, eta, temp = R.TOY_CHAINS[name]
    g = R.load(R.TOY_FILE)
    x_T, cond, uncond = _toy_inputs(g)
    noise = torch.from_numpy(g[name + ':noise']) if eta != 0 else None
    smp = (S.DDIMSampler if kind == 'ddim' else S.PLMSSampler)(R.toy_model, R.Schedule())
    seen = []
    out, inter = smp.sample(n_steps, x_T.shape[0], x_T.shape[1:], conditioning=cond, eta=eta, temperature=temp, x_T=x_T,
                            log_every_t=R.LOG_EVERY, unconditional_guidance_scale=R.TOY_SCALE, unconditional_conditioning=uncond,
                            noise_fn=(lambda k, shape: noise[k]) if eta != 0 else None, ddim_discretize=discr,
                            callback=seen.append, img_callback=lambda p, i: seen.append(tuple(p.shape)))
    assert inter['x_inter'][0] is inter['pred_x0'][0] and out is inter['x_inter'][-1]
    assert np.array_equal(torch.stack(inter['x_inter']).numpy(), g[name + ':x_inter32'])
    assert np.array_equal(torch.stack(inter['pred_x0']).numpy(), g[name + ':pred_x0_32'])
    total = len(smp.ddim_timesteps)
    assert seen[0::2] == list(range(total)) and set(seen[1::2]) == {tuple(x_T.shape)}
    assert len(mock.calls) == total + (1 if kind == 'plms' else 0)          # one launch per model evaluation
    assert all(c[0] for c in mock.calls) and all(c[2] == (eta != 0) for c in mock.calls)
    if kind == 'plms':
        assert [c[1] for c in mock.calls] == [0, 4, 1, 2] + [3] * (total - 3)


def test_unguided_paths_and_noise_draws(S):
    """scale == 1 or no unconditional conditioning: one model row per image (ddim.py:170).  Noise is drawn only when sigma != 0."""
    import mock_ops_ldm_sampler as mock
    g = R.load(R.TOY_FILE)
    x_T, cond, uncond = _toy_inputs(g)
    rows = []

    def model(x, t, c):
        rows.append(x.shape[0])
        return R.toy_model(x, t, c)
    smp = S.DDIMSampler(model, R.Schedule())
    a, _ = smp.sample(4, 2, x_T.shape[1:], conditioning=cond, x_T=x_T, unconditional_guidance_scale=1.0, unconditional_conditioning=uncond)
    b, _ = smp.sample(4, 2, x_T.shape[1:], conditioning=cond, x_T=x_T, unconditional_guidance_scale=3.0)
    assert rows == [2] * 8 and torch.equal(a, b) and not any(c[0] or c[2] for c in mock.calls)
    drawn = []

    def noise_fn(k, shape):
        drawn.append(k)
        return torch.zeros(shape)
    smp.sample(4, 2, x_T.shape[1:], conditioning=cond, x_T=x_T, noise_fn=noise_fn)
    assert drawn == []
    c, _ = smp.sample(4, 2, x_T.shape[1:], conditioning=cond, x_T=x_T, eta=1.0, noise_fn=noise_fn)
    assert drawn == [0, 1, 2, 3] and not torch.equal(c, a)                # zero noise, but c_dir shrinks with sigma
    gen = torch.Generator().manual_seed(3)
    d1, _ = smp.sample(4, 2, x_T.shape[1:], conditioning=cond, eta=1.0, generator=gen, device='cpu')
    gen = torch.Generator().manual_seed(3)
    d2, _ = smp.sample(4, 2, x_T.shape[1:], conditioning=cond, eta=1.0, generator=gen, device='cpu')
    assert torch.equal(d1, d2)


def test_plms_refuses_eta_and_both_refuse_what_is_left_out(S):
    g = R.load(R.TOY_FILE)
    x_T, cond, uncond = _toy_inputs(g)
    kw = dict(conditioning=cond, x_T=x_T, unconditional_guidance_scale=3.0, unconditional_conditioning=uncond)
    with pytest.raises(ValueError):
        S.PLMSSampler(R.toy_model, R.Schedule()).sample(4, 2, x_T.shape[1:], eta=0.5, **kw)
    for cls in (S.DDIMSampler, S.PLMSSampler):
        smp = cls(R.toy_model, R.Schedule())
        for bad in (dict(mask=torch.ones_like(x_T)), dict(x0=x_T), dict(quantize_x0=True), dict(noise_dropout=0.1),
                    dict(score_corrector=object()), dict(ddim_use_original_steps=True)):
            with pytest.raises(NotImplementedError):
                smp.sample(4, 2, x_T.shape[1:], **kw, **bad)
        with pytest.raises(TypeError):
            smp.sample(4, 2, x_T.shape[1:], no_such_keyword=1, **kw)
        smp.sample(4, 2, x_T.shape[1:], mask=None, quantize_x0=False, noise_dropout=0., score_corrector=None, **kw)    # unset: fine


# ---------------------------------------------------------------------------------------------- sample_classes over stand-ins
class _Embedder:
    def __init__(self):
        self.embedding = types.SimpleNamespace(weight=torch.randn(1001, R.TOY_CTX, generator=torch.Generator().manual_seed(7)))

    def __call__(self, ids):
        return self.embedding.weight[ids][:, None, :]


class _FirstStage:
    """decode(z).sample: a bounded image with values on both sides of the clamp of image_to_u8."""

    def decode(self, z, force_not_quantize=False):
        up = z.repeat_interleave(2, 2).repeat_interleave(2, 3)
        return types.SimpleNamespace(sample=up / (up.abs() * 0.5 + 1.0))


def _read(folder):
    from PIL import Image
    return {f: np.asarray(Image.open(os.path.join(folder, f)), dtype=np.uint8) for f in sorted(os.listdir(folder))}


def test_sample_classes_files_and_ranks(S, tmp_path):
    classes, ipc, bs = [3, 7, 1000 - 1], 5, 2
    kw = dict(classes=classes, ipc=ipc, batch_size=bs, ddim_steps=4, scale=3.0, seed=11, latent_shape=R.TOY_SHAPE[1:])

    def run(folder, **more):
        return S.sample_classes(S.DDIMSampler(R.toy_model, R.Schedule()), _Embedder(), _FirstStage(), str(tmp_path / folder), **kw, **more)
    # the reference's loop (sample_for_FID.py:75-105): a running counter over rounds, classes and images
    names, img_id = [], 0
    for _ in range(ipc // bs):
        for label in classes:
            for _i in range(bs):
                names.append('%d_%d.png' % (label, img_id))
                img_id += 1
    assert run('w1', rank=0, world=1) == len(names) == 12
    one = _read(str(tmp_path / 'w1'))
    assert sorted(one) == sorted(names)
    assert all(a.shape == (16, 16, 3) for a in one.values()) and len({a.tobytes() for a in one.values()}) == len(names)
    n0, n1 = run('w2', rank=0, world=2), run('w2', rank=1, world=2)
    assert (n0, n1) == (8, 4)                                            # positions 0 and 2 / position 1, two rounds each
    two = _read(str(tmp_path / 'w2'))
    assert sorted(two) == sorted(one) and all(np.array_equal(two[f], one[f]) for f in one)
    assert run('none', rank=0, world=1, save=False) == 12 and not os.path.exists(str(tmp_path / 'none'))
    # the bytes are image_to_u8 of the decoded sample of that (round, class) generator
    import mock_ops_ldm_sampler as mock
    smp, emb = S.DDIMSampler(R.toy_model, R.Schedule()), _Embedder()
    k = 1 * len(classes) + 1                                             # round 1, class position 1
    gen = torch.Generator().manual_seed(11 + k)
    x_T = torch.randn((bs,) + R.TOY_SHAPE[1:], generator=gen)
    z, _ = smp.sample(4, bs, R.TOY_SHAPE[1:], conditioning=emb(torch.tensor([7, 7])), x_T=x_T, unconditional_guidance_scale=3.0,
                      unconditional_conditioning=emb(torch.tensor([1000, 1000])))
    want = mock.image_to_u8(_FirstStage().decode(z).sample).numpy()
    assert np.array_equal(one['7_%d.png' % (k * bs)], want[0]) and np.array_equal(one['7_%d.png' % (k * bs + 1)], want[1])
    with pytest.raises(ValueError):
        S.sample_classes(S.PLMSSampler(R.toy_model, R.Schedule()), _Embedder(), _FirstStage(), str(tmp_path / 'p'), eta=0.5, **kw)


def test_max_class_batch_keeps_every_buffer_below_2_gib(S, monkeypatch):
    syn = pkg('synthetic')
    cfg = dict(syn.LDM_CIN256_CFG, num_heads=8)          # 8 heads: the [heads, T, T] scores of the 32 x 32 level lead
    monkeypatch.setattr(S.ops, 'FUSED_ATTN', False, raising=False)
    monkeypatch.setattr(S.ops, 'attention_fused_ok', lambda T, d, dv: False, raising=False)
    per_row = S.forward_row_bytes(cfg, (3, 64, 64))
    assert per_row == 4 * 8 * 1024 * 1024
    plain = S.forward_row_bytes(syn.LDM_CIN256_CFG, (3, 64, 64))
    assert plain == 4 * 8 * 384 * 1024                    # cin256-v2 itself: the GEGLU projection of the 32 x 32 level

    class Model:
        config = cfg

        def forward_cfg_pair(self):
            pass
    m = S.max_class_batch(Model(), (3, 64, 64))
    assert 2 * m * per_row < (1 << 31) <= 2 * (m + 1) * per_row and m < 50        # batch 50 of the FID job is split
    assert S.max_class_batch(R.toy_model, (3, 8, 8)) is None
