"""LDM finetune step (ldm_exp/main.py -t --load_pruned_model; ddpm.py:870-879, 1022-1056, 1372-1381; ema.py), CPU part: the fp64
restatement against the reference's own three training steps (tests/golden/ldm_finetune.{npz,json}), the step's control flow on
mocked kernels against the same fixture, the API pieces (learning rate, LitEma decay, checkpoint keys, id check, header <-> ctypes
table) and the data-parallel step's shard invariance (world_size 2, gloo, mocked kernels)."""
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import golden_common as gc
import ldm_finetune_ref as R
from helpers import load_json, load_npz, pkg

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope='module')
def fixture_runs():
    """(fx, gold, reference view, fp64 restatement view, initial view) -- the fp64 run takes a few seconds, shared by the tests."""
    fx, gold = load_json('ldm_finetune.json'), load_npz('ldm_finetune.npz')
    cfg = fx['config']
    assert cfg == R.FIXTURE_CFG
    x, ids, ts, noises = R.fixture_inputs(fx, cfg)
    P, E = R.initial_weights(cfg, torch.float64)
    run = R.finetune(P, E, cfg, x, ids, ts, noises, lr=fx['lr'], ema_decay=fx['ema_decay'])
    ref64 = R.run_view(run['losses'], run['grads1'], run['dE1'], run['params'], run['emb'], run['ema'])
    return fx, gold, R.fixture_view(fx, gold), ref64, R.initial_view(cfg), run


def test_restatement_reproduces_reference_steps(fixture_runs):
    """fp64 restatement vs the reference's fp32 steps.  Measured: losses 8e-8 .. 2e-7 relative, step-1 gradients <= 5.8e-6 per-tensor
    relative L2, global update L2 1.0e-4, 64 exactly-zero gradients in both; decay-only values within 3 ulp."""
    fx, gold, ref32, ref64, init, run = fixture_runs
    e = R.errors(ref32, ref64, init)
    print('e_ref32:', {k: v for k, v in e.items() if k != 'zero'})
    assert e['loss'] <= 1e-6
    assert e['grad'] <= 1e-5, (e['grad'], e['grad_name'])
    zero64 = sorted(n for n, g in ref64['grad1'].items() if not np.any(g))
    assert e['zero'] == zero64 == sorted(fx['grad1_zero']) and len(zero64) == 64
    assert all(n.endswith(('attn2.to_q.weight', 'attn2.to_k.weight', 'norm2.weight', 'norm2.bias')) for n in zero64)
    assert e['update'] <= 2e-4 and e['ema_update'] <= 2e-4
    assert e['decay_ulp'] <= 3 and e['ema_decay_ulp'] <= 3
    assert fx['ema_buffers'] == 690 and fx['ema_num_updates'] == 3
    assert fx['ema_decay_after'] == float(np.float32(0.9999))          # the buffer keeps the cap; the warm-up value is per update
    # full tensors: gradients of the named tensors and the touched embedding rows
    for n in fx['full']:
        g64, g32 = run['grads1'][n], torch.from_numpy(gold['grad1:' + n]).double()
        if float(g64.abs().max()) == 0.0:
            assert float(g32.abs().max()) == 0.0, n
        else:
            assert R.rel_l2(g32, g64) <= 1e-5, n
    rows = fx['grad1_emb_row_ids']
    assert R.rel_l2(gold['grad1_emb_rows'], run['dE1'][rows]) <= 1e-5
    untouched = [i for i in range(R.N_CLASSES) if i not in rows]
    assert float(run['dE1'][untouched].abs().max()) == 0.0


def test_decay_only_tensors_are_p_times_one_minus_lr_wd_cubed(fixture_runs):
    """A tensor whose gradient is exactly zero (an attn2.to_q.weight) and embedding row 7 end at p (1 - lr wd)^3, one rounding per
    step: the reference's fp32 values are within 3 ulp of p of it (measured 6.5e-8 absolute on row 7)."""
    fx, gold, *_ = fixture_runs
    cfg = fx['config']
    f = np.float32(1.0 - fx['lr'] * R.WD)
    name = 'input_blocks.4.1.transformer_blocks.0.attn2.to_q.weight'
    p0 = gc.det_param(name, gold['final:' + name].shape, R.UNET_SEED)
    e0 = gc.det_param('embedding.weight', (R.N_CLASSES, cfg['context_dim']), R.EMB_SEED)[7]
    row7 = gold['final_emb_rows'][fx['emb_rows'].index(7)]
    for p, got in ((p0, gold['final:' + name]), (e0, row7)):
        exact = p.astype(np.float64) * (1.0 - fx['lr'] * R.WD) ** 3
        assert float((np.abs(got - exact) / R.ulp32(p)).max()) <= 3
        stepwise = ((p * f) * f) * f                                   # fp32, one rounding per step
        assert float((np.abs(got.astype(np.float64) - stepwise) / R.ulp32(p)).max()) <= 3
    print('row 7: max |ref32 - exact| = %.2e' % float(np.abs(row7 - e0.astype(np.float64) * (1.0 - fx['lr'] * R.WD) ** 3).max()))


def _mock(monkeypatch):
    import _dist_worker_ldm_finetune as W
    import mock_ops_ldm
    ldm, ldm_train = pkg('ldm'), pkg('ldm_train')
    for sub in ('engine', 'ldm', 'ldm_sweep', 'ldm_train', 'pruning'):
        monkeypatch.setattr(pkg(sub), 'ops', mock_ops_ldm)

    def cpu_engine(self):
        if self._engine is None:
            self._engine = ldm.LdmEngine(self.config)
        self._engine.packs.rebind()
        self._engine.bind({n: p.detach() for n, p in self.named_parameters()}, None)
        return self._engine
    monkeypatch.setattr(ldm.UNetModel, 'engine', cpu_engine)
    monkeypatch.setattr(ldm_train, '_require_hip_device', lambda dev: None)
    return W


def _build(cfg, use_ema, **kw):
    ldm, ldm_sweep, ldm_train = pkg('ldm'), pkg('ldm_sweep'), pkg('ldm_train')
    model = ldm.UNetModel(**cfg)
    gc.det_init_(model, R.UNET_SEED)
    embedder = ldm_sweep.ClassEmbedder(cfg['context_dim'], R.N_CLASSES)
    with torch.no_grad():
        embedder.embedding.weight.copy_(torch.from_numpy(gc.det_param('embedding.weight', (R.N_CLASSES, cfg['context_dim']), R.EMB_SEED)))
    return model, embedder, ldm_train.LdmFinetuneEngine(model, embedder, lr=R.LR, use_ema=use_ema, **kw)


@pytest.mark.parametrize('use_ema', [True, False])
def test_step_control_flow_on_mocked_kernels_reproduces_reference_steps(fixture_runs, monkeypatch, use_ema):
    """LdmFinetuneEngine with every kernel replaced by its fp32 torch stand-in: the K = 3 reference steps by the rule the GPU test
    applies, max(4 e_ref32, floor) against the fp64 restatement -- the step's plumbing (per-image timesteps, context gradient into
    the embedding rows with a repeated id, weight decay on zero-gradient tensors, LitEma warm-up) is then right off the GPU."""
    fx, gold, ref32, ref64, init, _ = fixture_runs
    _mock(monkeypatch)
    cfg = fx['config']
    x, ids, ts, noises = R.fixture_inputs(fx, cfg)
    model, embedder, ft = _build(cfg, use_ema)
    losses, g1 = [], None
    for k in range(fx['steps']):
        losses.append(float(ft.step(x, ids, noise=noises[k], timesteps=ts[k])))
        if k == 0:
            g1 = {n: p.grad.clone() for n, p in model.named_parameters()}
            dE1 = embedder.embedding.weight.grad.clone()
    view = R.run_view(losses, g1, dE1, dict(model.named_parameters()), embedder.embedding.weight, ft.ema_state() if use_ema else None)
    zero64 = sorted(n for n, g in ref64['grad1'].items() if not np.any(g))
    R.check(R.errors(view, ref64, init), R.errors(ref32, ref64, init), zero64, what='mocked ema=%d' % use_ema)
    assert ft.num_updates == (fx['steps'] if use_ema else 0) and ft.step_count == fx['steps']
    if not use_ema:
        with pytest.raises(RuntimeError):
            ft.ema_state()


def test_header_and_ctypes_table_list_the_new_symbols():
    lib = pkg('_lib')
    with open(os.path.join(os.path.dirname(HERE), 'include', 'dp_hip.h')) as f:
        declared = set(re.findall(r'\bint\s+(dp_\w+)\s*\(', f.read()))
    for sym in ('dp_adamw_ema', 'dp_embedding_bwd'):
        assert sym in declared and sym in lib.SIGNATURES, sym
    assert len(lib.SIGNATURES['dp_adamw_ema']) == 16 and len(lib.SIGNATURES['dp_embedding_bwd']) == 6


def test_learning_rate_and_lit_ema_decay_sequence():
    ldm_train = pkg('ldm_train')
    assert ldm_train.learning_rate(2e-6, 16, 4) == 1.28e-4                       # run.sh: --scale_lr, 4 GPUs, batch 16
    assert ldm_train.learning_rate(2e-6, 16, 4, accumulate_grad_batches=2) == 2.56e-4
    seq = [ldm_train.lit_ema_decay(0.9999, n) for n in (1, 2, 3, 4)]
    assert np.allclose(seq, [2 / 11, 3 / 12, 4 / 13, 5 / 14], rtol=1e-7)
    assert seq == R.lit_ema_decays(0.9999, 4)
    assert ldm_train.lit_ema_decay(0.9999, 10 ** 6) == float(np.float32(0.9999))     # capped at ema_decay
    assert ldm_train.lit_ema_decay(0.5, 100) == 0.5


def test_class_id_range_check_raises(monkeypatch):
    ops = pkg('ops')
    assert ops.check_class_ids(torch.tensor([0, 1000]), 1001).dtype == torch.int64
    for bad in ([-1, 3], [3, 1001], [[1, 2]]):
        with pytest.raises(ValueError):
            ops.check_class_ids(torch.tensor(bad), 1001)
    with pytest.raises(ValueError):
        ops.check_class_ids(torch.tensor([0.5]), 1001)
    _mock(monkeypatch)
    model, embedder, ft = _build(gc.LDM_TINY_CFG, False)
    before = ft.flat_p.clone()
    x = torch.from_numpy(gc.det_noise((2, 3, 16, 16), 1))
    for bad in ([3, 1001], [-1, 0], [1, 2, 3]):
        with pytest.raises(ValueError):
            ft.step(x, torch.tensor(bad))
    assert torch.equal(before, ft.flat_p) and ft.step_count == 0                 # refused before anything ran
    with pytest.raises(TypeError):
        pkg('ldm_train').LdmFinetuneEngine(torch.nn.Conv2d(3, 3, 3), embedder)


def test_checkpoint_keys_round_trip_and_load_into_a_pruned_model(monkeypatch, tmp_path):
    """save_ldm_finetuned writes the reference's LatentDiffusion keys (model.diffusion_model.*, cond_stage_model.embedding.weight,
    model_ema.decay / num_updates / diffusion_model<name without dots>); load_ldm_finetuned reads them back into a pruned model,
    ignoring foreign keys as strict=False does, and refuses a known key of another shape."""
    ckpt, ldm, pruning = pkg('checkpoint'), pkg('ldm'), pkg('pruning')
    _mock(monkeypatch)
    cfg = gc.LDM_TINY_CFG
    model, embedder, ft = _build(cfg, True)
    x = torch.from_numpy(gc.det_noise((2, 3, 16, 16), 1))
    ft.step(x, torch.tensor([3, 1000]), noise=torch.from_numpy(gc.det_noise((2, 3, 16, 16), 2)), timesteps=torch.tensor([5, 700]))
    sd = ckpt.ldm_finetuned_state_dict(model, embedder, ft)
    n_unet = len(list(model.named_parameters()))
    assert 'cond_stage_model.embedding.weight' in sd and 'model.diffusion_model.input_blocks.0.0.weight' in sd
    assert 'model_ema.diffusion_modelinput_blocks41transformer_blocks0attn2to_vweight' in sd
    assert ckpt.lit_ema_key('out.2.bias') == 'model_ema.diffusion_modelout2bias'
    assert float(sd['model_ema.decay']) == float(np.float32(0.9999)) and int(sd['model_ema.num_updates']) == 1
    assert len(sd) == 2 * n_unet + 3 and not any('.' in k[len('model_ema.'):] for k in sd if k.startswith('model_ema.'))
    path = str(tmp_path / 'last.ckpt')
    ckpt.save_ldm_finetuned(path, model, embedder, ft)
    blob = torch.load(path, weights_only=True)
    blob['state_dict'].update({'first_stage_model.quant_conv.weight': torch.zeros(3, 3, 1, 1), 'betas': torch.zeros(1000),
                               'model_ema.something_else': torch.zeros(1)})
    torch.save(blob, path)
    m2, e2, _ = _build(cfg, False)
    with torch.no_grad():
        for p in list(m2.parameters()) + list(e2.parameters()):
            p.zero_()
    res = ckpt.load_ldm_finetuned(path, m2, e2)
    assert res['missing'] == [] and res['ema']['num_updates'] == 1
    assert all(torch.equal(a, b) for a, b in zip(m2.parameters(), model.parameters()))
    assert torch.equal(e2.embedding.weight, embedder.embedding.weight)
    shadow = ft.ema_state()
    assert all(torch.equal(res['ema']['shadow'][n], shadow[n]) for n in shadow)
    # a pruned model round-trips at its own shapes, and refuses the un-pruned file
    pm = ldm.UNetModel(**cfg)
    gc.det_init_(pm, 9)
    R.prune_ldm(pm)
    assert sum(p.numel() for p in pm.parameters()) < sum(p.numel() for p in model.parameters())
    ckpt.save_ldm_finetuned(path, pm, embedder)
    blob = torch.load(path, weights_only=True)
    assert not any(k.startswith('model_ema.') for k in blob['state_dict'])
    blob['state_dict']['first_stage_model.decoder.conv_in.weight'] = torch.zeros(2)
    torch.save(blob, path)
    pm2 = ldm.UNetModel(**cfg)
    gc.det_init_(pm2, 9)
    R.prune_ldm(pm2)                                   # the same masks, then other weights
    with torch.no_grad():
        for p in pm2.parameters():
            p.add_(1.0)
    res = ckpt.load_ldm_finetuned(path, pm2, e2)
    assert res['missing'] == [] and res['ema'] is None
    assert all(torch.equal(a, b) for a, b in zip(pm2.parameters(), pm.parameters()))
    with pytest.raises(ValueError):
        ckpt.load_ldm_finetuned(path, model, embedder)


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run(world, outdir):
    port = str(_free_port())
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, '_dist_worker_ldm_finetune.py'), str(r), str(world), port, outdir])
             for r in range(world)]
    for p in procs:
        assert p.wait(timeout=600) == 0


def test_two_rank_step_equals_single_process(tmp_path):
    """world_size 2 (gloo, mocked kernels): two ranks with half the batch each -- class id 3 on both -- take the step one rank takes
    with the whole batch: UNet and embedder gradients are summed over the ranks before the update, loss and gradient of a rank are
    its share of the global mean."""
    out = str(tmp_path)
    _run(1, out)
    _run(2, out)
    one = torch.load(os.path.join(out, 'ldmft_r0_w1.pt'))
    r0 = torch.load(os.path.join(out, 'ldmft_r0_w2.pt'))
    r1 = torch.load(os.path.join(out, 'ldmft_r1_w2.pt'))
    for a, b, c in zip(one['losses'], r0['losses'], r1['losses']):
        assert abs(a - b) <= 1e-5 * abs(a) and b == c
    assert torch.equal(r0['emb'], r1['emb'])
    keys = list(one['params'])
    init = {n: torch.from_numpy(gc.det_param(n, tuple(one['params'][n].shape), 9)) for n in keys}
    for n in keys:
        assert torch.equal(r0['params'][n], r1['params'][n]) and torch.equal(r0['ema'][n], r1['ema'][n]), n
    # same step: global relative L2 of the update (two steps of lr 1.28e-4), not element-wise (the issue's second trap)
    assert R.global_update_err(r0['params'], init, one['params'], keys) <= 2e-3
    assert R.global_update_err(r0['ema'], init, one['ema'], keys) <= 2e-3
    e0 = torch.from_numpy(gc.det_param('embedding.weight', tuple(one['emb'].shape), 61))
    assert R.global_update_err({'e': r0['emb']}, {'e': e0}, {'e': one['emb']}, ['e']) <= 2e-3
    assert not torch.equal(one['emb'][3], e0[3]) and not torch.equal(one['emb'][7], e0[7])       # touched row moves, every row decays
