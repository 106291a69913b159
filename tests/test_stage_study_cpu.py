"""The stage study on the host (`-m "not gpu"`): the control flow of sweep.taylor_sweep(stages=...) through a CPU step_fn, the study
(diff-pruning_amd/stage_study.py) over the CPU stand-ins of tests/mock_ops_stage_study.py against tests/golden/stage_study.json / .npz,
which make_golden_stage_study.py recorded from the reference's own stage loop (ddpm_exp/prune_ssim.py:252-272 with the reference's
model, loss and vendored pruner), the launch-site table of csrc/stage.hip, and a world_size-2 gloo run of the staged sweep."""
import os
import re
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import golden_common as gc
from helpers import load_json, load_npz, pkg
from test_cpu import _cpu_engine, _cpu_model, _cpu_step_init

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
FX = load_json('stage_study.json')


@pytest.fixture()
def mocked(monkeypatch):
    import mock_ops_stage_study as mock
    for sub in ('engine', 'sweep', 'train', 'diffusion', 'pruning', 'stage_study', 'ddpm_exp_sampler'):
        monkeypatch.setattr(pkg(sub), 'ops', mock)
    monkeypatch.setattr(pkg('unet').UNet2DModel, 'engine', _cpu_engine)
    monkeypatch.setattr(pkg('sweep').HipSweepStep, '__init__', _cpu_step_init)
    del mock.calls[:]
    return mock


# ------------------------------------------------------------------------------------------------ the fixture and the launch-site table
def test_fixture_conditions():
    """What the issue asks of the committed fixture, from the stored numbers: the stages, 20 losses, stage 0 unpruned, and every group
    that picks between two scores does so with gap >= 100 x the fp32-against-fp64 error of the reference's own scores."""
    assert FX['stages'] == [0, 1, 5, 10, 15, 20] and FX['timesteps'] == 20 == len(FX['losses']) and FX['ratio'] == 0.3
    assert FX['batch'] == 4 and FX['n_chain'] == 4 and len(FX['chain_seq']) == 5
    assert FX['per_stage']['0']['groups'] == []
    for s in FX['stages'][1:]:
        st = FX['per_stage'][str(s)]
        assert st['groups'] and st['params_after'] < FX['per_stage']['0']['params_after']
        for root, chg, ranges, gap, err in st['groups']:
            assert gap is None or gap >= 100 * err, (s, root, gap, err)
            assert (gap is None) == (not ranges), (s, root)
        assert any(g[3] is not None for g in st['groups']), s
    arr = load_npz('stage_study.npz')
    for name in ('stage_study.json', 'stage_study.npz'):
        assert os.path.getsize(os.path.join(HERE, 'golden', name)) <= 1 << 20
    assert arr['x_T'].shape == (4, 3, 16, 16) and arr['20/bytes'].dtype == np.uint8 and arr['20/bytes'].shape == (4, 16, 16, 3)


def test_every_launch_site_of_stage_hip_is_in_its_branch_table():
    """csrc/stage.hip launches through ST_LAUNCH, a macro of its own with the body of the library's launch macro, and its sites are
    tabled in tests/test_stage_study_gpu.py (the discipline of tests/test_prune_global_cpu.py): a new site changes the count, a new
    instantiation is in no table, an entry without a case fails -- before a GPU is needed.  The file stays out of the older tables'
    census, which counts the library macro's call text per file; it is in both build lists and declared with its binding."""
    import test_stage_study_gpu as T
    csrc = os.path.join(ROOT, 'diff-pruning_amd', 'csrc')
    assert list(T.LAUNCH_SITES) == ['stage.hip']
    src = open(os.path.join(csrc, 'stage.hip')).read()
    body = src.replace('#define ST_LAUNCH(', '')
    sites = re.findall(r'\bST_LAUNCH\((\(fold_sum_kernel<\d, (?:true|false)>\))', body)
    assert len(sites) == T.LAUNCH_SITES['stage.hip'] == body.count('ST_LAUNCH('), sites
    assert 'DP_' + 'LAUNCH(' not in src
    assert re.search(r'#define ST_LAUNCH\(k, \.\.\.\).*dp_launch_names\[dp_launches\+\+ & \(DP_LAUNCH_RING - 1\)\] = #k;.*'
                     r'hipLaunchKernelGGL\(k, __VA_ARGS__\)', src)
    assert sorted(sites) == sorted(T.BRANCHES) and len(set(T.BRANCHES)) == len(T.BRANCHES)
    assert all(e in T.CASES for e in T.BRANCHES), sorted(set(T.BRANCHES) - set(T.CASES))
    using = {f for f in os.listdir(csrc) if 'ST_LAUNCH(' in open(os.path.join(csrc, f)).read()}
    assert using == {'stage.hip'}
    assert 'csrc/stage.hip' in open(os.path.join(ROOT, 'build.sh')).read()
    assert "'csrc/stage.hip'" in open(os.path.join(ROOT, '__graft_entry__.py')).read()
    L = pkg('_lib')
    assert len(L.SIGNATURES['dp_fold_sum']) == 5
    assert 'int dp_fold_sum(float* out, const float* const* srcs, int k, long long n, void* stream);' in \
        open(os.path.join(ROOT, 'include', 'dp_hip.h')).read()


def test_mock_fold_sum_order_and_refusals(mocked):
    a = torch.tensor([1e8, 1.0, -0.0], dtype=torch.float32)
    b = torch.tensor([-1e8, 1e-8, -0.0], dtype=torch.float32)
    c = torch.tensor([1.0, 1e-8, 0.0], dtype=torch.float32)
    out = torch.empty(3)
    mocked.fold_sum(out, [a, b, c])
    assert torch.equal(out, (a + b) + c) and out[0] == 1.0 and not torch.equal(out, a + (b + c))
    with pytest.raises(ValueError):
        mocked.fold_sum(a, [a, b])
    with pytest.raises(ValueError):
        mocked.fold_sum(out, [a] * 5)


# ------------------------------------------------------------------------------------------------ taylor_sweep(stages=...) through a step_fn
class CpuStep:
    """A step_fn without a snapshot() method: timestep k adds a seeded, k-dependent update to `flat` (as a sweep accumulates) and
    returns a loss; `log` keeps what ran."""

    def __init__(self, flat):
        self.flat, self.log = flat, []

    def __call__(self, k):
        g = torch.Generator().manual_seed(100 + k)
        self.flat += torch.randn(self.flat.numel(), generator=g) * (1.0 + k)
        self.log.append(k)
        return torch.tensor([float(k) + 0.5])


def _step_sweep(num_steps, stages=None, **kw):
    sweep = pkg('sweep')
    flat = torch.zeros(257)
    clean = torch.zeros(2, 3, 4, 4)
    step = CpuStep(flat)
    res = sweep.taylor_sweep(None, None, clean, clean, num_steps=num_steps, step_fn=step, flat_grads=flat, stages=stages, **kw)
    return res, flat, step


def test_staged_sweep_through_a_cpu_step_fn():
    stages = [0, 1, 3, 4, 7, 12]
    res, flat, step = _step_sweep(12, stages)
    plain, flat_p, _ = _step_sweep(12)
    assert 'stage_grads' not in plain and list(res['stage_grads']) == stages
    assert res['losses'] == plain['losses'] == [k + 0.5 for k in range(12)] and res['steps'] == 12 and step.log == list(range(12))
    assert torch.equal(flat, flat_p)
    for s in stages:
        _, fresh, _ = _step_sweep(s)
        snap = res['stage_grads'][s]
        assert torch.equal(snap.view(torch.int32), fresh.view(torch.int32)), s
        assert snap.data_ptr() != flat.data_ptr()
    assert torch.equal(res['stage_grads'][12], flat) and not res['stage_grads'][0].any()
    # stages that end before num_steps; a single stage; none
    res2, flat2, _ = _step_sweep(12, [5])
    assert torch.equal(res2['stage_grads'][5], _step_sweep(5)[1]) and torch.equal(flat2, flat_p)
    assert _step_sweep(3, [])[0]['stage_grads'] == {}


@pytest.mark.parametrize('stages', [[3, 1], [1, 1], [13], [-1, 2], [0, 5, 5]])
def test_staged_sweep_refuses_bad_stages(stages):
    with pytest.raises(ValueError):
        _step_sweep(12, stages)


def test_staged_sweep_refuses_a_threshold_and_a_step_it_cannot_snapshot():
    with pytest.raises(ValueError):
        _step_sweep(12, [2], thr=0.05)
    sweep = pkg('sweep')
    clean = torch.zeros(2, 3, 4, 4)
    with pytest.raises(ValueError):
        sweep.taylor_sweep(None, None, clean, clean, num_steps=2, step_fn=lambda k: torch.zeros(1), stages=[1])


def test_snapshot_of_the_mocked_sweep_step(mocked):
    """HipSweepStep.snapshot over the CPU stand-ins: the flat buffer in one fold, view by view when the .grad tensors do not tile one
    buffer, bit-equal to a fresh sweep either way, and nothing of the step moves."""
    sweep, diffusion = pkg('sweep'), pkg('diffusion')
    clean = torch.from_numpy(gc.det_clean((2, 3, 16, 16), 1))
    noise = torch.from_numpy(gc.det_noise((2, 3, 16, 16), 2))

    def run(num_steps, stages=None):
        model = _cpu_model(gc.TINY_CFG, 5)
        res = sweep.taylor_sweep(model, diffusion.DDPMScheduler(), clean, noise, num_steps=num_steps, stages=stages)
        return res, torch.cat([p.grad.reshape(-1) for p in model.parameters()])

    res, final = run(3, [0, 2, 3])
    assert mocked.calls == [(1, final.numel())] * 3                              # one fold over the whole buffer per stage
    assert torch.equal(res['stage_grads'][3], final) and not res['stage_grads'][0].any()
    assert torch.equal(res['stage_grads'][2], run(2)[1])
    assert torch.equal(final, run(3)[1])
    # .grad tensors of their own: no flat buffer behind them, one fold per tensor, laid out in named_parameters() order
    model = _cpu_model(gc.TINY_CFG, 5)
    gen = torch.Generator().manual_seed(3)
    for p in model.parameters():
        p.grad = torch.randn(p.shape, generator=gen)
    step = sweep.HipSweepStep(model, diffusion.DDPMScheduler(), clean, noise, clean.numel())
    assert step._flat_of_grads() is None
    del mocked.calls[:]
    snap = step.snapshot()
    assert mocked.calls == [(1, p.numel()) for p in model.parameters()]
    assert torch.equal(snap, torch.cat([p.grad.reshape(-1) for p in model.parameters()]))
    assert step._tp_count == 0 and step._tp is None and step._half is None


# ------------------------------------------------------------------------------------------------ the study on the fixture
def exp_model(device='cpu'):
    ckpt, unet = pkg('checkpoint'), pkg('unet')
    c = FX['cfg']
    shapes = load_json('ddpm_original.json')['shapes']
    cfg = ckpt.unet2d_config_from_ddpm_original(c['ch'], c['ch_mult'], c['num_res_blocks'], c['attn_resolutions'], c['image_size'])
    orig = {n: torch.from_numpy(gc.det_param(n, tuple(s), FX['model_seed'])) for n, s in shapes.items()}
    model = unet.UNet2DModel(**cfg)
    model.load_state_dict(ckpt.convert_ddpm_original(orig))
    return model.to(device).eval(), ckpt.ddpm_original_key_map(orig.keys())


def expand(ranges):
    return [i for a, b in ranges for i in range(a, b)]


def group_key(root):
    """An attention block's q, k, v outputs and to_out inputs are ONE group in both trees (they meet in the attention product); the
    reference's tracer names it after `k`, the product's after `to_v`: the group is keyed by the block."""
    return re.sub(r'\.to_[qkv]$', '.to_qkv', root)


def reference_masks(stage, kmap):
    """{group key: pruned indices} of the groups of `stage` that lose channels, under the product's parameter names."""
    return {group_key(kmap[root + '.weight'][:-len('.weight')]): expand(r)
            for root, _, r, _, _ in FX['per_stage'][str(stage)]['groups'] if r}


def study_masks(per_stage):
    return {group_key(root): idxs for root, idxs in per_stage['pruned_idxs'].items() if idxs}


def _cpu_metrics(monkeypatch):
    """CPU stand-ins of the study's metric kernels: the oracle's SSIM, torch's MSE, ToTensor as a division, PIL for the PNGs."""
    from oracle import metrics_ref
    S, metrics = pkg('stage_study'), pkg('metrics')
    monkeypatch.setattr(S, '_to_unit', lambda u8, device: torch.as_tensor(u8).permute(0, 3, 1, 2).float() / 255)
    monkeypatch.setattr(metrics, 'ssim', lambda x, y, data_range=1.0: torch.as_tensor(metrics_ref.ssim(x, y, data_range)).reshape(-1).float())
    monkeypatch.setattr(metrics, 'mse_per_image', lambda x, y: (x - y).square().mean(dim=(1, 2, 3)))

    def image_batches(files, batch_size, device, res=None):
        from PIL import Image
        yield torch.from_numpy(np.stack([np.asarray(Image.open(f).convert('RGB'), dtype=np.uint8) for f in files])).permute(0, 3, 1, 2).float() / 255
    monkeypatch.setattr(metrics, '_image_batches', image_batches)


@pytest.fixture(scope='module')
def study(tmp_path_factory):
    """stage_study.run once over the mocked kernels on the fixture's model and inputs (shared, read-only)."""
    mp = pytest.MonkeyPatch()
    try:
        import mock_ops_stage_study as mock
        for sub in ('engine', 'sweep', 'train', 'diffusion', 'pruning', 'stage_study', 'ddpm_exp_sampler'):
            mp.setattr(pkg(sub), 'ops', mock)
        mp.setattr(pkg('unet').UNet2DModel, 'engine', _cpu_engine)
        mp.setattr(pkg('sweep').HipSweepStep, '__init__', _cpu_step_init)
        _cpu_metrics(mp)
        S, diffusion = pkg('stage_study'), pkg('diffusion')
        model, kmap = exp_model()
        before = {n: p.detach().clone() for n, p in model.named_parameters()}
        H, B = FX['cfg']['image_size'], FX['batch']
        clean = torch.from_numpy(gc.det_clean((B, 3, H, H), FX['clean_seed']))
        noise = torch.from_numpy(gc.det_noise((B, 3, H, H), FX['noise_seed']))
        x_T = torch.from_numpy(load_npz('stage_study.npz')['x_T'])
        out_dir = str(tmp_path_factory.mktemp('stage_study'))
        res = S.run(model, diffusion.DDPMScheduler(), clean, noise, x_T, FX['stages'], pruning_ratio=FX['ratio'], loss_kind='sum',
                    sampler_args=dict(timesteps=len(FX['chain_seq']), skip_type='uniform', eta=0.0, device='cpu'),
                    out_dir=out_dir, n_ssim=4)
        curve = S.ssim_curve(out_dir, FX['stages'], base=0, n_samples=4, device='cpu')
        yield dict(res=res, model=model, kmap=kmap, before=before, out_dir=out_dir, curve=curve)
    finally:
        mp.undo()


def test_study_masks_and_shapes_equal_the_references(study):
    res, kmap = study['res'], study['kmap']
    assert res['stages'] == FX['stages'] and [p['stage'] for p in res['per_stage']] == FX['stages']
    base = res['per_stage'][0]
    assert base['pruned_idxs'] == {} and base['params'] == FX['per_stage']['0']['params_after'] and abs(base['ssim'] - 1.0) < 1e-6 and base['mse'] == 0.0
    for p in res['per_stage'][1:]:
        st = FX['per_stage'][str(p['stage'])]
        mine = study_masks(p)
        assert len(mine) == sum(1 for i in p['pruned_idxs'].values() if i) and mine == reference_masks(p['stage'], kmap), p['stage']
        assert p['params'] == st['params_after'] and 0 < p['macs'] < base['macs']
        assert len(p['ssim_per_image']) == 4 and p['ssim'] == sum(p['ssim_per_image']) / 4 and p['ssim'] < 1.0 and p['mse'] > 0.0


def test_study_leaves_the_callers_model_alone(study):
    model = study['model']
    for n, p in model.named_parameters():
        assert torch.equal(p, study['before'][n]), n
        assert p.grad is not None and p.grad.shape == p.shape
    assert FX['per_stage']['0']['params_after'] == sum(p.numel() for p in model.parameters())


def test_study_losses_relative_loss_and_threshold_stage(study):
    S, res = pkg('stage_study'), study['res']
    assert len(res['losses']) == 20
    assert max(abs(a - b) / b for a, b in zip(res['losses'], FX['losses'])) < 2e-5       # tests/test_e2e_gpu.py's bound for this model's losses
    top = max(res['losses'])
    assert res['relative_loss'] == [l / top for l in res['losses']] and max(res['relative_loss']) == 1.0
    # steps_for_threshold on the STORED losses: the first k whose loss is below thr x the running maximum, compared in fp32
    losses = FX['losses']
    for thr in (0.999, 0.99, 0.9, 0.5, 0.05):
        want, top = None, 0.0
        for k, l in enumerate(losses):
            top = max(top, l)
            if np.float32(l) < np.float32(top) * np.float32(thr):
                want = k
                break
        assert S.steps_for_threshold(losses, thr) == want, thr
    assert S.steps_for_threshold(losses, 1e-9) is None and S.steps_for_threshold([1.0, 2.0, 1.0], 0.75) == 2
    assert S.steps_for_threshold(losses, 0.999) is not None


def test_ssim_curve_over_the_written_folders_equals_the_studys_values(study):
    res = study['res']
    for s in FX['stages']:
        assert sorted(os.listdir(os.path.join(study['out_dir'], str(s)))) == sorted('%d.png' % i for i in range(4))
    assert study['curve'] == [p['ssim'] for p in res['per_stage']]


def test_prune_at_stage_checks_the_layout(mocked):
    S = pkg('stage_study')
    model = _cpu_model(gc.TINY_CFG, 5)
    with pytest.raises(ValueError):
        S.prune_at_stage(model, torch.zeros(7), 0.3)
    with pytest.raises(ValueError):
        S.run(model, None, None, None, None, [5, 10])                # stage 0 is the base of every comparison


def test_attention_scale_switch_is_carried(mocked, tmp_path):
    """UNet2DModel.attention_scale_from_width (the original-DDPM model's run-time attention scale): off by default, set by
    train.load_teacher for an original-DDPM state dict, copied by prune_at_stage, written and read by save_pruned / load_pruned (and
    absent from the file of a model that does not have it), handed to the further pipelines' engines by sweep.Pipeline.another; the
    engine then scales by the q width of the (pruned) projection."""
    S, sweep, train, ckpt, engine = pkg('stage_study'), pkg('sweep'), pkg('train'), pkg('checkpoint'), pkg('engine')
    model, _ = exp_model()
    assert model.attention_scale_from_width is False and engine.UNetEngine(model.config).scale_from_q_width is False
    c = FX['cfg']
    orig = ckpt.convert_to_ddpm_original(model.state_dict())
    loaded = train.load_teacher(orig, 'cpu', ch=c['ch'], ch_mult=c['ch_mult'], num_res_blocks=c['num_res_blocks'],
                                attn_resolutions=c['attn_resolutions'], image_size=c['image_size'])
    assert loaded.attention_scale_from_width is True and train.load_teacher(model, 'cpu').attention_scale_from_width is False
    flat = torch.randn(sum(p.numel() for p in model.parameters()), generator=torch.Generator().manual_seed(1))
    for flag in (False, True):
        model.attention_scale_from_width = flag
        pruned, pruner = S.prune_at_stage(model, flat, 0.3)
        assert pruned.attention_scale_from_width is flag
        d = str(tmp_path / str(flag))
        meta = ckpt.save_pruned(pruned, d, pruner.pruning_history())
        assert ('attention_scale_from_width' in meta) == flag
        back = ckpt.load_pruned(d)
        assert back.attention_scale_from_width is flag
        assert {n: p.shape for n, p in back.named_parameters()} == {n: p.shape for n, p in pruned.named_parameters()}
    first = engine.UNetEngine(model.config)
    first.scale_from_q_width = True
    P = {n: p.detach() for n, p in model.named_parameters()}
    first.bind(P, None)
    assert sweep.Pipeline.another(first, P, P, 1, torch.device('cpu')).eng.scale_from_q_width is True
    # the engine's scale: q of the pruned attention blocks is 44 wide
    seen = []
    real = mocked.bmm_tn
    pruned.engine().scale_from_q_width = True            # what UNet2DModel.engine() does on the device (the host stand-in of
    try:                                                 # tests/test_cpu.py replaces that method): the engine object is kept
        mocked.bmm_tn = lambda a, b, alpha=1.0, **k: (seen.append((a.shape[1], alpha)), real(a, b, alpha=alpha, **k))[1]
        with torch.no_grad():
            pruned(torch.zeros(1, 3, 16, 16), 3)
    finally:
        mocked.bmm_tn = real
    assert seen and all(abs(alpha - float(d) ** -0.5) < 1e-12 for d, alpha in seen) and {d for d, _ in seen} == {44}


# ------------------------------------------------------------------------------------------------ world size 2 over gloo
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run(world, outdir):
    port = str(_free_port())
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, '_dist_worker_stage_study.py'), str(r), str(world), port, outdir])
             for r in range(world)]
    for p in procs:
        assert p.wait(timeout=600) == 0


def test_two_rank_snapshots_are_the_sum_of_the_local_ones_and_match_one_process(tmp_path):
    out = str(tmp_path)
    _run(1, out)
    _run(2, out)
    one = torch.load(os.path.join(out, 'stage_r0_w1.pt'))
    r0 = torch.load(os.path.join(out, 'stage_r0_w2.pt'))
    r1 = torch.load(os.path.join(out, 'stage_r1_w2.pt'))
    assert list(one['reduced']['stage_grads']) == [0, 2, 5, 6]
    assert one['reduced']['losses'] == one['local']['losses']
    for s, g in one['reduced']['stage_grads'].items():
        a, b = r0['reduced']['stage_grads'][s], r1['reduced']['stage_grads'][s]
        assert torch.equal(a, b)                                                 # all-reduced: identical on both ranks
        assert torch.equal(a, r0['local']['stage_grads'][s] + r1['local']['stage_grads'][s]), s       # the sum of the local ones, bit for bit
        assert torch.equal(one['local']['stage_grads'][s], g)
        off = 0
        for n in one['sizes']:                                                   # tests/test_dist_cpu.py's bound for shard linearity
            scale = float(g[off:off + n].abs().max())
            if scale > 1e-7:
                assert float((a[off:off + n] - g[off:off + n]).abs().max()) <= 2e-5 * scale, (s, off)
            off += n
    assert torch.equal(r0['reduced']['stage_grads'][6], r0['reduced']['final'])
    assert torch.equal(r0['local']['final'], r0['local']['stage_grads'][6]) and not torch.equal(r0['local']['final'], r0['reduced']['final'])
