"""CPU suite (`-m "not gpu"`): the oracle against the reference's golden vectors, the host logic (group
enumeration, schedules, pruner bookkeeping) and the C-ABI library surface.  No GPU compute is called."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

import golden_common as gc
import os as _os
GOLD_DIR = _os.path.join(_os.path.dirname(_os.path.abspath(__file__)), "golden")
from helpers import tp_like_groups, GOLD, load_json, load_npz, oracle_params, pkg, relerr, oracle_prune_replay

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------------------------- ABI
def test_library_exports_every_declared_symbol():
    L = pkg('_lib')
    hdr = open(os.path.join(ROOT, 'include', 'dp_hip.h')).read()
    declared = set(re.findall(r'^(?:int|long long) (dp_\w+)\(', hdr, re.M))
    assert declared == set(L.SIGNATURES), declared ^ set(L.SIGNATURES)
    lib = L.load()
    for name in declared:
        assert getattr(lib, name) is not None
    assert lib.dp_version() >= 100
    # struct sizes agree with the C header layout (all-int/pointer/long long members, natural alignment)
    assert ctypes.sizeof(L.ConvGeom) == 14 * 4 + 2 * 8
    assert ctypes.sizeof(L.Dropout) == 40 and lib.dp_launch_count() >= 0
    names = (ctypes.c_char_p * 8)()
    assert 0 <= lib.dp_recent_launches(names, 8) <= min(8, lib.dp_launch_count()) and lib.dp_recent_launches(names, 0) == 0


def test_every_launch_site_of_the_tabled_files_is_in_the_branch_table():
    """tests/test_dispatch_parity_gpu.py (the non-contraction launchers) and tests/test_contraction_dispatch_gpu.py (the contraction
    kernels) compare every dispatch branch of their files with fp64.  A new DP_LAUNCH site changes the count recorded there, a new
    kernel name is in none of the tables, a new .hip file with launches is in neither: each fails here, before a GPU is needed, so the
    table is edited (and a case written) together with the launcher."""
    import test_contraction_dispatch_gpu as K
    import test_dispatch_parity_gpu as D
    csrc = os.path.join(ROOT, 'diff-pruning_amd', 'csrc')
    names = {}
    for T in (D, K):
        tabled = {e.split(' | ')[0].split('<')[0] for e in T.BRANCHES}
        assert not set(T.UNREACHED) - set(T.BRANCHES)
        seen = {}
        for fname, want in T.LAUNCH_SITES.items():
            src = open(os.path.join(csrc, fname)).read()
            sites = re.findall(r'\bDP_LAUNCH\(\(?\s*([A-Za-z_]\w*)', src)
            assert len(sites) == want == src.count('DP_LAUNCH('), (fname, len(sites), want)
            seen.update({k: fname for k in sites})
        assert set(seen) == tabled, (T.__name__, 'launched, not tabled: %s' % sorted((seen[k], k) for k in set(seen) - tabled),
                                     'tabled, not launched: %s' % sorted(tabled - set(seen)))
        assert all(e in T.CASES or e in T.UNREACHED for e in T.BRANCHES) and not set(T.CASES) & set(T.UNREACHED), T.__name__
        assert all(r.strip() for r in T.UNREACHED.values())
        names[T] = tabled
    # the two tables together cover exactly the files that launch anything, and no kernel is tabled twice
    launching = {f for f in os.listdir(csrc) if f.endswith('.hip') and 'DP_LAUNCH(' in open(os.path.join(csrc, f)).read()}
    assert not set(D.LAUNCH_SITES) & set(K.LAUNCH_SITES)
    assert set(D.LAUNCH_SITES) | set(K.LAUNCH_SITES) == launching, sorted(launching ^ (set(D.LAUNCH_SITES) | set(K.LAUNCH_SITES)))
    assert not names[D] & names[K], sorted(names[D] & names[K])
    assert not {e.split(' | ')[0] for e in D.BRANCHES} & {e.split(' | ')[0] for e in K.BRANCHES}
    # the ring records the kernel expression of the launch site: its first macro argument, stringised
    hdr = open(os.path.join(csrc, 'dp_common.h')).read()
    assert re.search(r'#define DP_LAUNCH\(k, \.\.\.\).*= #k;.*hipLaunchKernelGGL\(k, __VA_ARGS__\)', hdr)


def test_contraction_dispatch_comparison_and_name_mirror():
    """The comparison tests/test_contraction_dispatch_gpu.py judges every case with (helpers.relerr: max-abs error over the reference's
    max-abs, then exceeding): a reference equal to the output passes, one element moved by twice the bound fails, a NaN in the output
    fails; and the one normalisation between a launch site's expression and ops._run's name."""
    import test_contraction_dispatch_gpu as K
    g = torch.Generator().manual_seed(3)
    y = torch.randn(3, 5, 7, generator=g)
    for bound in (K.B_WINO, K.B_DIRECT, 0.0):
        ok = dict(names=[], out=relerr(y, y.double()), bound=bound)
        assert not K.exceeding(ok), ok
        ref = y.double().clone()
        ref[1, 2, 3] += 2 * max(bound, 1e-7) * float(ref.abs().max())
        moved = dict(names=[], out=relerr(y, ref), bound=bound)
        assert list(K.exceeding(moved)) == ['out'] and moved['out'] > bound, moved
        bad = y.clone()
        bad[2, 4, 6] = float('nan')
        nan = dict(names=[], out=relerr(bad, y.double()), other=0.0, bound=bound)
        assert list(K.exceeding(nan)) == ['out'] and math.isnan(nan['out']), nan
    m = K.mirror_matches
    assert m('conv_gemm_kernel<BM, BN, false, true>', 'conv_gemm_kernel<64, 128, false, true>')
    assert not m('conv_gemm_kernel<BM, BN, false, true>', 'conv_gemm_kernel<64, 128, false, false>')
    assert m('conv_gemm_fast_kernel<BM, 128, TAILS, true>', 'conv_gemm_fast_kernel<96, 128, true, true>')
    assert not m('conv_gemm_fast_kernel<BM, 128, TAILS, true>', 'conv_gemm_fast_kernel<128, 64, false, true>')
    assert m('nt_gemm_kernel<BM, BN, true>', 'nt_gemm_kernel<128, 128, true, false>') and not m('nt_gemm_kernel<BM, BN, true>', 'nt_gemm_kernel<128, 128, true, true>')
    assert m('nt_gemm_kernel<64, 64, false, true>', 'nt_gemm_kernel<64, 64, false, true>') and not m('nt_gemm_kernel<64, 64, false, true>', 'nt_gemm_kernel<64, 64, false, false>')
    assert m('conv_wino_kernel<16, 2>', 'conv_wino_kernel<16, 2, 1>') and not m('conv_wino_kernel<16, 2>', 'conv_wino_kernel<16, 2, 2>')
    assert not m('conv_wino_kernel<16, 2>', 'conv_wino_kernel<8, 2, 1>') and not m('conv_wino2d_kernel<8, 2, false>', 'conv_wino2d_tail_kernel<8, 2, false>')
    assert m('conv_few_out_kernel', 'conv_few_out_kernel') and not m('conv_few_out_kernel', 'conv_gemm_kernel<64, 64, false, false>')


def test_diffusers_pipeline_directory_io(tmp_path):
    """DDPMPipeline.from_pretrained / save_pretrained (ddpm_prune.py:50,131) on a directory written by the vendored diffusers
    (tests/golden/pretrained_micro): same config, same weights, oracle forward equals the reference's recorded output; our
    own save_pretrained round-trips and writes the same file layout and JSON keys."""
    import os
    from oracle import unet_ref as U
    diffusion, unet = pkg('diffusion'), pkg('unet')
    src = os.path.join(GOLD_DIR, 'pretrained_micro')
    pipe = diffusion.DDPMPipeline.from_pretrained(src)
    assert isinstance(pipe.unet, unet.UNet2DModel) and isinstance(pipe.scheduler, diffusion.DDPMScheduler)
    assert pipe.scheduler.config.num_train_timesteps == 1000 and pipe.unet.config.sample_size == 8
    sd = pipe.unet.state_dict()
    for n, p in sd.items():
        assert torch.equal(p, torch.from_numpy(gc.det_param(n, tuple(p.shape), 71))), n
    cfg = {k: (list(v) if isinstance(v, tuple) else v) for k, v in dict(pipe.unet.config).items()}
    x = torch.from_numpy(gc.det_noise((1, 3, 8, 8), 72))
    with torch.no_grad():
        y = U.unet_forward({k: v.clone() for k, v in sd.items()}, cfg, x, torch.tensor([10]))
    want = np.load(os.path.join(src, 'expected.npz'))['fwd_out']
    assert float((y - torch.from_numpy(want)).abs().max()) < 1e-5
    # write it back: same files, same JSON key sets and values, weights identical
    pipe.set_progress_bar_config(disable=True)
    out = str(tmp_path / 'saved')
    pipe.save_pretrained(out)
    import json
    for rel in ('model_index.json', 'unet/config.json'):
        assert json.load(open(os.path.join(out, rel))) == json.load(open(os.path.join(src, rel))), rel
    ours, ref = json.load(open(os.path.join(out, 'scheduler/scheduler_config.json'))), json.load(open(os.path.join(src, 'scheduler/scheduler_config.json')))
    assert all(ref[k] == v for k, v in ours.items())                   # every key we write exists with the same value
    back = diffusion.DDPMPipeline.from_pretrained(out)
    assert all(torch.equal(v, sd[k]) for k, v in back.unet.state_dict().items())
    assert os.path.exists(os.path.join(out, 'unet', 'diffusion_pytorch_model.bin'))
    pipe.save_pretrained(str(tmp_path / 'safe'), safe_serialization=True)
    back = unet.UNet2DModel.from_pretrained(str(tmp_path / 'safe'), subfolder='unet')
    assert all(torch.equal(v, sd[k]) for k, v in back.state_dict().items())
    sched = diffusion.DDIMScheduler.from_pretrained(src, subfolder='scheduler')      # ddpm_prune.py:139-141
    assert sched.config.num_train_timesteps == 1000


def test_count_ops_and_params_matches_reference_c1():
    """tp.utils.count_ops_and_params (ddpm_prune.py:89,118): the un-pruned CIFAR UNet and the UNet pruned with the reference's
    C1 masks (replayed as a pruning history) give exactly the reference's MAC and parameter counts."""
    pruning, unet = pkg('pruning'), pkg('unet')
    fx = load_json('cifar_c1.json')
    model = unet.UNet2DModel(**gc.CIFAR_CFG)
    ex = {'sample': torch.randn(1, 3, 32, 32), 'timestep': torch.ones((1,)).long()}
    macs, params = pruning.utils.count_ops_and_params(model, ex)
    assert (macs, params) == (fx['base_macs'], fx['base_params'])
    pruning.DependencyGraph(model).load_pruning_history([[r['root'], True, r['pruned']] for r in fx['prune']])
    pruning.fix_static_attributes(model)
    macs, params = pruning.utils.count_ops_and_params(model, ex)
    assert (macs, params) == (fx['macs_after'], fx['params_after'])
    assert {n: list(p.shape) for n, p in model.named_parameters()} == fx['shapes_after']


def test_kernel_dispatch_heuristics():
    """Host-side dispatch rules of ops.py (pure arithmetic, no device): GroupNorm slicing, 96-row tiles for pruned
    widths, split-K of small grids."""
    ops = pkg('ops')
    L = pkg('_lib')

    class T:                                    # stand-in with the two attributes _gn_slices reads
        def __init__(self, ptr=0):
            self._p = ptr

        def data_ptr(self):
            return self._p
    assert ops._gn_slices(256, 32, 1024, (T(),), (4,)) == 0            # CIFAR batch 256: plenty of groups
    assert ops._gn_slices(4, 32, 65536, (T(), None), (4, 0)) == 16     # bedroom-256 batch 4: 16 slices of 4096 pixels
    assert ops._gn_slices(6, 32, 4096, (T(),), (4,)) == 1              # LDM latents: one slice per channel plane
    assert ops._gn_slices(4, 32, 65536, (T(8),), (4,)) == 0            # misaligned plane -> generic kernels
    assert ops._gn_slices(2, 8, 256, (T(),), (4,)) == 0                # small planes stay on the per-group kernel

    def conv_params(M, C=128, npix=4096, taps=9, stride=1, ups=0):
        p = L.ConvGemmParams()
        p.g = ops._geom(16, 16, 16, 16, 16 << ups, 16 << ups, 3, stride, 1, 1, 1, ups, C, 0, 0)
        p.M, p.C, p.NPIX, p.ntaps, p.batches, p.a_kc, p.tile = M, C, npix, taps, 1, 0, 0
        return p
    for M, want in ((90, 3), (180, 3), (128, 0), (256, 0), (359, 0), (64, 0)):
        p = conv_params(M)
        p.tile = ops.pick_tile(M, p.NPIX)
        before = p.tile
        ops._prefer_tile96(p)
        assert p.tile == (want if M > 64 else before), (M, p.tile)
    p = conv_params(90, stride=2)               # strided conv: general kernel keeps its tile
    p.tile = 1
    ops._prefer_tile96(p)
    assert p.tile == 1
    assert ops._cg_name(conv_params(256)) == 'conv_gemm_fast_kernel<128, 128, false, false>'       # x_guard not set: 4-byte loads
    assert ops._cg_name(conv_params(256, C=90)) == 'conv_gemm_fast_kernel<128, 128, true, false>'
    p = conv_params(256)
    p.x_guard = 1
    assert ops._cg_name(p) == 'conv_gemm_fast_kernel<128, 128, false, true>'
    # 128x64 tiles for launches below two rounds of 128x128 workgroups (and no split-K then); tails / unguarded inputs keep 128x128
    p = conv_params(256, C=256, npix=65536)
    p.x_guard = 1
    ops._conv_ksplit(p, None)
    assert p.tile == 0                                                 # the 128x64 experiment is off by default
    ops.CONV_N64_TILES = (512, 2048)
    ops._conv_ksplit(p, None)
    assert p.tile == 4 and p.ksplit == 1 and ops._cg_name(p) == 'conv_gemm_fast_kernel<128, 64, false, true>'
    p = conv_params(128, npix=262144)
    p.x_guard = 1
    ops._conv_ksplit(p, None)
    assert p.tile == 0 and p.ksplit == 1                               # 2048 tiles: two full rounds already
    p = conv_params(256, C=90, npix=65536)
    p.x_guard = 1
    ops._conv_ksplit(p, None)
    assert p.tile == 0
    ops.CONV_N64_TILES = None


def test_no_cpu_fallback():
    """The product refuses to run its hot path off-device instead of silently falling back."""
    unet = pkg('unet')
    m = unet.UNet2DModel(**gc.TINY_CFG)
    with pytest.raises(RuntimeError):
        m(torch.zeros(1, 3, 16, 16), 1)
    diffusion = pkg('diffusion')
    s = diffusion.DDPMScheduler()
    with pytest.raises(RuntimeError):
        s.add_noise(torch.zeros(1, 3, 4, 4), torch.zeros(1, 3, 4, 4), torch.tensor([1]))


def test_product_does_not_import_oracle():
    for fn in os.listdir(os.path.join(ROOT, 'diff-pruning_amd')):
        if fn.endswith('.py'):
            src = open(os.path.join(ROOT, 'diff-pruning_amd', fn)).read()
            assert not re.search(r'^\s*(from|import)\s+oracle', src, re.M), fn


# ------------------------------------------------------------------------------------- oracle vs golden
def test_oracle_schedule_and_embedding():
    from oracle import diffusion_ref as D, unet_ref as U
    g = load_npz('schedule.npz')
    acp = D.alphas_cumprod()
    assert np.array_equal(acp.numpy(), g['alphas_cumprod'])
    x0 = torch.from_numpy(gc.det_clean((2, 3, 4, 4), 11))
    eps = torch.from_numpy(gc.det_noise((2, 3, 4, 4), 12))
    for i, t in enumerate(g['ts']):
        out = D.add_noise(acp, x0, eps, torch.tensor([int(t)] * 2))
        assert np.array_equal(out.numpy(), g['add_noise'][i])
    e = U.timestep_embedding(torch.tensor([0, 1, 999]), 128, False, 1)
    assert np.allclose(e.numpy(), g['temb_128'], atol=1e-7)
    e = U.timestep_embedding(torch.tensor([0.0, 1.0, 999.0]), 32, True, 0)
    assert np.allclose(e.numpy(), g['temb_32_flip'], atol=1e-7)


def test_oracle_unet_forward_and_sweep_grads():
    from oracle import diffusion_ref as D, unet_ref as U
    cfg = gc.TINY_CFG
    P = oracle_params(cfg, 5)
    g = load_npz('tiny_unet.npz')
    clean = torch.from_numpy(gc.det_clean((2, 3, 16, 16), 1))
    noise = torch.from_numpy(gc.det_noise((2, 3, 16, 16), 2))
    t = torch.tensor([3, 500])
    with torch.no_grad():
        y = U.unet_forward(P, cfg, D.add_noise(D.alphas_cumprod(), clean, noise, t), t)
    # tolerance: the reference ran SDPA attention, the oracle restates the legacy baddbmm path -> fp32 rounding only
    assert float((y - torch.from_numpy(g['fwd_out'])).abs().max()) < 5e-6
    losses = D.taylor_sweep(P, cfg, clean, noise, 4)
    assert np.allclose(losses, g['losses'], rtol=1e-6)
    for k in g.files:
        if k.startswith('grad::'):
            assert relerr(P[k[6:]].grad, g[k]) < 2e-5, k
    st = load_json('tiny_prune.json')['grad_stats']
    assert set(st) == set(P)
    for n, (s, a, q) in st.items():
        gr = P[n].grad.double()
        # to_k.bias gradients are identically zero in exact arithmetic (softmax shift invariance): absolute floor
        assert abs(float(gr.abs().sum()) - a) <= 2e-5 * a + 1e-8 * gr.numel(), n


def test_oracle_optimizer_step_matches_reference_pieces():
    """clip_grad_norm_(1.0) -> torch.optim.Adam (ddpm_train.py:331-337 hyper-parameters) -> vendored EMAModel.step
    (training_utils.py:181-218), three consecutive steps on seeded tensors (first step clips, the others do not)."""
    from oracle import diffusion_ref as D
    fx = load_json('optim.json')
    shapes = [tuple(s) for s in fx['shapes']]
    params = [torch.from_numpy(gc.det_param('p%d.weight' % i, s, 61)).clone() for i, s in enumerate(shapes)]
    ema = [p.clone() for p in params]
    m = [torch.zeros_like(p) for p in params]
    v = [torch.zeros_like(p) for p in params]
    hp = fx['hp']
    for step, rec in enumerate(fx['steps']):
        grads = [torch.from_numpy(gc.det_param('g%d_%d.weight' % (i, step), shapes[i], 62)) * (3.0 if step == 0 else 0.05)
                 for i in range(len(shapes))]
        norm = D.adam_ema_step(params, grads, m, v, ema, step + 1, lr=hp['lr'], b1=hp['betas'][0], b2=hp['betas'][1],
                               eps=hp['eps'], ema_decay=fx['ema_decay'], max_norm=1.0)
        assert abs(norm - rec['norm']) <= 1e-6 * rec['norm']
        for p, e, rp, re_ in zip(params, ema, rec['params'], rec['ema']):
            assert relerr(p, torch.from_numpy(gc.b64_to_f32(rp)).view_as(p)) < 2e-6
            assert relerr(e, torch.from_numpy(gc.b64_to_f32(re_)).view_as(e)) < 2e-6


def test_oracle_bedroom_topology_matches_reference():
    """6-level bedroom/church-256 topology at tiny widths: oracle forward, sweep losses and gradient statistics against the
    reference UNet2DModel (tests/golden/tiny_bedroom.*)."""
    from oracle import diffusion_ref as D, unet_ref as U
    fx, g = load_json('tiny_bedroom.json'), load_npz('tiny_bedroom.npz')
    cfg = fx['cfg']
    P = oracle_params(cfg, 3)
    clean = torch.from_numpy(gc.det_clean((1, 3, 32, 32), 5))
    noise = torch.from_numpy(gc.det_noise((1, 3, 32, 32), 6))
    t = torch.tensor([250])
    with torch.no_grad():
        y = U.unet_forward(P, cfg, D.add_noise(D.alphas_cumprod(), clean, noise, t), t)
    assert float((y - torch.from_numpy(g['fwd_out'])).abs().max()) < 1e-5
    losses = D.taylor_sweep(P, cfg, clean, noise, 2)
    assert np.allclose(losses, g['losses'], rtol=1e-5)
    for n, (s, a, q) in fx['grad_stats'].items():
        gr = P[n].grad.double()
        assert abs(float(gr.abs().sum()) - a) <= 2e-5 * a + 1e-8 * gr.numel(), n


def test_oracle_prune_masks_match_reference_tiny():
    """Scores, masks and post-prune shapes of the full ratio-0.3 prune of the tiny UNet."""
    from oracle import diffusion_ref as D, unet_ref as U
    cfg = gc.TINY_CFG
    P = oracle_params(cfg, 5)
    clean = torch.from_numpy(gc.det_clean((2, 3, 16, 16), 1))
    noise = torch.from_numpy(gc.det_noise((2, 3, 16, 16), 2))
    D.taylor_sweep(P, cfg, clean, noise, 4)
    fx = load_json('tiny_prune.json')
    Pd = {n: p.detach().clone() for n, p in P.items()}
    Gd = {n: p.grad.clone() for n, p in P.items()}
    rec = oracle_prune_replay(Pd, Gd, cfg, 0.3, pkg('graph'))
    assert len(rec) == len(fx['prune'])
    for mine, ref in zip(rec, fx['prune']):
        assert mine['root'] == ref['root'] and mine['ch_groups'] == ref['ch_groups']
        assert relerr(mine['score'], gc.b64_to_f32(ref['score'])) < 1e-5, ref['root']
        assert mine['pruned'] == ref['pruned'], (ref['root'], mine['margin'])
    assert {n: list(t.shape) for n, t in Pd.items()} == fx['shapes_after']
    assert sum(t.numel() for t in Pd.values()) == fx['params_after']
    # post-prune forward (reference used the legacy AttnProcessor here)
    t = torch.tensor([3, 500])
    with torch.no_grad():
        y2 = U.unet_forward(Pd, cfg, D.add_noise(D.alphas_cumprod(), clean, noise, t), t)
    assert float((y2 - torch.from_numpy(gc.b64_to_f32(fx['fwd_after']))).abs().max()) < 5e-6


CRITERIA = ['full1', 'full2', 'abs', 'fisher', 'magnitude']


def _expand(ranges):
    return [i for a, b in ranges for i in range(a, b)]


@pytest.mark.parametrize('crit', CRITERIA)
def test_oracle_sibling_criteria_match_reference_tiny(crit):
    """FullTaylor(order 1, 2) / AbsTaylor / Fisher / Magnitude (ddpm_exp/prune.py:193-208): scores and masks of the
    whole sequential prune of the tiny UNet against the vectors recorded from the vendored classes."""
    from oracle import diffusion_ref as D
    cfg = gc.TINY_CFG
    P = oracle_params(cfg, 5)
    clean = torch.from_numpy(gc.det_clean((2, 3, 16, 16), 1))
    noise = torch.from_numpy(gc.det_noise((2, 3, 16, 16), 2))
    D.taylor_sweep(P, cfg, clean, noise, 4)
    fx = load_json('tiny_criteria.json')[crit]
    Pd = {n: p.detach().clone() for n, p in P.items()}
    Gd = {n: p.grad.clone() for n, p in P.items()}
    rec = oracle_prune_replay(Pd, Gd, cfg, 0.3, pkg('graph'), mode=crit)
    assert len(rec) == len(fx['groups'])
    for mine, ref in zip(rec, fx['groups']):
        assert mine['root'] == ref['root'] and mine['ch_groups'] == ref['ch_groups']
        assert relerr(mine['score'], gc.b64_to_f32(ref['score'])) < 2e-5, (crit, ref['root'])
        assert mine['pruned'] == _expand(ref['pruned']), (crit, ref['root'], mine['margin'])
    assert sum(t.numel() for t in Pd.values()) == fx['params_after']


def test_oracle_early_exit_step_count():
    from oracle import diffusion_ref as D
    cfg = gc.TINY_CFG
    fx = load_json('tiny_prune.json')['early_exit']
    P = oracle_params(cfg, 5)
    clean = torch.from_numpy(gc.det_clean((2, 3, 16, 16), 1))
    noise = torch.from_numpy(gc.det_noise((2, 3, 16, 16), 2))
    losses = D.taylor_sweep(P, cfg, clean, noise, 1000, thr=fx['thr'])
    assert len(losses) == fx['steps']
    assert np.allclose(losses, fx['losses'], rtol=1e-6)


def test_oracle_ddim():
    from oracle import diffusion_ref as D
    g = load_npz('ddim.npz')
    for skip in ('uniform', 'quad'):
        assert np.array_equal(D.ddim_timesteps(100, skip_type=skip).numpy(), g['timesteps_' + skip])
    cfg = gc.TINY_CFG
    P = oracle_params(cfg, 5, requires_grad=False)
    x = torch.from_numpy(gc.det_noise((2, 3, 16, 16), 21))
    _, trace = D.ddim_sample(P, cfg, x, 100, first_n=5)
    for i in range(5):
        # tolerance 5e-5 abs on |x| ~ 1: SDPA (reference) vs baddbmm (oracle) attention rounding through i+1 UNet calls
        assert float((trace[i] - torch.from_numpy(g['x_steps'][i])).abs().max()) < 5e-5
    x = torch.from_numpy(gc.det_noise((2, 3, 16, 16), 22))
    xf, _ = D.ddim_sample(P, cfg, x, 10)
    assert float((D.to_image(xf) - torch.from_numpy(g['chain10_image'])).abs().max()) < 2e-4   # 10 UNet calls, images in [0,1]


# ---------------------------------------------------------------------------------------- host logic
def _check_groups(cfg, table):
    from oracle import unet_ref as U
    G = pkg('graph')
    gr = G.UNetGraph(cfg)
    shapes = U.param_shapes(cfg)
    groups = list(G.all_groups(gr, lambda: G.ChannelView(shapes)))
    assert len(groups) == len(table)
    for ref, (root, mem) in zip(table, groups):
        assert ref['members'][0][0] == root
        refset = {(m[0], m[1]): gc.expand(m[2]) for m in ref['members']}
        myset = {(m.name, m.kind): m.idxs for m in mem}
        assert refset == myset, root
        has_gn = any(m.kind == 'gn' for m in mem)
        assert ref['ch_groups'] == (cfg['norm_num_groups'] if has_gn else 1)


def test_group_enumeration_matches_reference_cifar():
    _check_groups(gc.CIFAR_CFG, load_json('groups.json')['cifar'])


@pytest.mark.parametrize('variant', ['all_attn_3lvl_l1', 'no_attn_2lvl_l3', 'heads8_4lvl'])
def test_group_enumeration_matches_reference_other_topologies(variant):
    """The coupling graph is generic over UNet2DModel configs: all-attention blocks, other depths / layers_per_block,
    multi-head attention (attention_head_dim 8), non-uniform widths -- group order and member index sets equal to the
    vendored DependencyGraph's."""
    fx = load_json('groups_more.json')[variant]
    _check_groups(fx['cfg'], fx['groups'])


def test_multi_head_unet_magnitude_prune_with_head_groups(mocked):
    """ldm_prune.py:62-90 shape of use: a multi-head UNet2DModel (attention_head_dim 8) is built, pruned with
    MagnitudeImportance and channel_groups = attention heads (per-head channel selection), and reproduces the reference's
    pruned index lists, shapes and parameter count; running it is refused (the HIP attention path is single-head)."""
    pruning, unet = pkg('pruning'), pkg('unet')
    fx = load_json('groups_more.json')['heads8_4lvl']
    mp = fx['magnitude_prune']
    model = unet.UNet2DModel(**fx['cfg'])
    gc.det_init_(model, mp['seed'])
    channel_groups = {}
    for m in model.modules():
        if isinstance(m, unet.Attention):
            assert m.heads > 1
            channel_groups[m.to_q] = channel_groups[m.to_k] = channel_groups[m.to_v] = m.heads
    pr = pruning.MagnitudePruner(model, None, importance=pruning.MagnitudeImportance(), iterative_steps=1,
                                 channel_groups=channel_groups, ch_sparsity=0.3, ignored_layers=[model.conv_out])
    for g in pr.step(interactive=True):
        g.prune()
    assert [r[0] for r in pr.records] == [r['root'] for r in mp['records']]
    want = [[i for a, b in r['pruned'] for i in range(a, b)] for r in mp['records']]
    assert [r[3] for r in pr.records] == want
    # (16-channel layers under 8 GroupNorm groups lose 5 // 8 = 0 channels per sub-group: empty lists on both sides; the
    #  fixture's ch_groups of such an empty group was read from a root-only group and is not meaningful)
    assert all(r[1] == ref['ch_groups'] for r, ref, w in zip(pr.records, mp['records'], want) if w)
    assert any(ref['ch_groups'] not in (1, 8) for ref, w in zip(mp['records'], want) if w)      # head-grouped q/k/v present
    assert {n: list(p.shape) for n, p in model.named_parameters()} == mp['shapes_after']
    assert sum(p.numel() for p in model.parameters()) == mp['params_after']


def test_oracle_multi_head_attention_matches_reference():
    """Oracle UNet with attention_head_dim 8 (4 / 6 / 8 heads) against the reference UNet2DModel: forward, sweep losses and
    gradient statistics (the restatement next round's multi-head engine path will be checked against)."""
    from oracle import diffusion_ref as D, unet_ref as U
    cfg = load_json('groups_more.json')['heads8_4lvl']['cfg']
    fx, g = load_json('tiny_heads.json'), load_npz('tiny_heads.npz')
    P = oracle_params(cfg, 4)
    clean = torch.from_numpy(gc.det_clean((2, 3, 16, 16), 81))
    noise = torch.from_numpy(gc.det_noise((2, 3, 16, 16), 82))
    t = torch.tensor([5, 700])
    with torch.no_grad():
        y = U.unet_forward(P, cfg, D.add_noise(D.alphas_cumprod(), clean, noise, t), t)
    assert float((y - torch.from_numpy(g['fwd_out'])).abs().max()) < 1e-5
    losses = D.taylor_sweep(P, cfg, clean, noise, 2)
    assert np.allclose(losses, g['losses'], rtol=1e-5)
    for n, (s, a, q) in fx['grad_stats'].items():
        gr = P[n].grad.double()
        assert abs(float(gr.abs().sum()) - a) <= 2e-5 * a + 1e-8 * gr.numel(), n


def test_multi_head_engine_logic_matches_oracle_on_mocked_kernels(mocked, monkeypatch):
    """The engine's attention forward / backward with heads > 1 (head h = contiguous channel rows of every image -> batch
    index n*heads + h of the same batched products) against the pinned multi-head oracle, on mocked kernels.  (On the GPU
    UNet2DModel.engine() still refuses multi-head models until this path has run there.)"""
    from oracle import diffusion_ref as D
    sweep = pkg('sweep')
    monkeypatch.setattr(sweep.HipSweepStep, '__init__', _cpu_step_init)
    cfg = load_json('groups_more.json')['heads8_4lvl']['cfg']
    model = _cpu_model(cfg, 4)
    clean = torch.from_numpy(gc.det_clean((2, 3, 16, 16), 81))
    noise = torch.from_numpy(gc.det_noise((2, 3, 16, 16), 82))
    res = sweep.taylor_sweep(model, pkg('diffusion').DDPMScheduler(), clean, noise, num_steps=2)
    P = oracle_params(cfg, 4)
    losses = D.taylor_sweep(P, cfg, clean, noise, 2)
    assert np.allclose(res['losses'], losses, rtol=1e-5)
    for n, p in model.named_parameters():
        if P[n].grad.abs().max() > 1e-7:
            assert relerr(p.grad, P[n].grad) < 5e-5, n


def test_celeba_cifar100_and_config_datasets(tmp_path):
    """SURVEY §8(f) rank 4, host side: the CelebA split file + crop window + resize of ddpm_exp/datasets (celeba.py:50-107,
    __init__.py:60-93), CIFAR-100's pickle (utils.py:41-49) and the `data:` block dispatch (LSUN / FFHQ: test_lsun_ffhq_lmdb_datasets)."""
    import pickle
    from PIL import Image
    data = pkg('data')
    root = tmp_path / 'celeba'
    (root / 'Img' / 'img_align_celeba').mkdir(parents=True)
    (root / 'Eval').mkdir()
    rng = np.random.default_rng(0)
    names, arrs = [], {}
    for i in range(5):
        nm = '%06d.png' % (i + 1)                      # lossless stand-ins for the JPEGs: pixel values must survive
        arr = rng.integers(0, 256, size=(218, 178, 3), dtype=np.uint8)
        Image.fromarray(arr).save(root / 'Img' / 'img_align_celeba' / nm)
        names.append(nm)
        arrs[nm] = arr
    (root / 'Eval' / 'list_eval_partition.txt').write_text(''.join('%s %d\n' % (nm, sp) for nm, sp in zip(names, (0, 0, 1, 2, 0))))
    ds = data.CelebAAligned(str(root), 'train', image_size=128)
    assert len(ds) == 3 and ds.files == [names[0], names[1], names[4]]
    # Crop(x1=57, x2=185, y1=25, y2=153) -> F.crop(img, top=57, left=25, 128, 128): rows 57..184, columns 25..152
    assert np.array_equal(ds[2], arrs[names[4]][57:185, 25:153])
    assert len(data.CelebAAligned(str(root), 'test', 64)) == 1 and data.CelebAAligned(str(root), 'valid', 64)[0].shape == (64, 64, 3)
    small = data.CelebAAligned(str(root), 'train', image_size=64)[0]
    want = np.asarray(Image.fromarray(arrs[names[0]][57:185, 25:153]).resize((64, 64), Image.BILINEAR))
    assert np.array_equal(small, want)
    with pytest.raises(ValueError, match='Wrong split'):
        data.CelebAAligned(str(root), 'training')
    c100 = tmp_path / 'cifar-100-python'
    c100.mkdir()
    px = rng.integers(0, 256, size=(7, 3072), dtype=np.uint8)
    with open(c100 / 'train', 'wb') as f:
        pickle.dump({'data': px, 'fine_labels': list(range(7))}, f)
    d100, kw = data.get_dataset('CIFAR100', root=str(tmp_path))
    assert len(d100) == 7 and d100.hwc is False and np.array_equal(d100[3], px[3].reshape(3, 32, 32)) and kw == dict(crop=None)
    cfg = dict(dataset='CELEBA', image_size=64, random_flip=True, rescaled=True, uniform_dequantization=False,
               gaussian_dequantization=False, logit_transform=False)
    dsc, kw = data.dataset_from_config(cfg, root=str(tmp_path))
    assert isinstance(dsc, data.CelebAAligned) and len(dsc) == 3
    assert kw == dict(mode=data.RESCALE, flip_p=0.5, dequant=False, crop=None)
    assert data.dataset_from_config(cfg, root=str(tmp_path), train=False)[1]['flip_p'] == 0.0
    x = torch.tensor([-1.5, -1.0, 0.0, 1.0, 2.0])
    assert torch.equal(data.inverse_data_transform(x), torch.tensor([0.0, 0.0, 0.5, 1.0, 1.0]))


def test_fused_attention_lane_maps_restated_in_numpy():
    """The register-level algorithm of csrc/attention.hip restated lane by lane (host logic, no GPU): with the MFMA operand map
    a = A[lane & 31][lane >> 5], b = B[lane >> 5][lane & 31] and accumulator register r of a lane = D[(r & 3) + 8 (r >> 2) +
    4 (lane >> 5)][lane & 31] (csrc/gemm.hip), (1) S^T = K^T Q puts 16 keys of ONE query in each lane, (2) accumulator register
    r of the two lane halves is exactly the key pair MFMA step r of O^T += V P^T consumes, with V as component r & 3 of a 4-wide
    load -- so P never leaves the registers -- and (3) splitting the CHANNELS over four wavefronts (tiles w, w + 4, ...; zero
    fill past a ragged width, value width != key width) with the partial S^T tiles added in fixed order gives softmax attention.
    Pins the index arithmetic of the kernel's comments; the kernel itself is tested on the GPU (test_fused_attention_*)."""
    lane = np.arange(64)
    li, half = lane & 31, lane >> 5
    rowmap = np.array([[(r & 3) + 8 * (r >> 2) + 4 * (l >> 5) for r in range(16)] for l in range(64)])

    def mfma(a, b, acc):
        D = np.stack([a[:32], a[32:]], 1) @ np.stack([b[:32], b[32:]], 0)
        out = acc.copy()
        for r in range(16):
            out[:, r] += D[rowmap[:, r], li]
        return out

    def ld(x, c, j):                                     # raw buffer load: a channel past the slab reads 0
        c = np.asarray(c)
        return np.where(c < x.shape[0], x[np.minimum(c, x.shape[0] - 1), j], 0.0)

    def fused(q, k, v, scale):
        d, T = q.shape
        dv = v.shape[0]
        NT = -(-max(-(-d // 32), -(-dv // 32)) // 4)
        o = np.zeros((dv, T))
        for i0 in range(0, T, 32):
            m = np.full(64, -np.inf)
            l = np.zeros(64)
            oacc = [[np.zeros((64, 16)) for _ in range(NT)] for _ in range(4)]
            for j0 in range(0, T, 32):
                part = []
                for w in range(4):
                    sacc = np.zeros((64, 16))
                    for t in range(NT):
                        c0 = 32 * (w + 4 * t)
                        for s_ in range(16):
                            sacc = mfma(ld(k, c0 + 2 * s_ + half, j0 + li), ld(q, c0 + 2 * s_ + half, i0 + li), sacc)
                    part.append(sacc)
                sc = (((part[0] + part[1]) + part[2]) + part[3]) * scale
                bm = sc.max(1)
                bm = np.maximum(bm, bm[lane ^ 32])
                mn = np.maximum(m, bm)
                alpha = np.exp(m - mn)
                p = np.exp(sc - mn[:, None])
                l = l * alpha + p.sum(1)
                m = mn
                for w in range(4):
                    for t in range(NT):
                        oacc[w][t] *= alpha[:, None]
                        for g in range(4):
                            for e in range(4):           # component e of the 16-byte load at key 8 g + 4 half
                                vv = ld(v, 32 * (w + 4 * t) + li, j0 + 8 * g + 4 * half + e)
                                oacc[w][t] = mfma(vv, p[:, 4 * g + e], oacc[w][t])
            lt = l + l[lane ^ 32]
            for w in range(4):
                for t in range(NT):
                    for r in range(16):
                        c = 32 * (w + 4 * t) + rowmap[:, r]
                        ok = c < dv
                        o[c[ok], i0 + li[ok]] = (oacc[w][t][:, r] / lt)[ok]
        return o

    rng = np.random.default_rng(0)
    for d, dv, T in ((64, 64, 64), (179, 133, 64), (256, 256, 96)):
        q, k, v = rng.standard_normal((d, T)), rng.standard_normal((d, T)), rng.standard_normal((dv, T))
        s = d ** -0.5 * (q.T @ k)
        p = np.exp(s - s.max(1, keepdims=True))
        ref = v @ (p / p.sum(1, keepdims=True)).T
        assert np.abs(fused(q, k, v, d ** -0.5) - ref).max() < 1e-12, (d, dv, T)


def test_fused_attention_wiring_on_mocked_kernels(mocked, monkeypatch):
    """Engine wiring of the fused attention forward (ops.FUSED_ATTN): taken by forwards that keep nothing for a backward, with
    the head / value-width arguments the three-launch path uses (multi-head UNet at T = 64, LDM transformer block at T = 64 /
    256); the saving forward of a sweep step never takes it (its backward reads the materialised probabilities)."""
    cfg = dict(load_json('groups_more.json')['heads8_4lvl']['cfg'])
    model = _cpu_model(cfg, 4)
    x = torch.from_numpy(gc.det_clean((2, 3, 32, 32), 81))
    t = torch.tensor([3, 500])
    calls = []
    real = mocked.attention_fwd
    monkeypatch.setattr(mocked, 'attention_fwd', lambda *a, **kw: (calls.append(a[3]), real(*a, **kw))[1])
    with torch.no_grad():
        y0 = model.engine().forward(x, t, save=False)
        assert not calls
        monkeypatch.setattr(mocked, 'FUSED_ATTN', True)
        y1 = model.engine().forward(x, t, save=False)
    assert calls and all(h > 1 for h in calls) and relerr(y1, y0) < 1e-5
    n_fwd = len(calls)
    model.engine().forward(x, t, save=True)
    assert len(calls) == n_fwd                          # the saving forward keeps the three launches
    ldm = pkg('ldm')
    monkeypatch.setattr(ldm, 'ops', mocked)
    m2 = ldm.UNetModel(**dict(gc.LDM_TINY_CFG))
    gc.det_init_(m2, 9)
    eng = ldm.LdmEngine(m2.config)
    eng.bind({n: p.detach() for n, p in m2.named_parameters()}, None)
    xl = torch.from_numpy(gc.det_noise((2, 3, 16, 16), 5))
    ctx = torch.from_numpy(gc.det_noise((2, 1, 16), 6))
    with torch.no_grad():
        z1 = eng.forward(xl, t, ctx, save=False)
        monkeypatch.setattr(mocked, 'FUSED_ATTN', False)
        z0 = eng.forward(xl, t, ctx, save=False)
    assert len(calls) > n_fwd and relerr(z1, z0) < 1e-5


def test_multi_head_unet_needs_the_gpu_like_any_other():
    """Multi-head models run on the HIP engine since round 2 (tests/test_e2e_gpu.py::test_multi_head_*); on a CPU tensor the
    refusal is the generic no-CPU-fallback one."""
    m = pkg('unet').UNet2DModel(**load_json('groups_more.json')['heads8_4lvl']['cfg'])
    with pytest.raises(RuntimeError, match='no CPU'):
        m.engine()


def test_group_enumeration_matches_reference_bedroom_topology():
    cfg = dict(gc.BEDROOM_CFG, block_out_channels=[32, 32, 64, 64, 128, 128], sample_size=64)
    _check_groups(cfg, load_json('groups.json')['bedroom_topology'])


def test_group_enumeration_tiny_and_recorded_sequence():
    """Groups recomputed between prunes (channel counts shrink) -- compared with the per-group member tables the
    reference recorded DURING its interactive prune (tiny_prune.json 'prune' records)."""
    from oracle import unet_ref as U
    G = pkg('graph')
    cfg = gc.TINY_CFG
    fx = load_json('tiny_prune.json')
    _check_groups(cfg, fx['groups'])
    shapes = {n: tuple(s) for n, s in U.param_shapes(cfg).items()}
    gr = G.UNetGraph(cfg)
    it = G.all_groups(gr, lambda: G.ChannelView(shapes))
    for ref in fx['prune']:
        root, mem = next(it)
        assert root == ref['root']
        assert {(m.name, m.kind): m.idxs for m in mem} == {(m[0], m[1]): gc.expand(m[2]) for m in ref['members']}
        for m in G.coupled_members(gr, G.ChannelView(shapes), root, ref['pruned']):
            k = m.name + '.weight'
            s = list(shapes[k])
            s[1 if m.kind == 'in' else 0] -= len(m.idxs)
            shapes[k] = tuple(s)
            if m.kind != 'in' and (m.name + '.bias') in shapes:
                shapes[m.name + '.bias'] = (s[0],)
    assert {n: list(s) for n, s in shapes.items()} == fx['shapes_after']


def test_state_dict_keys_and_param_count():
    from oracle import unet_ref as U
    unet = pkg('unet')
    m = unet.UNet2DModel(**gc.CIFAR_CFG)
    sd = {n: tuple(p.shape) for n, p in m.named_parameters()}
    ref = U.param_shapes(gc.CIFAR_CFG)
    assert sd == {n: tuple(s) for n, s in ref.items()}
    assert sum(p.numel() for p in m.parameters()) == 35746307          # BASELINE.md known answer
    c1 = load_json('cifar_c1.json')
    assert set(c1['grad_stats']) == set(sd)
    assert c1['base_params'] == 35746307 and c1['params_after'] == 19851157


def test_ddim_scheduler_timesteps_and_antithetic():
    diffusion = pkg('diffusion')
    g = load_npz('ddim.npz')
    s = diffusion.DDIMScheduler()
    for skip in ('uniform', 'quad'):
        s.skip_type = skip
        s.set_timesteps(100)
        assert np.array_equal(s.timesteps.numpy(), g['timesteps_' + skip])
    sch = load_npz('schedule.npz')
    assert np.array_equal(s.alphas_cumprod.numpy(), sch['alphas_cumprod'])
    train = pkg('train')
    gen = torch.Generator().manual_seed(0)
    t = train.antithetic_timesteps(7, 1000, gen)
    gen = torch.Generator().manual_seed(0)
    r = torch.randint(0, 1000, (4,), generator=gen)
    assert torch.equal(t, torch.cat([r, 1000 - r - 1])[:7])


def test_pruner_bookkeeping_on_cpu_model():
    """MetaPruner target counts / sub-group selection (metapruner.py:225-249) with a stub importance, CPU tensors only."""
    pruning = pkg('pruning')
    unet = pkg('unet')
    cfg = gc.TINY_CFG
    m = unet.UNet2DModel(**cfg)
    fx = load_json('tiny_prune.json')

    class FromFixture(pruning.Importance):
        def __init__(self):
            self.k = 0

        def __call__(self, group, ch_groups=1):
            s = torch.from_numpy(gc.b64_to_f32(fx['prune'][self.k]['score']))
            self.k += 1
            return s

    pr = pruning.MagnitudePruner(m, None, importance=FromFixture(), iterative_steps=1, ch_sparsity=0.3,
                                 ignored_layers=[m.conv_out])
    for g in pr.step(interactive=True):
        g.prune()
    assert [r[3] for r in pr.records] == [r['pruned'] for r in fx['prune']]
    assert {n: list(p.shape) for n, p in m.named_parameters()} == fx['shapes_after']
    pruning.fix_static_attributes(m)
    assert m.down_blocks[0].downsamplers[0].channels == m.down_blocks[0].downsamplers[0].conv.in_channels


# ------------------------------------------------------------- engine graph / control flow on mocked kernels
@pytest.fixture()
def mocked(monkeypatch):
    """Swap the kernel wrappers for CPU stand-ins (tests/mock_ops.py) in every product module that uses them."""
    import mock_ops
    for sub in ('engine', 'sweep', 'train', 'diffusion', 'pruning'):
        monkeypatch.setattr(pkg(sub), 'ops', mock_ops)
    unet = pkg('unet')
    monkeypatch.setattr(unet.UNet2DModel, 'engine', _cpu_engine)
    return mock_ops


def _cpu_engine(self):
    engine = pkg('engine')
    if self._engine is None:
        self._engine = engine.UNetEngine(self.config)
    self._engine.packs.rebind()
    self._engine.bind({n: p.detach() for n, p in self.named_parameters()}, None)
    self._engine.set_dropout(self.dropout_table() if self.training else None, getattr(self, 'dropout_seed', 0),
                             getattr(self, '_dropout_step', 0))
    return self._engine


def _cpu_model(cfg, seed):
    m = pkg('unet').UNet2DModel(**cfg)
    gc.det_init_(m, seed)
    return m.eval()


def test_engine_backward_graph_matches_oracle_autograd(mocked, monkeypatch):
    """The engine's hand-written backward (skip-gradient routing, virtual concat, shared silu(temb), attention)
    reproduces autograd of the oracle when its kernels are replaced by CPU stand-ins."""
    from oracle import diffusion_ref as D
    sweep = pkg('sweep')
    monkeypatch.setattr(sweep.HipSweepStep, '__init__', _cpu_step_init)
    cfg = gc.TINY_CFG
    model = _cpu_model(cfg, 5)
    clean = torch.from_numpy(gc.det_clean((2, 3, 16, 16), 1))
    noise = torch.from_numpy(gc.det_noise((2, 3, 16, 16), 2))
    res = sweep.taylor_sweep(model, pkg('diffusion').DDPMScheduler(), clean, noise, num_steps=3)
    P = oracle_params(cfg, 5)
    losses = D.taylor_sweep(P, cfg, clean, noise, 3)
    assert np.allclose(res['losses'], losses, rtol=1e-5)
    for n, p in model.named_parameters():
        if P[n].grad.abs().max() > 1e-7:
            assert relerr(p.grad, P[n].grad) < 5e-5, n
    # bedroom-like topology (6 levels, attention in the 5th down / 2nd up block) on tiny widths
    cfgb = dict(gc.BEDROOM_CFG, block_out_channels=[16, 16, 32, 32, 64, 64], sample_size=32, norm_num_groups=8)
    modelb = _cpu_model(cfgb, 3)
    cb = torch.from_numpy(gc.det_clean((1, 3, 32, 32), 5))
    nb = torch.from_numpy(gc.det_noise((1, 3, 32, 32), 6))
    resb = sweep.taylor_sweep(modelb, pkg('diffusion').DDPMScheduler(), cb, nb, num_steps=2)
    Pb = oracle_params(cfgb, 3)
    lb = D.taylor_sweep(Pb, cfgb, cb, nb, 2)
    assert np.allclose(resb['losses'], lb, rtol=1e-5)
    for n, p in modelb.named_parameters():
        if Pb[n].grad.abs().max() > 1e-7:
            assert relerr(p.grad, Pb[n].grad) < 5e-5, n


def _cpu_step_init(self, model, scheduler, clean, noise, global_numel, loss_kind='mse', global_batch=None):
    self.model, self.scheduler = model, scheduler
    self.clean, self.noise = clean.contiguous().float(), noise.contiguous().float()
    self.B = clean.shape[0]
    if loss_kind == 'mse':
        self.gscale, self.lscale = 2.0 / global_numel, 1.0 / global_numel
    else:
        gb = global_batch if global_batch is not None else self.B
        self.gscale, self.lscale = 2.0 / gb, 1.0 / gb
    self.eng = model.engine()
    self._P = {n: p.detach() for n, p in model.named_parameters()}
    self._G = {n: p.grad for n, p in model.named_parameters()}
    self.eng.bind(self._P, self._G)
    self.acp = scheduler.alphas_cumprod


def test_gradient_views_and_further_pipelines(mocked, monkeypatch):
    """sweep.grad_views tiles one zeroed flat buffer with parameter-shaped views in parameter order; flatten_grads lays the
    .grad buffers out so that HipSweepStep._flat_of_grads finds the buffer (and finds none once a .grad is a tensor of its
    own); Pipeline.another builds engines that share the first one's packs, on their own slots and buffers."""
    sweep = pkg('sweep')
    monkeypatch.setattr(sweep.HipSweepStep, '__init__', _cpu_step_init)
    model = _cpu_model(gc.TINY_CFG, 5)
    params = dict(model.named_parameters())
    flat, views = sweep.grad_views(params)
    assert flat.dtype == torch.float32 and flat.dim() == 1 and flat.numel() == sum(p.numel() for p in params.values())
    assert not flat.any() and list(views) == list(params)
    off = flat.data_ptr()
    for n, p in params.items():
        assert views[n].shape == p.shape and views[n].is_contiguous() and views[n].data_ptr() == off, n
        off += 4 * p.numel()
    assert off == flat.data_ptr() + 4 * flat.numel()

    base = sweep.flatten_grads(model)
    clean, noise = torch.zeros(2, 3, 16, 16), torch.zeros(2, 3, 16, 16)
    sched = pkg('diffusion').DDPMScheduler()
    step = sweep.HipSweepStep(model, sched, clean, noise, clean.numel())
    assert step._flat_of_grads() is base and not base.any()
    G, name = step._G, list(params)[3]
    params[name].grad = torch.zeros_like(params[name])
    assert sweep.HipSweepStep(model, sched, clean, noise, clean.numel())._flat_of_grads() is None

    one, two = (sweep.Pipeline.another(step.eng, step._P, G, slot, clean.device) for slot in (1, 2))
    assert one.eng.packs is two.eng.packs is step.eng.packs and type(one.eng) is type(step.eng)
    assert (one.slot, one.eng.stream_slot, two.slot, two.eng.stream_slot) == (1, 1, 2, 2)
    assert one.stream is None and not one.started and not one['serial']
    assert one.eng.P is step._P and one.eng.G is one.G and [v.shape for v in one.G.values()] == [g.shape for g in G.values()]
    ends = sorted((b.data_ptr(), b.data_ptr() + 4 * b.numel()) for b in (base, one.flat, two.flat))
    assert all(a[1] <= b[0] for a, b in zip(ends, ends[1:]))
    assert all(one.G[n]._base is one.flat and two.G[n]._base is two.flat for n in G)


def test_prune_flow_on_mocked_kernels_matches_reference_masks(mocked, monkeypatch):
    """sweep -> TaylorImportance -> MagnitudePruner.step(interactive) -> group.prune() end to end (host logic +
    mocked kernels) reproduces the reference's masks for the tiny UNet."""
    sweep = pkg('sweep')
    monkeypatch.setattr(sweep.HipSweepStep, '__init__', _cpu_step_init)
    cfg = gc.TINY_CFG
    fx = load_json('tiny_prune.json')
    model = _cpu_model(cfg, 5)
    clean = torch.from_numpy(gc.det_clean((2, 3, 16, 16), 1))
    noise = torch.from_numpy(gc.det_noise((2, 3, 16, 16), 2))
    sweep.taylor_sweep(model, pkg('diffusion').DDPMScheduler(), clean, noise, num_steps=4)
    pr = sweep.prune_model(model, 0.3)
    assert [r[3] for r in pr.records] == [r['pruned'] for r in fx['prune']]
    assert {n: list(p.shape) for n, p in model.named_parameters()} == fx['shapes_after']
    # pruned model still runs forward + backward through the engine
    res = sweep.taylor_sweep(model, pkg('diffusion').DDPMScheduler(), clean, noise, num_steps=1)
    assert np.isfinite(res['losses'][0])


@pytest.mark.parametrize('crit', CRITERIA)
def test_sibling_criteria_flow_on_mocked_kernels(mocked, monkeypatch, crit):
    """The product's criterion classes (host logic + mocked reductions) reproduce the reference's masks."""
    sweep, pruning = pkg('sweep'), pkg('pruning')
    monkeypatch.setattr(sweep.HipSweepStep, '__init__', _cpu_step_init)
    cfg = gc.TINY_CFG
    fx = load_json('tiny_criteria.json')[crit]
    model = _cpu_model(cfg, 5)
    clean = torch.from_numpy(gc.det_clean((2, 3, 16, 16), 1))
    noise = torch.from_numpy(gc.det_noise((2, 3, 16, 16), 2))
    sweep.taylor_sweep(model, pkg('diffusion').DDPMScheduler(), clean, noise, num_steps=4)
    imp = dict(full1=lambda: pruning.FullTaylorImportance(order=1), full2=lambda: pruning.FullTaylorImportance(order=2),
               abs=pruning.AbsTaylorImportance, fisher=pruning.FisherImportance, magnitude=pruning.MagnitudeImportance)[crit]()
    pr = sweep.prune_model(model, 0.3, importance=imp)
    assert [r[3] for r in pr.records] == [_expand(g['pruned']) for g in fx['groups']]
    for r, g in zip(pr.records, fx['groups']):
        assert relerr(r[2], gc.b64_to_f32(g['score'])) < 2e-5, (crit, g['root'])
    assert sum(p.numel() for p in model.parameters()) == fx['params_after']


def test_ddpm_original_checkpoint_layout_matches_reference_twin():
    """Original-DDPM (`ddpm_exp/models/diffusion.py` Model) checkpoints: the key / shape table equals the reference class's,
    and the reference Model's forward on seeded weights equals the oracle UNet on the converted weights -- the independent
    twin implementation cross-checks both the converter and the UNet restatement."""
    from oracle import unet_ref as U
    ckpt, unet = pkg('checkpoint'), pkg('unet')
    fx = load_json('ddpm_original.json')
    want = load_npz('ddpm_original.npz')['out']
    c = fx['cfg']
    cfg = ckpt.unet2d_config_from_ddpm_original(c['ch'], c['ch_mult'], c['num_res_blocks'], c['attn_resolutions'], c['image_size'])
    # layout: our module's state dict, renamed to the original layout, has exactly the reference's keys and shapes
    ours = ckpt.convert_to_ddpm_original(unet.UNet2DModel(**cfg).state_dict())
    assert {k: list(v.shape) for k, v in ours.items()} == fx['shapes']
    # numerics: weights generated from the ORIGINAL names, converted, run through the oracle
    orig = {n: torch.from_numpy(gc.det_param(n, tuple(s), fx['seed'])) for n, s in fx['shapes'].items()}
    conv = ckpt.convert_ddpm_original(orig)
    assert {k: tuple(v.shape) for k, v in conv.items()} == {k: tuple(s) for k, s in U.param_shapes(cfg).items()}
    x = torch.from_numpy(gc.det_noise((2, 3, 16, 16), fx['input_seed']))
    with torch.no_grad():
        y = U.unet_forward(conv, cfg, x, torch.tensor(fx['timesteps']))
    assert float((y - torch.from_numpy(want)).abs().max()) < 2e-5
    back = ckpt.convert_to_ddpm_original(conv)
    assert all(torch.equal(back[k], orig[k]) for k in orig)


def test_ddpm_exp_sweep_flavour_matches_reference_twin(mocked, monkeypatch):
    """The ddpm_exp flavour of the Diff-Pruning sweep (ddpm_exp/prune.py:236-258: threshold test before backward, loss summed
    over C,H,W): oracle == the reference twin's recorded run (losses, stop step, gradient statistics), product == oracle."""
    from oracle import diffusion_ref as D
    ckpt, sweep = pkg('checkpoint'), pkg('sweep')
    fx = load_json('ddpm_original.json')
    sw, c = fx['sweep'], fx['cfg']
    cfg = ckpt.unet2d_config_from_ddpm_original(c['ch'], c['ch_mult'], c['num_res_blocks'], c['attn_resolutions'], c['image_size'])
    orig = {n: torch.from_numpy(gc.det_param(n, tuple(s), fx['seed'])) for n, s in fx['shapes'].items()}
    kmap = ckpt.ddpm_original_key_map(orig.keys())
    P = {k: v.clone().requires_grad_(True) for k, v in ckpt.convert_ddpm_original(orig).items()}
    clean = torch.from_numpy(gc.det_clean((2, 3, 16, 16), sw['clean_seed']))
    noise = torch.from_numpy(gc.det_noise((2, 3, 16, 16), sw['noise_seed']))
    losses = D.taylor_sweep(P, cfg, clean, noise, 1000, thr=sw['thr'], loss_kind='sum', accumulate_breaking_step=False)
    assert len(losses) == len(sw['losses']) and np.allclose(losses, sw['losses'], rtol=2e-5)
    for on, (s, a) in sw['grad_stats'].items():
        g = P[kmap[on]].grad.double()
        # biases in front of a one-channel-per-group GroupNorm (32 channels, 32 groups) have exactly zero gradient in exact
        # arithmetic: absolute floor (the summed loss is 768x the mean-squared one)
        assert abs(float(g.abs().sum()) - a) <= 5e-5 * a + 1e-5 * g.numel(), on
    # product control flow (host logic + mocked kernels)
    monkeypatch.setattr(sweep.HipSweepStep, '__init__', _cpu_step_init)
    model = pkg('unet').UNet2DModel(**cfg)
    model.load_state_dict({k: v.detach() for k, v in P.items()})
    res = sweep.taylor_sweep(model.eval(), pkg('diffusion').DDPMScheduler(), clean, noise, num_steps=1000, thr=sw['thr'],
                             loss_kind='sum', accumulate_breaking_step=False)
    assert res['steps'] == len(losses) and np.allclose(res['losses'], losses, rtol=1e-5)
    gmax = max(float(t.grad.abs().max()) for t in P.values())
    for n, p in model.named_parameters():
        if float(P[n].grad.abs().max()) > 1e-4 * gmax:          # skip the exactly-zero-in-theory bias gradients (noise)
            assert relerr(p.grad, P[n].grad) < 5e-5, n


def test_finetune_engine_control_flow_and_ema_swaps(mocked, monkeypatch):
    """FinetuneEngine (ddpm_train.py:453-469) on mocked kernels: two steps equal the oracle's loss / clip / Adam / EMA on the
    same data; EMAModel.store / copy_to / restore semantics (training_utils.py:220-262) around a checkpoint."""
    from oracle import diffusion_ref as D
    train = pkg('train')
    monkeypatch.setattr(train, '_require_hip_device', lambda dev: None)
    cfg = gc.TINY_CFG
    model = _cpu_model(cfg, 5)
    sched = pkg('diffusion').DDPMScheduler()
    monkeypatch.setattr(type(sched), '_acp_on', lambda self, dev: self.alphas_cumprod, raising=False)
    ft = train.FinetuneEngine(model, sched, lr=2e-4)
    names = [n for n, _ in model.named_parameters()]
    P = oracle_params(cfg, 5)
    plist = [P[n] for n in names]
    m = [torch.zeros_like(p) for p in plist]
    v = [torch.zeros_like(p) for p in plist]
    ema = [p.detach().clone() for p in plist]
    gen = torch.Generator().manual_seed(3)
    for step in range(2):
        clean = torch.from_numpy(gc.det_clean((2, 3, 16, 16), 10 + step))
        noise = torch.from_numpy(gc.det_noise((2, 3, 16, 16), 20 + step))
        t = train.antithetic_timesteps(2, 1000, gen)
        loss = ft.step(clean, noise, t)
        for p in plist:
            p.grad = None
        lo = D.finetune_loss(P, cfg, clean, noise, t)
        lo.backward()
        with torch.no_grad():
            D.adam_ema_step([p.data for p in plist], [p.grad for p in plist], m, v, ema, step + 1, lr=2e-4)
        assert abs(float(loss) - float(lo.detach())) <= 1e-5 * abs(float(lo.detach()))
    live = {n: p.detach().clone() for n, p in model.named_parameters()}
    for n, p in zip(names, plist):
        assert relerr(live[n], p.detach()) < 2e-4, n                  # Adam amplifies rounding on near-zero gradients
    es = ft.ema_state()
    for n, e in zip(names, ema):
        assert relerr(es[n], e) < 1e-5, n
    ft.ema_store(); ft.ema_copy_to()
    assert all(torch.equal(p.detach(), es[n]) for n, p in model.named_parameters())       # the module now holds the EMA weights
    ft.ema_restore()
    assert all(torch.equal(p.detach(), live[n]) for n, p in model.named_parameters())
    with pytest.raises(RuntimeError):
        ft.ema_restore()


def test_micro_batched_sweep_equals_full_shard(mocked, monkeypatch):
    """taylor_sweep(micro_batch=m): walking the shard in micro-batches inside every timestep gives the same losses and
    accumulated gradients (global loss scaling, fp32 re-association only) and the same early-exit step."""
    sweep = pkg('sweep')
    monkeypatch.setattr(sweep.HipSweepStep, '__init__', _cpu_step_init)
    cfg = gc.TINY_CFG
    clean = torch.from_numpy(gc.det_clean((3, 3, 16, 16), 1))
    noise = torch.from_numpy(gc.det_noise((3, 3, 16, 16), 2))
    sched = pkg('diffusion').DDPMScheduler()
    full, micro = _cpu_model(cfg, 5), _cpu_model(cfg, 5)
    r_full = sweep.taylor_sweep(full, sched, clean, noise, num_steps=1000, thr=0.99)
    r_micro = sweep.taylor_sweep(micro, sched, clean, noise, num_steps=1000, thr=0.99, micro_batch=2)   # chunks of 2 + 1
    assert r_full['steps'] == r_micro['steps'] and np.allclose(r_full['losses'], r_micro['losses'], rtol=1e-6)
    for (n, a), (_, b) in zip(full.named_parameters(), micro.named_parameters()):
        if a.grad.abs().max() > 1e-7:
            assert relerr(b.grad, a.grad) < 1e-5, n


def test_pruned_checkpoint_roundtrips(mocked, monkeypatch, tmp_path):
    """a pruned model chains into finetune / sampling three ways -- the replayable pruning history
    (dependency.py:278-293 format) + safetensors, the whole-module pickle of ddpm_prune.py:135, and a shape-aware load of a
    bare pruned state dict.  The recorded history equals the reference's pruned index lists."""
    sweep, pruning, ckpt = pkg('sweep'), pkg('pruning'), pkg('checkpoint')
    monkeypatch.setattr(sweep.HipSweepStep, '__init__', _cpu_step_init)
    cfg = gc.TINY_CFG
    fx = load_json('tiny_prune.json')
    model = _cpu_model(cfg, 5)
    clean = torch.from_numpy(gc.det_clean((2, 3, 16, 16), 1))
    noise = torch.from_numpy(gc.det_noise((2, 3, 16, 16), 2))
    sweep.taylor_sweep(model, pkg('diffusion').DDPMScheduler(), clean, noise, num_steps=4)
    pr = sweep.prune_model(model, 0.3)
    hist = pr.pruning_history()
    assert [h[0] for h in hist] == [r['root'] for r in fx['prune']] and all(h[1] for h in hist)
    assert [sorted(h[2]) for h in hist] == [r['pruned'] for r in fx['prune']]
    want = {k: v.clone() for k, v in model.state_dict().items()}

    # 1. safetensors + JSON with the history
    meta = ckpt.save_pruned(model, str(tmp_path / 'pruned'), hist)
    assert meta['num_parameters'] == fx['params_after']
    m1 = ckpt.load_pruned(str(tmp_path / 'pruned'))
    assert {k: list(v.shape) for k, v in m1.state_dict().items()} == fx['shapes_after']
    assert all(torch.equal(v, want[k]) for k, v in m1.state_dict().items())
    assert all(u.conv.in_channels == u.channels for u in m1.modules() if hasattr(u, 'channels') and hasattr(u, 'conv'))

    # 2. whole-module pickle (the engine is not part of it)
    model.engine()                                              # make sure an engine object exists before pickling
    torch.save(model, str(tmp_path / 'unet_pruned.pth'))
    m2 = torch.load(str(tmp_path / 'unet_pruned.pth'), weights_only=False)
    assert m2._engine is None and all(torch.equal(v, want[k]) for k, v in m2.state_dict().items())
    res = sweep.taylor_sweep(m2, pkg('diffusion').DDPMScheduler(), clean, noise, num_steps=1)     # still runs
    assert np.isfinite(res['losses'][0])

    # 3. bare pruned state dict onto a fresh un-pruned module
    m3 = ckpt.adopt_state_dict(_cpu_model(cfg, 7), want)
    assert all(torch.equal(v, want[k]) for k, v in m3.state_dict().items())
    assert m3.conv_norm_out.num_channels == want['conv_norm_out.weight'].shape[0]
    # an inconsistent dict (one conv with a foreign width) is rejected
    bad = dict(want)
    k = 'mid_block.resnets.0.conv1.weight'
    bad[k] = bad[k][:-1]
    bad['mid_block.resnets.0.conv1.bias'] = bad['mid_block.resnets.0.conv1.bias'][:-1]
    with pytest.raises((ValueError, RuntimeError)):
        ckpt.adopt_state_dict(_cpu_model(cfg, 7), bad)

    # replay on a fresh model through the pruner surface (metapruner.py:138)
    m4 = _cpu_model(cfg, 5)
    p4 = pruning.MagnitudePruner(m4, None, importance=pruning.TaylorImportance(), ch_sparsity=0.3, ignored_layers=[m4.conv_out])
    p4.load_pruning_history(hist)
    assert {k: list(v.shape) for k, v in m4.state_dict().items()} == fx['shapes_after']


# ------------------------------------------------------------------------------------------------ LDM (row a17)
def test_ldm_oracle_matches_reference_unet():
    """oracle/ldm_ref.py vs the reference's own UNetModel (fixtures from make_golden_ldm.py): bit-exact forward, loss and
    gradients on the reduced-width config; full cin256-v2 parameter table (400 920 579 parameters)."""
    from oracle import ldm_ref as L
    cfg = gc.LDM_TINY_CFG
    fx = load_json('ldm_unet_stats.json')
    S = L.ldm_param_shapes(cfg)
    assert {n: list(s) for n, s in S.items()} == fx['shapes']
    SF = L.ldm_param_shapes(gc.LDM_CIN256_CFG)
    assert {n: list(s) for n, s in SF.items()} == fx['cin256_shapes']
    assert sum(int(np.prod(s)) for s in SF.values()) == fx['cin256_params'] == 400920579
    P = {n: torch.from_numpy(gc.det_param(n, s, 9)).requires_grad_(True) for n, s in S.items()}
    g = load_npz('ldm_unet.npz')
    x, ctx, noise, t = _ldm_inputs()
    y = L.ldm_unet_forward(P, cfg, x, t, ctx)
    assert float((y.detach() - torch.from_numpy(g['fwd_out'])).abs().max()) < 1e-6
    loss = (y - noise).square().mean(dim=(1, 2, 3)).mean()
    loss.backward()
    assert abs(float(loss.detach()) - float(g['loss'])) < 1e-6
    for k in g.files:
        if k.startswith('grad::'):
            assert relerr(P[k[6:]].grad, g[k]) < 1e-5 or float(np.abs(g[k]).max()) == 0.0, k
    for n, (s, a) in fx['grad_stats'].items():
        assert abs(float(P[n].grad.double().abs().sum()) - a) <= 2e-5 * a + 1e-8 * P[n].numel(), n


def _ldm_inputs():
    x = torch.from_numpy(gc.det_noise((2, 3, 16, 16), 31))
    ctx = torch.from_numpy(gc.det_noise((2, 1, 16), 32))
    noise = torch.from_numpy(gc.det_noise((2, 3, 16, 16), 33))
    return x, ctx, noise, torch.tensor([7, 640])


def test_ldm_engine_backward_graph_matches_oracle(mocked, monkeypatch):
    """LdmEngine's hand-written backward (SpatialTransformer incl. the single-token cross-attention shortcut, GEGLU,
    LayerNorm, skip routing) vs autograd of the oracle, kernels replaced by CPU stand-ins."""
    from oracle import ldm_ref as L
    ldm = pkg('ldm')
    monkeypatch.setattr(ldm, 'ops', mocked)
    cfg = gc.LDM_TINY_CFG
    model = ldm.UNetModel(**cfg)
    gc.det_init_(model, 9)
    state_names = [n for n, _ in model.named_parameters()]
    assert set(state_names) == set(L.ldm_param_shapes(cfg))
    eng = ldm.LdmEngine(model.config)
    grads = {n: torch.zeros_like(p) for n, p in model.named_parameters()}
    eng.bind({n: p.detach() for n, p in model.named_parameters()}, grads)
    x, ctx, noise, t = _ldm_inputs()
    y = eng.forward(x, t, ctx, save=True)
    n = y.numel()
    loss, dout = mocked.mse_fwd_bwd(y, noise, 2.0 / n, 1.0 / n)
    eng.backward(dout)
    P = {k: torch.from_numpy(gc.det_param(k, s, 9)).requires_grad_(True) for k, s in L.ldm_param_shapes(cfg).items()}
    yo = L.ldm_unet_forward(P, cfg, x, t, ctx)
    lo = (yo - noise).square().mean(dim=(1, 2, 3)).mean()
    lo.backward()
    assert float((y - yo.detach()).abs().max()) < 1e-5
    assert abs(float(loss) - float(lo.detach())) < 1e-6
    for k in P:
        ref = P[k].grad
        if float(ref.abs().max()) > 1e-7:
            assert relerr(grads[k], ref) < 5e-5, k
        else:
            assert float(grads[k].abs().max()) < 1e-6, k        # norm2 / attn2.to_q / attn2.to_k: exactly zero


@pytest.mark.parametrize('L_ctx', [3, 5])
def test_ldm_engine_general_cross_attention_matches_oracle(mocked, monkeypatch, L_ctx):
    """Round 5: cross-attention over L > 1 context tokens (ldm/modules/attention.py:152-193 takes any context; the configurations
    the reference prunes pass ONE class token, for which the engine keeps its closed form).  LdmEngine's general attn2 -- context
    as channel-major tokens, K / V 1x1 projections, the three attention launches, norm2 / to_q / to_k now with gradients --
    against autograd of the oracle (whose cross_attention is the reference's einsum form, pinned bit-identical to the reference's
    UNetModel for L = 1), kernels replaced by CPU stand-ins: forward, loss and every parameter gradient; then a no-grad CFG pair
    (shared stem) and the context cache of a sampling loop against the plain forward."""
    from oracle import ldm_ref as L
    ldm = pkg('ldm')
    monkeypatch.setattr(ldm, 'ops', mocked)
    cfg = gc.LDM_TINY_CFG
    model = ldm.UNetModel(**cfg)
    gc.det_init_(model, 9)
    eng = ldm.LdmEngine(model.config)
    grads = {n: torch.zeros_like(p) for n, p in model.named_parameters()}
    eng.bind({n: p.detach() for n, p in model.named_parameters()}, grads)
    x, ctx1, noise, t = _ldm_inputs()
    ctx = torch.from_numpy(gc.det_noise((x.shape[0], L_ctx, ctx1.shape[2]), 123))
    y = eng.forward(x, t, ctx, save=True)
    n = y.numel()
    loss, dout = mocked.mse_fwd_bwd(y, noise, 2.0 / n, 1.0 / n)
    eng.backward(dout)
    P = {k: torch.from_numpy(gc.det_param(k, s, 9)).requires_grad_(True) for k, s in L.ldm_param_shapes(cfg).items()}
    yo = L.ldm_unet_forward(P, cfg, x, t, ctx)
    lo = (yo - noise).square().mean(dim=(1, 2, 3)).mean()
    lo.backward()
    assert float((y - yo.detach()).abs().max()) < 1e-5
    assert abs(float(loss) - float(lo.detach())) < 1e-6
    nonzero = 0
    for k in P:
        ref = P[k].grad
        if float(ref.abs().max()) > 1e-7:
            assert relerr(grads[k], ref) < 5e-5, k
            nonzero += ('attn2.to_q' in k or 'attn2.to_k' in k or '.norm2.' in k)
        else:
            assert float(grads[k].abs().max()) < 1e-6, k
    assert nonzero > 0                                  # with L > 1 keys the softmax is not constant any more
    # CFG pair (the context-free stem evaluated once) and the per-sampling-loop context cache == two plain forwards
    ctx2 = torch.cat([torch.from_numpy(gc.det_noise(tuple(ctx.shape), 124)), ctx])
    plain = eng.forward(torch.cat([x, x]), torch.cat([t, t]), ctx2, save=False)
    with eng.context_cache(ctx2):
        pair_a = eng.forward(x, t, ctx2, save=False, cfg_pair=True)
        pair_b = eng.forward(x, t, ctx2, save=False, cfg_pair=True)          # second call: K / V of every block from the cache
    assert float((pair_a - plain).abs().max()) < 1e-5 and torch.equal(pair_a, pair_b)


def _ldm_sweep_fixture(steps=3, n=2):
    emb_w = torch.from_numpy(gc.det_noise((1001, 16), 77))
    rng = np.random.default_rng(5)
    draws = []
    for t in range(steps):
        xc = torch.tensor(rng.choice(1000, size=n, replace=False))
        draws.append((xc, torch.from_numpy(gc.det_noise((n, 3, 16, 16), 300 + t)),
                      torch.from_numpy(gc.det_noise((n, 3, 16, 16), 400 + t))))
    return emb_w, draws


def _ldm_oracle_sweep(cfg, emb_w, draws, S, thr):
    from oracle import ldm_ref as L
    P = {k: torch.from_numpy(gc.det_param(k, s, 9)).requires_grad_(True) for k, s in L.ldm_param_shapes(cfg).items()}
    acp = L.ldm_alphas_cumprod()
    n = draws[0][0].shape[0]
    uc = emb_w[torch.tensor(n * [1000])][:, None, :]
    losses, max_loss = [], -1.0
    for t, (xc, x_T, noise) in enumerate(draws):
        c = emb_w[xc][:, None, :]
        Pd = {k: v.detach() for k, v in P.items()}
        x0 = L.ddim_sample_cfg(Pd, cfg, acp, x_T, c, uc, S=S, scale=3.0)
        loss = L.ldm_loss_at_t(P, cfg, acp, x0, torch.full((n,), t, dtype=torch.long), c, noise)
        lv = float(loss.detach())
        losses.append(lv)
        max_loss = max(max_loss, lv)
        if thr is not None and lv / max_loss < thr:
            break
        loss.backward()
    return P, losses


def test_ldm_importance_sweep_control_flow_matches_oracle(mocked, monkeypatch):
    """prune_ldm.py:101-131 driver (CFG DDIM sampling -> loss at t -> break-before-backward) on mocked kernels."""
    ldm, ldm_sweep, sweep = pkg('ldm'), pkg('ldm_sweep'), pkg('sweep')
    for m in (ldm, ldm_sweep):
        monkeypatch.setattr(m, 'ops', mocked)

    def cpu_engine(self):
        if self._engine is None:
            self._engine = ldm.LdmEngine(self.config)
        self._engine.bind({n: p.detach() for n, p in self.named_parameters()}, None)
        return self._engine
    monkeypatch.setattr(ldm.UNetModel, 'engine', cpu_engine)
    cfg = gc.LDM_TINY_CFG
    emb_w, draws = _ldm_sweep_fixture()
    # thr 1.5: loss/max_loss = 1 < 1.5 at t = 0 -> break, nothing accumulated; pipelines 2: odd steps on a second engine + buffer
    for thr, expect_steps, pipelines in ((None, 3, 1), (1.5, 1, 1), (None, 3, 2), (1.5, 1, 2)):
        model = ldm.UNetModel(**cfg)
        gc.det_init_(model, 9)
        embedder = ldm_sweep.ClassEmbedder(16, 1001)
        with torch.no_grad():
            embedder.embedding.weight.copy_(emb_w)
        res = ldm_sweep.ldm_importance_sweep(model, embedder, num_steps=3, thr=thr, n_samples=2, ddim_steps=4, pipelines=pipelines,
                                             latent_shape=(3, 16, 16), draws=lambda t: draws[min(t, 2)])
        P, losses = _ldm_oracle_sweep(cfg, emb_w, draws, 4, thr)
        assert res['steps'] == len(losses) == expect_steps
        assert np.allclose(res['losses'], losses, rtol=2e-5)
        if thr is None:
            for k, p in model.named_parameters():
                ref = P[k].grad
                if float(ref.abs().max()) > 1e-7:
                    assert relerr(p.grad, ref) < 1e-4, k
        else:
            assert res['accumulated'] == 0 and float(res['flat_grads'].abs().max()) == 0.0


def test_ldm_sampler_matches_reference_ddim_sampler():
    """The CFG DDIM sampler of the LDM importance pass and its noise schedule against the reference's own DDIMSampler
    (ldm/models/diffusion/ddim.py:57-203) run over the reference UNetModel: schedule tables exact to fp64 rounding, 20-step
    guided sample within fp32 accumulation."""
    from oracle import ldm_ref as R
    g = load_npz('ldm_sampler.npz')
    cfg = gc.LDM_TINY_CFG
    acp = R.ldm_alphas_cumprod()
    assert np.allclose(np.asarray(acp, dtype=np.float64), g['alphas_cumprod'], rtol=1e-12, atol=0)
    steps, a, a_prev, sig = R.ddim_schedule(acp, 20)
    assert [int(s) for s in steps] == [int(s) for s in g['ddim_timesteps']]
    assert np.allclose(np.asarray(a, dtype=np.float64), g['ddim_alphas'], rtol=1e-6)
    P = {n: torch.from_numpy(gc.det_param(n, s, 9)) for n, s in R.ldm_param_shapes(cfg).items()}
    H = cfg['image_size']
    x_T = torch.from_numpy(gc.det_noise((2, cfg['in_channels'], H, H), 51))
    cond = torch.from_numpy(gc.det_noise((2, 1, cfg['context_dim']), 52))
    uncond = torch.from_numpy(gc.det_noise((2, 1, cfg['context_dim']), 53))
    with torch.no_grad():
        x = R.ddim_sample_cfg(P, cfg, acp, x_T, cond, uncond, S=20, scale=3.0)
    assert relerr(x, torch.from_numpy(g['samples'])) < 2e-4


def test_ldm_group_enumeration_matches_reference():
    from oracle import ldm_ref as L
    G = pkg('graph')
    cfg = gc.LDM_TINY_CFG
    table = load_json('ldm_groups.json')['tiny']
    shapes = L.ldm_param_shapes(cfg)
    groups = list(G.all_groups(G.LdmGraph(cfg), lambda: G.ChannelView(shapes), ('out', 'out.0', 'out.1', 'out.2')))
    assert len(groups) == len(table) == 109
    for ref, (root, mem) in zip(table, groups):
        assert ref['members'][0][0] == root
        assert {(m[0], m[1]): gc.expand(m[2]) for m in ref['members']} == {(m.name, m.kind): m.idxs for m in mem}, root


@pytest.mark.parametrize('variant', ['small_2lvl', 'deep_3lvl'])
def test_ldm_group_enumeration_other_configs(variant):
    """LdmGraph over other members of the LDM UNet family (depths, widths, attention levels, res-block counts)."""
    from oracle import ldm_ref as L
    G = pkg('graph')
    cfgs = {'small_2lvl': dict(gc.LDM_TINY_CFG, image_size=8, model_channels=32, channel_mult=[1, 2],
                               attention_resolutions=[1, 2], num_res_blocks=1),
            'deep_3lvl': dict(gc.LDM_TINY_CFG, image_size=16, model_channels=32, channel_mult=[1, 1, 3],
                              attention_resolutions=[4], num_res_blocks=3)}
    cfg = cfgs[variant]
    table = load_json('ldm_groups_more.json')[variant]
    shapes = L.ldm_param_shapes(cfg)
    groups = list(G.all_groups(G.LdmGraph(cfg), lambda: G.ChannelView(shapes), ('out', 'out.0', 'out.1', 'out.2')))
    assert len(groups) == len(table)
    for ref, (root, mem) in zip(table, groups):
        assert ref['members'][0][0] == root
        assert {(m[0], m[1]): gc.expand(m[2]) for m in ref['members']} == {(m.name, m.kind): m.idxs for m in mem}, root


def _ldm_grads_oracle():
    from oracle import ldm_ref as L
    cfg = gc.LDM_TINY_CFG
    P = {k: torch.from_numpy(gc.det_param(k, s, 9)).requires_grad_(True) for k, s in L.ldm_param_shapes(cfg).items()}
    x, ctx, noise, t = _ldm_inputs()
    loss = (L.ldm_unet_forward(P, cfg, x, t, ctx) - noise).square().mean(dim=(1, 2, 3)).mean()
    loss.backward()
    return cfg, P


def test_ldm_oracle_prune_masks_match_reference():
    """Vendored Taylor scores + masks (ratio 0.3, round_to 2, GEGLU split coupling, LayerNorm members) for the LDM UNet."""
    from oracle import ldm_ref as L
    G = pkg('graph')
    cfg, P = _ldm_grads_oracle()
    fx = load_json('ldm_prune.json')
    Pd = {n: p.detach().clone() for n, p in P.items()}
    Gd = {n: p.grad.clone() for n, p in P.items()}
    rec = oracle_prune_replay(Pd, Gd, cfg, 0.3, G, graph=G.LdmGraph(cfg), ignored=('out', 'out.0', 'out.1', 'out.2'),
                              gn_groups=32, round_to=2)
    ref_nonempty = [r for r in fx['prune'] if r['pruned']]      # GN groups of 32 channels prune 10 // 32 = 0 per sub-group
    assert len(rec) == len(ref_nonempty)
    for mine, ref in zip(rec, ref_nonempty):
        assert mine['root'] == ref['root'] and mine['ch_groups'] == ref['ch_groups'], (mine['root'], ref['root'])
        assert relerr(mine['score'], gc.b64_to_f32(ref['score'])) < 1e-5, ref['root']
        assert mine['pruned'] == ref['pruned'], (ref['root'], mine['margin'])
    assert {n: list(t.shape) for n, t in Pd.items()} == fx['shapes_after']
    x, ctx, noise, t = _ldm_inputs()
    with torch.no_grad():
        y2 = L.ldm_unet_forward(Pd, cfg, x, t, ctx)
    assert float((y2 - torch.from_numpy(gc.b64_to_f32(fx['fwd_after']))).abs().max()) < 1e-5


def test_ldm_prune_flow_on_mocked_kernels(mocked, monkeypatch):
    """MagnitudePruner(round_to=2, head channel_groups) on the product's LDM UNetModel reproduces the reference masks."""
    ldm, pruning = pkg('ldm'), pkg('pruning')
    cfg, P = _ldm_grads_oracle()
    fx = load_json('ldm_prune.json')
    model = ldm.UNetModel(**cfg)
    gc.det_init_(model, 9)
    for n, p in model.named_parameters():
        p.grad = P[n].grad.clone()
    channel_groups = {}
    for m in model.modules():
        if isinstance(m, ldm.CrossAttention):
            channel_groups[m.to_q] = channel_groups[m.to_k] = channel_groups[m.to_v] = m.heads
    pr = pruning.MagnitudePruner(model, None, importance=pruning.TaylorImportance(), iterative_steps=1,
                                 channel_groups=channel_groups, ch_sparsity=0.3, ignored_layers=[model.out], round_to=2)
    for g in pr.step(interactive=True):
        g.prune()
    assert [r[0] for r in pr.records] == [r['root'] for r in fx['prune']]
    assert [r[3] for r in pr.records] == [r['pruned'] for r in fx['prune']]
    assert {n: list(p.shape) for n, p in model.named_parameters()} == fx['shapes_after']
    assert sum(p.numel() for p in model.parameters()) == fx['params_after']
    # the pruned LDM UNet survives the pickle-free checkpoint (history replay over the LDM coupling graph, GEGLU / head
    # groups included) and the shape-aware load of its bare state dict
    import tempfile
    ckpt = pkg('checkpoint')
    with tempfile.TemporaryDirectory() as d:
        ckpt.save_pruned(model, d, pr.pruning_history())
        back = ckpt.load_pruned(d)
    sd = model.state_dict()
    assert all(torch.equal(v, sd[k]) for k, v in back.state_dict().items()) and len(back.state_dict()) == len(sd)
    fresh = ldm.UNetModel(**cfg)
    ckpt.adopt_state_dict(fresh, sd)
    assert {n: list(p.shape) for n, p in fresh.named_parameters()} == fx['shapes_after']


def _ldm_heads_case(tag):
    from oracle import ldm_ref as L
    rec = load_json('ldm_heads.json')[tag]
    cfg = rec['cfg']
    S = L.ldm_param_shapes(cfg)
    P = {n: torch.from_numpy(gc.det_param(n, s, 9)).requires_grad_(True) for n, s in S.items()}
    x = torch.from_numpy(gc.det_noise((2, 3, 16, 16), 31))
    ctx = torch.from_numpy(gc.det_noise((2, rec['context_tokens'], cfg['context_dim']), 32))
    noise = torch.from_numpy(gc.det_noise((2, 3, 16, 16), 33))
    return rec, cfg, S, P, (x, ctx, noise, torch.tensor([7, 640]))


@pytest.mark.parametrize('tag', ['h2d2', 'hc16_L3'])
def test_ldm_multi_head_and_depth_oracle_matches_reference(tag):
    """Round 6: the LDM UNet family beyond cin256-v2 -- `num_heads` > 1 / `num_head_channels` (openaimodel.py:542-549; heads split as
    'b n (h d) -> (b h) n d', attention.py:177) and `transformer_depth` > 1 (attention.py:253-254) -- oracle/ldm_ref.py against the
    reference's own UNetModel (make_golden_ldm.py heads): parameter table, forward, loss, gradients, and the group table of the
    product's LdmGraph against the vendored torch_pruning's (with its head channel groups)."""
    from oracle import ldm_ref as L
    G = pkg('graph')
    rec, cfg, S, P, (x, ctx, noise, t) = _ldm_heads_case(tag)
    g = load_npz('ldm_heads.npz')
    assert {n: list(s) for n, s in S.items()} == rec['shapes']
    y = L.ldm_unet_forward(P, cfg, x, t, ctx)
    assert float((y.detach() - torch.from_numpy(g[tag + '::fwd_out'])).abs().max()) < 1e-6
    loss = (y - noise).square().mean(dim=(1, 2, 3)).mean()
    loss.backward()
    assert abs(float(loss.detach()) - float(g[tag + '::loss'])) < 1e-6
    n_full = 0
    for k in g.files:
        if k.startswith(tag + '::grad::'):
            ref = g[k]
            assert relerr(P[k.split('::grad::')[1]].grad, ref) < 1e-5 or float(np.abs(ref).max()) == 0.0, k
            n_full += 1
    assert n_full == 9
    for n, (s_, a) in rec['grad_stats'].items():
        assert abs(float(P[n].grad.double().abs().sum()) - a) <= 2e-5 * a + 1e-8 * P[n].numel(), n
    groups = list(G.all_groups(G.LdmGraph(cfg), lambda: G.ChannelView(S), ('out', 'out.0', 'out.1', 'out.2')))
    assert len(groups) == len(rec['groups'])
    heads = {n: h for n, h in rec['heads'].items()}
    for ref, (root, mem) in zip(rec['groups'], groups):
        assert ref['members'][0][0] == root
        assert {(m[0], m[1]): gc.expand(m[2]) for m in ref['members']} == {(m.name, m.kind): m.idxs for m in mem}, root
        # the reference's channel groups: 32 for groups with a GroupNorm member, the head count for to_q / to_k / to_v groups
        mine = 32 if any(m.kind == 'gn' for m in mem) else next((heads[m.name.rsplit('.', 1)[0]] for m in mem
                                                                  if m.name.rsplit('.', 1)[-1] in ('to_q', 'to_k', 'to_v')), 1)
        assert mine == ref['ch_groups'], root


@pytest.mark.parametrize('tag', ['h2d2', 'hc16_L3'])
def test_ldm_multi_head_prune_masks_match_reference(tag, mocked):
    """Vendored Taylor scores + masks with head channel groups (prune_ldm.py:78-82: every head loses the same number of its own
    lowest-scored channels) for the multi-head / deeper LDM UNets: the oracle's arithmetic over the oracle's gradients, then the
    product's MagnitudePruner on the product's UNetModel (mocked kernels) -- records, shapes and parameter count after."""
    from oracle import ldm_ref as L
    G = pkg('graph')
    ldm, pruning = pkg('ldm'), pkg('pruning')
    rec, cfg, S, P, (x, ctx, noise, t) = _ldm_heads_case(tag)
    g = load_npz('ldm_heads.npz')
    loss = (L.ldm_unet_forward(P, cfg, x, t, ctx) - noise).square().mean(dim=(1, 2, 3)).mean()
    loss.backward()
    Pd = {n: p.detach().clone() for n, p in P.items()}
    Gd = {n: p.grad.clone() for n, p in P.items()}
    cg = {a + s_: h for a, h in rec['heads'].items() for s_ in ('.to_q', '.to_k', '.to_v')}
    mine = oracle_prune_replay(Pd, Gd, cfg, 0.3, G, graph=G.LdmGraph(cfg), ignored=('out', 'out.0', 'out.1', 'out.2'),
                               gn_groups=32, round_to=2, channel_groups=cg)
    ref_nonempty = [r for r in rec['prune'] if r['pruned']]
    assert len(mine) == len(ref_nonempty) and any(r['ch_groups'] not in (1, 32) for r in ref_nonempty)
    for a, ref in zip(mine, ref_nonempty):
        assert a['root'] == ref['root'] and a['ch_groups'] == ref['ch_groups'], (a['root'], ref['root'])
        assert relerr(a['score'], gc.b64_to_f32(ref['score'])) < 1e-5, ref['root']
        assert a['pruned'] == ref['pruned'], (ref['root'], a['margin'])
    assert {n: list(t_.shape) for n, t_ in Pd.items()} == rec['shapes_after']
    with torch.no_grad():
        y2 = L.ldm_unet_forward(Pd, cfg, x, t, ctx)
    assert float((y2 - torch.from_numpy(g[tag + '::fwd_after'])).abs().max()) < 1e-5
    # the product's pruner over the product's model
    model = ldm.UNetModel(**cfg)
    gc.det_init_(model, 9)
    assert {n: list(p.shape) for n, p in model.named_parameters()} == rec['shapes']
    for n, p in model.named_parameters():
        p.grad = P[n].grad.clone()
    channel_groups = {}
    for name, m in model.named_modules():
        if isinstance(m, ldm.CrossAttention):
            assert m.heads == rec['heads'][name]
            channel_groups[m.to_q] = channel_groups[m.to_k] = channel_groups[m.to_v] = m.heads
    pr = pruning.MagnitudePruner(model, None, importance=pruning.TaylorImportance(), iterative_steps=1,
                                 channel_groups=channel_groups, ch_sparsity=0.3, ignored_layers=[model.out], round_to=2)
    for grp in pr.step(interactive=True):
        grp.prune()
    assert [r[0] for r in pr.records] == [r['root'] for r in rec['prune']]
    assert [r[1] for r in pr.records] == [r['ch_groups'] for r in rec['prune']]
    assert [r[3] for r in pr.records] == [r['pruned'] for r in rec['prune']]
    assert {n: list(p.shape) for n, p in model.named_parameters()} == rec['shapes_after']
    assert sum(p.numel() for p in model.parameters()) == rec['params_after']
    # the pruned multi-head / deeper model survives the pickle-free checkpoint (config incl. num_head_channels / transformer_depth,
    # history replay with the head channel groups)
    import tempfile
    ckpt = pkg('checkpoint')
    with tempfile.TemporaryDirectory() as d:
        ckpt.save_pruned(model, d, pr.pruning_history())
        back = ckpt.load_pruned(d)
    sd = model.state_dict()
    assert all(torch.equal(v, sd[k]) for k, v in back.state_dict().items()) and len(back.state_dict()) == len(sd)
    assert back.config['transformer_depth'] == cfg.get('transformer_depth', 1)
    assert [m.heads for m in back.modules() if isinstance(m, ldm.CrossAttention)] == [m.heads for m in model.modules() if isinstance(m, ldm.CrossAttention)]


# ------------------------------------------------------------------------------------------------------------------
# round 2: dropout masks, LR schedules, DDPM ancestral sampling, long accumulation, torch_pruning-shaped groups
# ------------------------------------------------------------------------------------------------------------------
def test_philox_known_answers():
    """oracle/philox_ref.py against the published known-answer vectors of Philox4x32-10 (Random123 kat_vectors)."""
    from oracle import philox_ref as PH
    kat = [((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
           ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
           ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
            (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))]
    for ctr, key, want in kat:
        assert tuple(int(x) for x in PH.philox4x32_10(*ctr, *key)) == want
    m = PH.dropout_multipliers(1 << 16, 0.1, 5, 'down_blocks.0.resnets.0.dropout', 2)
    assert set(np.unique(m)) == {np.float32(0.0), np.float32(1.0 / 0.9)}
    assert abs(float((m == 0).mean()) - 0.1) < 0.01
    # a window of the same stream equals the stream restricted to the window (element-indexed, not draw-ordered)
    w = PH.dropout_multipliers(1000, 0.1, 5, 'down_blocks.0.resnets.0.dropout', 2, idx0=4321)
    assert np.array_equal(w, m[4321:5321])


def test_lr_schedules_match_reference():
    """train.get_scheduler vs diffusers/optimization.py:282 (values recorded from the reference with a torch optimizer)."""
    train = pkg('train')
    fx = load_json('lr_schedules.json')
    for name, case in fx['cases'].items():
        if name == 'piecewise_constant':
            with pytest.raises(TypeError):                         # optimization.py:321 (reference behaviour)
                train.get_scheduler(name, fx['base_lr'], **case['kwargs'])
            sch = train.get_piecewise_constant_schedule(fx['base_lr'], **case['kwargs'])
        else:
            sch = train.get_scheduler(name, fx['base_lr'], **case['kwargs'])
        got = []
        for _ in case['lrs']:
            got.append(sch.get_last_lr()[0])
            sch.step()
        assert np.allclose(got, case['lrs'], rtol=1e-12, atol=0), name
    with pytest.raises(ValueError):
        train.get_scheduler('cosine', 1e-4)                        # needs num_warmup_steps
    with pytest.raises(ValueError):
        train.get_scheduler('nope', 1e-4)


def test_oracle_and_scheduler_ddpm_steps_match_reference(mocked):
    """DDPMScheduler.step / set_timesteps / DDPMPipeline (scheduling_ddpm.py:185-236,312-406; pipeline_ddpm.py:24-105):
    the oracle restatement and the product's host logic (on mocked kernels) against sequences recorded from the reference."""
    from oracle import diffusion_ref as D, unet_ref as U
    diffusion = pkg('diffusion')
    g = load_npz('ddpm.npz')
    cfg = gc.TINY_CFG
    P = oracle_params(cfg, 5, requires_grad=False)
    acp = D.alphas_cumprod()
    model = _cpu_model(cfg, 5)
    for tag, n_inf, vt in (('full', 1000, 'fixed_small'), ('s50', 50, 'fixed_small'), ('large', 50, 'fixed_large')):
        assert np.array_equal(D.ddpm_timesteps(n_inf).numpy(), g['timesteps_' + tag])
        sch = diffusion.DDPMScheduler(variance_type=vt)
        sch.set_timesteps(n_inf)
        assert np.array_equal(sch.timesteps.numpy(), g['timesteps_' + tag])
        gen_o, gen_p = torch.Generator().manual_seed(123), torch.Generator().manual_seed(123)
        xo = xp = torch.from_numpy(gc.det_noise((2, 3, 16, 16), 23))
        with torch.no_grad():
            for i, t in enumerate(sch.timesteps[:4]):
                noise = torch.randn(xo.shape, generator=gen_o)
                xo = D.ddpm_step(acp, U.unet_forward(P, cfg, xo, t), t, xo, n_inf, variance_noise=noise, variance_type=vt)
                xp = sch.step(model(xp, t).sample, t, xp, generator=gen_p).prev_sample
                ref = torch.from_numpy(g['x_' + tag][i])
                assert float((xo - ref).abs().max()) < 5e-5, (tag, i)
                assert float((xp - ref).abs().max()) < 5e-5, (tag, i)
    x = torch.from_numpy(gc.det_noise((2, 3, 16, 16), 24))
    sch = diffusion.DDPMScheduler()
    with torch.no_grad():
        y = sch.step(model(x, 0).sample, 0, x, generator=torch.Generator().manual_seed(5)).prev_sample
    assert float((y - torch.from_numpy(g['x_t0'])).abs().max()) < 5e-5              # t = 0: no noise is added
    pipe = diffusion.DDPMPipeline(model, diffusion.DDPMScheduler())
    img = pipe(batch_size=2, generator=torch.Generator().manual_seed(9), num_inference_steps=6, output_type='numpy').images
    assert img.shape == (2, 16, 16, 3) and float(np.abs(img - g['pipe6']).max()) < 2e-4


def test_dropout_placement_and_masks_match_reference(mocked, monkeypatch):
    """Training-mode forward/backward with dropout 0.1 on every nn.Dropout (utils.set_dropout): the oracle (Philox masks applied
    at resnet.py:628 and attention_processor.py:457) and the product's engine on mocked kernels against the reference
    UNet2DModel run with the same masks (tests/golden/tiny_dropout.json)."""
    from oracle import diffusion_ref as D, philox_ref as PH
    train = pkg('train')
    fx = load_json('tiny_dropout.json')
    cfg = gc.TINY_CFG
    model = _cpu_model(cfg, 5)
    train.set_dropout(model, fx['p'])
    table = model.dropout_table()
    assert len(table) == fx['sites'] and all(n.endswith('.dropout') or n.endswith('.to_out.1') for n in table)
    clean = torch.from_numpy(gc.det_clean((4, 3, 16, 16), 3))
    noise = torch.from_numpy(gc.det_noise((4, 3, 16, 16), 4))
    t = torch.tensor([1, 250, 500, 998])
    P = oracle_params(cfg, 5)
    lo = D.finetune_loss(P, cfg, clean, noise, t, PH.DropSpec(table, fx['seed'], fx['step'], 0))
    lo.backward()
    assert abs(float(lo.detach()) - fx['loss']) <= 1e-5 * fx['loss']
    for n, (s, a, q) in fx['grad_stats'].items():
        gr = P[n].grad.double()
        assert abs(float(gr.abs().sum()) - a) <= 2e-5 * a + 1e-8 * gr.numel(), n
    # product engine (mocked kernels): same loss and gradients through FinetuneEngine's forward/backward
    monkeypatch.setattr(train, '_require_hip_device', lambda dev: None)
    sched = pkg('diffusion').DDPMScheduler()
    monkeypatch.setattr(type(sched), '_acp_on', lambda self, dev: self.alphas_cumprod, raising=False)
    ft = train.FinetuneEngine(model, sched, lr=0.0, dropout_seed=fx['seed'])
    ft.step_count = fx['step'] - 1                                 # the engine draws the masks of step_count + 1
    loss = ft.step(clean, noise, t)
    assert abs(float(loss) - fx['loss']) <= 1e-5 * fx['loss']
    for n, p in model.named_parameters():
        if float(P[n].grad.abs().max()) > 1e-6:
            assert relerr(p.grad, P[n].grad) < 5e-5, n
    # eval mode: no dropout
    model.eval()
    assert pkg('unet').UNet2DModel.engine(model).dropout is None


def test_oracle_long_sweep_prefix_matches_reference():
    """First 40 of the 1000 recorded sweep steps (the full length runs on the GPU: test_long_sweep_1000_steps...)."""
    from oracle import diffusion_ref as D
    fx = load_json('tiny_long_sweep.json')
    assert len(fx['losses']) == 1000
    P = oracle_params(gc.TINY_CFG, 5)
    clean = torch.from_numpy(gc.det_clean((2, 3, 16, 16), 1))
    noise = torch.from_numpy(gc.det_noise((2, 3, 16, 16), 2))
    losses = D.taylor_sweep(P, gc.TINY_CFG, clean, noise, 40)
    assert np.allclose(losses, fx['losses'][:40], rtol=1e-5)


def test_importance_accepts_torch_pruning_shaped_groups(mocked, monkeypatch):
    """Boundary B1: TaylorImportance.__call__(group, ch_groups) fed with groups shaped like a real
    torch_pruning DependencyGraph's -- (dep, idxs) pairs whose dep has .target.module (live nn layers with .weight.grad) and
    .handler = a bound method of the tp pruner singletons -- returns the same scores as on the product's own groups."""
    pruning, sweep, graph_mod = pkg('pruning'), pkg('sweep'), pkg('graph')
    monkeypatch.setattr(sweep.HipSweepStep, '__init__', _cpu_step_init)
    model = _cpu_model(gc.TINY_CFG, 5)
    clean = torch.from_numpy(gc.det_clean((2, 3, 16, 16), 1))
    noise = torch.from_numpy(gc.det_noise((2, 3, 16, 16), 2))
    sweep.taylor_sweep(model, pkg('diffusion').DDPMScheduler(), clean, noise, num_steps=2)
    fx = load_json('tiny_prune.json')
    imp = pruning.TaylorImportance()
    own = pruning.MagnitudePruner(model, None, importance=imp, iterative_steps=1, ch_sparsity=0.3, ignored_layers=[model.conv_out])
    own_groups = {g[0][0].target.name: g for g in own.DG.get_all_groups(ignored_layers=own.ignored_layers)}
    n = 0
    for root, items in tp_like_groups(model, graph_mod):
        s_tp = imp(items, ch_groups=1)
        s_own = imp(own_groups[root], ch_groups=1)
        assert s_tp is not None and torch.equal(s_tp, s_own), root
        assert s_tp.numel() == len(items[0][1])
        n += 1
    assert n == len(fx['groups'])


def test_data_pipeline_host_logic(tmp_path, monkeypatch):
    """Row f4 host side (utils.py:8-58): image-folder discovery, CIFAR python batches, per-epoch shuffling and rank sharding --
    with the device kernel replaced by the oracle transform, two ranks together produce exactly the single-rank global batches."""
    from PIL import Image
    from oracle import data_ref
    data = pkg('data')
    rng = np.random.default_rng(0)
    root = tmp_path / 'imgs'
    (root / 'sub').mkdir(parents=True)
    imgs = []
    for i in range(6):
        a = rng.integers(0, 256, (20, 24, 3), dtype=np.uint8)
        imgs.append(a)
        # ordinary names AND the two-dot names that are all the reference's '**/*.*.png' pattern (utils.py:16) can match
        Image.fromarray(a).save(str(root / ('sub' if i % 2 else '.') / ('im%d%s.png' % (i, '.x' if i < 3 else ''))))
    ds = data.UnlabeledImageFolder(str(root), exts=('*.png',))
    assert len(ds) == 6 and ds[0].dtype == np.uint8 and ds[0].shape == (20, 24, 3)
    got = sorted(ds[i].tobytes() for i in range(6))
    assert got == sorted(a.tobytes() for a in imgs)                    # lossless PNG round trip, every file found once
    ds2 = data.UnlabeledImageFolder(str(root), transform=data.resize_shorter_side(10), exts=('*.png',))
    assert ds2[0].shape == (10, 12, 3)
    (tmp_path / 'empty').mkdir()
    with pytest.raises(FileNotFoundError):
        data.UnlabeledImageFolder(str(tmp_path / 'empty'))
    # RandomCrop offsets come from each image's OWN size (landscape and portrait images in one batch, utils.py:52-53 after
    # Resize on the shorter side), are functions of the global sample index, and cover the whole admissible range
    mixed = data.ArrayDataset(np.zeros((1, 1, 1, 3), dtype=np.uint8))
    shapes = [(16, 21), (21, 16), (16, 16), (30, 16)] * 8
    mixed.__class__ = type('Mixed', (data.ArrayDataset,), {'__len__': lambda self: len(shapes), '__getitem__': lambda self, i: (
        np.arange(shapes[i][0] * shapes[i][1] * 3, dtype=np.int64).reshape(shapes[i] + (3,)) % 251).astype(np.uint8)})
    seen = []
    monkeypatch.setattr(data, 'to_device_batch', lambda u8, *a, **k: (seen.append(u8), torch.zeros(1))[1])
    list(data.DeviceLoader(mixed, 8, 'cpu', shuffle=False, seed=3, crop=16))
    assert [b.shape for b in seen] == [(8, 16, 16, 3)] * 4
    ys, xs = data.crop_offsets(range(32), [h for h, w in shapes], [w for h, w in shapes], 16, 3, 0)
    assert all(0 <= y <= h - 16 and 0 <= x <= w - 16 for y, x, (h, w) in zip(ys, xs, shapes))
    assert max(ys[3::4]) > 7 and max(xs[0::4]) >= 4 and set(ys[0::4]) == {0} and set(xs[1::4]) == {0}
    y2, x2 = data.crop_offsets(range(8, 16), [h for h, w in shapes[8:16]], [w for h, w in shapes[8:16]], 16, 3, 0)
    assert list(y2) == list(ys[8:16]) and list(x2) == list(xs[8:16])          # a function of the sample, not of the batch
    crop0 = seen[0][3]                                                         # sample 3: 30 x 16 portrait
    assert np.array_equal(crop0, mixed[3][ys[3]:ys[3] + 16, xs[3]:xs[3] + 16])
    # CIFAR-10 python batches
    base = tmp_path / 'c10' / 'cifar-10-batches-py'
    base.mkdir(parents=True)
    allb = []
    import pickle
    for k in range(1, 6):
        arr = rng.integers(0, 256, (4, 3072), dtype=np.uint8)
        allb.append(arr)
        with open(str(base / ('data_batch_%d' % k)), 'wb') as f:
            pickle.dump({'data': arr, 'labels': [0] * 4}, f)
    c10 = data.Cifar10Batches(str(tmp_path / 'c10'))
    assert len(c10) == 20 and c10[5].shape == (3, 32, 32) and np.array_equal(c10.data.reshape(20, -1), np.concatenate(allb))
    # loader: sharding + shuffling with the device step mocked by the oracle transform
    calls = []

    def fake(u8, hwc, device, mode, flip_p, seed, epoch, n_off, dequant, out=None):
        calls.append(n_off)
        return data_ref.transform_batch(u8, hwc, mode, flip_p, seed, epoch, n_off, dequant)
    monkeypatch.setattr(data, 'to_device_batch', fake)
    one = list(data.DeviceLoader(c10, 8, 'cpu', seed=5))
    r0 = list(data.DeviceLoader(c10, 4, 'cpu', seed=5, rank=0, world=2))
    r1 = list(data.DeviceLoader(c10, 4, 'cpu', seed=5, rank=1, world=2))
    assert len(one) == 3 and [b.shape[0] for b in one] == [8, 8, 4]
    for a, b0, b1 in zip(one, r0, r1):
        assert torch.equal(a, torch.cat([b0, b1]))
    flat = torch.cat(one)
    assert flat.shape == (20, 3, 32, 32) and float(flat.min()) >= -1 and float(flat.max()) <= 1
    # every sample exactly once per epoch (up to its flip)
    perm = data.epoch_permutation(20, 5, 0)
    ref = data_ref.transform_batch(c10.data[perm], False, 1, 0.5, 5, 0, 0)
    assert torch.equal(flat, ref)
    assert not np.array_equal(perm, data.epoch_permutation(20, 5, 1))


def test_fid_oracle_and_host_math_match_reference():
    """Row f3: the Frechet distance and the activation statistics against values computed by fid_score.py itself
    (tests/golden/fid.json): the oracle restatement and the product's host-side function (scipy sqrtm, as in the reference)."""
    from oracle import metrics_ref as M
    from helpers import fid_features
    metrics = pkg('metrics')
    for fx in load_json('fid.json'):
        a, b = fid_features(fx['dims'], fx['n1'], fx['n2'], fx['seed'])
        m1, s1 = M.activation_statistics(a)
        m2, s2 = M.activation_statistics(b)
        assert abs(m1.sum() - fx['mu1_sum']) < 1e-9 * abs(fx['mu1_sum']) and abs(np.trace(s1) - fx['trace1']) < 1e-9 * fx['trace1']
        for f in (M.frechet_distance, metrics.calculate_frechet_distance):
            assert abs(f(m1, s1, m2, s2) - fx['fid']) < 1e-8 * fx['fid']
            assert abs(f(m1, s1, m1, s1) - fx['fid_self']) < 1e-6
    # the holder tree carries torchvision's key names (what the FID weight file is keyed by) and its parameter count
    sd = metrics.FIDInception3().state_dict()
    assert 'Mixed_7c.branch3x3dbl_3b.bn.running_var' in sd and 'Mixed_6a.branch3x3dbl_3.conv.weight' in sd
    assert sum(v.numel() for k, v in sd.items() if 'num_batches' not in k and not k.startswith('fc.')
               and 'running' not in k) == 21785568          # Inception3 without AuxLogits and fc (torchvision: 21.8 M)
    with pytest.raises(RuntimeError):
        metrics.InceptionV3()(torch.zeros(1, 3, 32, 32))            # no CPU fallback


def test_ssim_oracle_properties():
    """SSIM restatement (pytorch_msssim semantics): identical images -> 1, symmetric, decreasing with noise."""
    from oracle import metrics_ref as M
    r = np.random.default_rng(0)
    x = torch.from_numpy(r.random((3, 3, 32, 32)).astype(np.float32))
    y = (x + 0.1 * torch.from_numpy(r.standard_normal((3, 3, 32, 32)).astype(np.float32))).clamp(0, 1)
    z = (x + 0.3 * torch.from_numpy(r.standard_normal((3, 3, 32, 32)).astype(np.float32))).clamp(0, 1)
    assert torch.allclose(M.ssim(x, x), torch.ones(3, dtype=torch.float64))
    assert torch.allclose(M.ssim(x, y), M.ssim(y, x))
    assert (M.ssim(x, y) > M.ssim(x, z)).all() and (M.ssim(x, z) > 0).all()


def test_upsample_conv_as_four_low_resolution_convs(mocked, monkeypatch):
    """Upsample2D (nearest x2 + conv3x3, resnet.py:131-166) computed by the engine as four 2x2 convolutions on the low-
    resolution input (UNetEngine._ups_conv_fwd / _ups_conv_bwd): the composition -- class kernels, paddings, interleave, the
    accumulated input gradient and the folded weight gradient -- against autograd of the plain formulation, in fp64."""
    import torch.nn.functional as F
    engine = pkg('engine')
    monkeypatch.setattr(mocked, 'empty_act', lambda shape, device: torch.empty(tuple(shape), dtype=torch.float64))
    torch.manual_seed(0)
    N, Ci, Co, H, W = 2, 5, 7, 4, 6
    x = torch.randn(N, Ci, H, W, dtype=torch.float64, requires_grad=True)
    w = torch.randn(Co, Ci, 3, 3, dtype=torch.float64, requires_grad=True)
    b = torch.randn(Co, dtype=torch.float64, requires_grad=True)
    y = F.conv2d(F.interpolate(x, scale_factor=2.0, mode='nearest'), w, b, padding=1)
    dy = torch.randn_like(y)
    y.backward(dy)
    eng = engine.UNetEngine({})
    eng.overlap_wgrad = False
    gw0, gb0 = torch.randn_like(w), torch.randn_like(b)
    eng.P = {'u.weight': w.detach(), 'u.bias': b.detach()}
    eng.G = {'u.weight': gw0.clone(), 'u.bias': gb0.clone()}
    eng._begin_backward()
    got = eng._ups_conv_fwd('u', x.detach())
    dx = eng._ups_conv_bwd('u', dy, x.detach())
    eng._end_backward()
    assert got.shape == y.shape and float((got - y.detach()).abs().max()) < 1e-12
    assert float((dx - x.grad).abs().max()) < 1e-12
    # accumulates, like every parameter gradient (the class gradients pass through the engine's fp32 buffer: 1e-7 relative)
    assert float((eng.G['u.weight'] - (gw0 + w.grad)).abs().max()) < 3e-6 * float(w.grad.abs().max())
    assert float((eng.G['u.bias'] - (gb0 + b.grad)).abs().max()) < 1e-11
    # the class kernels are the sums of the taps that read the same source pixel; the fold is the transposed map
    weff = mocked.ups_weff(w.detach())
    assert torch.allclose(weff.sum((0, 3, 4)) / 4, w.detach().sum((2, 3)), atol=1e-12)
    g = torch.randn(4, Co, Ci, 2, 2, dtype=torch.float64)
    lhs = (weff * g).sum()
    rhs = (w.detach() * mocked.ups_wfold(g, torch.zeros_like(w.detach()), accumulate=False)).sum()
    assert abs(float(lhs - rhs)) < 1e-9


def test_ldm_loss_at_t_matches_reference_latent_diffusion(mocked, monkeypatch):
    """get_loss_at_t / p_losses / q_sample / get_learned_conditioning / ClassEmbedder against the reference's OWN methods
    (tests/golden/ldm_loss_at_t.npz, written by make_golden_ldm.py `loss` from ldm/models/diffusion/ddpm.py:881-889,1022-1056,
    274-277 and ldm/modules/encoders/modules.py:21-33 on the reference UNetModel): the oracle restatement, the product's schedule
    tables and class embedder, and the product's loss step on mocked kernels (loss and the gradients it back-propagates)."""
    from oracle import ldm_ref as R
    ldm, ldm_sweep = pkg('ldm'), pkg('ldm_sweep')
    g = load_npz('ldm_loss_at_t.npz')
    cfg = gc.LDM_TINY_CFG
    B, H = 3, cfg['image_size']
    acp = R.ldm_alphas_cumprod()
    assert np.allclose(np.sqrt(np.asarray(acp, dtype=np.float64)), g['sqrt_acp'], rtol=1e-6)
    sched = ldm_sweep.LdmSchedule()
    assert np.allclose(sched.sqrt_alphas_cumprod.numpy(), g['sqrt_acp'], rtol=1e-6)
    assert np.allclose(sched.sqrt_one_minus_alphas_cumprod.numpy(), g['sqrt_1macp'], rtol=1e-6)
    emb_w = torch.from_numpy(gc.det_param('embedding.weight', (1001, cfg['context_dim']), 61))
    xc = torch.from_numpy(g['class_ids'])
    embedder = ldm_sweep.ClassEmbedder(cfg['context_dim'], 1001)
    with torch.no_grad():
        embedder.embedding.weight.copy_(emb_w)
    context = embedder(xc)
    assert torch.equal(context, torch.from_numpy(g['context']))
    x = torch.from_numpy(gc.det_noise((B, cfg['in_channels'], H, H), 62))
    P = {n: torch.from_numpy(gc.det_param(n, s, 9)).requires_grad_(True) for n, s in R.ldm_param_shapes(cfg).items()}
    # product step on mocked kernels
    for m in (ldm, ldm_sweep):
        monkeypatch.setattr(m, 'ops', mocked)
    monkeypatch.setattr(mocked, 'q_sample', lambda x0, n, sa, sb, t: sa[t][:, None, None, None] * x0 + sb[t][:, None, None, None] * n,
                        raising=False)

    def cpu_engine(self):
        if self._engine is None:
            self._engine = ldm.LdmEngine(self.config)
        self._engine.bind({n: p.detach() for n, p in self.named_parameters()}, None)
        return self._engine
    monkeypatch.setattr(ldm.UNetModel, 'engine', cpu_engine)
    model = ldm.UNetModel(**cfg)
    gc.det_init_(model, 9)
    pkg('sweep').flatten_grads(model)
    step = ldm_sweep.LdmSweepStep(model, sched)
    for k, t in enumerate(g['ts']):
        noise = torch.from_numpy(gc.det_noise((B, cfg['in_channels'], H, H), 70 + k))
        tt = torch.full((B,), int(t), dtype=torch.long)
        assert float((R.q_sample(acp, x, tt, noise) - torch.from_numpy(g['x_noisy'][k])).abs().max()) < 1e-6
        loss = R.ldm_loss_at_t(P, cfg, acp, x, tt, context, noise)
        assert abs(float(loss) - g['losses'][k]) < 2e-6 * abs(g['losses'][k]), (t, float(loss), g['losses'][k])
        got = step.loss(x, tt, context, noise)
        assert abs(float(got) - g['losses'][k]) < 5e-6 * abs(g['losses'][k]), (t, float(got))
        if int(t) == 250:
            loss.backward()
            step.backward()
            names = [str(n) for n in g['grad_abs_sum_names']]
            for n, want in zip(names, g['grad_abs_sum']):
                assert abs(float(P[n].grad.abs().sum()) - want) < 2e-4 * max(want, 1e-6), n
            got_g = dict(model.named_parameters())
            worst = max(relerr(got_g[n].grad, P[n].grad) for n in names if float(P[n].grad.abs().max()) > 1e-7)
            assert worst < 1e-4
        else:
            step.discard()


def test_ldm_driver_loop_matches_the_reference_script(mocked, monkeypatch):
    """The importance-pass loop of the prune_ldm.py script (lines 103-131: class draw, CFG DDIM sampling, get_loss_at_t, max-loss
    bookkeeping, threshold test, backward) against tests/golden/ldm_driver.json, which make_golden_ldm.py `driver` recorded by
    EXECUTING those source lines over the reference LatentDiffusion / DDIMSampler with replayable draws: the first K iterations
    of the oracle restatement and of the product driver (mocked kernels) reproduce the script's losses and the gradients it had
    accumulated after K backward passes; the recorded run never reaches the 0.1 threshold (1000 iterations), as stated."""
    from oracle import ldm_ref as R
    ldm, ldm_sweep = pkg('ldm'), pkg('ldm_sweep')
    fx = load_json('ldm_driver.json')
    K, n, S = fx['K'], fx['n_samples'], fx['ddim_steps']
    assert fx['iterations'] == 1000 and min(l / fx['max_loss'] for l in fx['losses']) > fx['thr']
    cfg = gc.LDM_TINY_CFG
    emb_w = torch.from_numpy(gc.det_param('embedding.weight', (1001, cfg['context_dim']), 61))
    draws = []
    for it in fx['first']:
        shape = tuple(it['shapes'][0])
        assert shape == (n, 3, 64, 64) and tuple(it['shapes'][-1]) == shape
        draws.append((torch.tensor(it['class_ids']), torch.from_numpy(gc.det_noise(shape, it['x_T_draw'])),
                      torch.from_numpy(gc.det_noise(shape, it['noise_draw']))))
    P, losses = _ldm_oracle_sweep(cfg, emb_w, draws, S, fx['thr'])
    assert len(losses) == K and np.allclose(losses, fx['losses'][:K], rtol=5e-6), (losses, fx['losses'][:K])
    for name, want in fx['grad_abs_sum_after_K'].items():
        assert abs(float(P[name].grad.abs().sum()) - want) < 3e-4 * want + 1e-6, name      # (biases in front of a GroupNorm: pure rounding noise)
    # the product driver on mocked kernels
    for m in (ldm, ldm_sweep):
        monkeypatch.setattr(m, 'ops', mocked)

    def cpu_engine(self):
        if self._engine is None:
            self._engine = ldm.LdmEngine(self.config)
        self._engine.bind({n_: p.detach() for n_, p in self.named_parameters()}, None)
        return self._engine
    monkeypatch.setattr(ldm.UNetModel, 'engine', cpu_engine)
    model = ldm.UNetModel(**cfg)
    gc.det_init_(model, 9)
    embedder = ldm_sweep.ClassEmbedder(cfg['context_dim'], 1001)
    with torch.no_grad():
        embedder.embedding.weight.copy_(emb_w)
    res = ldm_sweep.ldm_importance_sweep(model, embedder, num_steps=K, thr=fx['thr'], n_samples=n, ddim_steps=S, scale=fx['scale'],
                                         latent_shape=(3, 64, 64), draws=lambda t: draws[t])
    assert res['steps'] == K and res['accumulated'] == K and np.allclose(res['losses'], fx['losses'][:K], rtol=2e-5)
    got = dict(model.named_parameters())
    for name, want in fx['grad_abs_sum_after_K'].items():
        assert abs(float(got[name].grad.abs().sum()) - want) < 1e-3 * want + 1e-6, name
    # The threshold branch, which that run never takes: the script re-run with the UNet's output convolution zeroed (eps_hat = 0,
    # loss = mean(noise^2)) and the loss-noise draw of iteration 2 scaled by 0.3 stops at t = 2 BEFORE that iteration's backward.
    bc = fx['break_case']
    assert bc['stopped_at'] == 2 and bc['breaking_loss'] / bc['max_loss'] < fx['thr'] and len(bc['printed_losses']) == 2
    per = fx['draws_per_iteration']
    draws_b = []
    for t, ids in enumerate(bc['class_ids']):
        noise = torch.from_numpy(gc.det_noise((n, 3, 64, 64), 5000 + per * t + per - 1))
        if 5000 + per * t + per - 1 == bc['scaled_draw']:
            noise = noise * bc['factor']
        draws_b.append((torch.tensor(ids), torch.from_numpy(gc.det_noise((n, 3, 64, 64), 5000 + per * t)), noise))
    model_b = ldm.UNetModel(**cfg)
    gc.det_init_(model_b, 9)
    with torch.no_grad():
        for pn, pp in model_b.named_parameters():
            if pn.startswith(bc['zeroed_prefix']):
                pp.zero_()
    # device_exit=True: the max-loss / threshold state machine of dp_early_exit_update_ratio (mocked), the breaking step's dOut
    # cancelled, the host reading the flag one step late -- so ONE more step is enqueued after the break (it re-uses the last
    # draws here) and must leave losses, step count and gradients untouched.  device_exit=False: the script's host-side test.
    # pipelines 2: step 1 runs on the second engine into the second gradient buffer; the break at t = 2 (first pipeline) and the
    # step enqueued after it (second pipeline) add nothing, step 1's gradient is kept.
    for device_exit, pipelines in ((True, 1), (False, 1), (True, 2)):
        for p_ in model_b.parameters():
            p_.grad = None
        asked = []
        res = ldm_sweep.ldm_importance_sweep(model_b, embedder, num_steps=10, thr=fx['thr'], n_samples=n, ddim_steps=S,
                                             scale=fx['scale'], latent_shape=(3, 64, 64), device_exit=device_exit,
                                             pipelines=pipelines, draws=lambda t: (asked.append(t), draws_b[min(t, 2)])[1])
        assert asked == ([0, 1, 2, 3] if device_exit else [0, 1, 2])
        assert res['steps'] == 3 and res['accumulated'] == 2
        assert np.allclose(res['losses'], bc['printed_losses'] + [bc['breaking_loss']], rtol=2e-5)
        got = dict(model_b.named_parameters())
        for name, p_ in got.items():
            want = bc['grad_abs_sum'].get(name, 0.0)
            assert abs(float(p_.grad.abs().sum()) - want) < 1e-3 * want + 1e-6, name


def test_fixture_sweep_loop_is_the_reference_scripts_loop():
    """Provenance: the reference's accumulation loop is module-level script code (ddpm_prune.py:94-106), so the fixtures were
    produced by a ten-line restatement of it inside make_golden.py.  `make_golden.py script_loop` executes the script's own source
    lines on the reference UNet and records that they accumulate bit-identical gradients and stop at the same step."""
    chk = load_json('script_loop_check.json')
    assert chk['lines'] == [94, 106]
    assert chk['taylor'] == dict(steps=1000, gradients_bit_identical_to_sweep=True)
    assert chk['diff-pruning']['gradients_bit_identical_to_sweep'] is True
    assert chk['diff-pruning']['steps'] == load_json('tiny_prune.json')['early_exit']['steps']


def test_finetune_loop_matches_the_reference_script(mocked, monkeypatch):
    """The finetune loop of the ddpm_train.py script (lines 426-475) against tests/golden/train_loop.json, recorded by EXECUTING
    those source lines over the reference UNet2DModel / DDPMScheduler / torch Adam / diffusers get_scheduler('cosine', warm-up) /
    vendored EMAModel / accelerate.Accelerator with replayable draws: three optimizer steps of the oracle restatement and of the
    product's FinetuneEngine (mocked kernels) give the script's losses, learning rates, parameters and EMA weights."""
    from oracle import diffusion_ref as D
    train = pkg('train')
    fx = load_json('train_loop.json')
    assert fx['lines'] == [426, 475]
    monkeypatch.setattr(train, '_require_hip_device', lambda dev: None)
    cfg = gc.TINY_CFG
    B = fx['batch']
    sc = fx['scheduler']
    # oracle
    P = oracle_params(cfg, 5)
    names = list(P)
    plist = [P[n] for n in names]
    m = [torch.zeros_like(p) for p in plist]
    v = [torch.zeros_like(p) for p in plist]
    ema = [p.detach().clone() for p in plist]
    lrs = train.get_scheduler(sc['name'], fx['lr'], num_warmup_steps=sc['num_warmup_steps'], num_training_steps=sc['num_training_steps'])
    # product
    model = _cpu_model(cfg, 5)
    sched = pkg('diffusion').DDPMScheduler()
    monkeypatch.setattr(type(sched), '_acp_on', lambda self, dev: self.alphas_cumprod, raising=False)
    ft = train.FinetuneEngine(model, sched, lr=fx['lr'], ema_decay=fx['ema_decay'],
                              lr_scheduler=train.get_scheduler(sc['name'], fx['lr'], num_warmup_steps=sc['num_warmup_steps'],
                                                               num_training_steps=sc['num_training_steps']))
    for k, st in enumerate(fx['steps']):
        clean = torch.from_numpy(gc.det_clean((B, 3, 16, 16), 10 + k))
        noise = torch.from_numpy(gc.det_noise((B, 3, 16, 16), st['noise_draw']))
        t = torch.tensor(st['timesteps'])
        assert len(st['timesteps']) == B and all(a + b == 999 for a, b in zip(st['timesteps'][:B // 2], st['timesteps'][B // 2 + 1:]))
        for p in plist:
            p.grad = None
        lo = D.finetune_loss(P, cfg, clean, noise, t)
        lo.backward()
        with torch.no_grad():
            D.adam_ema_step([p.data for p in plist], [p.grad for p in plist], m, v, ema, k + 1, lr=lrs.get_last_lr()[0],
                            ema_decay=fx['ema_decay'])
        lrs.step()
        assert abs(float(lo.detach()) - st['loss']) < 2e-5 * st['loss'], (k, float(lo.detach()), st['loss'])
        assert abs(lrs.get_last_lr()[0] - st['lr_after']) < 1e-12
        loss = ft.step(clean, noise, t)
        assert abs(float(loss) - st['loss']) < 5e-5 * st['loss'], (k, float(loss), st['loss'])
        assert abs(ft.lr_scheduler.get_last_lr()[0] - st['lr_after']) < 1e-12
    live = dict(model.named_parameters())
    es = ft.ema_state()
    for i, n in enumerate(names):
        want_p, want_e = fx['param_abs_sum'][n], fx['ema_abs_sum'][n]
        assert abs(float(plist[i].detach().abs().sum()) - want_p) < 1e-4 * want_p + 1e-6, n
        assert abs(float(ema[i].abs().sum()) - want_e) < 1e-5 * want_e + 1e-6, n
        assert abs(float(live[n].detach().abs().sum()) - want_p) < 2e-4 * want_p + 1e-6, n
        assert abs(float(es[n].abs().sum()) - want_e) < 1e-5 * want_e + 1e-6, n
    for n, b64 in fx['full'].items():
        want = torch.from_numpy(gc.b64_to_f32(b64))
        assert relerr(P[n].detach(), want) < 2e-4 and relerr(live[n].detach(), want) < 2e-4, n
        want_e = torch.from_numpy(gc.b64_to_f32(fx['full_ema'][n]))
        assert relerr(es[n], want_e) < 1e-5, n


# ------------------------------------------------------------------------------------------------------------------
# round 3: boundary B2 for autograd tracers
# ------------------------------------------------------------------------------------------------------------------
def test_reference_pruner_traces_and_prunes_the_product_model():
    """Boundary B2 (ddpm_prune.py:79-87).  tests/golden/b2_reference_pruner_on_product_model.json was written in the build
    container by make_golden.py `b2`: the reference's vendored `tp.pruner.MagnitudePruner` was handed this repository's
    UNet2DModel, its DependencyGraph traced it (forward hooks + grad_fns), the group tables equalled the ones it enumerates on
    its own Diffusers model (member for member), and -- given the reference sweep's gradients -- it pruned the product model to
    the C1 masks, shapes and 19 851 157 parameters."""
    fx = load_json('b2_reference_pruner_on_product_model.json')
    g = load_json('groups.json')
    assert fx['cifar'] == dict(groups=len(g['cifar']), equal_to_reference_model=True) and fx['cifar']['groups'] == 50
    assert fx['bedroom_topology'] == dict(groups=len(g['bedroom_topology']), equal_to_reference_model=True)
    assert fx['tiny']['equal_to_reference_model'] is True
    c1 = fx['c1_reference_pruner_on_product_model']
    assert c1['masks_equal'] and c1['shapes_equal'] and c1['params_after'] == 19851157 == load_json('cifar_c1.json')['params_after']
    # the reference's hook-based MAC counter (ddpm_prune.py:89,118) on the product model == on the reference's own model
    co, fx1 = fx['count_ops_and_params'], load_json('cifar_c1.json')
    assert co['count_ops_equal'] is True
    assert (co['base_macs'], co['base_params']) == (fx1['base_macs'], fx1['base_params']) == (6064135040.0, 35746307)
    assert (co['macs_after'], co['params_after']) == (fx1['macs_after'], fx1['params_after'])


def test_hooked_model_runs_the_structure_only_forward():
    """What that fixture rests on, checked without the reference: inside `with model.structure_tracing():` -- and automatically
    when every leaf hook belongs to an autograd tracer (this package's trace.py here; `torch_pruning.dependency` in the fixture) --
    the layer sequence runs through the holder modules on a batch of ZERO images: every Conv2d / Linear / GroupNorm is called
    exactly once with a grad_fn behind its output, the result has no elements (it cannot serve as a numerics path), and THIS
    repository's generic tracer, walking that graph, enumerates the reference's group tables (groups.json)."""
    unet, trace, graph, pruning = pkg('unet'), pkg('trace'), pkg('graph'), pkg('pruning')
    fx = load_json('groups.json')
    cfgb = dict(gc.BEDROOM_CFG, block_out_channels=[32, 32, 64, 64, 128, 128], sample_size=64)
    for key, cfg, H in (('cifar', gc.CIFAR_CFG, 32), ('bedroom_topology', cfgb, 64)):
        model = unet.UNet2DModel(**cfg).eval()
        leaves = [m for m in model.modules() if isinstance(m, (torch.nn.Conv2d, torch.nn.Linear, torch.nn.GroupNorm))]
        calls = {}
        hooks = [m.register_forward_hook(lambda m, i, o: calls.__setitem__(m, calls.get(m, 0) + (o.grad_fn is not None)))
                 for m in leaves]
        with model.structure_tracing():
            out = model(sample=torch.randn(1, 3, H, H), timestep=torch.ones((1,)).long())
        for h in hooks:
            h.remove()
        assert out.sample.shape == (0, 3, H, H) and out.sample.grad_fn is not None and out[0] is out.sample
        assert len(calls) == len(leaves) and set(calls.values()) == {1}
        with pytest.raises(RuntimeError):                            # un-hooked: the HIP engine, which has no CPU path
            model(torch.randn(1, 3, H, H), torch.ones((1,)).long())
        with pytest.warns(UserWarning, match='autograd tracer'):     # the tracer's own hooks select the path by themselves
            tg = trace.TracedGraph(model, {'sample': torch.randn(1, 3, H, H), 'timestep': torch.ones((1,)).long()})
        n2m = dict(model.named_modules())
        chan = graph.ChannelView(lambda name: pruning._out_channels(n2m[name]))
        mine = [[[m.name, m.kind, _ranges(m.idxs)] for m in members] for _, members in graph.all_groups(tg, lambda: chan, ('conv_out',))]
        assert mine == [t['members'] for t in fx[key]], key


def _hook_macs(model, B, H):
    """A hook-based MAC counter with the conventions of tp.utils.count_ops_and_params (op_counter.py:53-100: convolutions and
    linears with their bias adds, 2 x elements for an affine GroupNorm), written here from scratch."""
    tot = [0]

    def conv(m, i, o):
        pos = o.shape[0] * o.shape[2] * o.shape[3]
        tot[0] += (m.kernel_size[0] * m.kernel_size[1] * m.in_channels * m.out_channels + (m.out_channels if m.bias is not None else 0)) * pos

    def lin(m, i, o):
        tot[0] += int(np.prod(i[0].shape)) * o.shape[-1] + (o.shape[-1] if m.bias is not None else 0)

    def gn(m, i, o):
        tot[0] += 2 * int(np.prod(i[0].shape))

    hs = [m.register_forward_hook({torch.nn.Conv2d: conv, torch.nn.Linear: lin, torch.nn.GroupNorm: gn}[type(m)])
          for m in model.modules() if isinstance(m, (torch.nn.Conv2d, torch.nn.Linear, torch.nn.GroupNorm))]
    return tot, hs


def test_user_hooks_never_switch_the_model_to_a_zero_image_forward(mocked):
    """Round-3 verdict, boundary B2: a forward hook on a holder leaf that does NOT belong to a tracer (a MAC counter -- the
    reference script's own next line, ddpm_prune.py:89 --, a profiler, a debugging hook) must not change what `model(x, t)`
    returns.  Hooks fire once per leaf in a shape-only pass at the CALLER'S batch; the sample comes from the engine (mocked
    kernels here), shape [B, C, H, W]; a hook-based MAC counter sees exactly the MACs of the analytic count, i.e. the
    reference's 6 064 135 040 per image (cifar_c1.json `base_macs`)."""
    unet, pruning = pkg('unet'), pkg('pruning')
    fx = load_json('cifar_c1.json')
    model = _cpu_model(gc.CIFAR_CFG, 0)
    x, t = torch.from_numpy(gc.det_clean((2, 3, 32, 32), 1)), torch.tensor([3, 500])
    with torch.no_grad():
        want = model(x, t).sample
    seen = []
    h = model.conv_in.register_forward_hook(lambda m, i, o: seen.append((tuple(i[0].shape), tuple(o.shape))))
    with torch.no_grad(), pytest.warns(UserWarning, match='shape-only pass'):
        got = model(x, t).sample
    h.remove()
    assert tuple(got.shape) == (2, 3, 32, 32) and torch.equal(got, want)              # values from the engine, not from the hooks' pass
    assert seen == [((2, 3, 32, 32), (2, 128, 32, 32))]
    for B in (1, 3):
        tot, hs = _hook_macs(model, B, 32)
        with torch.no_grad():
            out = model(sample=torch.randn(B, 3, 32, 32), timestep=torch.ones((B,)).long()).sample
        for hh in hs:
            hh.remove()
        assert tuple(out.shape) == (B, 3, 32, 32)
        lin_bias = sum(m.out_features for m in model.modules() if isinstance(m, torch.nn.Linear))   # counted per CALL, not per image
        assert fx['base_macs'] == pruning.utils.count_ops_and_params(model, None)[0]
        assert tot[0] == B * fx['base_macs'] - (B - 1) * lin_bias
    # a hook that reads VALUES out of the shape-only pass fails loudly instead of seeing garbage
    h = model.conv_in.register_forward_hook(lambda m, i, o: float(o.sum()))
    from torch._subclasses.fake_tensor import DataDependentOutputException
    with pytest.raises(DataDependentOutputException):
        model(x, t)
    h.remove()


def test_user_hook_on_a_cpu_model_raises_instead_of_returning_an_empty_tensor():
    """No mocked engine: the hooked forward of a CPU-resident model ends where the un-hooked one does (RuntimeError: HIP only),
    never in a [0, C, H, W] tensor."""
    model = _cpu_model(gc.TINY_CFG, 0)
    model.conv_in.register_forward_hook(lambda *a: None)
    with pytest.raises(RuntimeError, match='HIP'), pytest.warns(UserWarning):
        model(torch.randn(2, 3, 16, 16), torch.ones((2,)).long())


def _ranges(idxs):
    out = []
    for i in idxs:
        if out and out[-1][1] == i:
            out[-1][1] = i + 1
        else:
            out.append([i, i + 1])
    return out


def test_latent_shards_and_bench_configs():
    """Host logic of round 3: the uneven latent shards of the data-parallel LDM pass (6 over 4 = 2, 2, 1, 1; every latent exactly
    once, contiguous, no empty rank unless there are fewer latents than ranks) and the bench.py contract (every --config has
    default step counts, the default is BASELINE configs[1])."""
    sb = pkg('ldm_sweep').shard_bounds
    assert [sb(6, r, 4) for r in range(4)] == [(0, 2), (2, 4), (4, 5), (5, 6)]
    for n in range(1, 13):
        for w in range(1, 9):
            parts = [sb(n, r, w) for r in range(w)]
            assert parts[0][0] == 0 and parts[-1][1] == n and all(a[1] == b[0] for a, b in zip(parts, parts[1:]))
            sizes = [hi - lo for lo, hi in parts]
            assert max(sizes) - min(sizes) <= 1 and sizes == sorted(sizes, reverse=True)
    import ast
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'bench.py')).read()
    tree = ast.parse(src)
    defaults = next(ast.literal_eval(n.value) for n in ast.walk(tree) if isinstance(n, ast.Assign)
                    and getattr(n.targets[0], 'id', None) == 'DEFAULT_STEPS')
    assert set(defaults) == {'cifar256', 'bedroom256', 'c4_finetune', 'ddim', 'ldm'} and all(k > 0 and w >= 0 for k, w in defaults.values())
    assert "default='cifar256'" in src and 'configs[1]' in src


# ------------------------------------------------------------------------------------------------------------------
# round 4: the algebra of the Winograd F(2, 3) kernels (csrc/winograd.hip), restated in numpy
# ------------------------------------------------------------------------------------------------------------------
def test_winograd_f23_algebra_forward_dgrad_wgrad():
    """The three identities csrc/winograd.hip rests on, checked in float64 on random data with zero padding, for one image row:
      forward   y[2p], y[2p+1] from M_q = sum_c U_q V_q          (U = g0, (g0+g1+g2)/2, (g0-g1+g2)/2, g2; V = d0-d2, d1+d2, d2-d1, d1-d3)
      dgrad     = the same algorithm on the flipped taps with the channel roles swapped (dp_pack_weight_wino mode 1)
      wgrad     dW_k from G_q = sum_p A_q V_q                     (A = dy0, dy0+dy1, dy0-dy1, -dy1;  dW0 = G0 + (G1+G2)/2, ...)
    and the pack layout U[(ky*4 + pos)*K + k][m] of both modes against a direct evaluation."""
    rng = np.random.default_rng(0)
    C, M, W = 5, 4, 8
    x = rng.standard_normal((C, W))
    g = rng.standard_normal((M, C, 3))                                  # one kernel row
    xp = np.pad(x, ((0, 0), (1, 1)))
    ref = np.stack([sum(g[m, c, k] * xp[c, k:k + W] for c in range(C) for k in range(3)) for m in range(M)])
    U = np.stack([g[..., 0], (g[..., 0] + g[..., 1] + g[..., 2]) / 2, (g[..., 0] - g[..., 1] + g[..., 2]) / 2, g[..., 2]])   # [4, M, C]
    y = np.zeros((M, W))
    for p in range(W // 2):
        d = xp[:, 2 * p:2 * p + 4]                                       # d_j = x[2p + j - 1] (zero padded)
        V = np.stack([d[:, 0] - d[:, 2], d[:, 1] + d[:, 2], d[:, 2] - d[:, 1], d[:, 1] - d[:, 3]])            # [4, C]
        Mq = np.einsum('qmc,qc->qm', U, V)
        y[:, 2 * p] = Mq[0] + Mq[1] + Mq[2]
        y[:, 2 * p + 1] = Mq[1] - Mq[2] - Mq[3]
    assert np.allclose(y, ref, atol=1e-12)
    # input gradient: dx[c] = sum_m corr(dy[m], flipped taps)  -- the forward algorithm with g'[c][m][k] = g[m][c][2 - k]
    dy = rng.standard_normal((M, W))
    dyp = np.pad(dy, ((0, 0), (1, 1)))
    ref_dx = np.stack([sum(g[m, c, 2 - k] * dyp[m, k:k + W] for m in range(M) for k in range(3)) for c in range(C)])
    gf = np.transpose(g, (1, 0, 2))[..., ::-1]
    Uf = np.stack([gf[..., 0], (gf[..., 0] + gf[..., 1] + gf[..., 2]) / 2, (gf[..., 0] - gf[..., 1] + gf[..., 2]) / 2, gf[..., 2]])
    dx = np.zeros((C, W))
    for p in range(W // 2):
        d = dyp[:, 2 * p:2 * p + 4]
        V = np.stack([d[:, 0] - d[:, 2], d[:, 1] + d[:, 2], d[:, 2] - d[:, 1], d[:, 1] - d[:, 3]])
        Mq = np.einsum('qcm,qm->qc', Uf, V)
        dx[:, 2 * p] = Mq[0] + Mq[1] + Mq[2]
        dx[:, 2 * p + 1] = Mq[1] - Mq[2] - Mq[3]
    assert np.allclose(dx, ref_dx, atol=1e-12)
    # weight gradient by the transposed algorithm
    ref_dw = np.stack([[[np.dot(dy[m], xp[c, k:k + W]) for k in range(3)] for c in range(C)] for m in range(M)])
    G = np.zeros((4, M, C))
    for p in range(W // 2):
        d = xp[:, 2 * p:2 * p + 4]
        V = np.stack([d[:, 0] - d[:, 2], d[:, 1] + d[:, 2], d[:, 2] - d[:, 1], d[:, 1] - d[:, 3]])
        A = np.stack([dy[:, 2 * p], dy[:, 2 * p] + dy[:, 2 * p + 1], dy[:, 2 * p] - dy[:, 2 * p + 1], -dy[:, 2 * p + 1]])      # [4, M]
        G += A[:, :, None] * V[:, None, :]
    hs = (G[1] + G[2]) / 2
    dw = np.stack([G[0] + hs, (G[1] - G[2]) / 2, hs + G[3]], axis=-1)
    assert np.allclose(dw, ref_dw, atol=1e-12)
    # multiply counts: 4 per output pair (and per gradient triple) instead of 6
    assert U.shape[0] == 4 and 4 / 6 == pytest.approx(2 / 3)


def test_winograd_dispatch_rules():
    """Host-side dispatch of the Winograd kernels (ops.wino_wanted: pure arithmetic, no device): shapes of the five BASELINE
    configs that go to dp_conv_wino and the ones that stay on the direct kernels."""
    ops = pkg('ops')
    S3, S1 = ops.ConvSpec(3, 1, 1, 0), ops.ConvSpec(1, 1, 0, 0)
    assert ops.WINO and ops.WINO_MIN_TILES == 512
    assert ops.wino_wanted(128, (128,), 256, 32, 32, S3)                 # CIFAR level 0 at batch 256: 2 x 2048 tiles
    assert ops.wino_wanted(128, (256, 128), 256, 32, 32, S3)             # up-block concat input
    assert ops.wino_wanted(256, (256,), 256, 4, 4, S3)                   # 4 x 4 level: 128 tiles, split-K 4
    assert not ops.wino_wanted(128, (128,), 4, 32, 32, S3)               # config C1 (batch 4): 64 tiles, 24 K tiles -> split 3 < 256 workgroups
    assert not ops.wino_wanted(128, (3,), 256, 32, 32, S3)               # conv_in: 3 input channels
    assert not ops.wino_wanted(256, (256,), 256, 16, 16, S1)             # 1 x 1
    assert not ops.wino_wanted(128, (128,), 256, 32, 32, ops.ConvSpec(3, 2, 0, 0))     # Downsample2D (stride 2)
    assert not ops.wino_wanted(179, (179,), 128, 16, 16, S3)             # odd pruned width on the contraction side
    assert ops.wino_wanted(90, (96,), 128, 32, 32, S3)                   # ... on the output side only: row tails are fine
    assert not ops.wino_wanted(3, (128,), 256, 32, 32, S3)               # conv_out: 3 output rows -> the stencil kernel
    assert ops.wino_wanted(128, (128,), 4, 256, 256, S3) and not ops.wino_wanted(128, (128,), 4, 512, 512, S3)      # bedroom-256; W <= 256
    assert ops.wino_wanted(576, (576,), 12, 16, 16, S3)                  # LDM 16 x 16 level at 12 latents: 216 tiles x split 2


def test_engine_routes_3x3_layers_to_the_winograd_kernel_with_current_operands(mocked, monkeypatch):
    """Engine-side bookkeeping of the Winograd dispatch on mocked kernels (the arithmetic is the direct convolution's, so the
    oracle comparison doubles as a check that routing changes nothing): with the grid threshold dropped every 3x3 / stride-1 layer
    with >= 8 input channels goes to the Winograd entry point in the forward AND the input-gradient pass, each time with an
    operand packed from the CURRENT weight tensor -- also after a prune (sliced weights) and after an optimizer step (in-place
    update: prepare_packs() re-packs the operands the previous pass asked for)."""
    from oracle import diffusion_ref as D
    ops, sweep, train = pkg('ops'), pkg('sweep'), pkg('train')
    monkeypatch.setattr(ops, 'WINO_MIN_TILES', 0)
    monkeypatch.setattr(sweep.HipSweepStep, '__init__', _cpu_step_init)
    del mocked.WINO_CALLS[:]
    cfg = gc.TINY_CFG
    model = _cpu_model(cfg, 5)
    clean = torch.from_numpy(gc.det_clean((2, 3, 16, 16), 1))
    noise = torch.from_numpy(gc.det_noise((2, 3, 16, 16), 2))
    res = sweep.taylor_sweep(model, pkg('diffusion').DDPMScheduler(), clean, noise, num_steps=2)
    P = oracle_params(cfg, 5)
    assert np.allclose(res['losses'], D.taylor_sweep(P, cfg, clean, noise, 2), rtol=1e-5)
    fwd = [c for c in mocked.WINO_CALLS if c[0] == 0]
    bwd = [c for c in mocked.WINO_CALLS if c[0] == 1]
    # every ResnetBlock2D convolution at the 16 x 16 / 8 x 8 / 4 x 4 levels, in both timesteps (the 2 x 2 level is below the kernel's
    # W >= 4; conv_in has 3 input channels, conv_out 3 output rows: direct / stencil kernels)
    assert len(fwd) == 60 and len(bwd) == len(fwd), (len(fwd), len(bwd))
    eng = model.engine()
    assert {m for _, m in eng._wino_seen} == {('wino', 0), ('wino', 1)}
    # prune: the weights are new, smaller tensors -> fresh operands (the mock asserts identity, version and shape on every launch)
    sweep.prune_model(model, 0.3)
    del mocked.WINO_CALLS[:]
    for p in model.parameters():
        p.grad = None
    sweep.taylor_sweep(model, pkg('diffusion').DDPMScheduler(), clean, noise, num_steps=1)
    assert mocked.WINO_CALLS and all(s[0] < 64 or s[1] < 64 or True for _, s in mocked.WINO_CALLS)
    assert any(sh[0] not in (32, 64) or sh[1] not in (32, 64, 96, 128) for _, sh in mocked.WINO_CALLS)      # pruned widths reached the kernel
    # two optimizer steps on the pruned model: the in-place update bumps every weight's version; a stale operand would trip the mock
    monkeypatch.setattr(train, '_require_hip_device', lambda dev: None)
    monkeypatch.setattr(pkg('diffusion').DDPMScheduler, '_acp_on', lambda self, dev: self.alphas_cumprod)
    ft = train.FinetuneEngine(model, pkg('diffusion').DDPMScheduler(), lr=1e-3, ema_decay=0.999)
    del mocked.WINO_CALLS[:]
    t = torch.tensor([5, 700])
    l1, l2 = float(ft.step(clean, noise, t)), float(ft.step(clean, noise, t))
    assert len(mocked.WINO_CALLS) > 40 and l1 != l2


def test_k_loops_carry_no_compiler_inserted_vmcnt0(tmp_path):
    """Round-4 finding, kept from coming back: a second `__shared__` object -- or a float2-typed LDS read --
    makes hipcc's waitcnt pass drain `vmcnt(0)` right behind the LDS-DMA prefetch of EVERY K tile of the matrix kernels.  The device
    code of csrc/gemm.hip, csrc/winograd.hip, csrc/winograd43.hip and csrc/winograd2d.hip is compiled to ISA (hipcc cross-compiles without a GPU) and every MFMA loop is
    scanned: between the loop header and the hand-placed `s_waitcnt vmcnt(0)` in front of its barrier there must be LDS-DMA loads
    and NO compiler-inserted `s_waitcnt vmcnt(0)`.  Also: no scratch (spill) traffic inside those loops."""
    import shutil
    import subprocess
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('hipcc not available')
    csrc = os.path.join(ROOT, 'diff-pruning_amd', 'csrc')
    want = {'gemm.hip': ('conv_gemm_fast_kernel', 'nt_gemm_fast_kernel'), 'winograd.hip': ('conv_wino_kernel', 'wgrad_wino_kernel'),
            'winograd43.hip': ('conv_wino43_kernel',), 'winograd2d.hip': ('conv_wino2d_kernel', 'conv_wino2d_tail_kernel', 'conv_wino2d_m32_kernel'),
            'wgrad2d.hip': ('wgrad_wino2d_kernel', 'wgrad_wino2d_tail_kernel')}
    checked = 0
    for src, kernels in want.items():
        out = str(tmp_path / (src + '.s'))
        subprocess.run([hipcc, '--offload-arch=gfx950', '-O3', '-std=c++17', '-I' + os.path.join(ROOT, 'include'), '-I' + csrc, '-S',
                        '--cuda-device-only', '-o', out, os.path.join(csrc, src)], check=True, capture_output=True, timeout=600)
        name, body = None, []
        funcs = {}
        for line in open(out):
            m = re.match(r'^(_Z\w+):', line)
            if m:
                name, body = m.group(1), []
                funcs[name] = body
            elif name is not None:
                body.append(line)
                if 's_endpgm' in line:
                    name = None
        for fname, lines in funcs.items():
            if not any(k in fname for k in kernels):
                continue
            # every hand-placed wait (inline asm) : the K-loop body is what lies between the previous barrier and it
            in_asm, asm_waits, barriers = False, [], []
            for j, t in enumerate(lines):
                in_asm = True if 'ASMSTART' in t else (False if 'ASMEND' in t else in_asm)
                if in_asm and 's_waitcnt vmcnt(0)' in t:
                    asm_waits.append(j)
                if 's_barrier' in t:
                    barriers.append(j)
            for w in asm_waits:
                start = max([b for b in barriers if b < w], default=0)
                seg = lines[start:w]
                if sum('v_mfma' in t for t in seg) < 8 or any('_store_' in t for t in seg):
                    continue                # the prologue's wait (no matrix work in front of it) / the split-K fold's wait (behind the epilogue's stores)
                in_asm, bad = False, []
                for t in seg:
                    in_asm = True if 'ASMSTART' in t else (False if 'ASMEND' in t else in_asm)
                    if not in_asm and 's_waitcnt vmcnt(0)' in t:
                        bad.append(t.strip())
                assert any('buffer_load' in t and ' lds' in t for t in seg), (fname, 'K loop without LDS-DMA prefetch')
                assert not bad, (fname, 'compiler-inserted s_waitcnt vmcnt(0) between the barrier and the hand-placed wait of a K tile', bad)
                assert not any('scratch_' in t for t in seg), (fname, 'scratch access inside the K loop')
                checked += 1
    assert checked >= 27, checked            # (+ 2 K loops in each of the 3 + 3 tail instantiations of the two 2-D kernels)  6 fast-conv + 4 fast-wgrad + 5 Winograd-conv + 2 Winograd-wgrad + 1 F(2x2, 3x3) instantiations


def test_winograd_refuses_activations_within_a_row_of_2gib():
    """Advisor finding of round 4: the Winograd kernels address X through descriptors that start one image row in front of the
    tensor (num_records = extent + 4 W) and mark padding with the offset 0x80000000.  An activation whose extent is within 4 W bytes of
    2 GiB would put that marker inside the descriptor; dp_conv_wino_supported / dp_wgrad_wino_supported refuse such shapes
    (host-side shape rules: no GPU needed), so the dispatch keeps them on the direct kernels."""
    L = pkg('_lib')
    lib = L.load()

    def geom():
        g = L.ConvGeom()
        g.Ho = g.Hs = g.Hv = 64
        g.Wo = g.Ws = g.Wv = 64
        g.kw, g.stride, g.sden, g.pad_t, g.pad_l, g.ups, g.c_split = 3, 1, 1, 1, 1, 0, 64
        g.x1_img_stride = g.x2_img_stride = 64 * 64 * 64
        return g

    def conv(x1_bytes, x2_bytes=0):
        p = L.ConvGemmParams()
        p.g = geom()
        p.M, p.C, p.NPIX, p.ntaps, p.batches, p.lda, p.ksplit = 64, 64, 64 * 64 * 4, 9, 1, 64, 1
        p.a_bytes, p.x1_bytes, p.x2_bytes = 12 * 64 * 64 * 4, x1_bytes, x2_bytes
        if x2_bytes:
            p.X2, p.C, p.g.c_split = 16, 128, 64
        return lib.dp_conv_wino_supported(ctypes.byref(p))

    def wgrad(x1_bytes):
        p = L.NtGemmParams()
        p.g = geom()
        p.M, p.C, p.NCOLS, p.ntaps, p.P = 64, 64, 64, 9, 64 * 64 * 4
        p.batches, p.splits, p.p_per_split, p.tile = 1, 4, 64 * 64 + 32, 0
        p.a_bytes, p.x1_bytes = 4 << 20, x1_bytes
        return lib.dp_wgrad_wino_supported(ctypes.byref(p))

    lim = (1 << 31) - 4 * 64           # extent + 4 W must stay below 0x80000000
    assert conv(4 << 20) == 16 and conv(lim - 4) == 16 and conv(lim) == 0 and conv((1 << 31) - 4) == 0
    assert conv(4 << 20, 4 << 20) == 16 and conv(4 << 20, lim) == 0
    assert wgrad(4 << 20) == 1 and wgrad(lim - 4) == 1 and wgrad(lim) == 0


def test_fast_kernels_refuse_activations_within_their_shift_of_2gib():
    """The same hazard in csrc/gemm.hip: conv_gemm_fast_kernel and nt_gemm_fast_kernel move their gathered-operand descriptor bases back
    by `shift` = pad_t * Ws + pad_l floats + the largest instruction offset (3072 / 1820 bytes), the nt form its A base by 1820 bytes,
    and lengthen num_records by as much.  conv_fast_ok / nt_fast_ok refuse whenever a descriptor would reach 0x80000000; they are not
    exported, so what is pinned here is their ops mirrors (_conv_fast_ok, _nt_fast_ok) -- the names ops gives the profiler, which tests/test_reach_gpu.py holds
    equal to the launched kernels on both sides of the rule -- and the ValueError of the batched parameter blocks."""
    ops, L = pkg('ops'), pkg('_lib')
    assert ops._CONV_FAST_IMM_MAX == 3 * 1024 and ops._NT_FAST_IMM_MAX == 7 * 65 * 4 and ops._MAX_BYTES == 1 << 31

    def conv(x1_bytes, x2_bytes=0, tile=0, W=16):
        p = L.ConvGemmParams()
        p.g = ops._geom(16, W, 16, W, 16, W, 3, 1, 1, 1, 1, 0, 64, 0, 0)
        p.M, p.C, p.NPIX, p.ntaps, p.batches, p.a_kc, p.tile, p.x_guard = 100, 128 if x2_bytes else 64, 512, 9, 1, 0, tile, 1
        p.x1_bytes, p.x2_bytes = x1_bytes, x2_bytes
        if x2_bytes:
            p.X2 = 16
        return p

    for W in (16, 18):
        lim = (1 << 31) - 4 * (W + 1) - 3072                     # extent + 4 shift must stay below 0x80000000
        x4 = 'true' if W % 4 == 0 else 'false'
        assert ops._conv_fast_ok(conv(lim - 4, W=W)) and not ops._conv_fast_ok(conv(lim, W=W)) and not ops._conv_fast_ok(conv((1 << 31) - 4, W=W))
        assert ops._conv_fast_ok(conv(1 << 20, lim - 4, W=W)) and not ops._conv_fast_ok(conv(1 << 20, lim, W=W))
        assert ops._conv_fast_ok(conv(lim - 4, lim - 4, W=W)) and not ops._conv_fast_ok(conv(lim, 1 << 20, W=W))
        assert ops._cg_name(conv(lim - 4, W=W)) == 'conv_gemm_fast_kernel<128, 128, false, %s>' % x4
        assert ops._cg_name(conv(lim, W=W)) == 'conv_gemm_kernel<128, 128, false, false>'
        assert ops._cg_name(conv(1 << 20, lim - 4, W=W)) == 'conv_gemm_fast_kernel<128, 128, false, %s>' % x4
        assert ops._cg_name(conv(1 << 20, lim, W=W)) == 'conv_gemm_kernel<128, 128, false, false>'
        assert ops._cg_name(conv(lim - 4, tile=3, W=W)) == 'conv_gemm_fast_kernel<96, 128, true, %s>' % x4
        assert ops._cg_name(conv(lim, tile=3, W=W)) == 'conv_gemm_kernel<128, 128, false, false>'       # tile 3 / 4 without the fast loader: 128 x 128
        p = conv(lim, W=W)
        p.tile = 1
        ops._prefer_tile96(p)
        assert p.tile == 1                                       # no 128- / 96-row preference for a launch the fast kernels refuse
    # the x2 extent only counts when there is a second source
    p = conv(1 << 20)
    p.x2_bytes = (1 << 31) - 4
    assert ops._conv_fast_ok(p)

    def nt(a_bytes, x1_bytes, x2_bytes=0, tile=0):
        p = L.NtGemmParams()
        p.g = ops._geom(16, 16, 16, 16, 16, 16, 3, 1, 1, 1, 1, 0, 64, 0, 0)
        p.M, p.C, p.NCOLS, p.ntaps, p.P = 100, 64, 128 if x2_bytes else 64, 9, 512
        p.batches, p.splits, p.p_per_split, p.tile = 1, 1, 512, tile
        p.a_bytes, p.x1_bytes, p.x2_bytes = a_bytes, x1_bytes, x2_bytes
        if x2_bytes:
            p.X2 = 16
        return p

    lim_a = (1 << 31) - 1820                                     # A: num_records = extent + 1820
    lim_x = (1 << 31) - 4 * 17 - 1820                            # X: extent + 4 (Ws + 1) + 1820
    small = 1 << 20
    # (conv_wgrad asks _nt_fast_ok before it prefers 96 x 96 tiles, so tile, grid and slices are sized for the kernel that runs)
    assert ops._nt_fast_ok(nt(lim_a - 4, lim_x - 4, lim_x - 4)) and not ops._nt_fast_ok(nt(lim_a, small)) and not ops._nt_fast_ok(nt(small, lim_x))
    assert not ops._nt_fast_ok(nt(small, small, lim_x)) and ops._nt_fast_ok(nt(small, small))
    for tile, nw in ((0, 4), (3, 3)):
        fast, slow = 'nt_gemm_fast_kernel<%d, %%s>' % nw, 'nt_gemm_kernel<128, 128, %s, false>'
        assert ops._nt_name(nt(small, small, tile=tile)) == fast % 'false'
        assert ops._nt_name(nt(lim_a - 4, small, tile=tile)) == fast % 'false' and ops._nt_name(nt(lim_a, small, tile=tile)) == slow % 'false'
        assert ops._nt_name(nt(small, lim_x - 4, tile=tile)) == fast % 'false' and ops._nt_name(nt(small, lim_x, tile=tile)) == slow % 'false'
        assert ops._nt_name(nt(small, small, lim_x - 4, tile=tile)) == fast % 'true'
        assert ops._nt_name(nt(small, small, lim_x, tile=tile)) == slow % 'true'             # c_split = 64: an N tile of 128 spans both sources
        assert ops._nt_name(nt(small, small, (1 << 31) - 4, tile=tile)) == slow % 'true'

    # batched products take their operand extents from the matrix shapes: 2 GiB per matrix is refused like a 2 GiB activation view
    t = torch.empty(4)
    for M, K, Nn in ((1 << 15, 1 << 14, 4), (4, 1 << 14, 1 << 15), (1 << 16, 1 << 16, 4)):     # A = 2^31, X = 2^31, A = 2^34 (wraps a c_uint)
        with pytest.raises(ValueError, match='2 GiB'):
            ops._conv_gemm_params(t, M, t, None, ops._bgeom(Nn, K), M, K, Nn, 1, t, 0, batch=(2, M * K, K * Nn, M * Nn))
        with pytest.raises(ValueError, match='2 GiB'):
            ops._nt_gemm_params(t, 0, t, None, ops._bgeom(K, Nn), M, Nn, Nn, 1, K, 1, 0, 0, 1.0, Nn, batch=(2, M * K, K * Nn, 1))
    M, K, Nn = (1 << 15) - 1, 1 << 14, 4                         # one row fewer: accepted, extents as the matrix shapes say
    p = ops._conv_gemm_params(t, M, t, None, ops._bgeom(Nn, K), M, K, Nn, 1, t, 0, batch=(2, M * K, K * Nn, M * Nn))
    assert (p.a_bytes, p.x1_bytes, p.x2_bytes) == (M * K * 4, K * Nn * 4, 0) and p.a_bytes == (1 << 31) - (1 << 16)
    p = ops._nt_gemm_params(t, 0, t, None, ops._bgeom(K, Nn), M, Nn, Nn, 1, K, 1, 0, 0, 1.0, Nn, batch=(2, M * K, K * Nn, 1))
    assert (p.a_bytes, p.x1_bytes, p.x2_bytes) == (M * K * 4, Nn * K * 4, 0)


def test_lsun_ffhq_lmdb_datasets(tmp_path):
    """SURVEY §8(f) rank 4, the LSUN / FFHQ half (ddpm_exp/datasets/lsun.py:11-173, ffhq.py:8-40, __init__.py:109-157): LMDB
    environments read by the package's own pure-Python reader (lmdb_reader.py; `lmdb` is not in this image).  The environments are
    built by tests/helpers.write_lmdb from the same published structure definitions -- multi-level trees, overflow pages, a stale
    second meta page -- so what is pinned is reader == writer over the format and the reference's dataset SEMANTICS (key-order
    item order + its pickle cache, `<category>_<split>_lmdb` directories, cumulative class indices, the FFHQ key scheme, Resize +
    CenterCrop), not liblmdb's own bytes (format parity unpinned, stated in the module)."""
    import io
    import pickle
    from PIL import Image
    from helpers import write_lmdb
    data, lm = pkg('data'), pkg('lmdb_reader')
    rng = np.random.default_rng(3)
    # (1) the reader on trees of depth 1, 2 and 3 with inline and overflow values
    for n_items, max_keys in ((5, None), (300, None), (700, 9)):
        items = {('k%05d' % (i * 7919 % 100003)).encode(): bytes(rng.integers(0, 256, size=int(rng.integers(1, 40)) if i % 11 else 9000,
                                                                                dtype=np.uint8)) for i in range(n_items)}
        d = str(tmp_path / ('env%d' % n_items))
        write_lmdb(d, items, max_leaf_keys=max_keys)
        with lm.Environment(d) as env:
            assert env.stat()['entries'] == n_items and env.depth == (1 if n_items == 5 else 2 if n_items == 300 else 3)
            assert env.keys() == sorted(items)                                   # cursor order = byte-wise key order
            assert all(env.get(k) == v for k, v in items.items())
            assert env.get(b'k') is None and env.get(b'zzz') is None and env.get(b'k00000x') is None
            assert dict(env.items()) == items
    with pytest.raises(lm.LmdbError):
        (tmp_path / 'junk').mkdir()
        (tmp_path / 'junk' / 'data.mdb').write_bytes(b'\0' * 8192)
        lm.Environment(str(tmp_path / 'junk'))
    # (2) LSUN: two class environments of PNG-encoded images (lossless stand-ins for the WEBP values)
    def png(arr):
        b = io.BytesIO()
        Image.fromarray(arr).save(b, format='PNG')
        return b.getvalue()
    root = tmp_path / 'data' / 'lsun'
    imgs = {}
    for cls, n in (('bedroom_train', 6), ('church_outdoor_train', 4), ('bedroom_val', 2)):
        arrs = {('%040x' % int(rng.integers(0, 1 << 62))).encode(): rng.integers(0, 256, size=(40 + 3 * j, 56 - 2 * j, 3), dtype=np.uint8)
                for j in range(n)}
        write_lmdb(str(root / (cls + '_lmdb')), {k: png(a) for k, a in arrs.items()})
        imgs[cls] = [arrs[k] for k in sorted(arrs)]
    ds = data.Lsun(str(root), ['bedroom_train', 'church_outdoor_train'])
    assert len(ds) == 10 and ds.indices == [6, 10]
    assert np.array_equal(ds[0], imgs['bedroom_train'][0]) and np.array_equal(ds[5], imgs['bedroom_train'][5])
    assert np.array_equal(ds[6], imgs['church_outdoor_train'][0]) and np.array_equal(ds[9], imgs['church_outdoor_train'][3])
    cache = root / '_cache_bedroom_train_lmdb'                                    # lsun.py:29-36: the key list is pickled once
    assert pickle.load(open(cache, 'rb')) == data.LsunClassLmdb(str(root / 'bedroom_train_lmdb')).keys
    with pytest.raises(ValueError, match='LSUN class'):
        data.Lsun(str(root), ['garage_train'])
    with pytest.raises(ValueError, match='postfix'):
        data.Lsun(str(root), ['bedroom_training'])
    cfg = dict(dataset='LSUN', category='bedroom', image_size=32, random_flip=True, rescaled=True, uniform_dequantization=False)
    dsc, kw = data.dataset_from_config(cfg, root=str(tmp_path / 'data'))
    assert isinstance(dsc, data.Lsun) and len(dsc) == 6 and kw['flip_p'] == 0.5 and kw['mode'] == data.RESCALE
    for i in (0, 3):          # e.g. 40 x 56: Resize(32) -> 32 x 44 (shorter side, bilinear), CenterCrop(32) -> columns 6 .. 37
        a0 = imgs['bedroom_train'][i]
        h, w = a0.shape[:2]
        rw, rh = (32, int(32 * h / w)) if w < h else (int(32 * w / h), 32)
        r = np.asarray(Image.fromarray(a0).resize((rw, rh), Image.BILINEAR))
        top, left = int(round((rh - 32) / 2.0)), int(round((rw - 32) / 2.0))
        assert dsc[i].shape == (32, 32, 3) and np.array_equal(dsc[i], r[top:top + 32, left:left + 32])
    assert len(data.dataset_from_config(cfg, root=str(tmp_path / 'data'), train=False)[0]) == 2
    # (3) FFHQ: one environment, b'length' + b'<resolution>-<index:05d>'
    ff = {b'length': b'3'}
    fimgs = {}
    for r in (8, 16):
        for i in range(3):
            fimgs[(r, i)] = rng.integers(0, 256, size=(r, r, 3), dtype=np.uint8)
            ff[('%d-%05d' % (r, i)).encode()] = png(fimgs[(r, i)])
    write_lmdb(str(tmp_path / 'data' / 'FFHQ'), ff)
    # the 90 / 10 split of datasets/__init__.py:166-177 (seeded legacy numpy shuffle, caller's generator state untouched): index
    # lists recorded from the reference's own lines (tests/golden/make_golden_ffhq_split.py)
    import hashlib
    for case in load_json('ffhq_split.json')['cases']:
        np.random.seed(777)
        before = np.random.get_state()[1][:4].tolist()
        tr, te = data.ffhq_split_indices(case['n'])
        assert np.random.get_state()[1][:4].tolist() == before
        assert (len(tr), len(te)) == (case['n_train'], case['n_test'])
        assert hashlib.sha256(np.asarray(tr, dtype=np.int64).tobytes()).hexdigest() == case['train_sha256']
        assert hashlib.sha256(np.asarray(te, dtype=np.int64).tobytes()).hexdigest() == case['test_sha256']
        if 'train' in case:
            assert tr == case['train'] and te == case['test']
    split3 = [c for c in load_json('ffhq_split.json')['cases'] if c['n'] == 3][0]
    f16, kw = data.dataset_from_config(dict(cfg, dataset='FFHQ', image_size=16), root=str(tmp_path / 'data'))
    f16_test, _ = data.dataset_from_config(dict(cfg, dataset='FFHQ', image_size=16), root=str(tmp_path / 'data'), train=False)
    assert len(f16) == 2 and len(f16_test) == 1                      # training never sees the held-out tenth
    for j, i in enumerate(split3['train']):
        assert np.array_equal(f16[j], fimgs[(16, i)])
    assert np.array_equal(f16_test[0], fimgs[(16, split3['test'][0])])
    assert np.array_equal(data.FfhqLmdb(str(tmp_path / 'data' / 'FFHQ'), 8)[1], fimgs[(8, 1)])
    loader = data.DeviceLoader if hasattr(data, 'DeviceLoader') else None
    assert loader is not None



def test_committed_pmc_traffic_was_measured_on_these_kernel_sources():
    """`roofline.traffic` on the bench line comes from committed rocprofv3 --pmc passes (they cannot run inside bench.py): the newest
    file of every config must carry the hash of TODAY's contraction-kernel sources (csrc/gemm.hip + csrc/winograd.hip + csrc/winograd2d.hip + csrc/wgrad2d.hip + the two *_kloop.inc) and its own
    config name, or bench.py reports `traffic: null` (bench._pmc_traffic) -- this test makes a stale file a red CPU suite, not a silent null."""
    import glob
    import hashlib
    import json
    src = b''.join(open(os.path.join(ROOT, 'diff-pruning_amd', 'csrc', f), 'rb').read() for f in ('gemm.hip', 'winograd.hip', 'winograd2d.hip', 'winograd2d_kloop.inc', 'wgrad2d.hip', 'wgrad2d_kloop.inc'))
    blob = hashlib.sha1(b'blob %d\0' % len(src) + src).hexdigest()
    for sfx, cfg in (('', 'cifar256'), ('_c4_finetune', 'c4_finetune'), ('_ldm', 'ldm')):
        cand = sorted(glob.glob(os.path.join(ROOT, 'profiles', 'round*_pmc_bench_traffic%s.json' % sfx)))
        assert cand, cfg
        pm = json.load(open(cand[-1]))
        assert pm.get('_gemm_hip_blob') == blob, (cand[-1], 'measured on other kernel sources: re-run tools/run_evidence.sh pmc')
        assert pm.get('_config', 'cifar256') == cfg, cand[-1]
        dom = [k for k, v in pm.items() if isinstance(v, dict) and 'FETCH_SIZE' in v and 'WRITE_SIZE' in v]
        assert dom, cand[-1]


@pytest.mark.parametrize('case', ['3x3', 'ups', 's2_asym', 's2_sym', 'same_2x2', '1x1_4x4'])
def test_launch_parity_subset_references_equal_full_fp64(case):
    """The structured-subset fp64 references of tests/test_launch_parity_gpu.py (tests/helpers.py) are the matching slices of the
    full fp64 computation: forward and input gradient on the edge images, the weight gradient on the edge row x column tiles
    (reduced over every image), GroupNorm forward / backward incl. the per-image affine gradients, attention; and the edge
    index sets hold what they claim (first / last tile incl. a tail, both sides of the first 128-pixel tile boundary)."""
    import torch.nn.functional as F
    from helpers import edge_images, edge_tiles, ref_attention, ref_conv_dgrad, ref_conv_fwd, ref_conv_wgrad, ref_groupnorm
    ops = pkg('ops')
    assert edge_tiles(179, 64) == list(range(64)) + list(range(128, 179)) and edge_tiles(40, 32) == list(range(40))
    assert edge_images(256, 16) == [0, 7, 8, 255] and edge_images(256, 64) == [0, 1, 2, 255] and edge_images(256, 1024) == [0, 255]
    assert edge_images(1, 16) == [0]
    spec, N, Cin, Cout, H = {'3x3': (ops.ConvSpec(3, 1, 1, 0), 10, 40, 70, 8), 'ups': (ops.ConvSpec(3, 1, 1, 1), 5, 24, 33, 4),
                             's2_asym': (ops.ConvSpec(3, 2, 0, 0), 6, 36, 20, 8), 's2_sym': (ops.ConvSpec(3, 2, 1, 0), 6, 36, 20, 8),
                             'same_2x2': (ops.ConvSpec.same(2, 2, 1, 0), 7, 20, 90, 6),
                             '1x1_4x4': (ops.ConvSpec(1, 1, 0, 0), 40, 100, 67, 4)}[case]
    g = torch.Generator().manual_seed(3)
    x = torch.randn(N, Cin, H, H, generator=g, dtype=torch.float64)
    w = torch.randn(Cout, Cin, spec.kh, spec.kw, generator=g, dtype=torch.float64).requires_grad_(True)
    # full fp64 reference by autograd through the plain F.conv2d definition of each geometry
    xv = x.repeat_interleave(2, 2).repeat_interleave(2, 3) if spec.ups else x
    xv = xv.clone().requires_grad_(True)
    if spec.keep:
        xp = F.pad(xv, (spec.pad_w, spec.kw - 1 - spec.pad_w, spec.pad_h, spec.kh - 1 - spec.pad_h))
        y = F.conv2d(xp, w)
    elif spec.stride == 2 and spec.pad == 0:
        y = F.conv2d(F.pad(xv, (0, 1, 0, 1)), w, stride=2)
    else:
        y = F.conv2d(xv, w, stride=spec.stride, padding=spec.pad)
    assert y.shape[2:] == spec.out_hw(H, H)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64)
    y.backward(dy)
    imgs = edge_images(N, y.shape[2] * y.shape[3])
    assert torch.allclose(ref_conv_fwd(x[imgs], w.detach(), spec), y.detach()[imgs], rtol=1e-12, atol=1e-12)
    dimgs = edge_images(N, xv.shape[2] * xv.shape[3])
    assert torch.allclose(ref_conv_dgrad(dy[dimgs], w.detach(), spec, tuple(xv.shape[2:])), xv.grad[dimgs], rtol=1e-12, atol=1e-12)
    rows, cols = edge_tiles(Cout, 64), edge_tiles(Cin, 32)
    got = ref_conv_wgrad(dy[:, rows], x[:, cols], spec, spec.kh, spec.kw, max_elems=5000)      # several image chunks
    assert torch.allclose(got, w.grad[rows][:, cols], rtol=1e-10, atol=1e-10)
    # GroupNorm (+ SiLU) with per-image affine gradients, attention over channel-major tokens
    G, C = 8, 48
    xg = torch.randn(N, C, H, H, generator=g, dtype=torch.float64).requires_grad_(True)
    gm, bt = (1 + 0.2 * torch.randn(C, generator=g, dtype=torch.float64)).requires_grad_(True), torch.randn(C, generator=g, dtype=torch.float64).requires_grad_(True)
    z = F.silu(F.group_norm(xg, G, gm, bt, 1e-6))
    dz = torch.randn(z.shape, generator=g, dtype=torch.float64)
    z.backward(dz)
    gi = edge_images(N, H * H)
    xr = xg.detach()[gi].clone().requires_grad_(True)
    gmi = gm.detach()[None].repeat(len(gi), 1).requires_grad_(True)
    bti = bt.detach()[None].repeat(len(gi), 1).requires_grad_(True)
    zr = ref_groupnorm(xr, gmi, bti, G, 1e-6, True)
    zr.backward(dz[gi])
    assert torch.allclose(zr, z.detach()[gi], atol=1e-12) and torch.allclose(xr.grad, xg.grad[gi], atol=1e-10)
    if len(gi) == N:           # the per-image affine gradients sum to the full ones when every image is in the subset
        assert torch.allclose(gmi.grad.sum(0), gm.grad, atol=1e-10) and torch.allclose(bti.grad.sum(0), bt.grad, atol=1e-10)
    yg = F.group_norm(xg.detach(), G, gm.detach(), bt.detach(), 1e-6)
    dyg = dz * torch.sigmoid(yg) * (1 + yg * (1 - torch.sigmoid(yg)))               # dL/d(affine output), per image
    assert torch.allclose(bti.grad, dyg[gi].sum((2, 3)), atol=1e-10)
    q, k, v = (torch.randn(N, 2 * 12, H, H, generator=g, dtype=torch.float64) for _ in range(3))
    full = F.scaled_dot_product_attention(q.view(N, 2, 12, -1).transpose(2, 3), k.view(N, 2, 12, -1).transpose(2, 3),
                                          v.view(N, 2, 12, -1).transpose(2, 3), scale=0.3).transpose(2, 3).reshape(q.shape)
    assert torch.allclose(ref_attention(q[gi], k[gi], v[gi], 2, 0.3), full[gi], atol=1e-12)


# ----------------------------------------------------------------------------------- full-size sampling (teacher-forced)
def _c1_pruned_oracle_params(dtype):
    """The seeded CIFAR parameters with the reference's C1 pruned index lists (cifar_c1.json) sliced out, group by group: the
    parameters of the ratio-0.3 pruned model without running the sweep again."""
    from oracle import pruning_ref as R
    G = pkg('graph')
    fx = load_json('cifar_c1.json')
    P = {n: t.to(dtype) for n, t in oracle_params(gc.CIFAR_CFG, 0, requires_grad=False).items()}
    gr = G.UNetGraph(gc.CIFAR_CFG)
    for r in fx['prune']:
        for m in G.coupled_members(gr, G.ChannelView({n: tuple(t.shape) for n, t in P.items()}), r['root'], r['pruned']):
            R.slice_member(P, {}, m.name, 'gn' if m.kind == 'ln' else m.kind, m.idxs)
    assert {n: list(t.shape) for n, t in P.items()} == fx['shapes_after']
    assert sum(t.numel() for t in P.values()) == 19851157
    return P


def _fp64_matches_fixture(got64, fixture32, sums=None):
    """`got64` (fp64) against an fp64 result the reference wrote rounded to fp32: within half an fp32 ulp of the stored value (+1e-9),
    and, where the fixture kept them, the fp64 sum / abs-sum / sum of squares of the unrounded result to 1e-9 relative."""
    ref = torch.from_numpy(fixture32).double()
    half_ulp = torch.from_numpy(np.spacing(np.abs(fixture32)).astype(np.float64)) / 2
    err = float(((got64 - ref).abs() - half_ulp).max())
    assert err <= 1e-9, err
    if sums is not None:
        mine = [float(got64.sum()), float(got64.abs().sum()), float((got64 * got64).sum())]
        for a, b in zip(mine, sums):
            assert abs(a - b) <= 1e-9 * max(1.0, abs(b)), (mine, list(sums))


@pytest.mark.parametrize('model', ['full', 'pruned'])
def test_oracle_reproduces_full_size_sampling_fixtures(model):
    """tests/golden/sampling_cifar*.npz (make_golden_sampling.py): the reference's fp64 eps and DDIMScheduler.step outputs on x_k of
    its fp64 100-step trajectory of the full-size CIFAR UNet and of the C1 ratio-0.3 pruned one.  The oracle in fp64
    (unet_ref.unet_forward, diffusion_ref.ddim_step) reproduces them at three stored steps (t = 999, 494 and 0, where the step uses
    final_alpha_cumprod); on the full model also the eta 0.5, quad-schedule and DDPM (t = 999, 500, 1, 0) steps."""
    from oracle import diffusion_ref as D, unet_ref as U
    g = load_npz('sampling_cifar.npz' if model == 'full' else 'sampling_cifar_pruned.npz')
    P = ({n: t.double() for n, t in oracle_params(gc.CIFAR_CFG, int(g['model_seed']), requires_grad=False).items()}
         if model == 'full' else _c1_pruned_oracle_params(torch.float64))
    assert sum(t.numel() for t in P.values()) == int(g['params'])
    acp = D.alphas_cumprod()
    steps = [int(k) for k in g['steps']]
    n = int(g['n_steps'])
    assert np.array_equal(D.ddim_timesteps(n).numpy()[steps], g['timesteps'])
    with torch.no_grad():
        for i in (steps.index(0), steps.index(50), steps.index(99)):
            t = int(g['timesteps'][i])
            x = torch.from_numpy(g['x'][i]).double()
            eps = U.unet_forward(P, gc.CIFAR_CFG, x, torch.tensor([t]))
            _fp64_matches_fixture(eps, g['eps'][i], g['eps_sums'][i])
            _fp64_matches_fixture(D.ddim_step(acp, eps, t, x, n), g['out'][i], g['out_sums'][i])
        if model == 'pruned':
            return
        e = load_npz('sampling_cifar_edges.npz')
        for kind in ('eta', 'quad', 'ddpm'):
            for j in range(int(e['n_' + kind])):
                f = lambda k: e['%s:%d:%s' % (kind, j, k)]
                t = int(f('t'))
                x = torch.from_numpy(f('x')).double()
                eps = U.unet_forward(P, gc.CIFAR_CFG, x, torch.tensor([t]))
                _fp64_matches_fixture(eps, f('eps'))
                if kind == 'eta':
                    out = D.ddim_step(acp, eps, t, x, n, eta=float(e['eta']), variance_noise=torch.from_numpy(f('noise')).double())
                elif kind == 'quad':
                    assert int(e['quad_timesteps'][int(f('step'))]) == t == int(D.ddim_timesteps(n, skip_type='quad')[int(f('step'))])
                    out = D.ddim_step(acp, eps, t, x, n)
                else:
                    out = D.ddpm_step(acp, eps, t, x, 1000, variance_noise=torch.from_numpy(f('noise')).double())
                _fp64_matches_fixture(out, f('out'), f('out_sums'))
