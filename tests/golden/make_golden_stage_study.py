#!/usr/bin/env python3
"""Fixture of the stage study (build container only, on the CPU): the reference's own ddpm_exp model (models/diffusion.py), loss
(functions/losses.py), sampler step (functions/denoising.generalized_steps) and vendored torch_pruning, driven through the stage loop
of ddpm_exp/prune_ssim.py:252-272 as written -- model.zero_grad(); for step_k in range(stage): loss = loss_registry['simple'](model,
x, t, e, b); loss.backward(); then `for g in pruner.step(interactive=True): g.prune()` -- once per stage in STAGES, each on a fresh
copy of one seeded model, in fp32 and in fp64 (model, inputs and betas upcast), at ratio 0.3 with the script's pruner arguments
(:208-217).  After each prune a 5-step generalized_steps chain (eta = 0) runs from one stored x_T (n = 4).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_stage_study.py [model seed]

Writes stage_study.json, stage_study.npz and stage_study.samples.npz (data only, each under 1 MiB):
  json   cfg (the tiny original-DDPM configuration of ddpm_original.json), seeds, stages, ratio, chain seq, the 20 fp32 losses of the
         longest run (a shorter run's losses are its prefix: asserted), param_names (the reference's named_parameters() order before
         pruning) and per stage: groups = [[root, ch_groups, ranges of pruned indices, gap, err64] ...] in the pruner's order, shapes_after
         {name: shape}, params_after, chain_gap (the fp32 chain's final state against the fp64 one, max abs);
         gap    smallest relative gap between the last pruned and the first kept fp32 score over the group's selections (one per
                sub-group of a GroupNorm-grouped root, metapruner.py:232-247); null when nothing is picked (groups that lose no
                channel are yielded with an empty list, and recorded);
         err64  largest relative difference between a score of the fp32 run and of the fp64 run of that group.
         CONDITION asserted here for every group of every stage that picks: gap >= 100 * err64 (the rule of make_golden_global.py), and both
         runs prune the same channels.
  npz    sample_idx, sample_count up to 96 sampled flat positions of every parameter (seeded by its position), concatenated in
                                  parameter order, and how many each parameter has; shared by every stage
         <stage>/norm64           per-parameter L2 norm of the fp64 run's accumulated gradients before the prune
         <stage>/norm_err32       |norm32 - norm64| / norm64 of the fp32 run (0 where norm64 is 0)
         <stage>/samples64        the fp64 gradients at the sampled positions, concatenated likewise (in stage_study.samples.npz)
         <stage>/sample_err32     per parameter ||g32[idx] - g64[idx]|| / ||g64[idx]|| of the fp32 run (0 where the norm is 0)
         <stage>/chain64, chain32 the chain's final state in both precisions; <stage>/bytes  uint8 [4, 16, 16, 3] of the fp32 state:
         (unsigned char) clamp(clamp((x + 1) / 2, 0, 1) * 255 + 0.5, 0, 255), inverse_data_transform + save_image's conversion
         x_T                      the chain's start
Stage 0 is the unpruned model (prune_ssim.py:236 `args.stage > 0`): no gradients, no groups, the chain of the seeded model."""
import copy
import json
import os
import sys
from types import SimpleNamespace as NS

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import numpy as np                                                  # noqa: E402
import torch                                                        # noqa: E402
import golden_common as gc                                          # noqa: E402
import make_golden as mg                                            # noqa: E402  (reference import shim: sys.path, cwd, torch_pruning)
import make_golden_ddpm_exp_sampler as mgs                          # noqa: E402  (on_cpu: the reference's .to('cuda') on this host)
import models.diffusion as MD                                       # noqa: E402  (reference, ddpm_exp)
from models.diffusion import Model                                  # noqa: E402
from functions.losses import loss_registry                          # noqa: E402
from functions.denoising import generalized_steps                   # noqa: E402

tp = mg.tp
CFG = dict(ch=32, ch_mult=[1, 2, 2, 2], num_res_blocks=2, attn_resolutions=[8], image_size=16)
MODEL_SEED = 24                                                     # the first seed from 21 on for which the CONDITION holds
CLEAN_SEED, NOISE_SEED, XT_SEED = 141, 142, 143
B, N_CHAIN, T = 4, 4, 20
STAGES = (0, 1, 5, 10, 15, 20)
RATIO = 0.3
CHAIN_SEQ = list(range(0, 1000, 200))                                # runners/diffusion.py:498-503, 'uniform', 5 timesteps
N_SAMPLES = 96


def build(seed):
    config = NS(model=NS(type='simple', in_channels=3, out_ch=3, ch=CFG['ch'], ch_mult=CFG['ch_mult'],
                         num_res_blocks=CFG['num_res_blocks'], attn_resolutions=CFG['attn_resolutions'], dropout=0.0,
                         resamp_with_conv=True),
                data=NS(image_size=CFG['image_size']), diffusion=NS(num_diffusion_timesteps=1000))
    model = Model(config).eval()
    with torch.no_grad():
        for n, p in model.named_parameters():
            p.copy_(torch.from_numpy(gc.det_param(n, tuple(p.shape), seed)))
    return model


_EMB_DTYPE = [torch.float32]
_real_embedding = MD.get_timestep_embedding
# models/diffusion.py:18-21 builds the sinusoidal embedding in fp32 whatever the model's dtype, and a double Linear refuses it: the
# fp64 run is handed the reference's own fp32 embedding, upcast (an input of the network, like x and e; identity for the fp32 run)
MD.get_timestep_embedding = lambda t, dim: _real_embedding(t, dim).to(_EMB_DTYPE[0])


class Recorder:
    """The criterion handed to the pruner: the reference's own, with every call logged."""

    def __init__(self, imp):
        self.imp, self.log = imp, []

    def __call__(self, group, ch_groups=1):
        s = self.imp(group, ch_groups=ch_groups)
        self.log.append(None if s is None else (s.detach().clone(), int(ch_groups)))
        return s


def stage_run(seed_model, stage, dtype, x, e, b, x_T):
    """prune_ssim.py:208-217 (the pruner), :236-272 (the stage loop and the prune), then the chain.  Everything in `dtype`."""
    model = copy.deepcopy(seed_model).to(dtype)
    _EMB_DTYPE[0] = dtype
    x, e, b, x_T = x.to(dtype), e.to(dtype), b.to(dtype), x_T.to(dtype)
    n = x.size(0)
    rec = Recorder(tp.importance.TaylorImportance())
    example_inputs = {'x': torch.randn(1, 3, CFG['image_size'], CFG['image_size']).to(dtype), 't': torch.ones(1).to(dtype)}
    pruner = tp.pruner.MagnitudePruner(model, example_inputs, importance=rec, iterative_steps=1, channel_groups={},
                                       ch_sparsity=RATIO, ignored_layers=[model.conv_out],
                                       root_module_types=[torch.nn.Conv2d, torch.nn.Linear])
    names = mg.name_of(model)
    loss_list, grads, groups = [], None, []
    if stage > 0:
        model.zero_grad()
        for step_k in range(0, stage):
            t = torch.ones(n, dtype=torch.long) * step_k
            loss = loss_registry['simple'](model, x, t, e, b)
            loss_list.append(loss.item())
            loss.backward()
        grads = [p.grad.detach().clone() for _, p in model.named_parameters()]
        asked, real = {}, pruner.DG.get_pruning_group           # root -> the index list prune_local hands to get_pruning_group

        def logged(module, fn, idxs):
            asked[names[module]] = sorted(int(i) for i in idxs)
            return real(module, fn, idxs)
        pruner.DG.get_pruning_group = logged
        for g in pruner.step(interactive=True):
            root = names[g[0][0].target.module]
            groups.append((root, asked[root]))
            g.prune()
        pruner.DG.get_pruning_group = real
    scores = [s for s in rec.log if s is not None]
    with torch.no_grad():
        with mgs.on_cpu([torch.zeros_like(x_T).double()]):
            xs, _ = generalized_steps(x_T, CHAIN_SEQ, model, b, eta=0.0)
    assert xs[-1].dtype == dtype
    return dict(losses=loss_list, grads=grads, groups=groups, scores=scores, final=xs[-1],
                shapes={k: list(p.shape) for k, p in model.named_parameters()})


def group_margin(s32, s64, ch_groups, n_pruned):
    """(gap, err64) of one group.  gap: the smallest relative distance between the last pruned and the first kept fp32 score over the
    selections prune_local makes (metapruner.py:232-247: one argsort per sub-group of a GroupNorm-grouped root, n_pruned // ch_groups
    each); None when no selection picks between two scores (nothing or everything of every sub-group goes)."""
    size, k = len(s32) // ch_groups, n_pruned // ch_groups
    gaps = []
    for c in range(ch_groups):
        srt = torch.sort(s32[c * size:(c + 1) * size].double()).values
        if 0 < k < size:
            gaps.append(float((srt[k] - srt[k - 1]) / srt[k]))
    err = float(((s32.double() - s64).abs() / s64.abs()).max())
    return (min(gaps) if gaps else None), err


def main(seed):
    torch.manual_seed(0)
    seed_model = build(seed)
    H = CFG['image_size']
    x = torch.from_numpy(gc.det_clean((B, 3, H, H), CLEAN_SEED))
    e = torch.from_numpy(gc.det_noise((B, 3, H, H), NOISE_SEED))
    x_T = torch.from_numpy(gc.det_noise((N_CHAIN, 3, H, H), XT_SEED))
    b = torch.from_numpy(np.linspace(0.0001, 0.02, 1000, dtype=np.float64)).float()      # runners/diffusion.py:88-96
    params = list(seed_model.named_parameters())
    meta = dict(cfg=CFG, model_seed=seed, clean_seed=CLEAN_SEED, noise_seed=NOISE_SEED, xT_seed=XT_SEED, batch=B, n_chain=N_CHAIN,
                timesteps=T, stages=list(STAGES), ratio=RATIO, chain_seq=CHAIN_SEQ, param_names=[n for n, _ in params], per_stage={})
    arrays = {'x_T': x_T.numpy()}
    idx, samples = [], {}
    for i, (_, p) in enumerate(params):
        r = np.random.default_rng(1000 + i)
        idx.append(np.sort(r.choice(p.numel(), size=min(N_SAMPLES, p.numel()), replace=False)).astype(np.int32))
    arrays['sample_idx'] = np.concatenate(idx)
    arrays['sample_count'] = np.array([len(v) for v in idx], np.int32)
    worst, run_losses = (np.inf, None), {}
    for stage in STAGES:
        r32 = stage_run(seed_model, stage, torch.float32, x, e, b, x_T)
        r64 = stage_run(seed_model, stage, torch.float64, x, e, b, x_T)
        run_losses[stage] = r32['losses']
        if stage == T:
            meta['losses'] = r32['losses']
            meta['losses64'] = r64['losses']
        st = dict(groups=[], shapes_after=r32['shapes'], params_after=int(sum(int(np.prod(s)) for s in r32['shapes'].values())))
        assert [g[0] for g in r32['groups']] == [g[0] for g in r64['groups']] and len(r32['scores']) == len(r64['scores'])
        if stage > 0:
            assert len(r32['scores']) == len(r32['groups']), 'a scored group that was not pruned: restate the bookkeeping'
            for (root, pruned), (_, pruned64), (s32, chg), (s64, chg64) in zip(r32['groups'], r64['groups'], r32['scores'], r64['scores']):
                assert chg == chg64 and len(pruned) == (len(pruned) // chg) * chg
                gap, err = group_margin(s32, s64, chg, len(pruned))
                assert pruned == pruned64, (stage, root)
                assert gap is None or gap >= 100 * err, ('the fixture condition does not hold: move the seed', stage, root, gap, err)
                if gap is not None and gap / max(err, 1e-300) < worst[0]:
                    worst = (gap / max(err, 1e-300), (stage, root, gap, err))
                st['groups'].append([root, chg, mg.compress(pruned), gap, err])
            n64, ne, se, picked = [], [], [], []
            for i, (g32, g64) in enumerate(zip(r32['grads'], r64['grads'])):
                a, c = g32.double().reshape(-1), g64.reshape(-1)
                n64.append(float(c.norm()))
                ne.append(abs(float(a.norm()) - n64[-1]) / n64[-1] if n64[-1] > 0 else 0.0)
                sa, sc = a[idx[i].astype(np.int64)], c[idx[i].astype(np.int64)]
                se.append(float((sa - sc).norm() / sc.norm()) if float(sc.norm()) > 0 else 0.0)
                picked.append(sc.numpy())
            samples['%d/samples64' % stage] = np.concatenate(picked)
            arrays['%d/norm64' % stage] = np.array(n64, np.float64)
            arrays['%d/norm_err32' % stage] = np.array(ne, np.float64)
            arrays['%d/sample_err32' % stage] = np.array(se, np.float64)
        else:
            assert not r32['groups'] and not r32['scores']
        f32, f64 = r32['final'], r64['final']
        st['chain_gap'] = float((f32.double() - f64).abs().max())
        arrays['%d/chain64' % stage] = f64.numpy()
        arrays['%d/chain32' % stage] = f32.numpy()
        u = torch.clamp((f32 + 1.0) / 2.0, 0.0, 1.0)
        arrays['%d/bytes' % stage] = torch.clamp(u * 255 + 0.5, 0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous().numpy()
        meta['per_stage'][str(stage)] = st
        print('stage %2d: %2d groups, params %d, chain gap %.2e' % (stage, len(st['groups']), st['params_after'], st['chain_gap']))
    for stage, l in run_losses.items():                             # a shorter run's losses are a prefix of the longest run's
        assert l == meta['losses'][:stage], stage
    print('thinnest group: gap / err64 = %.1f at %r' % worst)
    path = os.path.join(HERE, 'stage_study.json')
    with open(path, 'w') as f:
        json.dump(meta, f, separators=(',', ':'))
    mgs._savez('stage_study.npz', arrays)
    mgs._savez('stage_study.samples.npz', samples)
    for name in ('stage_study.json', 'stage_study.npz', 'stage_study.samples.npz'):
        size = os.path.getsize(os.path.join(HERE, name))
        assert size < (1 << 20), (name, size)
        print(name, size, 'bytes')


if __name__ == '__main__':
    main(int(sys.argv[1]) if len(sys.argv) > 1 else MODEL_SEED)
