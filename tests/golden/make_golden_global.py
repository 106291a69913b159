#!/usr/bin/env python3
"""Golden vectors for GLOBAL pruning -- build container only; imports the reference's own vendored torch_pruning and model code
through the shims of make_golden.py / make_golden_ldm.py and drives the reference's own `MagnitudePruner(global_pruning=True)`
(ddpm_exp/torch_pruning/pruner/algorithms/metapruner.py:126-133, 256-297).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_global.py

Writes tests/golden/global_prune.json and, for the number arrays, global_prune.npz beside it (data only).  Per case and pruning step:
  initial_total_channels, n_pruned, the threshold (an fp32 value), and per scored group a row [root, ch_groups, number of ranked
  scores, yielded (0 / 1), pruned indices as ranges (empty lists included)]; in the .npz under `<case>/<step>/score32` the ranked fp32
  scores of all groups in group order, exactly as the reference's prune_global ranks them (the first sub-group's for a grouped root),
  and under `.../score64` the same scores computed in fp64 by the reference's own criterion on the model converted to double;
  gap      relative gap between the k-th and the (k+1)-th smallest ranked score, (s[k] - s[k-1]) / s[k]  (k = n_pruned);
  err64    the largest relative difference between a ranked fp32 score and its fp64 value.
CONDITION asserted here for every committed case: gap >= 100 * err64 -- the mask is decided with two orders of magnitude to spare
over fp32 rounding, so an implementation that sums in another order still has to reproduce it.
After the last step: shapes_after (the parameter shapes in named_parameters() order) and, in the .npz, `<case>/fwd_after` (the pruned
reference model's output on the stored input).  tests/test_prune_global_cpu.py `load_fixture` puts the two files together again."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import numpy as np
import torch
import golden_common as gc
import make_golden as mg                                            # the reference import shim + helpers (no fixture is written)
import make_golden_ldm as mgl                                       # the LDM UNetModel of the reference

tp = mg.tp


class Recorder:
    """The criterion handed to the pruner: the reference's own, with every call logged."""

    def __init__(self, imp):
        self.imp, self.log = imp, []

    def __call__(self, group, ch_groups=1):
        s = self.imp(group, ch_groups=ch_groups)
        self.log.append((group, ch_groups, s))
        return s


def global_step(model, pruner, rec, names):
    """One `pruner.step(interactive=True)` of the reference with global_pruning=True, pruning every yielded group."""
    del rec.log[:]
    asked = {}                                                      # root -> the index list prune_global hands to get_pruning_group
    real = pruner.DG.get_pruning_group

    def logged(module, fn, idxs):
        asked[names[module]] = [int(i) for i in idxs]
        return real(module, fn, idxs)
    pruner.DG.get_pruning_group = logged
    gen = pruner.step(interactive=True)
    first = next(gen, None)                                         # prune_global has scored every group now; nothing is pruned yet
    scored = [(g, c, s) for g, c, s in rec.log if s is not None]
    ranked32 = [(s[:len(s) // c] if c > 1 else s).detach().clone() for _, c, s in scored]
    model.double()                                                  # parameters AND accumulated gradients, in place
    try:
        ranked64 = []
        for g, c, _ in scored:
            s = rec.imp(g, ch_groups=c)
            assert s.dtype == torch.float64
            ranked64.append((s[:len(s) // c] if c > 1 else s).detach().clone())
    finally:
        model.float()
    cat32, cat64 = torch.cat(ranked32), torch.cat(ranked64)
    n_pruned = len(cat32) - int(pruner.initial_total_channels * (1 - pruner.per_step_ch_sparsity[pruner.current_step]))
    assert 0 < n_pruned < len(cat32)
    srt = torch.sort(cat32).values
    thres = torch.topk(cat32, k=n_pruned, largest=False)[0][-1]
    assert float(srt[n_pruned - 1]) == float(thres)
    gap = float((srt[n_pruned].double() - srt[n_pruned - 1].double()) / srt[n_pruned].double())
    err64 = float(((cat32.double() - cat64).abs() / cat64.abs()).max())
    assert gap >= 100 * err64, ('the fixture condition does not hold: move the seed or the ratio', gap, err64)
    yielded = set()
    g = first
    while g is not None:
        root = names[g[0][0].target.module]
        assert root not in yielded
        yielded.add(root)
        g.prune()
        g = next(gen, None)
    pruner.DG.get_pruning_group = real
    groups = []
    for (grp, c, _), s32, s64 in zip(scored, ranked32, ranked64):
        root = names[grp[0][0].target.module]
        idxs = asked[root]
        base = (s32 <= thres).nonzero().view(-1).tolist()           # what prune_global computes, restated: <= threshold, replicated
        full = [i + (len(grp[0][1]) // c) * j for j in range(c) for i in base] if c > 1 else base
        if pruner.round_to:
            full = full[:len(full) - len(full) % pruner.round_to]
        assert full == idxs, root
        groups.append([root, int(c), len(s32), int(root in yielded), mg.compress(idxs)])
    return dict(n_pruned=int(n_pruned), n_ranked=int(len(cat32)), threshold=float(thres), gap=gap, err64=err64,
                groups=groups), cat32.numpy(), cat64.numpy()


def run_case(model, ex, imp, ratio, steps, ignored, channel_groups, round_to, forward):
    rec = Recorder(imp)
    pruner = tp.pruner.MagnitudePruner(model, ex, importance=rec, global_pruning=True, iterative_steps=steps,
                                       channel_groups=channel_groups, ch_sparsity=ratio, ignored_layers=ignored, round_to=round_to)
    names = mg.name_of(model)
    out = dict(ratio=ratio, iterative_steps=steps, initial_total_channels=int(pruner.initial_total_channels), steps=[])
    arrays = {}
    for i in range(steps):
        st, arrays['%d/score32' % i], arrays['%d/score64' % i] = global_step(model, pruner, rec, names)
        out['steps'].append(st)
    for m in model.modules():
        if isinstance(m, (mg.Upsample2D, mg.Downsample2D)):
            m.channels = m.conv.in_channels
        if isinstance(m, mg.Attention):
            m.set_processor(mg.AttnProcessor())
    with torch.no_grad():
        y = forward(model)
    out.update(shapes_after=[list(p.shape) for _, p in model.named_parameters()],
               params_after=int(sum(p.numel() for p in model.parameters())))
    arrays['fwd_after'] = y.numpy()
    return out, arrays


def tiny_case(crit, ratio, steps=1):
    cfg = gc.TINY_CFG
    H = cfg['sample_size']
    model = mg.build_ref_unet(cfg, 5)
    sched = mg.DDPMScheduler(num_train_timesteps=1000)
    clean = torch.from_numpy(gc.det_clean((2, 3, H, H), 1))
    noise = torch.from_numpy(gc.det_noise((2, 3, H, H), 2))
    t = torch.tensor([3, 500])
    mg.sweep(model, sched, clean, noise, 4)
    ex = {'sample': torch.randn(1, 3, H, H), 'timestep': torch.ones((1,)).long()}
    imp = tp.importance.TaylorImportance() if crit == 'taylor' else tp.importance.MagnitudeImportance()
    return run_case(model, ex, imp, ratio, steps, [model.conv_out], {}, None,
                    lambda m: m(sched.add_noise(clean, noise, t), t).sample)


def heads_case(ratio):
    cfg = json.load(open(os.path.join(HERE, 'groups_more.json')))['heads8_4lvl']['cfg']
    model = mg.build_ref_unet(cfg, 4)
    sched = mg.DDPMScheduler(num_train_timesteps=1000)
    clean = torch.from_numpy(gc.det_clean((2, 3, 16, 16), 81))
    noise = torch.from_numpy(gc.det_noise((2, 3, 16, 16), 82))
    t = torch.tensor([5, 700])
    mg.sweep(model, sched, clean, noise, 2)
    channel_groups = {}
    for m in model.modules():
        if isinstance(m, mg.Attention):
            channel_groups[m.to_q] = channel_groups[m.to_k] = channel_groups[m.to_v] = m.heads
    ex = {'sample': torch.randn(1, 3, 16, 16), 'timestep': torch.ones((1,)).long()}
    return run_case(model, ex, tp.importance.TaylorImportance(), ratio, 1, [model.conv_out], channel_groups, None,
                    lambda m: m(sched.add_noise(clean, noise, t), t).sample)


def ldm_case(ratio):
    from ldm.modules.attention import CrossAttention
    cfg = gc.LDM_TINY_CFG
    m = mgl.UNetModel(**cfg).eval()
    gc.det_init_(m, 9)
    H = cfg['image_size']
    x = torch.from_numpy(gc.det_noise((2, 3, H, H), 31))
    ctx = torch.from_numpy(gc.det_noise((2, 1, cfg['context_dim']), 32))
    noise = torch.from_numpy(gc.det_noise((2, 3, H, H), 33))
    t = torch.tensor([7, 640])
    ex = {'x': torch.randn(2, 3, H, H), 'timesteps': torch.full((2,), 1, dtype=torch.long), 'context': torch.randn(2, 1, cfg['context_dim'])}
    channel_groups = {}
    for mod in m.modules():
        if isinstance(mod, CrossAttention):
            channel_groups[mod.to_q] = channel_groups[mod.to_k] = channel_groups[mod.to_v] = mod.heads
    m.zero_grad()
    (m(x, t, context=ctx) - noise).square().mean(dim=(1, 2, 3)).mean().backward()
    # the pruner is built AFTER the backward here (its constructor only traces); prune_ldm.py:89-100 arguments
    return run_case(m, ex, tp.importance.TaylorImportance(), ratio, 1, [m.out], channel_groups, 2, lambda mm: mm(x, t, context=ctx))


CASES = {
    'tiny_taylor_0.1': lambda: tiny_case('taylor', 0.1),
    'tiny_taylor_0.3': lambda: tiny_case('taylor', 0.3),
    'tiny_taylor_0.5': lambda: tiny_case('taylor', 0.5),
    'tiny_magnitude_0.3': lambda: tiny_case('magnitude', 0.3),
    'tiny_taylor_0.3_two_steps': lambda: tiny_case('taylor', 0.3, steps=2),
    'tiny_heads_taylor_0.3': lambda: heads_case(0.3),
    'ldm_tiny_taylor_0.3': lambda: ldm_case(0.3),
}


if __name__ == '__main__':
    out, arrays = {}, {}
    for name, fn in CASES.items():
        out[name], arr = fn()
        arrays.update({name + '/' + k: v for k, v in arr.items()})
        print(name, 'total', out[name]['initial_total_channels'],
              [(s['n_pruned'], len(s['groups']), sum(g[3] for g in s['groups']), sum(1 for g in s['groups'] if not g[4]),
                '%.2e' % s['gap'], '%.2e' % s['err64']) for s in out[name]['steps']], 'params', out[name]['params_after'])
    path = os.path.join(HERE, 'global_prune.json')
    with open(path, 'w') as f:                                      # one line per case
        f.write('{\n' + ',\n'.join('%s: %s' % (json.dumps(k), json.dumps(v, separators=(',', ':'))) for k, v in out.items()) + '\n}\n')
    np.savez_compressed(os.path.join(HERE, 'global_prune.npz'), **arrays)
    print('global_prune.json', os.path.getsize(path), 'bytes; global_prune.npz', os.path.getsize(path[:-4] + 'npz'), 'bytes')
