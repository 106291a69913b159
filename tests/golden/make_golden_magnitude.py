#!/usr/bin/env python3
"""Golden vectors for the data-free magnitude criteria -- build container only; imports the reference's own vendored torch_pruning and
model code through the shims of make_golden.py / make_golden_ldm.py and runs the reference's own `MagnitudeImportance`
(ddpm_exp/torch_pruning/importance.py:18-126), `LAMPImportance` (:154-219) and `MagnitudePruner`.

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_magnitude.py [--masks-only]      (--masks-only keeps the score tables)

Writes tests/golden/magnitude_family.json and, for the number arrays, magnitude_family_<model>.npz beside it (data only; one file per
model keeps each under the size limit of a committed file).  Models: `tiny` (golden_common.TINY_CFG), `heads` (the 8-head four-level
UNet of groups_more.json, heads as channel_groups) and `ldm` (LDM_TINY_CFG, heads as channel_groups).

Scores.  Per model `groups` = [root, width] of every scored group in enumeration order, and per criterion configuration
  `<class>/<p>/<reduction>/<normalizer>`, from the reference's class on the model converted with .double():  in the .npz `.../ref`,
  per group, the fp64 scores at the channels magnitude_ref.sample_positions(width) followed by the vector's max-abs, all groups
  concatenated, stored as float32; in the .json e_ref32 = the largest helpers.relerr (max-abs error over the group's max-abs score) of
  a group's FULL fp32 vector, as the reference's class returns it, against its full fp64 one.
  Why samples, and float32: the three models have 3008 / 2400 / 23584 scored channels and there are 120 (122) configurations, so
  the full vectors in both precisions are 42 MB; every group of every configuration is still held to the reference's own numbers.
  Rounding the fp64 value to float32 moves it by 6e-8 of itself, 1/160 of the smallest bound a score is judged with (1e-5).  The
  mask cases below pin complete vectors through their decisions.
  MagnitudeImportance: p in 1, 2, 3, 0.5 x five reductions x six normalisers on all three models; LAMPImportance: p in 1, 2 on the
  two DDPM-family models (on the LDM UNet the vendored class raises for 16 groups).
Masks.  Per case the reference's own MagnitudePruner with the named criterion, at ratio 0.3 or the first of RATIOS at which the
  condition below holds (recorded as `ratio`): per yielded group [root, ch_groups, pruned
  indices as ranges], shapes_after, in the .npz `<case>/fwd_after`, and the numbers of the condition below.
CONDITIONS asserted here:
  * every mask case decides with a gap of at least 100 times the reference's own fp32-against-fp64 score error: global cases as
    global_prune.json does (relative gap between the k-th and (k+1)-th smallest ranked score against the largest element-wise relative
    error); local cases per ranked (sub-)group, the gap and the error both over the group's max-abs score ('standarization' crosses
    zero, where an element-wise relative error means nothing);
  * no LAMP vector holds two equal scores;
  * at least one global case yields a mask that the same criterion WITHOUT its normaliser does not yield (what a build that ignores
    `normalizer` would give): recorded per global case as `differs_without_normalizer`.
`parent_default/*` arrays (the bits of MagnitudeImportance(2, 'mean', 'mean') recorded from the commit before csrc/magnitude.hip, over
tests/mock_ops.py) are carried over from the existing files, not regenerated."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(1, os.path.dirname(HERE))
import numpy as np
import torch
import golden_common as gc
import make_golden as mg                                            # the reference import shim + helpers (no fixture is written)
import make_golden_ldm as mgl                                       # the LDM UNetModel of the reference
from magnitude_ref import sample_positions

tp = mg.tp
PS = [1, 2, 3, 0.5]
REDUCTIONS = ['sum', 'mean', 'max', 'prod', 'first']
NORMALIZERS = [None, 'sum', 'standarization', 'mean', 'max', 'gaussian']
RATIOS = [0.3, 0.29, 0.31, 0.28, 0.32, 0.27, 0.33]          # 0.3; the next one where a case's deciding gap is too narrow


def build(model_name):
    """-> (model, example inputs, ignored layers, channel_groups, forward)"""
    if model_name == 'ldm':
        from ldm.modules.attention import CrossAttention
        cfg = gc.LDM_TINY_CFG
        m = mgl.UNetModel(**cfg).eval()
        gc.det_init_(m, 9)
        H = cfg['image_size']
        x = torch.from_numpy(gc.det_noise((2, 3, H, H), 31))
        ctx = torch.from_numpy(gc.det_noise((2, 1, cfg['context_dim']), 32))
        t = torch.tensor([7, 640])
        ex = {'x': torch.randn(2, 3, H, H), 'timesteps': torch.full((2,), 1, dtype=torch.long),
              'context': torch.randn(2, 1, cfg['context_dim'])}
        chg = {}
        for mod in m.modules():
            if isinstance(mod, CrossAttention):
                chg[mod.to_q] = chg[mod.to_k] = chg[mod.to_v] = mod.heads
        return m, ex, [m.out], chg, lambda mm: mm(x, t, context=ctx)
    if model_name == 'heads':
        cfg, seed, cs, ns, t = json.load(open(os.path.join(HERE, 'groups_more.json')))['heads8_4lvl']['cfg'], 4, 81, 82, [5, 700]
    else:
        cfg, seed, cs, ns, t = gc.TINY_CFG, 5, 1, 2, [3, 500]
    H = cfg['sample_size']
    model = mg.build_ref_unet(cfg, seed)
    sched = mg.DDPMScheduler(num_train_timesteps=1000)
    clean = torch.from_numpy(gc.det_clean((2, 3, H, H), cs))
    noise = torch.from_numpy(gc.det_noise((2, 3, H, H), ns))
    t = torch.tensor(t)
    chg = {}
    if model_name == 'heads':
        for m in model.modules():
            if isinstance(m, mg.Attention):
                chg[m.to_q] = chg[m.to_k] = chg[m.to_v] = m.heads
    ex = {'sample': torch.randn(1, 3, H, H), 'timestep': torch.ones((1,)).long()}
    return model, ex, [model.conv_out], chg, lambda m: m(sched.add_noise(clean, noise, t), t).sample


def criterion(cls, p, red, norm):
    return getattr(tp.importance, cls)(p=p, group_reduction=red, normalizer=norm)


def relerr(a, ref):
    return float(np.max(np.abs(a.astype(np.float64) - ref)) / np.max(np.abs(ref)))


def score_table(model_name):
    model, ex, ignored, chg, _ = build(model_name)
    pruner = tp.pruner.MagnitudePruner(model, ex, importance=tp.importance.MagnitudeImportance(), iterative_steps=1, channel_groups=chg,
                                       ch_sparsity=0.3, ignored_layers=ignored)
    names = mg.name_of(model)
    groups = list(pruner.DG.get_all_groups(ignored_layers=pruner.ignored_layers, root_module_types=pruner.root_module_types))
    configs = [('MagnitudeImportance', p, r, n) for p in PS for r in REDUCTIONS for n in NORMALIZERS]
    if model_name != 'ldm':
        configs += [('LAMPImportance', p, 'mean', 'mean') for p in (1, 2)]
    out, arrays, widths = {}, {}, None
    for cls, p, red, norm in configs:
        imp = criterion(cls, p, red, norm)
        s32 = [imp(g, ch_groups=pruner.get_channel_groups(g)) for g in groups]
        model.double()
        try:
            s64 = [imp(g, ch_groups=pruner.get_channel_groups(g)) for g in groups]
        finally:
            model.float()
        assert all(s is not None and s.dtype == torch.float32 and s.dim() == 1 for s in s32) and all(s.dtype == torch.float64 for s in s64)
        w = [[names[g[0][0].target.module], len(s)] for g, s in zip(groups, s32)]
        assert widths is None or widths == w
        widths = w
        a32, a64 = [s.numpy() for s in s32], [s.numpy() for s in s64]
        if cls == 'LAMPImportance':
            assert all(len(np.unique(a)) == len(a) for a in a32), 'a LAMP vector holds two equal scores'
        key = '%s/%s/%s/%s' % (cls, p, red, norm)
        out[key] = dict(e_ref32=max(relerr(a, b) for a, b in zip(a32, a64)))
        arrays[key + '/ref'] = np.concatenate([np.append(b[sample_positions(len(b))], np.max(np.abs(b))) for b in a64]).astype(np.float32)
    return dict(groups=widths, scores=out), arrays


class Recorder:
    """The criterion handed to the pruner: the reference's own, with every call logged."""

    def __init__(self, imp):
        self.imp, self.log = imp, []

    def __call__(self, group, ch_groups=1):
        s = self.imp(group, ch_groups=ch_groups)
        self.log.append((group, ch_groups, s))
        return s


def mask_case(model_name, cls, p, red, norm, global_pruning, round_to=None, forward_too=True, RATIO=0.3):
    model, ex, ignored, chg, forward = build(model_name)
    rec = Recorder(criterion(cls, p, red, norm))
    pruner = tp.pruner.MagnitudePruner(model, ex, importance=rec, global_pruning=global_pruning, iterative_steps=1, channel_groups=chg,
                                       ch_sparsity=RATIO, ignored_layers=ignored, round_to=round_to)
    names = mg.name_of(model)
    asked, real = {}, pruner.DG.get_pruning_group

    def logged(module, fn, idxs):
        asked[names[module]] = [int(i) for i in idxs]
        return real(module, fn, idxs)
    pruner.DG.get_pruning_group = logged
    out = dict(model=model_name, criterion=[cls, p, red, norm], global_pruning=bool(global_pruning), round_to=round_to, ratio=RATIO)
    if global_pruning:
        gen = pruner.step(interactive=True)
        first = next(gen, None)                                     # every group is scored now; nothing is pruned yet
        scored = [(g, c, s) for g, c, s in rec.log if s is not None]
        r32 = [(s[:len(s) // c] if c > 1 else s).detach().clone() for _, c, s in scored]
        model.double()
        try:
            r64 = [rec.imp(g, ch_groups=c) for g, c, _ in scored]
            r64 = [(s[:len(s) // c] if c > 1 else s).detach().clone() for (_, c, _), s in zip(scored, r64)]
        finally:
            model.float()
        cat32, cat64 = torch.cat(r32), torch.cat(r64)
        k = len(cat32) - int(pruner.initial_total_channels * (1 - pruner.per_step_ch_sparsity[pruner.current_step]))
        assert 0 < k < len(cat32)
        srt = torch.sort(cat32).values.double()
        gap = float((srt[k] - srt[k - 1]) / srt[k].abs())
        err = float(((cat32.double() - cat64).abs() / cat64.abs()).max())
        assert gap >= 100 * err, ('the fixture condition does not hold: move the seed or the ratio', out, gap, err)
        out.update(initial_total_channels=int(pruner.initial_total_channels), n_pruned=int(k), threshold=float(srt[k - 1]), gap=gap, err64=err)
        groups, g = [], first
        while g is not None:
            groups.append(g)
            g = next(gen, None)
    else:
        groups, margins = [], []
        for g in pruner.step(interactive=True):                     # local pruning scores a group after the earlier ones are pruned
            grp, c, s = rec.log[-1]
            model.double()
            try:
                s64 = rec.imp(grp, ch_groups=c)
            finally:
                model.float()
            n = len(asked[names[g[0][0].target.module]]) // c
            gs = len(s) // c
            for j in range(c):                                      # metapruner.py:237-249: each sub-group ranks its own slice
                a, b = s[j * gs:(j + 1) * gs].double(), s64[j * gs:(j + 1) * gs]
                srt = torch.sort(a).values
                if 0 < n < gs:
                    margins.append((float((srt[n] - srt[n - 1]) / s64.abs().max()), float((s.double() - s64).abs().max() / s64.abs().max())))
            groups.append(g)
            g.prune()
        assert all(gap >= 100 * err for gap, err in margins), ('the fixture condition does not hold', out, min(margins))
        tight = min(margins, key=lambda m: m[0] / max(m[1], 1e-300))      # the (sub-)group that decides with the least to spare
        out.update(gap=tight[0], err64=tight[1])
    chg_of = {names[g[0][0].target.module]: c for g, c, _ in rec.log}      # the ch_groups the pruner ranked each root with
    rows = []
    for g in groups:
        root = names[g[0][0].target.module]
        rows.append([root, int(chg_of[root]), mg.compress(sorted(asked[root]))])
        if global_pruning:
            g.prune()
    pruner.DG.get_pruning_group = real
    out.update(groups=rows, shapes_after=[list(q.shape) for _, q in model.named_parameters()],
               params_after=int(sum(q.numel() for q in model.parameters())))
    arrays = {}
    if forward_too:
        for m in model.modules():
            if isinstance(m, (mg.Upsample2D, mg.Downsample2D)):
                m.channels = m.conv.in_channels
            if isinstance(m, mg.Attention):
                m.set_processor(mg.AttnProcessor())
        with torch.no_grad():
            arrays['fwd_after'] = forward(model).numpy()
    return out, arrays


MASKS = {}
for _m in ('tiny', 'heads'):
    MASKS.update({
        _m + '_local_p1_mean_mean': (_m, 'MagnitudeImportance', 1, 'mean', 'mean', False),
        _m + '_local_p2_max_standarization': (_m, 'MagnitudeImportance', 2, 'max', 'standarization', False),
        _m + '_global_p1_sum_max': (_m, 'MagnitudeImportance', 1, 'sum', 'max', True),
        _m + '_global_p2_mean_sum': (_m, 'MagnitudeImportance', 2, 'mean', 'sum', True),
        _m + '_global_lamp_p2': (_m, 'LAMPImportance', 2, 'mean', 'mean', True),
    })
MASKS['ldm_global_p1_sum_max_round2'] = ('ldm', 'MagnitudeImportance', 1, 'sum', 'max', True, 2)


if __name__ == '__main__':
    out, per_model = dict(models={}, masks={}), {m: {} for m in ('tiny', 'heads', 'ldm')}
    path = os.path.join(HERE, 'magnitude_family.json')
    for m in per_model:
        if '--masks-only' in sys.argv:                              # keep the score tables of the existing files
            old = np.load(os.path.join(HERE, 'magnitude_family_%s.npz' % m))
            out['models'][m] = json.load(open(path))['models'][m]
            per_model[m].update({k: old[k] for k in old.files if k.startswith('scores/')})
            continue
        out['models'][m], arr = score_table(m)
        per_model[m].update({'scores/' + k: v for k, v in arr.items()})
        print(m, len(out['models'][m]['groups']), 'groups', sum(w for _, w in out['models'][m]['groups']), 'channels',
              'worst e_ref32 %.2e' % max(v['e_ref32'] for v in out['models'][m]['scores'].values()))
    for name, spec in MASKS.items():
        for ratio in RATIOS:
            try:
                case, arr = mask_case(*spec, RATIO=ratio)
                break
            except AssertionError as e:
                print(name, 'ratio', ratio, 'refused:', e.args[0][-2:] if e.args else e)
        else:
            raise SystemExit('no ratio gives %s its gap' % name)
        if case['global_pruning']:                                  # the same criterion without its normaliser: another mask?
            try:
                bare = mask_case(spec[0], spec[1], spec[2], spec[3], None, True, *spec[6:], forward_too=False, RATIO=case['ratio'])[0]['groups']
            except AssertionError:
                bare = None                                         # too narrow a gap to say
            case['differs_without_normalizer'] = bare is not None and bare != case['groups']
        out['masks'][name] = case
        per_model[spec[0]].update({'masks/%s/%s' % (name, k): v for k, v in arr.items()})
        print(name, 'gap %.2e err64 %.2e' % (case['gap'], case['err64']), 'groups', len(case['groups']), 'params', case['params_after'],
              case.get('differs_without_normalizer'))
    assert any(c.get('differs_without_normalizer') for c in out['masks'].values())
    path = os.path.join(HERE, 'magnitude_family.json')
    with open(path, 'w') as f:
        json.dump(out, f, separators=(',', ':'))
        f.write('\n')
    print('magnitude_family.json', os.path.getsize(path), 'bytes')
    for m, arrays in per_model.items():
        p = os.path.join(HERE, 'magnitude_family_%s.npz' % m)
        if os.path.exists(p):
            old = np.load(p)
            arrays.update({k: old[k] for k in old.files if k.startswith('parent_default/')})
        np.savez_compressed(p, **arrays)
        print(os.path.basename(p), os.path.getsize(p), 'bytes')
        assert os.path.getsize(p) < (1 << 20) and os.path.getsize(path) < (1 << 20)
