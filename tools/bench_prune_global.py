#!/usr/bin/env python3
"""Global pruning on one MI355X: what `prune_model(global_pruning=True)` costs beside the local path, and its two launchers alone.
  cifar    the CIFAR-10 UNet (35.7 M parameters) after an 8-step Taylor sweep at B = 4, ratio 0.3
  cin256   the cin256-v2 LDM UNet (400.9 M parameters) after one forward / backward of two 3 x 64 x 64 latents, ratio 0.3, head
           channel groups and round_to = 2 (ldm_sweep.prune_ldm_model)
Per leg, median of `--repeat` runs, each on a fresh copy of the swept model (weights and gradients), device synchronised around it:
  prune_global_s / prune_local_s   wall time of the whole prune (scoring, selection, slicing every group, attribute fix-up)
  score_groups_ms                  dp_score_groups alone (the C call on the table the prune built: validation, table upload, the launch
                                   pair), HIP events over 10 calls; score_groups_gbs = 8 bytes x the parameters its members cover / that
                                   time; of_achievable = that over the 6.3 TB/s the README measures streaming kernels against
  select_smallest_ms               dp_select_smallest alone (13 launches, the one device-to-host copy, the stream wait), wall time
One JSON line per leg, appended to --out.
    python tools/bench_prune_global.py [--legs cifar,cin256] [--repeat 3] [--out profiles/prune_global_bench.jsonl]"""
import argparse
import copy
import importlib
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests', 'golden')):
    if p not in sys.path:
        sys.path.insert(0, p)

ACHIEVABLE_TBS = 6.3


def pkg(sub):
    return importlib.import_module('diff-pruning_amd.' + sub)


def swept_model(name, dev):
    import torch
    import golden_common as gc
    ops, sweep = pkg('ops'), pkg('sweep')
    if name == 'cifar':
        model = pkg('unet').UNet2DModel(**gc.CIFAR_CFG)
        gc.det_init_(model, 0)
        model = model.to(dev).eval()
        clean = torch.from_numpy(gc.det_clean((4, 3, 32, 32), 1)).to(dev)
        noise = torch.from_numpy(gc.det_noise((4, 3, 32, 32), 2)).to(dev)
        sweep.taylor_sweep(model, pkg('diffusion').DDPMScheduler(), clean, noise, num_steps=8)
        return model
    cfg = gc.LDM_CIN256_CFG
    model = pkg('ldm').UNetModel(**cfg)
    gc.det_init_(model, 9)
    model = model.to(dev).eval()
    sweep.flatten_grads(model)
    x = torch.from_numpy(gc.det_noise((2, 3, 64, 64), 31)).to(dev)
    ctx = torch.from_numpy(gc.det_noise((2, 1, cfg['context_dim']), 32)).to(dev)
    noise = torch.from_numpy(gc.det_noise((2, 3, 64, 64), 33)).to(dev)
    t = torch.tensor([7, 640], device=dev)
    eng = model.engine()
    eng.bind(eng.P, {n: p.grad for n, p in model.named_parameters()})
    y = eng.forward(x, t, ctx, save=True)
    _, dout = ops.mse_fwd_bwd(y, noise, 2.0 / y.numel(), 1.0 / y.numel())
    eng.backward(dout)
    return model


def fresh(master):
    """A copy of the swept model with gradients of its own (Parameter.__deepcopy__ leaves .grad behind)."""
    m = copy.deepcopy(master)
    src = dict(master.named_parameters())
    for n, p in m.named_parameters():
        p.grad = src[n].grad.detach().clone()
    return m


def prune(name, model, global_pruning):
    if name == 'cifar':
        return pkg('sweep').prune_model(model, 0.3, global_pruning=global_pruning)
    return pkg('ldm_sweep').prune_ldm_model(model, 0.3, global_pruning=global_pruning)


def make_pruner(name, model):
    pruning = pkg('pruning')
    if name == 'cifar':
        return pruning.MagnitudePruner(model, None, importance=pruning.TaylorImportance(), global_pruning=True, ch_sparsity=0.3,
                                       ignored_layers=[model.conv_out])
    chg = {}
    for mod in model.modules():
        if isinstance(mod, pkg('ldm').CrossAttention):
            chg[mod.to_q] = chg[mod.to_k] = chg[mod.to_v] = mod.heads
    return pruning.MagnitudePruner(model, None, importance=pruning.TaylorImportance(), global_pruning=True, channel_groups=chg,
                                   ch_sparsity=0.3, ignored_layers=[model.out], round_to=2)


def leg(name, repeat):
    import torch
    ops = pkg('ops')
    dev = torch.device('cuda', 0)
    master = swept_model(name, dev)
    params = sum(p.numel() for p in master.parameters())
    rec = dict(leg=name, params=params, repeat=repeat)
    for key, glob in (('prune_global_s', True), ('prune_local_s', False)):
        times = []
        for _ in range(repeat + 1):                    # the first run warms the allocator and is dropped
            m = fresh(master)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            pr = prune(name, m, glob)
            torch.cuda.synchronize()
            times.append(time.perf_counter() - t0)
            rec['groups_' + key[6:-2]] = len(pr.records)
            rec['params_after_' + key[6:-2]] = sum(p.numel() for p in m.parameters())
            del m, pr
        rec[key] = statistics.median(times[1:])
    # ---- the two launchers alone, on what the prune itself hands them
    seen = {}
    real_score, real_select = ops.score_groups, ops.select_smallest

    def score_groups(groups, idx_dev, scratch, scores):
        seen['score'] = (groups, idx_dev, scratch, scores)
        return real_score(groups, idx_dev, scratch, scores)

    def select_smallest(scores, offsets, k, raw=False):
        seen['select'] = (scores.clone(), list(offsets), k)
        return real_select(scores, offsets, k, raw)
    ops.score_groups, ops.select_smallest = score_groups, select_smallest
    try:
        m = fresh(master)
        next(make_pruner(name, m).step(interactive=True), None)        # prune_global scores and selects; nothing is pruned yet
    finally:
        ops.score_groups, ops.select_smallest = real_score, real_select
    groups, idx_dev, scratch, scores = seen['score']
    arr, table = scores._dp_table
    covered = sum(mm['w'].numel() for members, _ in groups for mm in members)
    lib, L = ops._lib(), ops.L
    n_entries = sum(len(members) for members, _ in groups)

    def call():
        L.check(lib.dp_score_groups(arr, n_entries, ops._p(table), ops._p(idx_dev), 0 if idx_dev is None else idx_dev.numel(),
                                    ops._p(scratch), scratch.numel(), ops._p(scores), scores.numel(), ops._stream()), 'dp_score_groups')
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(10):
        call()
    e.record()
    torch.cuda.synchronize()
    ms = s.elapsed_time(e) / 10
    rec.update(score_groups_ms=ms, score_groups_members=n_entries, score_groups_groups=len(groups), covered_params=covered,
               score_groups_gbs=8.0 * covered / (ms * 1e-3) / 1e9)
    rec['of_achievable'] = rec['score_groups_gbs'] / (ACHIEVABLE_TBS * 1e3)
    x, offsets, k = seen['select']
    times = []
    for _ in range(repeat + 2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        real_select(x, offsets, k)
        times.append(time.perf_counter() - t0)
    rec.update(select_smallest_ms=statistics.median(times[2:]) * 1e3, select_n=x.numel(), select_k=int(k), select_groups=len(offsets) - 1)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--legs', default='cifar,cin256')
    ap.add_argument('--repeat', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'prune_global_bench.jsonl'))
    args = ap.parse_args()
    for name in args.legs.split(','):
        rec = leg(name, args.repeat)
        line = json.dumps(rec)
        print(line, flush=True)
        with open(args.out, 'a') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
