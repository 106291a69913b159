#!/usr/bin/env python3
"""The data-free magnitude criteria on one MI355X: what a whole prune costs with csrc/magnitude.hip beside the default configuration's
path and beside the reference's torch expressions, and the two kernels alone.
  cifar    the CIFAR-10 UNet (35.7 M parameters), ratio 0.3
  cin256   the cin256-v2 LDM UNet (400.9 M parameters), ratio 0.3, head channel groups and round_to = 2 (ldm_sweep.prune_ldm_model)
Per leg and criterion, local and global, median of `--repeat` runs, each on a fresh copy of the model, device synchronised around it:
  criteria   mag_p1_mean_max  MagnitudeImportance(1, 'mean', 'max')      csrc/magnitude.hip
             lamp_p2          LAMPImportance(2)                          csrc/magnitude.hip
             default          MagnitudeImportance(2, 'mean', 'mean')     the path that configuration always had (csrc/importance.hip /
                              prune_global.hip, one scalar read per group)
             torch_p1 / torch_lamp   the first two through the reference's torch expressions, group by group on the device
  *_s        wall time of the whole prune (scoring, selection, slicing every group, attribute fix-up)
  *_reads    device tensors read on the host during it (Tensor.cpu / item / tolist / numpy / float() / int() / bool()), and
  *_selects  calls of ops.select_smallest, each of which makes one device-to-host copy inside the library
Kernels alone, on the tables a global step of mag_p1_mean_max and of lamp_p2 builds (the C calls: validation, table upload, launch), HIP
events over 10 calls:  rows_ms, rows_gbs = 4 bytes x the parameters the members cover / that time, rows_of_achievable = that over the
6.3 TB/s streaming kernels are measured against;  finish_ms, finish_groups, finish_widest.
One JSON line per leg, appended to --out.
    python tools/bench_magnitude.py [--legs cifar,cin256] [--repeat 3] [--out profiles/magnitude_bench.jsonl]"""
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
READS = ('cpu', 'item', 'tolist', 'numpy', '__float__', '__int__', '__bool__')


def pkg(sub):
    return importlib.import_module('diff-pruning_amd.' + sub)


def build(name, dev):
    import golden_common as gc
    if name == 'cifar':
        model = pkg('unet').UNet2DModel(**gc.CIFAR_CFG)
        gc.det_init_(model, 0)
    else:
        model = pkg('ldm').UNetModel(**gc.LDM_CIN256_CFG)
        gc.det_init_(model, 9)
    return model.to(dev).eval()


def criteria():
    P = pkg('pruning')

    def torch_path(cls):
        return type('Torch' + cls.__name__, (cls,), {'_on_kernels': lambda self, live: [False] * len(live)})
    return {'mag_p1_mean_max': lambda: P.MagnitudeImportance(1, 'mean', 'max'), 'lamp_p2': lambda: P.LAMPImportance(2),
            'default': lambda: P.MagnitudeImportance(2, 'mean', 'mean'),
            'torch_p1': lambda: torch_path(P.MagnitudeImportance)(1, 'mean', 'max'), 'torch_lamp': lambda: torch_path(P.LAMPImportance)(2)}


def prune(name, model, imp, global_pruning):
    if name == 'cifar':
        return pkg('sweep').prune_model(model, 0.3, importance=imp, global_pruning=global_pruning)
    return pkg('ldm_sweep').prune_ldm_model(model, 0.3, importance=imp, global_pruning=global_pruning)


class CountReads:
    """Counts host reads of device tensors and select_smallest calls while active."""

    def __enter__(self):
        import torch
        self.reads, self.selects, self.saved = 0, 0, {a: getattr(torch.Tensor, a) for a in READS}
        for a, real in self.saved.items():
            def wrapper(t, *args, _real=real, **kw):
                self.reads += int(t.is_cuda)
                return _real(t, *args, **kw)
            setattr(torch.Tensor, a, wrapper)
        ops = pkg('ops')
        self.select = ops.select_smallest

        def select(*a, **k):
            self.selects += 1
            return self.select(*a, **k)
        ops.select_smallest = select
        return self

    def __exit__(self, *exc):
        import torch
        for a, real in self.saved.items():
            setattr(torch.Tensor, a, real)
        pkg('ops').select_smallest = self.select
        return False


def timed_calls(fn):
    import torch
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(10):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / 10


def kernels_alone(name, master, make_imp, tag, rec):
    import torch
    ops, P = pkg('ops'), pkg('pruning')
    seen = {}
    real_rows, real_finish = ops.magnitude_rows, ops.magnitude_finish

    def rows_(*a):
        seen['rows'] = a
        return real_rows(*a)

    def finish_(*a):
        seen['finish'] = a
        return real_finish(*a)
    ops.magnitude_rows, ops.magnitude_finish = rows_, finish_
    try:
        m = copy.deepcopy(master)
        kw = dict(ignored_layers=[m.conv_out]) if name == 'cifar' else dict(ignored_layers=[m.out], round_to=2, channel_groups={
            q: mod.heads for mod in m.modules() if isinstance(mod, pkg('ldm').CrossAttention) for q in (mod.to_q, mod.to_k, mod.to_v)})
        pr = P.MagnitudePruner(m, None, importance=make_imp(), global_pruning=True, ch_sparsity=0.3, **kw)
        next(pr.step(interactive=True), None)                       # prune_global scores and selects; nothing is pruned yet
    finally:
        ops.magnitude_rows, ops.magnitude_finish = real_rows, real_finish
    covered = sum(mm['w'].numel() for mm in seen['rows'][0])
    ms = timed_calls(lambda: real_rows(*seen['rows']))
    rec.update({tag + '_rows_ms': ms, tag + '_rows_members': len(seen['rows'][0]), tag + '_covered_params': covered,
                tag + '_rows_gbs': 4.0 * covered / (ms * 1e-3) / 1e9})
    rec[tag + '_rows_of_achievable'] = rec[tag + '_rows_gbs'] / (ACHIEVABLE_TBS * 1e3)
    rec.update({tag + '_finish_ms': timed_calls(lambda: real_finish(*seen['finish'])), tag + '_finish_groups': len(seen['finish'][0]),
                tag + '_finish_widest': max(n0 for _, n0, _ in seen['finish'][0])})


def leg(name, repeat):
    import torch
    dev = torch.device('cuda', 0)
    master = build(name, dev)
    rec = dict(leg=name, params=sum(p.numel() for p in master.parameters()), repeat=repeat)
    for cname, make_imp in criteria().items():
        for glob in (False, True):
            key = '%s_%s' % (cname, 'global' if glob else 'local')
            times = []
            try:
                for _ in range(repeat + 1):                         # the first run warms the allocator and is dropped
                    m = copy.deepcopy(master)
                    torch.cuda.synchronize()
                    with CountReads() as c:
                        t0 = time.perf_counter()
                        pr = prune(name, m, make_imp(), glob)
                        torch.cuda.synchronize()
                        times.append(time.perf_counter() - t0)
                    rec[key + '_reads'], rec[key + '_selects'], rec[key + '_groups'] = c.reads, c.selects, len(pr.records)
                    del m, pr
                rec[key + '_s'] = statistics.median(times[1:])
            except RuntimeError as e:                               # LAMP on the LDM UNet: members shorter than their group, as there
                rec[key + '_refused'] = str(e)[:160]
    kernels_alone(name, master, criteria()['mag_p1_mean_max'], 'p1', rec)
    if 'lamp_p2_global_s' in rec:
        kernels_alone(name, master, criteria()['lamp_p2'], 'lamp', rec)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--legs', default='cifar,cin256')
    ap.add_argument('--repeat', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'magnitude_bench.jsonl'))
    args = ap.parse_args()
    for name in args.legs.split(','):
        rec = leg(name, args.repeat)
        line = json.dumps(rec)
        print(line, flush=True)
        with open(args.out, 'a') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
