#!/usr/bin/env python3
"""Gate of the nine-product weight gradient of Upsample2D's convolution (csrc/ups9_wgrad.hip): per shape class, the launch pair
dp_ups9_wgrad + dp_ups9_wgrad_reduce against what it replaces -- deinterleave2x2, four class weight gradients (2x2 taps each, with their
split-K reductions) and ups_wfold.  Shapes: the headline's (batch 256, 256 channels), the ratio-0.3 pruned model's (batch 128, the
c4_finetune step), bedroom256's (4 images per GPU) and the LDM cin256-v2 UNet's (6 latents, 960 / 576 / 384 channels).
Executed TFLOP/s of the new path = 18 * Cin * Cout * pixels / time.  ms per call, fastest of `reps` windows of `n` back-to-back calls, and
the spread (slowest - fastest window) of either side.  --blocks: also time the launch pair at other split targets.

    python tools/bench_ups9_wgrad.py [--out profiles/ups9_wgrad_gate.txt] [--check] [--blocks 256,512,1024]"""
import argparse
import importlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ops = importlib.import_module('diff-pruning_amd.ops')


def timeit(fn, n=20, reps=3):
    """Fastest of `reps` windows of `n` back-to-back calls, ms per call (the windows' spread is returned next to it)."""
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        for _ in range(n):
            fn()
        e.record()
        torch.cuda.synchronize()
        ts.append(s.elapsed_time(e) / n)
    return min(ts), max(ts) - min(ts)


SHAPES = [(256, 256, 256, h) for h in (4, 8, 16)] + [(128, 180, 180, h) for h in (4, 8, 16)] + [(128, 179, 179, 16), (256, 128, 128, 16)]
# bedroom256: 4 images per GPU, 512 / 512 / 256 / 256 / 128 channels at 8 .. 128 low-resolution pixels a side
SHAPES += [(4, 512, 512, 8), (4, 512, 512, 16), (4, 256, 256, 32), (4, 256, 256, 64), (4, 128, 128, 128)]
# LDM cin256-v2: 6 latents, 960 / 576 / 384 channels at 8 / 16 / 32 low-resolution pixels a side
SHAPES += [(6, 960, 960, 8), (6, 576, 576, 16), (6, 384, 384, 32)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--check', action='store_true', help='also print each form\'s error against fp64 autograd (8 images)')
    ap.add_argument('--blocks', default='', help='comma-separated split targets (ops.UPS9_WGRAD_BLOCKS) to time beside the default')
    args = ap.parse_args()
    dev = torch.device('cuda')
    extra = [int(b) for b in args.blocks.split(',') if b]
    lines = ['weight gradient of Upsample2D\'s convolution: deinterleave2x2 + 4 class launches (16 taps) + ups_wfold vs dp_ups9_wgrad + reduce '
             '(9 taps, %d x %d tile, %d-pixel K tiles, target %d workgroups); ms per call, fastest of 3 windows of 20' % (
                 ops.UPS9_WGRAD_TILE + (ops.UPS9_WGRAD_BLOCKS,)),
             'shape                       class path | ups9 pair (TF/s) splits | gate  speed-up  spread class / ups9' +
             ''.join('  | blocks=%d' % b for b in extra)]
    for (B, Cin, Cout, H) in SHAPES:
        dy = ops.empty_act((B, Cout, 2 * H, 2 * H), dev).normal_()
        x = ops.empty_act((B, Cin, H, H), dev).normal_()
        gwc = torch.zeros(Cout, Cin, 3, 3, device=dev)
        gw9 = torch.zeros(Cout, Cin, 3, 3, device=dev)
        gweff = torch.empty(4, Cout, Cin, 2, 2, device=dev)

        def class_path(accumulate=False):
            q = ops.deinterleave2x2(dy)
            for c, spec in enumerate(ops.UPS_CLASS_SPECS):
                ops.conv_wgrad(q[c], x, None, gweff[c], spec, accumulate=False)
            ops.ups_wfold(gweff, gwc, accumulate=accumulate)

        def pair(accumulate=False):
            ops.ups9_wgrad(dy, x, gw9, accumulate=accumulate)

        tc, sc = timeit(class_path)
        t9, s9 = timeit(pair)
        splits, _ = ops.ups9_wgrad_splits(B, Cin, Cout, H, H)
        line = 'B%-3d %3d->%3d @%3dx%-3d      %.4f     |  %.4f  (%5.1f)  %4d   | %-4s  %.2fx     %.4f / %.4f' % (
            B, Cin, Cout, H, H, tc, t9, 18.0 * Cin * Cout * B * H * H / t9 / 1e9, splits, 'on' if ops.ups9_wgrad_gate(B, Cin, Cout, H, H) else 'off',
            tc / t9, sc, s9)
        default = ops.UPS9_WGRAD_BLOCKS
        for b in extra:
            ops.UPS9_WGRAD_BLOCKS = b
            tb, _ = timeit(pair)
            line += '  | %.4f (%d)' % (tb, ops.ups9_wgrad_splits(B, Cin, Cout, H, H)[0])
        ops.UPS9_WGRAD_BLOCKS = default
        if args.check:
            nb = min(B, 8)
            w = torch.zeros(Cout, Cin, 3, 3, dtype=torch.float64, device=dev, requires_grad=True)
            y = torch.nn.functional.conv2d(torch.nn.functional.interpolate(x[:nb].double(), scale_factor=2, mode='nearest'), w, padding=1)
            y.backward(dy[:nb].double())
            q = ops.deinterleave2x2(dy[:nb])
            for c, spec in enumerate(ops.UPS_CLASS_SPECS):
                ops.conv_wgrad(q[c], x[:nb], None, gweff[c], spec, accumulate=False)
            ops.ups_wfold(gweff, gwc, accumulate=False)
            ops.ups9_wgrad(dy[:nb], x[:nb], gw9, accumulate=False)
            line += '   err class %.1e  ups9 %.1e' % tuple(float((t.double() - w.grad).abs().max() / w.grad.abs().max()) for t in (gwc, gw9))
        lines.append(line)
        print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
