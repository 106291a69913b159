#!/usr/bin/env python3
"""Gate of the nine-product upsample convolution (csrc/ups9.hip): per level and shape class, the new input-gradient launch (every pixel
tile) against what it replaces -- the four class launches, with and without the de-interleave pass in front of them (the pass stays for
the class weight gradients while only the input gradient runs in the new form, but leaves the main stream).  Shapes: the headline's
(batch 256, 256 channels), the ratio-0.3 pruned model's (batch 128, the c4_finetune step; the ddim loop has no backward) and
bedroom256's (4 images per GPU).
Executed TFLOP/s = 2 * taps * Cin * Cout * pixels / time with taps = 9 (new) or 16 (class launches).

    python tools/bench_ups9.py [--out profiles/ups9_gate.txt] [--check]"""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--check', action='store_true', help='also print each form\'s error against fp64 autograd (8 images)')
    args = ap.parse_args()
    dev = torch.device('cuda')
    lines = ['input gradient of Upsample2D\'s convolution: class launches (16 taps) vs dp_ups9_dgrad (9 taps); ms per call, fastest of 3 windows of 20',
             'shape                       4 class   +deint    | ups9 t32 (TF/s)   t64 (TF/s)   t128 (TF/s) | default tile  vs 4 class  vs +deint  spread']
    shapes = [(256, 256, 256, h) for h in (4, 8, 16)] + [(128, 180, 180, h) for h in (4, 8, 16)] + [(128, 179, 179, 16), (256, 128, 128, 16)]
    # bedroom256: 4 images per GPU, 512 / 512 / 256 / 256 / 128 channels at 8 .. 128 low-resolution pixels a side
    shapes += [(4, 512, 512, 8), (4, 512, 512, 16), (4, 256, 256, 32), (4, 256, 256, 64), (4, 128, 128, 128)]
    for (B, Cin, Cout, H) in shapes:
        w = torch.randn(Cout, Cin, 3, 3, device=dev) / (3.0 * Cin ** 0.5)
        dy = ops.empty_act((B, Cout, 2 * H, 2 * H), dev).normal_()
        weff = ops.ups_weff(w)
        cls = [ops.pack_weight(weff[c], 1) for c in range(4)]
        up, ldu = ops.pack_weight(ops.ups9_u(w), 1)
        dxc, dx9 = ops.empty_act((B, Cin, H, H), dev), ops.empty_act((B, Cin, H, H), dev)
        dyq = ops.deinterleave2x2(dy)

        def class4():
            for c, spec in enumerate(ops.UPS_CLASS_SPECS):
                ops.conv_dgrad(dyq[c], cls[c][0], cls[c][1], Cin, spec, (H, H), out=dxc, accumulate=c > 0)

        def class4_deint():
            q = ops.deinterleave2x2(dy)
            for c, spec in enumerate(ops.UPS_CLASS_SPECS):
                ops.conv_dgrad(q[c], cls[c][0], cls[c][1], Cin, spec, (H, H), out=dxc, accumulate=c > 0)

        t4, s4 = timeit(class4)
        t4d, _ = timeit(class4_deint)
        fl9 = 2.0 * 9 * Cin * Cout * B * H * H
        t9 = [timeit(lambda t=t: ops.ups9_dgrad(dy, up, ldu, Cin, out=dx9, tile=t)) for t in (0, 1, 2)]
        d = ops.ups9_tile(B, Cin, H, H)
        line = 'B%-3d %3d->%3d @%2dx%-2d        %.4f    %.4f   |' % (B, Cout, Cin, H, H, t4, t4d)
        line += ''.join('  %.4f (%5.1f)' % (t, fl9 / t / 1e9) for t, _ in t9)
        line += ' | t%-3d          %.2fx      %.2fx     %.4f / %.4f' % (ops.UPS9_TILE_PIX[d], t4 / t9[d][0], t4d / t9[d][0], s4, t9[d][1])
        if args.check:
            nb = min(B, 8)
            x = torch.zeros(nb, Cin, H, H, dtype=torch.float64, device=dev, requires_grad=True)
            y = torch.nn.functional.conv2d(torch.nn.functional.interpolate(x, scale_factor=2, mode='nearest'), w.double(), padding=1)
            y.backward(dy[:nb].double())
            class4()
            ops.ups9_dgrad(dy, up, ldu, Cin, out=dx9, tile=d)
            line += '   err class %.1e  ups9 %.1e' % tuple(float((t[:nb].double() - x.grad).abs().max() / x.grad.abs().max()) for t in (dxc, dx9))
        lines.append(line)
        print(line, flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
