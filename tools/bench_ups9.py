#!/usr/bin/env python3
"""Gate of the nine-product upsample convolution (csrc/ups9.hip): per level and shape class, the new input-gradient launch (every pixel
tile) against what it replaces -- the four class launches, with and without the de-interleave pass in front of them (the pass stays for
the class weight gradients while only the input gradient runs in the new form, but leaves the main stream).  Shapes: the headline's
(batch 256, 256 channels), the ratio-0.3 pruned model's (batch 128, the c4_finetune step; the ddim loop has no backward) and
bedroom256's (4 images per GPU).
Executed TFLOP/s = 2 * taps * Cin * Cout * pixels / time with taps = 9 (new) or 16 (class launches).

With --pass fwd the same table for the forward pass: the four class launches with and without their interleave pass against dp_ups9_fwd
errors against fp64 conv2d(interpolate(x, 2), w, padding=1).

    python tools/bench_ups9.py [--pass dgrad|fwd] [--out profiles/ups9_gate.txt | profiles/ups9_fwd_gate.txt] [--check]"""
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


def forward_table(args, dev):
    lines = ['forward of Upsample2D\'s convolution: class launches (16 taps) vs dp_ups9_fwd (9 taps, %d x %d tile); ms per call, fastest of 3 windows of 20'
             % ops.UPS9_FWD_TILE,
             'shape                       4 class   +interl   | ups9    (TF/s)  | gate  vs 4 class  vs +interl  spread']
    for (B, Cin, Cout, H) in SHAPES:
        w = torch.randn(Cout, Cin, 3, 3, device=dev) / (3.0 * Cin ** 0.5)
        bias = torch.randn(Cout, device=dev)
        x = ops.empty_act((B, Cin, H, H), dev).normal_()
        weff = ops.ups_weff(w)
        cls = [ops.pack_weight(weff[c], 0) for c in range(4)]
        up, ldu = ops.pack_weight(ops.ups9_u(w), 0)
        q = ops.empty_act((4, B, Cout, H, H), dev)
        y9 = ops.empty_act((B, Cout, 2 * H, 2 * H), dev)

        def class4():
            for c, spec in enumerate(ops.UPS_CLASS_SPECS):
                ops.conv_forward(x, None, cls[c][0], cls[c][1], Cout, spec, bias=bias, out=q[c])

        def class4_interleave():
            class4()
            return ops.interleave2x2(q)

        t4, _ = timeit(class4)
        t4i, s4 = timeit(class4_interleave)
        t9, s9 = timeit(lambda: ops.ups9_fwd(x, up, ldu, Cout, bias=bias, out=y9))
        line = 'B%-3d %3d->%3d @%2dx%-2d        %.4f    %.4f   |  %.4f (%5.1f) | %-4s  %.2fx      %.2fx      %.4f / %.4f' % (
            B, Cin, Cout, H, H, t4, t4i, t9, 2.0 * 9 * Cin * Cout * B * H * H / t9 / 1e9, 'on' if ops.ups9_fwd_gate(B, Cin, Cout, H, H) else 'off',
            t4 / t9, t4i / t9, s4, s9)
        if args.check:
            nb = min(B, 8)
            ref = torch.nn.functional.conv2d(torch.nn.functional.interpolate(x[:nb].double(), scale_factor=2, mode='nearest'), w.double(),
                                             bias.double(), padding=1)
            errs = [float((t[:nb].double() - ref).abs().max() / ref.abs().max()) for t in (class4_interleave(), y9)]
            line += '   err class %.1e  ups9 %.1e' % tuple(errs)
        lines.append(line)
        print(line, flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--pass', dest='which', default='dgrad', choices=('dgrad', 'fwd'))
    ap.add_argument('--check', action='store_true', help='also print each form\'s error against fp64 (8 images)')
    args = ap.parse_args()
    dev = torch.device('cuda')
    if args.which == 'fwd':
        lines = forward_table(args, dev)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, 'w') as f:
                f.write('\n'.join(lines) + '\n')
        return
    lines = ['input gradient of Upsample2D\'s convolution: class launches (16 taps) vs dp_ups9_dgrad (9 taps); ms per call, fastest of 3 windows of 20',
             'shape                       4 class   +deint    | ups9 t32 (TF/s)   t64 (TF/s)   t128 (TF/s) | default tile  vs 4 class  vs +deint  spread']
    for (B, Cin, Cout, H) in SHAPES:
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
