#!/usr/bin/env python3
"""The LDM finetune step at the cin256-v2 shapes (ldm_exp/configs/latent-diffusion/cin256-v2.yaml: B = 16 latents of 3 x 64 x 64
per GPU, one 512-wide class token), seeded weights, one MI355X.  Per leg (`unpruned`, `pruned`: ratio 0.3 by the LDM prune path
over stand-in gradients) a child interpreter under its own time limit reports
  step_ms            median device-event interval between consecutive LdmFinetuneEngine.step calls (>= 20 steps after warm-up)
  adamw_ms / _tbps   dp_adamw_ema alone on the engine's flat buffers, and its rate over the 28 algorithmic bytes per element
                     (36 with the LitEma shadow) -- to be read against the ~6.3 TB/s achievable HBM rate
  torch_foreach_ms   the same update by torch.optim.AdamW(foreach=True) over per-parameter views of the same buffers, in the same
                     process: what a user would otherwise run
  ctx_grad_ms        scored forward + backward with want_context_grad on minus off (the sixteen M = B input-gradient launches)
  embedding_bwd_ms   dp_embedding_bwd alone
  reserved_gb        peak reserved memory of the process
The parent runs the legs one after the other, `--rounds` times, and stops at the first leg that does not exit with status 0.
Prints one JSON line per leg and a final summary line.
    python tools/bench_ldm_finetune.py [--steps 20] [--warmup 3] [--rounds 2] [--batch 16] [--legs unpruned,pruned]"""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tests', 'golden')):
    if p not in sys.path:
        sys.path.insert(0, p)


def pkg(sub):
    return importlib.import_module('diff-pruning_amd.' + sub)


def timed(fn, steps, warmup):
    """Median ms between consecutive device events recorded after each call (the call's span on the device, gaps included)."""
    import torch
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(steps + 1)]
    ev[0].record()
    for k in range(steps):
        fn()
        ev[k + 1].record()
    torch.cuda.synchronize()
    return statistics.median(ev[k].elapsed_time(ev[k + 1]) for k in range(steps))


def leg(name, args):
    import torch
    import golden_common as gc
    assert torch.cuda.is_available(), 'bench_ldm_finetune needs the GPU'
    dev = torch.device('cuda', 0)
    ldm, ldm_sweep, ldm_train, ops = pkg('ldm'), pkg('ldm_sweep'), pkg('ldm_train'), pkg('ops')
    cfg = gc.LDM_CIN256_CFG
    model = ldm.UNetModel(**cfg)
    gc.det_init_(model, 9)
    model = model.to(dev).eval()
    if name == 'pruned':
        from ldm_finetune_ref import prune_ldm
        prune_ldm(model, 0.3)
    embedder = ldm_sweep.ClassEmbedder(cfg['context_dim'], 1001)
    with torch.no_grad():
        embedder.embedding.weight.copy_(torch.from_numpy(gc.det_param('embedding.weight', (1001, cfg['context_dim']), 61)))
    embedder = embedder.to(dev)
    B = args.batch
    out = dict(leg=name, batch=B, params=sum(p.numel() for p in model.parameters()))
    x = torch.from_numpy(gc.det_noise((B, 3, 64, 64), 300)).to(dev)
    noise = torch.from_numpy(gc.det_noise((B, 3, 64, 64), 400)).to(dev)
    gen = torch.Generator().manual_seed(0)
    ids = torch.randint(0, 1001, (B,), generator=gen)
    for use_ema in (False, True):
        ft = ldm_train.LdmFinetuneEngine(model, embedder, lr=1.28e-4, use_ema=use_ema)
        tag = '_ema' if use_ema else ''

        def step():
            ft.step(x, ids, noise=noise, timesteps=torch.randint(0, 1000, (B,), generator=gen))
        out['step_ms' + tag] = timed(step, args.steps, args.warmup)
        n = ft.n_unet if use_ema else ft.flat_p.numel()
        bufs = [b[:n] for b in (ft.flat_p, ft.flat_g, ft.m, ft.v)]
        k = [ft.step_count]

        def fused():
            k[0] += 1
            ops.adamw_ema(bufs[0], bufs[1], bufs[2], bufs[3], ft.ema, ft.lr, 0.9, 0.999, 1e-8, 1e-2, k[0], 0.9999)
        ms = timed(fused, args.steps, args.warmup)
        out['adamw_ms' + tag] = ms
        out['adamw_tbps' + tag] = (36 if use_ema else 28) * n / (ms * 1e-3) / 1e12
        if not use_ema:
            params = list(model.parameters()) + list(embedder.parameters())
            opt = torch.optim.AdamW(params, lr=1.28e-4, foreach=True)
            out['torch_foreach_ms'] = timed(opt.step, args.steps, args.warmup)
            del opt
            eng = model.engine()
            P = {n_: p.detach() for n_, p in model.named_parameters()}
            G = {n_: p.grad for n_, p in model.named_parameters()}
            sa, sb = ft.schedule.tables(dev)
            t = torch.randint(0, 1000, (B,), generator=gen).to(dev)
            c = embedder(ids.to(dev))

            def fb(want):
                def run():
                    eng.bind(P, G)
                    y = eng.forward(ops.q_sample(x, noise, sa, sb, t), t, c, save=True)
                    _, dout = ops.mse_fwd_bwd(y, noise, 2.0 / y.numel(), 1.0 / y.numel())
                    eng.backward(dout, want_context_grad=want)
                return run
            with model.pin_weights():
                off = [timed(fb(False), args.steps, args.warmup) for _ in range(2)]
                on = [timed(fb(True), args.steps, args.warmup) for _ in range(2)]
            out['fwd_bwd_ms'], out['fwd_bwd_ctx_ms'] = min(off), min(on)
            out['ctx_grad_ms'] = min(on) - min(off)
            dctx = torch.randn(B, cfg['context_dim'], device=dev)
            out['embedding_bwd_ms'] = timed(lambda: ops.embedding_bwd(ids.to(dev), dctx, embedder.embedding.weight.grad), args.steps,
                                            args.warmup)
        del ft
    out['reserved_gb'] = torch.cuda.max_memory_reserved() / 2 ** 30
    print(json.dumps(out, sort_keys=True), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--rounds', type=int, default=2)
    ap.add_argument('--batch', type=int, default=16)
    ap.add_argument('--legs', default='unpruned,pruned')
    ap.add_argument('--leg-timeout', type=int, default=420, help='seconds one leg may take')
    ap.add_argument('--leg', default=None, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.steps < 20:
        ap.error('--steps >= 20 (medians over fewer steps are not reported)')
    if args.leg is not None:
        return leg(args.leg, args)
    results = []
    for rnd in range(args.rounds):
        for name in args.legs.split(','):
            cmd = [sys.executable, os.path.abspath(__file__), '--leg', name, '--steps', str(args.steps), '--warmup', str(args.warmup),
                   '--batch', str(args.batch)]
            try:
                p = subprocess.run(cmd, timeout=args.leg_timeout, capture_output=True, text=True)
            except subprocess.TimeoutExpired:
                print(json.dumps(dict(leg=name, round=rnd, error='time limit of %d s' % args.leg_timeout)), flush=True)
                return 124                         # nothing more is started on the device
            if p.returncode != 0:
                print(json.dumps(dict(leg=name, round=rnd, error='exit status %d' % p.returncode, tail=p.stderr[-2000:])), flush=True)
                return p.returncode                # the first failing leg ends the run
            line = [ln for ln in p.stdout.splitlines() if ln.startswith('{')][-1]
            results.append(dict(json.loads(line), round=rnd))
            print(json.dumps(results[-1], sort_keys=True), flush=True)
    print(json.dumps(dict(summary=results), sort_keys=True))
    return 0


if __name__ == '__main__':
    sys.exit(main())
