#!/usr/bin/env python3
"""The KL-f8 first stage (KL_F8_CFG: block_out_channels [128, 256, 512, 512], 2 layers per block, 4 latent channels) on the HIP
engine, seeded weights, and the two kernels of csrc/vae.hip beside torch's eager expressions.  Appends one JSON line per
measurement to profiles/vae_bench.jsonl (or --out), each the median of 3 runs timed with device events after one warm run:
  encode / decode        256 x 256 at batch 1, 4, 16 (weights pinned), and the decode of 1024 x 1024 untiled
  tiled_decode           1024 x 1024 and 2048 x 2048 at sample_size 512 (64-latent tiles); the 2048 case untiled must raise ValueError
  tile_blend             one launch beside the reference's eager loop, one 512-pixel tile with both neighbours
  gaussian_posterior     one launch beside the eager expression at [16, 8, 32, 32] and at 2^26 elements, the latter as a share of
                         the 6.3 TB/s achievable HBM rate over its algorithmic bytes
    python tools/bench_vae.py [--out profiles/vae_bench.jsonl] [--skip-model]"""
import argparse
import importlib
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
HBM_TBS = 6.3


def pkg(sub):
    return importlib.import_module('diff-pruning_amd.' + sub)


def timed(fn, iters=3, warmup=1):
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def eager_blend(b, a, l, e):
    """The eager form of the blend: one slice assignment per blended row, then one per blended column (2 e in all), as the
    reference's blend_v / blend_h loops issue them."""
    Ha, Wl = a.shape[2], l.shape[3]
    for k in range(e):
        w = k / e
        row = b[:, :, k, :]
        row.copy_(a[:, :, Ha - e + k, :] * (1 - w) + row * w)
    for k in range(e):
        w = k / e
        col = b[:, :, :, k]
        col.copy_(l[:, :, :, Wl - e + k] * (1 - w) + col * w)
    return b


def eager_posterior(m, noise, scale):
    mean, lv = torch.chunk(m, 2, dim=1)
    lv = torch.clamp(lv, -30.0, 20.0)
    std, var = torch.exp(0.5 * lv), torch.exp(lv)
    z = scale * (mean + std * noise)
    kl = 0.5 * torch.sum(torch.pow(mean, 2) + var - 1.0 - lv, dim=[1, 2, 3])
    return lv, std, var, z, kl


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'vae_bench.jsonl'))
    ap.add_argument('--skip-model', action='store_true')
    args = ap.parse_args()
    vae, syn, ops = pkg('vae'), pkg('synthetic'), pkg('ops')
    dev = torch.device('cuda')
    lines = []

    def emit(**kw):
        lines.append(kw)
        print(json.dumps(kw), flush=True)

    with torch.no_grad():
        # ---- the kernels
        for shape in ((16, 8, 32, 32), (16, 8, 512, 1024)):
            m = torch.randn(shape, device=dev)
            noise = torch.randn(shape[0], shape[1] // 2, shape[2], shape[3], device=dev)
            n = noise.numel()
            full = dict(logvar=torch.empty_like(noise), std=torch.empty_like(noise), var=torch.empty_like(noise), z=torch.empty_like(noise), kl=True)
            for what, kw, nbytes in (('all_outputs', full, 4 * n * (3 + 4)), ('sample_only', dict(z=full['z']), 4 * n * (3 + 1))):
                ms = timed(lambda: ops.gaussian_posterior(m, noise=noise, scale=0.18215, **kw))
                ems = timed(lambda: eager_posterior(m, noise, 0.18215))
                emit(what='gaussian_posterior', outputs=what, shape=list(shape), elements=n, hip_ms=round(ms, 4), eager_all_ms=round(ems, 4),
                     algorithmic_bytes=nbytes, tb_per_s=round(nbytes / ms / 1e9, 3), share_of_hbm=round(nbytes / ms / 1e9 / HBM_TBS, 3))
            del m, noise, full
        b0, a, l = (torch.randn(1, 3, 512, 512, device=dev) for _ in range(3))
        out = torch.empty(1, 3, 1024, 1024, device=dev)
        b = b0.clone()
        ms = timed(lambda: ops.tile_blend(b, a, l, 128, out, 384, 384, 384))
        ems = timed(lambda: eager_blend(b, a, l, 128))
        emit(what='tile_blend', tile=[1, 3, 512, 512], blend_extent=128, hip_ms=round(ms, 4), hip_launches=1, eager_loop_ms=round(ems, 3),
             eager_slice_assignments=2 * 128)
        if args.skip_model:
            return finish(args, lines)
        # ---- the model
        model = vae.AutoencoderKL(**syn.KL_F8_CFG)
        syn.det_init_(model, 7)
        model = model.to(dev).eval()
        with model.pin_weights():
            eng = model.engine()
            for B in (1, 4, 16):
                x = torch.from_numpy(syn.det_clean((B, 3, 256, 256), 6)).to(dev)
                z = torch.from_numpy(syn.det_noise((B, 4, 32, 32), 5)).to(dev)
                for what, fn in (('encode', lambda: eng.encode(x)), ('decode', lambda: eng.decode(z))):
                    ms = timed(fn)
                    emit(what=what, image=256, batch=B, ms=round(ms, 3), ms_per_image=round(ms / B, 3))
            z = torch.from_numpy(syn.det_noise((1, 4, 128, 128), 5)).to(dev)
            ms = timed(lambda: model.decode(z))
            emit(what='decode_untiled', image=1024, batch=1, ms=round(ms, 2))
            model.tile_sample_min_size, model.tile_latent_min_size = 512, 64
            for px in (1024, 2048):
                z = torch.from_numpy(syn.det_noise((1, 4, px // 8, px // 8), 5)).to(dev)
                model.enable_tiling()
                torch.cuda.reset_peak_memory_stats()
                ms = timed(lambda: model.decode(z))
                peak = torch.cuda.max_memory_allocated() / 2 ** 30
                model.disable_tiling()
                untiled = 'not run'
                if px == 2048:
                    try:
                        model.decode(z)
                        untiled = 'ran'
                    except ValueError as e:
                        untiled = 'ValueError: ' + str(e)[:60]
                emit(what='tiled_decode', image=px, batch=1, tile=512, tiles=len(vae.tile_spans(px // 8, 64, 48)) ** 2, ms=round(ms, 2),
                     peak_gib=round(peak, 2), untiled=untiled)
    finish(args, lines)


def finish(args, lines):
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'a') as f:
        for kw in lines:
            f.write(json.dumps(kw) + '\n')


if __name__ == '__main__':
    main()
