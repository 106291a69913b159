#!/usr/bin/env python3
"""The VQ-f4 first stage of cin256-v2 (VQ_F4_CFG: 55.3 M parameters, 64 x 64 x 3 latents, 256 x 256 images, 8192 codes) on the
HIP engine, seeded weights.  Prints one JSON line with:
  decode / encode        ms per image and images/s at batch 1, 4, 16 (weights pinned), reference-arithmetic TFLOP/s
  mid_attention          decoder mid-block attention at T = 4096, d = 512: the one-kernel form against the three launches, alone
                         and inside the batch-16 decode
  quantizer              the HIP vector quantizer alone at batch 16, and its share of the batch-16 decode
  peak_gib               peak allocated device memory of the batch-16 decode
  ldm_pipeline           LDMPipeline, 100 DDIM steps at batch 16 with the CelebA-HQ-shaped UNet (UNet2DModel defaults,
                         attention_head_dim 32, sample_size 64), and the decode's share of it
  cpu_decode             one image decoded by the fp32 restatement (tests/vq_ref.py) on 16 CPU threads, and the speed ratio
The MAC counts are recounted from the model's layers (torch.utils.flop_counter over the restatement on the meta device).
Each GPU figure is the median over --iters runs timed with device events, after --warmup runs.
    python tools/bench_vq.py [--iters 5] [--warmup 2] [--no-pipeline] [--no-cpu]"""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)
import vq_ref   # noqa: E402


def pkg(sub):
    return importlib.import_module('diff-pruning_amd.' + sub)


def timed(fn, iters, warmup):
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


def macs(cfg):
    from torch.utils.flop_counter import FlopCounterMode
    P = {k: torch.empty(s, device='meta') for k, s in vq_ref.param_shapes(cfg).items()}
    out = {}
    for name, fn in (('decode', lambda: vq_ref.decode(P, cfg, torch.empty(1, 3, 64, 64, device='meta'), force_not_quantize=True)),
                     ('encode', lambda: vq_ref.encode(P, cfg, torch.empty(1, 3, 256, 256, device='meta')))):
        with FlopCounterMode(display=False) as fc:
            fn()
        out[name] = fc.get_total_flops() / 2.0
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--no-pipeline', action='store_true')
    ap.add_argument('--no-cpu', action='store_true')
    args = ap.parse_args()
    vq, syn, ops, diffusion, unet = pkg('vq'), pkg('synthetic'), pkg('ops'), pkg('diffusion'), pkg('unet')
    dev = torch.device('cuda')
    cfg = syn.VQ_F4_CFG
    P = vq_ref.params(cfg, 7, torch.float32)
    model = vq.VQModel(**cfg)
    model.load_state_dict(P)
    model = model.to(dev).eval()
    mac = macs(cfg)
    res = dict(tool='bench_vq', config='VQ_F4_CFG', gmac_per_image={k: round(v / 1e9, 1) for k, v in mac.items()},
               fused_mid_attn_default=vq.VQEngine.FUSED_MID_ATTN, decode={}, encode={})
    eng_of = model.engine
    with torch.no_grad(), model.pin_weights():
        eng = eng_of()
        for B in (1, 4, 16):
            z = torch.from_numpy(syn.det_noise((B, 3, 64, 64), 5)).to(dev)
            x = torch.from_numpy(syn.det_clean((B, 3, 256, 256), 6)).to(dev)
            for what, fn in (('decode', lambda: eng.decode(z)), ('encode', lambda: eng.encode(x))):
                ms = timed(fn, args.iters, args.warmup)
                res[what]['b%d' % B] = dict(ms_per_image=round(ms / B, 3), images_per_s=round(1000.0 * B / ms, 2),
                                            tflops=round(2.0 * mac[what] * B / ms / 1e9, 1))
        # attention A/B at T = 4096, batch 16
        B = 16
        z = torch.from_numpy(syn.det_noise((B, 3, 64, 64), 5)).to(dev)
        h = torch.from_numpy(syn.det_noise((B, 512, 64, 64), 8)).to(dev)
        pre = 'decoder.mid_block.attentions.0'
        ab = {}
        for name, fused in (('fused', True), ('three_launch', False)):
            attn_ms = timed(lambda: eng.attn_fwd(pre, h, 512 ** -0.5, 1.0, None, 1, fused_attn=fused), args.iters, args.warmup)
            eng.fused_mid_attn = fused
            dec_ms = timed(lambda: eng.decode(z), args.iters, args.warmup)
            ab[name] = dict(attention_ms=round(attn_ms, 3), decode_b16_ms=round(dec_ms, 2))
        eng.fused_mid_attn = vq.VQEngine.FUSED_MID_ATTN
        o1 = eng.attn_fwd(pre, h, 512 ** -0.5, 1.0, None, 1, fused_attn=True)
        o3 = eng.attn_fwd(pre, h, 512 ** -0.5, 1.0, None, 1, fused_attn=False)
        ab['max_abs_diff'] = float((o1 - o3).abs().max())
        res['mid_attention'] = ab
        E = eng.P['quantize.embedding.weight']
        q_ms = timed(lambda: ops.vq_quantize(z, E, want_indices=False, want_loss=False), args.iters, args.warmup)
        q_full = timed(lambda: ops.vq_quantize(z, E), args.iters, args.warmup)
        dec16 = timed(lambda: eng.decode(z), args.iters, args.warmup)
        res['quantizer'] = dict(b16_ms=round(q_ms, 4), b16_with_indices_loss_ms=round(q_full, 4), decode_b16_ms=round(dec16, 2),
                                share_of_decode=round(q_ms / dec16, 5), distance_evals=B * 64 * 64 * cfg['num_vq_embeddings'])
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        eng.decode(z)
        torch.cuda.synchronize()
        res['peak_gib'] = dict(decode_b16=round(torch.cuda.max_memory_allocated() / 2 ** 30, 2))
    if not args.no_pipeline:
        u = unet.UNet2DModel(attention_head_dim=32, sample_size=64)
        syn.det_init_(u, 3)
        pipe = diffusion.LDMPipeline(vqvae=model, unet=u.eval(), scheduler=diffusion.DDIMScheduler(
            beta_schedule='scaled_linear', beta_start=0.0015, beta_end=0.0195, clip_sample=False)).to(dev)
        run = lambda: pipe(batch_size=16, generator=torch.Generator().manual_seed(0), num_inference_steps=100, output_type='numpy')  # noqa: E731
        run()                                                 # warm: code objects, packs, the captured forward
        torch.cuda.synchronize()
        t0 = time.time()
        run()
        torch.cuda.synchronize()
        total = (time.time() - t0) * 1000.0
        z = torch.from_numpy(syn.det_noise((16, 3, 64, 64), 5)).to(dev)
        dec = timed(lambda: model.decode(z), max(args.iters, 1), 1)
        res['ldm_pipeline'] = dict(steps=100, batch=16, unet_params_m=round(sum(p.numel() for p in u.parameters()) / 1e6, 1),
                                   total_ms=round(total, 1), decode_ms=round(dec, 1), decode_share=round(dec / total, 4))
    if not args.no_cpu:
        torch.set_num_threads(16)
        z1 = torch.from_numpy(syn.det_noise((1, 3, 64, 64), 5))
        with torch.no_grad():
            vq_ref.decode(P, cfg, z1)
            t0 = time.time()
            vq_ref.decode(P, cfg, z1)
        cpu_ms = (time.time() - t0) * 1000.0
        res['cpu_decode'] = dict(threads=16, ms_per_image=round(cpu_ms, 1),
                                 speedup_hip_b1=round(cpu_ms / res['decode']['b1']['ms_per_image'], 1),
                                 speedup_hip_b16=round(cpu_ms / res['decode']['b16']['ms_per_image'], 1))
    print(json.dumps(res))


if __name__ == '__main__':
    main()
