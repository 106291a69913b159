"""VQ first stage and LDMPipeline on the MI355X: the HIP vector quantizer (csrc/vq.hip) against fp64, VQModel on the reference's
fixtures (tests/golden/vq_tiny.npz), the micro LDMPipeline (tests/golden/ldm_pipeline_micro), decode_first_stage, and the
full-size VQ-f4 decode.  Bounds: max(4 e_ref32, 2e-5 max|y|) against fp64, e_ref32 the reference's own fp32 error (the sampling
tests' form); quantizer indices may differ from fp64 only where the fp64 relative margin is below 1e-6."""
import json
import os
import time

import numpy as np
import pytest
import torch

from conftest import isolated
from helpers import pkg
import vq_ref

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
MICRO = os.path.join(GOLD, 'ldm_pipeline_micro')
NEAR_TIE = 1e-6
EPS_FACTOR, EPS_FLOOR, STEP_ABS, U8_SHARE = 4.0, 2e-5, 2e-6, 0.005        # tests/test_sampling_gpu.py


def _fx():
    return dict(np.load(os.path.join(GOLD, 'vq_tiny.npz')))


def _err(a, b):
    return float((torch.as_tensor(a).double().cpu() - torch.as_tensor(b).double().cpu()).abs().max())


def _bound(ref32, ref64):
    return max(EPS_FACTOR * _err(ref32, ref64), 2e-5 * float(np.abs(ref64).max()))


def _check_indices(idx, idx64, margin, report=None, key=None):
    """Indices that differ from fp64 must sit at an fp64 near-tie; returns the number of such flips."""
    idx, idx64 = idx.cpu(), idx64.cpu()
    bad = idx != idx64
    flips = int(bad.sum())
    if flips:
        assert float(margin[bad].max()) < NEAR_TIE, ('index differs from fp64 away from a near-tie', float(margin[bad].max()))
    if report is not None:
        report[key] = flips
    return flips


@pytest.mark.parametrize('K', [1, 7, 64, 1000, 8192, 16384])
@pytest.mark.parametrize('D', [1, 3, 4, 8, 16])
def test_vq_quantize_kernel_matches_fp64(report, K, D):
    ops = pkg('ops')
    g = torch.Generator().manual_seed(1000 * K + D)
    big = torch.randn(3, D + 2, 7, 9, generator=g)                      # odd N * H * W = 189 pixels
    E = (torch.randn(K, D, generator=g) / D ** 0.5).contiguous()
    zd = big.to(DEV)[:, 1:D + 1]                                         # image stride (D + 2) H W: not contiguous
    assert not zd.is_contiguous()
    zq, loss, idx = ops.vq_quantize(zd, E.to(DEV))
    torch.cuda.synchronize()
    z = big[:, 1:D + 1].contiguous()
    zq64, loss64, idx64, margin = vq_ref.quantize(z.double(), E.double())
    flips = _check_indices(idx, idx64, margin, report.setdefault('vq/kernel_flips', {}), 'K%d_D%d' % (K, D))
    idx = idx.cpu()
    zf = z.permute(0, 2, 3, 1).reshape(-1, D)
    expect = (zf + (E[idx] - zf)).reshape(3, 7, 9, D).permute(0, 3, 1, 2)      # fp32, the reference's two roundings
    assert torch.equal(zq.cpu(), expect)
    e = (E.double()[idx] - zf.double())
    loss_own = (1.25 * (e ** 2).mean())
    assert abs(float(loss) / float(loss64) - 1) < 1e-6 or flips
    assert abs(float(loss) / float(loss_own) - 1) < 1e-6
    # without the optional outputs the same z_q comes out
    zq2, l2, i2 = ops.vq_quantize(zd, E.to(DEV), want_indices=False, want_loss=False)
    assert l2 is None and i2 is None and torch.equal(zq2.cpu(), zq.cpu())


def test_vq_quantize_ties_pick_the_lowest_index():
    ops = pkg('ops')
    g = torch.Generator().manual_seed(5)
    base = torch.randn(40, 3, generator=g)
    E = torch.cat([base, base, base[:7]])                               # every code of the first 40 appears two or three times
    E = E[torch.randperm(E.shape[0], generator=g)]
    z = torch.randn(2, 3, 5, 7, generator=g)
    _, _, idx = ops.vq_quantize(z.to(DEV), E.to(DEV))
    idx = idx.cpu()
    _, _, idx64, margin = vq_ref.quantize(z.double(), base.double())           # margins among the distinct codes
    assert float(margin.min()) > NEAR_TIE and torch.equal(E[idx], base[idx64])              # the nearest code vector ...
    first = torch.stack([torch.nonzero((E == E[i]).all(1))[0, 0] for i in idx.tolist()])
    assert torch.equal(idx, first)                                                          # ... at its lowest index
    # exact ties: z at the origin, codes +-e are all at the same distance
    E2 = torch.tensor([[3.0, 0, 0], [1.0, 0, 0], [-1.0, 0, 0], [0, 1.0, 0], [0, 0, -1.0]])
    z2 = torch.zeros(1, 3, 3, 3)
    _, _, idx2 = ops.vq_quantize(z2.to(DEV), E2.to(DEV))
    assert idx2.cpu().tolist() == [1] * 9
    with pytest.raises(NotImplementedError):
        ops.vq_quantize(torch.zeros(1, 17, 2, 2, device=DEV), torch.zeros(4, 17, device=DEV))


def _tiny(seed=None):
    vq, syn = pkg('vq'), pkg('synthetic')
    fx = _fx()
    model = vq.VQModel(**syn.VQ_TINY_CFG)
    model.load_state_dict({k: v.float() for k, v in vq_ref.params(syn.VQ_TINY_CFG, int(fx['seed'] if seed is None else seed)).items()})
    return model.to(DEV).eval(), fx


def test_vq_model_tiny_matches_the_reference_fixture(report):
    model, fx = _tiny()
    x = torch.from_numpy(fx['x']).to(DEV)
    lat = model.encode(x).latents
    assert _err(lat, fx['latents64']) <= _bound(fx['latents32'], fx['latents64'])
    lat_in = torch.from_numpy(fx['latents64']).float().to(DEV)
    zq, loss, (_, _, idx) = model.quantize(lat_in)
    assert torch.equal(idx.cpu(), torch.from_numpy(fx['idx64']))                   # margins >= 1e-5: 0 flips
    assert _err(zq, fx['zq64']) <= _bound(fx['zq32'], fx['zq64'])
    assert abs(float(loss) / float(fx['loss64']) - 1) < 1e-6
    errs = {}
    for name, out in (('decode', model.decode(lat_in).sample), ('decode_nq', model.decode(lat_in, force_not_quantize=True).sample),
                      ('forward', model(x).sample)):
        errs[name] = (_err(out, fx[name + '64']), _bound(fx[name + '32'], fx[name + '64']))
        assert errs[name][0] <= errs[name][1], (name, errs[name])
    assert model.decode(lat_in, return_dict=False)[0].shape == (2, 3, 16, 16)
    report['vq/tiny_err_bound'] = errs


def test_vq_model_from_ldm_keys_is_bit_identical():
    ckpt, vq, syn = pkg('checkpoint'), pkg('vq'), pkg('synthetic')
    model, fx = _tiny()
    with open(os.path.join(GOLD, 'vq_ldm_keys.json')) as f:
        keys = json.load(f)['keys']
    P = vq_ref.params(syn.VQ_TINY_CFG, int(fx['seed']), torch.float32)
    other = vq.VQModel(**syn.VQ_TINY_CFG)
    other.load_state_dict(ckpt.convert_ldm_first_stage({'first_stage_model.' + lk: P[dk].reshape(s) for lk, (dk, s) in keys.items()}))
    other = other.to(DEV).eval()
    lat = torch.from_numpy(fx['latents64']).float().to(DEV)
    x = torch.from_numpy(fx['x']).to(DEV)
    assert torch.equal(model.decode(lat).sample, other.decode(lat).sample)
    assert torch.equal(model.encode(x).latents, other.encode(x).latents)


def test_vq_model_sees_in_place_weight_swaps():
    model, fx = _tiny()
    lat = torch.from_numpy(fx['latents64']).float().to(DEV)
    a = model.decode(lat).sample.clone()
    other, _ = _tiny(seed=int(fx['seed']) + 1)
    for p, q in zip(model.parameters(), other.parameters()):
        p.data.copy_(q.data)                                # invisible to _version: the packed operands must not be reused
    b = model.decode(lat).sample
    assert not torch.equal(a, b) and torch.equal(b, other.decode(lat).sample)
    with model.pin_weights():                               # pinned: packed once, same bits
        assert torch.equal(model.decode(lat).sample, b) and torch.equal(model.decode(lat).sample, b)


def test_vq_model_runs_a_large_batch_in_micro_batches(monkeypatch, report):
    """encode / decode split a batch whose largest per-image tensor would take one call past 2 GiB (32-bit buffer offsets); the
    limit is lowered here so that the tiny model splits 7 images.  Every image against the fp64 restatement."""
    vq, syn = pkg('vq'), pkg('synthetic')
    cfg = syn.VQ_TINY_CFG
    model, fx = _tiny()
    x = torch.from_numpy(syn.det_clean((7, 3, 16, 16), 73))
    eng = model.engine()
    monkeypatch.setattr(vq.VQEngine, 'MAX_CALL_BYTES', 3 * eng.per_image_bytes(x.shape, False))
    calls = []
    for name in ('_encode', '_decode'):
        def wrap(self, t, *a, real=getattr(vq.VQEngine, name), name=name, **k):
            calls.append((name, t.shape[0]))
            return real(self, t, *a, **k)
        monkeypatch.setattr(vq.VQEngine, name, wrap)
    lat = model.encode(x.to(DEV)).latents
    out = model.decode(lat).sample
    _, _, (_, _, idx) = model.quantize(lat)
    enc = [n for k, n in calls if k == '_encode']
    dec = [n for k, n in calls if k == '_decode']
    assert enc == [3, 3, 1] and sum(dec) == 7 and len(dec) > 1, calls
    assert lat.shape == (7, 3, 8, 8) and out.shape == (7, 3, 16, 16)
    P64 = vq_ref.params(cfg, int(fx['seed']))
    P32 = {k: v.float() for k, v in P64.items()}
    e64, e32 = vq_ref.encode(P64, cfg, x.double()), vq_ref.encode(P32, cfg, x)
    zl = lat.cpu()
    _, _, idx64, margin = vq_ref.quantize(zl.double(), P64['quantize.embedding.weight'])
    flips = _check_indices(idx, idx64, margin)
    d64 = vq_ref.decode(P64, cfg, zl.double(), indices=idx.cpu())
    d32 = vq_ref.decode(P32, cfg, zl, indices=idx.cpu())
    for i in range(7):
        assert _err(lat[i], e64[i]) <= _bound(e32[i], e64[i]), ('encode', i)
        assert _err(out[i], d64[i]) <= _bound(d32[i], d64[i]), ('decode', i)
    report['vq/micro_batches'] = dict(encode=enc, decode=dec, flips=flips)


def _micro_pipe():
    diffusion, vq, unet, syn = pkg('diffusion'), pkg('vq'), pkg('unet'), pkg('synthetic')

    def cfg(rel):                                          # the reference-written configs; the weights are det_param by name
        with open(os.path.join(MICRO, rel)) as f:
            return {k: v for k, v in json.load(f).items() if not k.startswith('_')}
    fx = _fx()
    vqm = vq.VQModel(**cfg('vqvae/config.json'))
    vqm.load_state_dict({k: v.float() for k, v in vq_ref.params(dict(vqm.config), int(fx['seed'])).items()})
    u = unet.UNet2DModel(**cfg('unet/config.json'))
    syn.det_init_(u, 81)
    sc = cfg('scheduler/scheduler_config.json')
    sched = diffusion.DDIMScheduler(beta_schedule=sc['beta_schedule'], beta_start=sc['beta_start'], beta_end=sc['beta_end'],
                                    clip_sample=sc['clip_sample'])
    return diffusion.LDMPipeline(vqvae=vqm, unet=u, scheduler=sched).to(DEV)


def test_ldm_pipeline_micro(report, tmp_path):
    diffusion = pkg('diffusion')
    ex = dict(np.load(os.path.join(MICRO, 'expected.npz')))
    pipe = _micro_pipe()
    B = ex['x_T'].shape[0]
    x_T = diffusion.randn_tensor(ex['x_T'].shape, generator=torch.Generator().manual_seed(82))
    assert torch.equal(x_T, torch.from_numpy(ex['x_T']))
    # teacher-forced steps of the fp64 chain
    pipe.scheduler.set_timesteps(len(ex['timesteps']))
    assert [int(t) for t in pipe.scheduler.timesteps] == ex['timesteps'].tolist()
    worst = []
    with torch.no_grad():
        for k, t in enumerate(ex['timesteps'].tolist()):
            xk = torch.from_numpy(ex['x_k'][k]).float().to(DEV)
            eps = pipe.unet(xk, t).sample
            e = _err(eps, ex['eps_k'][k])
            assert e <= max(EPS_FACTOR * float(ex['e_ref32'][k]), EPS_FLOOR), (k, e)
            ek = torch.from_numpy(ex['eps_k'][k]).float()
            step = pipe.scheduler.step(ek.to(DEV), t, xk).prev_sample
            # the fp64 step on the same fp32-rounded inputs, within the sampling tests' 2e-6 scaled by the size of the x0 term
            # (10 steps of a scaled_linear schedule start at alpha_t = 0.0009: 1 / sqrt(alpha_t) amplifies every rounding of x_k)
            sc = pipe.scheduler
            a_t = float(sc.alphas_cumprod[t])
            tp = t - sc.config.num_train_timesteps // sc.num_inference_steps
            a_p = float(sc.alphas_cumprod[tp]) if tp >= 0 else float(sc.final_alpha_cumprod)
            xd, ed = xk.cpu().double(), ek.double()
            x0 = (xd - (1 - a_t) ** 0.5 * ed) / a_t ** 0.5
            step64 = a_p ** 0.5 * x0 + (1 - a_p) ** 0.5 * ed
            amp = max(1.0, float((a_p ** 0.5 * x0).abs().max()))         # fp32 ulps of the x0 term set the scale at large t
            s = _err(step, step64)
            assert s <= STEP_ABS * amp, (k, s, amp)
            assert _err(step64, ex['step_out'][k]) <= 5 * STEP_ABS * amp, (k, _err(step64, ex['step_out'][k]), amp)
            worst.append((e, s))
    # the free-running pipeline: at most 0.5 % of the uint8 values differ from the reference's fp32 run
    # the x_T the pipeline itself draws: the first sample its loop hands to the scheduler
    drawn, scale_input = [], pipe.scheduler.scale_model_input

    def record(sample, t=None):
        if not drawn:
            drawn.append(sample.detach().cpu().clone())
        return scale_input(sample, t)
    pipe.scheduler.scale_model_input = record
    try:
        img = pipe(batch_size=B, generator=torch.Generator().manual_seed(82), num_inference_steps=10, output_type='numpy').images
    finally:
        del pipe.scheduler.scale_model_input
    assert len(drawn) == 1 and torch.equal(drawn[0], torch.from_numpy(ex['x_T']))
    u8 = (img * 255).round().astype(np.uint8)
    share = float((u8 != ex['u8_ref32']).mean())
    assert img.shape == (B, 16, 16, 3) and share <= U8_SHARE, share
    pil = pipe(batch_size=B, generator=torch.Generator().manual_seed(82), num_inference_steps=10).images
    assert len(pil) == B and np.array_equal(np.asarray(pil[0]), u8[0])
    tup = pipe(batch_size=B, generator=torch.Generator().manual_seed(82), num_inference_steps=10, output_type='numpy',
               return_dict=False)
    assert isinstance(tup, tuple) and np.array_equal(tup[0], img)
    # save / load on the device: the same images
    pipe.save_pretrained(str(tmp_path / 'p'))
    back = diffusion.LDMPipeline.from_pretrained(str(tmp_path / 'p')).to(DEV)
    img2 = back(batch_size=B, generator=torch.Generator().manual_seed(82), num_inference_steps=10, output_type='numpy').images
    assert np.array_equal(img2, img)
    # the decoded fp64 chain's end point
    dec = pipe.vqvae.decode(torch.from_numpy(ex['step_out'][-1]).float().to(DEV)).sample
    assert _err(dec, ex['decoded64']) <= _bound(ex['decoded32_of64'], ex['decoded64'])
    report['vq/micro_pipeline'] = dict(worst_eps_step=worst, u8_share=share)


def test_ldm_pipeline_sample_to_dir_with_feature_stats(tmp_path):
    metrics = pkg('metrics')
    pipe = _micro_pipe()
    dims = 8                                               # (FeatureStats takes multiples of 4)
    proj = torch.randn(3 * 16 * 16, dims, generator=torch.Generator().manual_seed(3)).to(DEV)

    def inception(batch):
        return ((batch.reshape(batch.shape[0], -1) @ proj)[:, :, None, None],)
    stats = metrics.FeatureStats(dims, torch.device(DEV))
    n = metrics.sample_to_dir(pipe, str(tmp_path), total_samples=4, batch_size=2, seed=3, num_inference_steps=3, stats=stats,
                              inception=inception, rank=0, world=1)
    assert n == 4 and sorted(os.listdir(str(tmp_path / 'process_0'))) == ['0.png', '1.png', '2.png', '3.png']
    mu, sigma = stats.finalize()
    assert mu.shape == (dims,) and sigma.shape == (dims, dims) and np.isfinite(sigma).all()


def test_decode_first_stage_on_ldm_sampler_latents(report):
    ldm, ldm_sweep, syn = pkg('ldm'), pkg('ldm_sweep'), pkg('synthetic')
    cfg = syn.LDM_TINY_CFG
    unet = ldm.UNetModel(**cfg)
    syn.det_init_(unet, 9)
    unet = unet.to(DEV).eval()
    g = torch.Generator().manual_seed(11)
    x_T = torch.randn(2, 3, 16, 16, generator=g).to(DEV)
    c = torch.randn(2, 1, cfg['context_dim'], generator=g).to(DEV)
    uc = torch.randn(2, 1, cfg['context_dim'], generator=g).to(DEV)
    with torch.no_grad():
        z = ldm_sweep.ddim_sample_cfg(unet, ldm_sweep.LdmSchedule(), x_T, c, uc, S=4, scale=3.0)
    model, fx = _tiny()
    out = ldm_sweep.decode_first_stage(model, z, scale_factor=0.5)
    zs = (z * 2.0).cpu()                                       # 1 / 0.5 * z: exact in fp32
    _, _, (_, _, idx) = model.quantize(zs.to(DEV))
    P64 = vq_ref.params(syn.VQ_TINY_CFG, int(fx['seed']))
    _, _, idx64, margin = vq_ref.quantize(zs.double(), P64['quantize.embedding.weight'])
    flips = _check_indices(idx, idx64, margin)
    ref64 = vq_ref.decode(P64, syn.VQ_TINY_CFG, zs.double(), indices=idx.cpu())
    ref32 = vq_ref.decode({k: v.float() for k, v in P64.items()}, syn.VQ_TINY_CFG, zs, indices=idx.cpu())
    assert out.shape == (2, 3, 32, 32) and _err(out, ref64) <= _bound(ref32, ref64)
    nq = ldm_sweep.decode_first_stage(model, z, scale_factor=0.5, force_not_quantize=True)
    ref64 = vq_ref.decode(P64, syn.VQ_TINY_CFG, zs.double(), force_not_quantize=True)
    ref32 = vq_ref.decode({k: v.float() for k, v in P64.items()}, syn.VQ_TINY_CFG, zs, force_not_quantize=True)
    assert _err(nq, ref64) <= _bound(ref32, ref64)
    report['vq/decode_first_stage_flips'] = flips


@isolated(timeout=900)
def test_vq_f4_full_size_decode(report):
    vq, syn = pkg('vq'), pkg('synthetic')
    cfg = syn.VQ_F4_CFG
    P = vq_ref.params(cfg, 7, torch.float32)
    model = vq.VQModel(**cfg)
    model.load_state_dict(P)
    model = model.to(DEV).eval()
    z = torch.from_numpy(syn.det_noise((4, 3, 64, 64), 5))
    torch.cuda.reset_peak_memory_stats()
    _, _, (_, _, idx) = model.quantize(z.to(DEV))
    out = model.decode(z.to(DEV)).sample
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() / 2 ** 30
    assert out.shape == (4, 3, 256, 256) and bool(torch.isfinite(out).all())
    P64 = {k: v.double() for k, v in P.items()}
    _, _, idx64, margin = vq_ref.quantize(z.double(), P64['quantize.embedding.weight'], chunk=512)
    flips = _check_indices(idx, idx64, margin)
    t0 = time.time()
    with torch.no_grad():
        ref64 = vq_ref.decode(P64, cfg, z[:1].double(), indices=idx.cpu()[:64 * 64])
        ref32 = vq_ref.decode(P, cfg, z[:1], indices=idx.cpu()[:64 * 64])
    e_hip, e_32 = _err(out[:1], ref64), _err(ref32, ref64)
    assert e_hip <= 4 * e_32, (e_hip, e_32)
    report['vq/f4_full'] = dict(flips=flips, pixels=int(idx.numel()), err_hip=e_hip, err_cpu32=e_32, peak_gib=peak,
                                min_margin=float(margin.min()), cpu_ref_s=time.time() - t0)


@isolated(timeout=900)
def test_vq_f4_decode_above_the_single_pass_limit(report):
    """VQ-f4 at batch 32: a single pass would give the upsampled 256-channel 256 x 256 activation 2 GiB (64 MiB per image), past
    the kernels' 32-bit offsets; the engine decodes 31 + 1.  The first and the last image against CPU fp64 decodes, within 4x the
    fp32 restatement's own error."""
    vq, syn = pkg('vq'), pkg('synthetic')
    cfg = syn.VQ_F4_CFG
    P = vq_ref.params(cfg, 7, torch.float32)
    model = vq.VQModel(**cfg)
    model.load_state_dict(P)
    model = model.to(DEV).eval()
    B = 32
    z = torch.from_numpy(syn.det_noise((B, 3, 64, 64), 9))
    assert model.engine().micro_batch(z.shape, True) == 31
    torch.cuda.reset_peak_memory_stats()
    out = model.decode(z.to(DEV)).sample
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() / 2 ** 30
    assert out.shape == (B, 3, 256, 256) and bool(torch.isfinite(out).all())
    _, _, (_, _, idx) = model.quantize(z.to(DEV))
    idx = idx.cpu().view(B, -1)
    P64 = {k: v.double() for k, v in P.items()}
    errs = {}
    for i in (0, B - 1):
        _, _, idx64, margin = vq_ref.quantize(z[i:i + 1].double(), P64['quantize.embedding.weight'], chunk=512)
        flips = _check_indices(idx[i], idx64, margin)
        with torch.no_grad():
            ref64 = vq_ref.decode(P64, cfg, z[i:i + 1].double(), indices=idx[i])
            ref32 = vq_ref.decode(P, cfg, z[i:i + 1], indices=idx[i])
        e_hip, e_32 = _err(out[i:i + 1], ref64), _err(ref32, ref64)
        assert e_hip <= 4 * e_32, (i, e_hip, e_32)
        errs[i] = dict(err_hip=e_hip, err_cpu32=e_32, flips=flips)
    report['vq/f4_batch32'] = dict(images=errs, peak_gib=peak)
