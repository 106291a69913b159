"""The ldm_exp samplers on the MI355X: dp_cfg_denoise_step (csrc/ldm_sampler.hip) and the loops of diff-pruning_amd/ldm_sampler.py
on the HIP LDM UNet and VQ first stage, against the fixtures the reference wrote (tests/golden/make_golden_ldm_sampler.py).

Bounds (none fixed by hand):
  * the kernel equals its CPU stand-in (tests/mock_ops_ldm_sampler.py: separately rounded fp32 torch ops in the kernel's order)
    bit for bit: both are sequences of correctly rounded IEEE operations on the same operands;
  * a fixture step equals the reference's fp32 result bit for bit and lies within max(4 e_ref32, 4 * 2^-24 * max|y64|) of the
    fixture's fp64 result, e_ref32 being the reference's own fp32 distance stored beside it (tests/ddpm_exp_sampler_ref.py's rule);
  * a logged chain state or x0 prediction lies within max(10 x the reference fp32 chain's own gap at that state, the single-step
    floor 4 * 2^-24 * max|y64|) of the fp64 fixture: CHAIN_FACTOR of tests/test_ddpm_exp_sampler_gpu.py.  Against the reference's
    fp32 run of ldm_sampler.npz the triangle inequality adds that run's own gap: 11 x the gap;
  * PNG bytes and FID statistics are compared for equality.
profiles/ldm_sampler_gpu_tests.txt holds every measured value beside its bound."""
import ctypes
import os

import numpy as np
import pytest
import torch

import golden_common as gc
import ldm_sampler_ref as R
import mock_ops_ldm_sampler as mock
import vq_ref
from helpers import pkg

pytestmark = pytest.mark.gpu
DEV = 'cuda'
CAP = 4096 * 256 * 4                               # elements one launch covers without a second grid-stride trip (16-byte path)
SIZES = [1, 3, 4, 5, 255, 1027, 1028, CAP + 1028, CAP + 1029]      # 1028s: a multiple of 4, so the guided pair shares one alignment
CHAIN_FACTOR = 10.0
COEF = (0.8660254, 0.5, 0.70710677, 0.61237246, 0.35355338)        # any five fp32 scalars: the stand-in is handed the same ones


def _launched(lib, before):
    n = lib.dp_launch_count() - before
    arr = (ctypes.c_char_p * 256)()
    k = lib.dp_recent_launches(arr, 256)
    return [arr[i].decode() for i in range(k)][k - n:] if n else []


def _kernel(order, guided):
    return '(cfg_denoise_step_kernel<%d, %s>)' % (order, 'true' if guided else 'false')


def _line(report, key, **kw):
    report['ldm_sampler/' + key] = kw
    print('ldm_sampler/%s %s' % (key, ' '.join('%s=%.3e' % (k, v) if isinstance(v, float) else '%s=%s' % (k, v) for k, v in kw.items())))


# ---------------------------------------------------------------------------------------------- the kernel against the stand-in
@pytest.fixture(scope='module')
def seeded():
    """x, eps pair [2, n + 1] (so that either half can start at element offset 0 or 1), h1 .. h3, z: host and device copies."""
    n = SIZES[-1] + 1
    gen = torch.Generator().manual_seed(17)
    host = {k: torch.randn(n, generator=gen) for k in ('x', 'e_u', 'e_c', 'h1', 'h2', 'h3', 'z')}
    return host, {k: v.to(DEV) for k, v in host.items()}


@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('order', [0, 1, 2, 3, 4])
def test_kernel_equals_the_stand_in(n, order, seeded):
    """Every size at element offsets 0 (16-byte aligned) and 1 (a scalar head of 3), guided (the [2n] eps read in place) and
    unguided, with and without z, x0_out and eg_out, in place, and with an output of another alignment (all scalar): next, x0
    and the guided eps equal the stand-in's bit for bit, and the launch is the instantiation of (order, guided)."""
    ops, L = pkg('ops'), pkg('_lib')
    lib = L.load()
    host, dev = seeded
    need = (0, 1, 2, 3, 1)[order]
    combos = [(True, True), (True, False), (False, True), (False, False)]
    for off in (0, 1):
        sl = slice(off, off + n)
        for guided, noisy in combos:
            def args(src):
                e = torch.cat([src['e_u'][sl], src['e_c'][sl]]) if guided else src['e_u'][sl].clone()
                return src['x'][sl], e, [src[h][sl] for h in ('h1', 'h2', 'h3')][:need], src['z'][sl] if noisy else None
            kw = dict(scale=3.0 if guided else None, order=order, temperature=0.8)
            x, e, hist, z = args(host)
            want0, wantg = torch.empty(n), torch.empty(n)
            want = mock.cfg_denoise_step(x, e, COEF, hist=hist, z=z, x0_out=want0, eg_out=wantg, **kw)
            x, e, hist, z = args(dev)
            e = torch.empty(e.numel() + 1, device=DEV)[off:off + e.numel()].copy_(e)      # eps at the offset under test as well
            assert x.data_ptr() % 16 == 4 * off and e.data_ptr() % 16 == 4 * off
            buf = torch.empty(n + 1, device=DEV)[sl]
            buf0 = torch.full((n + 2,), 7.0, device=DEV)
            bufg = torch.full((n + 2,), 7.0, device=DEV)
            before = lib.dp_launch_count()
            nxt = ops.cfg_denoise_step(x, e, COEF, hist=hist, z=z, out=buf, x0_out=buf0[sl], eg_out=bufg[sl], **kw)
            assert _launched(lib, before) == [_kernel(order, guided)]
            assert float(buf0[off + n]) == 7.0 and float(bufg[off + n]) == 7.0                        # nothing written past the end
            assert torch.equal(nxt.cpu(), want) and torch.equal(buf0[sl].cpu(), want0) and torch.equal(bufg[sl].cpu(), wantg), \
                (n, off, guided, noisy, float((nxt.cpu() - want).abs().max()))
            plain = ops.cfg_denoise_step(x, e, COEF, hist=hist, z=z, out=torch.empty(n + 1, device=DEV)[sl], **kw)
            assert torch.equal(plain, nxt)                                                              # x0_out / eg_out off
            xc = torch.empty(n + 1, device=DEV)[sl].copy_(x)
            assert ops.cfg_denoise_step(xc, e, COEF, hist=hist, z=z, out=xc, **kw) is xc and torch.equal(xc, nxt)     # in place
            before = lib.dp_launch_count()
            mis = ops.cfg_denoise_step(x, e, COEF, hist=hist, z=z, out=torch.empty(n + 2, device=DEV)[1 - off:1 - off + n], **kw)
            assert _launched(lib, before) == [_kernel(order, guided)] and torch.equal(mis, nxt)       # two alignments: all scalar


def test_op_refuses_aliased_outputs_and_short_histories(seeded):
    ops = pkg('ops')
    _, dev = seeded
    x, e, h = dev['x'][:64], dev['e_u'][:64].clone(), dev['h1'][:64]
    with pytest.raises(AssertionError):
        ops.cfg_denoise_step(x, e, COEF, x0_out=x)
    with pytest.raises(AssertionError):
        ops.cfg_denoise_step(x, e, COEF, out=e)
    with pytest.raises(AssertionError):
        ops.cfg_denoise_step(x, e, COEF, order=2, hist=[h])
    with pytest.raises(AssertionError):
        ops.cfg_denoise_step(x, e, COEF, scale=3.0)                       # guided needs the [2n] pair


# ---------------------------------------------------------------------------------------------- fixture steps
@pytest.mark.parametrize('name', list(R.STEP_CASES))
def test_kernel_on_the_reference_single_steps(name, report):
    ops, S = pkg('ops'), pkg('ldm_sampler')
    g = R.load(R.STEPS_FILE)
    nxt, x0, eg = R.run_step(ops, S, g, name, DEV)
    same = bool(np.array_equal(nxt.cpu().numpy(), g[name + ':next_32']) and np.array_equal(x0.cpu().numpy(), g[name + ':x0_32']))
    if eg is not None:
        same = same and bool(np.array_equal(eg.cpu().numpy(), g[name + ':eg32']))
    errs = {}
    for got, what in ((nxt, 'next'), (x0, 'x0')):
        y64 = g['%s:%s_64' % (name, what)]
        errs[what] = (float(np.abs(got.double().cpu().numpy() - y64).max()), R.single_step_bound(g['%s:e_ref32_%s' % (name, what)], y64))
    _line(report, 'step/' + name, err_next=errs['next'][0], bound_next=errs['next'][1], err_x0=errs['x0'][0], bound_x0=errs['x0'][1],
          equals_reference_fp32=same)
    assert same
    assert all(e <= b for e, b in errs.values()), errs


# ---------------------------------------------------------------------------------------------- chains on the HIP tiny UNet
def _tiny_unet():
    ldm = pkg('ldm')
    model = ldm.UNetModel(**gc.LDM_TINY_CFG)
    gc.det_init_(model, R.UNET_SEED)
    return model.to(DEV).eval()


@pytest.fixture(scope='module')
def tiny():
    return _tiny_unet()


def _chain_inputs():
    cfg = gc.LDM_TINY_CFG
    H = cfg['image_size']
    return (torch.from_numpy(gc.det_noise((2, cfg['in_channels'], H, H), R.X_T_SEED)).to(DEV),
            torch.from_numpy(gc.det_noise((2, 1, cfg['context_dim']), R.COND_SEED)).to(DEV),
            torch.from_numpy(gc.det_noise((2, 1, cfg['context_dim']), R.UNCOND_SEED)).to(DEV))


@pytest.mark.parametrize('name', list(R.UNET_CHAINS))
def test_chains_on_the_hip_unet_against_the_reference(name, tiny, report):
    S, ldm_sweep = pkg('ldm_sampler'), pkg('ldm_sweep')
    kind, eta, temp = R.UNET_CHAINS[name]
    g = R.load(R.CHAINS_FILE)
    x_T, cond, uncond = _chain_inputs()
    noise = torch.from_numpy(g[name + ':noise']).to(DEV) if eta != 0 else None
    smp = (S.DDIMSampler if kind == 'ddim' else S.PLMSSampler)(tiny)
    assert torch.equal(smp.schedule.alphas_cumprod, R.alphas_cumprod32())
    out, inter = smp.sample(R.UNET_S, 2, x_T.shape[1:], conditioning=cond, eta=eta, temperature=temp, x_T=x_T, log_every_t=R.LOG_EVERY,
                            unconditional_guidance_scale=R.UNET_SCALE, unconditional_conditioning=uncond,
                            noise_fn=(lambda k, shape: noise[k]) if eta != 0 else None)
    assert out is inter['x_inter'][-1] and inter['x_inter'][0] is x_T
    for what, key in (('x_inter', ':x_inter64'), ('pred_x0', ':pred_x0_64')):
        y64, gaps = g[name + key], g[name + ':gap_' + what]
        got = inter[what]
        assert len(got) == y64.shape[0] == 1 + R.UNET_S // R.LOG_EVERY + 1
        errs = [float(np.abs(t.double().cpu().numpy() - y64[k]).max()) for k, t in enumerate(got)]
        bounds = [max(CHAIN_FACTOR * float(gaps[k]), 4 * R.U * float(np.abs(y64[k]).max())) for k in range(len(got))]
        _line(report, 'chain/%s/%s' % (name, what), worst_err=max(errs), worst_err_over_bound=max(e / b for e, b in zip(errs, bounds)),
              errs=' '.join('%.1e' % v for v in errs), bounds=' '.join('%.1e' % v for v in bounds))
        assert all(e <= b for e, b in zip(errs, bounds)), (name, what, errs, bounds)
    if name == 'ddim:eta0':
        old = R.load('ldm_sampler.npz')                                # the reference's fp32 run of the same chain
        y64, gaps = g[name + ':x_inter64'], g[name + ':gap_x_inter']
        errs = [float(np.abs(t.cpu().numpy().astype(np.float64) - old['x_inter'][k]).max()) for k, t in enumerate(inter['x_inter'])]
        bounds = [max((CHAIN_FACTOR + 1) * float(gaps[k]), 4 * R.U * float(np.abs(y64[k]).max())) for k in range(len(errs))]
        sweep = ldm_sweep.ddim_sample_cfg(tiny, ldm_sweep.LdmSchedule(), x_T, cond, uncond, S=R.UNET_S, scale=R.UNET_SCALE)
        _line(report, 'chain/%s/against_ldm_sampler_npz' % name, worst_err=max(errs), worst_err_over_bound=max(e / b for e, b in zip(errs, bounds)),
              distance_from_ddim_sample_cfg=float((sweep - out).abs().max()), max_abs_sample=float(out.abs().max()))
        assert all(e <= b for e, b in zip(errs, bounds)), (errs, bounds)


# ---------------------------------------------------------------------------------------------- sample_classes
def test_sample_classes_bytes_stats_and_ranks(tiny, tmp_path, report):
    """Tiny UNet, VQ_TINY_CFG, a seeded ClassEmbedder, classes [3, 7], ipc 4, batch 2, 4 steps.  The statistics gathered on the
    fly equal those read back from the folder in the order the files were written (the same bytes through the same kernels in the
    same batches); metrics.compute_statistics_of_path reads them sorted by name, which swaps two batches of the fp32
    accumulation: that distance is reported."""
    from PIL import Image
    S, ops, metrics, ldm_sweep, vq, syn = (pkg(m) for m in ('ldm_sampler', 'ops', 'metrics', 'ldm_sweep', 'vq', 'synthetic'))
    cfg = gc.LDM_TINY_CFG
    first = vq.VQModel(**syn.VQ_TINY_CFG)
    first.load_state_dict({k: v.float() for k, v in vq_ref.params(syn.VQ_TINY_CFG, 3).items()})
    first = first.to(DEV).eval()
    emb = ldm_sweep.ClassEmbedder(cfg['context_dim'], 1001)
    with torch.no_grad():
        emb.embedding.weight.copy_(torch.from_numpy(gc.det_noise((1001, cfg['context_dim']), 77)))
    emb = emb.to(DEV)
    shape = (cfg['in_channels'], cfg['image_size'], cfg['image_size'])
    classes, bs, steps, seed = [3, 7], 2, 4, 21
    kw = dict(classes=classes, ipc=4, batch_size=bs, ddim_steps=steps, scale=3.0, seed=seed, latent_shape=shape, scale_factor=0.5)
    dims = 8
    proj = torch.randn(3 * 32 * 32, dims, generator=torch.Generator().manual_seed(3)).to(DEV)

    def inception(batch):
        return ((batch.reshape(batch.shape[0], -1) @ proj)[:, :, None, None],)
    stats = metrics.FeatureStats(dims, torch.device(DEV))
    smp = S.DDIMSampler(tiny)
    one = str(tmp_path / 'w1')
    assert S.sample_classes(smp, emb, first, one, rank=0, world=1, stats=stats, inception=inception, **kw) == 8
    order = [(rnd, pos) for rnd in range(2) for pos in range(2)]
    names = ['%d_%d.png' % (classes[pos], (rnd * 2 + pos) * bs + i) for rnd, pos in order for i in range(bs)]
    assert sorted(os.listdir(one)) == sorted(names)
    got = np.stack([np.asarray(Image.open(os.path.join(one, f)), dtype=np.uint8) for f in names])
    want = []
    for rnd, pos in order:
        gen = torch.Generator(device=DEV).manual_seed(seed + rnd * 2 + pos)
        x_T = torch.randn((bs,) + shape, device=DEV, generator=gen)
        z, _ = smp.sample(steps, bs, shape, conditioning=emb(torch.tensor(bs * [classes[pos]])), x_T=x_T,
                          unconditional_guidance_scale=3.0, unconditional_conditioning=emb(torch.tensor(bs * [1000])))
        want.append(ops.image_to_u8(ldm_sweep.decode_first_stage(first, z, 0.5)))
    want = torch.cat(want).cpu().numpy()
    assert got.shape == (8, 32, 32, 3) and np.array_equal(got, want) and got.min() != got.max()
    mu, sigma = stats.finalize()
    files = [os.path.join(one, f) for f in names]
    mu2, sigma2 = metrics.get_activations(metrics._image_batches(files, bs, DEV), inception, bs, dims, DEV).finalize()
    e_mu, e_sg = float(np.abs(mu - mu2).max()), float(np.abs(sigma - sigma2).max())
    mu3, sigma3 = metrics.compute_statistics_of_path(one, inception, bs, dims, DEV)
    _line(report, 'sample_classes', mu_abs_diff=e_mu, sigma_abs_diff=e_sg, mu_abs_diff_sorted_read=float(np.abs(mu - mu3).max()),
          sigma_abs_diff_sorted_read=float(np.abs(sigma - sigma3).max()), max_abs_mu=float(np.abs(mu).max()))
    assert e_mu == 0.0 and e_sg == 0.0
    two = str(tmp_path / 'w2')                                           # world 2 by arguments, in one process
    assert [S.sample_classes(smp, emb, first, two, rank=r, world=2, **kw) for r in (0, 1)] == [4, 4]
    assert sorted(os.listdir(two)) == sorted(names)
    assert all(open(os.path.join(one, f), 'rb').read() == open(os.path.join(two, f), 'rb').read() for f in names)
