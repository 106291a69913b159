"""The ddpm_exp sampler on the MI355X: dp_denoise_step and dp_image_to_u8 (csrc/sampler.hip) and the loops of
diff-pruning_amd/ddpm_exp_sampler.py on the HIP UNet2DModel, against the fixtures the reference wrote
(tests/golden/make_golden_ddpm_exp_sampler.py).

Bounds (none fixed by hand):
  * a fixture step lies within max(4 e_ref32, 4 * 2^-24 * max|y64|) of the fixture's fp64 result y64, e_ref32 being the
    reference's own fp32 distance stored beside it;
  * a step on seeded data lies within 8 * 2^-24 * M of the fp64 evaluation from the same fp32 scalars (x0: 3 * 2^-24 * A): at
    most 8 (3) roundings, each relative to a partial result that the term-magnitude sum M (A) bounds -- ddpm_exp_sampler_ref.py;
  * a chain state lies within max(10 x the reference fp32 chain's own gap at that state, the single-step floor
    4 * 2^-24 * max|y64|): the gap is one sample of a rounding walk (tests/test_sampling_gpu.py gives a free-running chain the same
    margin).
Measured on one MI355X (profiles/ddpm_exp_sampler_gpu_tests.txt holds every value beside its bound): all 21 fixture steps equal
the reference's fp32 result bit for bit (worst error 0.25 of the bound), the size sweep at most 0.45 of its bound, the chains at
most 0.20 of theirs (worst state 1.0e-4 from fp64), the FID statistics differ by exactly 0."""
import ctypes
import os

import numpy as np
import pytest
import torch

import golden_common as gc
import ddpm_exp_sampler_ref as R
from helpers import make_model, pkg

pytestmark = pytest.mark.gpu
DEV = 'cuda'
CAP = 4096 * 256 * 4                               # elements one launch covers without a second grid-stride trip (16-byte path)
SIZES = [1, 3, 4, 5, 1023, 1025, CAP + 1029]
CHAIN_FACTOR = 10.0


def _launched(lib, before):
    n = lib.dp_launch_count() - before
    arr = (ctypes.c_char_p * 256)()
    k = lib.dp_recent_launches(arr, 256)
    return [arr[i].decode() for i in range(k)][k - n:] if n else []


def _betas():
    return pkg('ddpm_exp_sampler').linear_betas()


def _coefs(kind, i, j, eta=0.0):
    S = pkg('ddpm_exp_sampler')
    table = S.alpha_table(_betas())
    c = S.generalized_coefs(table, i, j, eta) if kind == 'gen' else S.ddpm_coefs(table, i, j)
    return [float(v) for v in c]


def _line(report, key, **kw):
    report['ddpm_exp_sampler/' + key] = kw
    print('ddpm_exp_sampler/%s %s' % (key, ' '.join('%s=%.3e' % (k, v) if isinstance(v, float) else '%s=%s' % (k, v) for k, v in kw.items())))


# ---------------------------------------------------------------------------------------------- dp_denoise_step, fixture steps
@pytest.fixture(scope='module')
def steps():
    g = R.load(R.STEPS_FILE)
    return {k: g[k] for k in g.files}


@pytest.mark.parametrize('name', R.step_case_names())
def test_denoise_step_on_the_reference_single_steps(name, steps, report):
    ops, L = pkg('ops'), pkg('_lib')
    g = steps
    i, j = [int(v) for v in g[name + ':ij']]
    scale, eta = float(g[name + ':scale']), float(g[name + ':eta'])
    x, e, z = (torch.from_numpy(g[k]).to(DEV) for k in ('x', 'e', 'z'))
    x, e = x * scale, e * scale
    gen = name.startswith('gen')
    mode = ops.DENOISE_GENERALIZED if gen else ops.DENOISE_DDPM
    coef = _coefs('gen' if gen else 'ddpm', i, j, eta)
    noisy = (eta != 0) if gen else (i != 0)
    lib = L.load()
    before = lib.dp_launch_count()
    x0 = torch.empty_like(x)
    nxt = ops.denoise_step(x, e, mode, coef, z=z if noisy else None, x0_out=x0)
    assert _launched(lib, before) == ['denoise_step_kernel<%d>' % mode]
    e_next = float(np.abs(nxt.double().cpu().numpy() - g[name + ':next64']).max())
    e_x0 = float(np.abs(x0.double().cpu().numpy() - g[name + ':x0_64']).max())
    b_next = R.single_step_bound(g[name + ':e_ref32_next'], g[name + ':next64'])
    b_x0 = R.single_step_bound(g[name + ':e_ref32_x0'], g[name + ':x0_64'])
    same32 = bool(np.array_equal(nxt.cpu().numpy(), g[name + ':next32']) and np.array_equal(x0.cpu().numpy(), g[name + ':x0_32']))
    _line(report, 'step/' + name, err_next=e_next, bound_next=b_next, err_x0=e_x0, bound_x0=b_x0, equals_reference_fp32=same32)
    assert e_next <= b_next and e_x0 <= b_x0, (e_next, b_next, e_x0, b_x0)
    if not noisy and gen:                                     # z == NULL against eta = 0 with a noise tensor supplied: c1 is exactly 0
        assert coef[3] == 0.0 and torch.equal(ops.denoise_step(x, e, mode, coef, z=z), nxt)
    if name.startswith('ddpm_clamp'):
        share = float((x0.abs() == 1.0).double().mean())
        assert abs(share - float(g[name + ':clamp_share'])) < 0.01 and 0.1 <= share <= 0.9


# ---------------------------------------------------------------------------------------------- dp_denoise_step, sizes and paths
@pytest.fixture(scope='module')
def seeded():
    n = SIZES[-1] + 1
    gen = torch.Generator().manual_seed(11)
    return tuple(torch.randn(n, generator=gen).to(DEV) for _ in range(3))


@pytest.mark.parametrize('n', SIZES)
@pytest.mark.parametrize('mode', [0, 1])
def test_denoise_step_sizes_alignments_and_variants(n, mode, seeded, report):
    """Every size at element offsets 0 (16-byte aligned) and 1 (scalar head of 3), with and without x0_out, with and without z, in
    place and out of place: against fp64 from the same fp32 scalars, and bit-equal across the variants."""
    ops, L = pkg('ops'), pkg('_lib')
    lib = L.load()
    coef = _coefs('gen', 500, 490, 0.5) if mode == 0 else _coefs('ddpm', 500, 490)
    worst = dict(next=0.0, x0=0.0)
    for off in (0, 1):
        x, e, z = (t[off:off + n] for t in seeded)
        assert x.data_ptr() % 16 == 4 * off
        for zz in (z, None):
            want, want0, m, a = R.denoise64(mode, x, e, zz, coef)
            buf = torch.empty(n + 1, device=DEV)
            buf0 = torch.full((n + 2,), 7.0, device=DEV)
            before = lib.dp_launch_count()
            nxt = ops.denoise_step(x, e, mode, coef, z=zz, out=buf[off:off + n], x0_out=buf0[off:off + n])
            assert _launched(lib, before) == ['denoise_step_kernel<%d>' % mode]
            assert float(buf0[off + n]) == 7.0                                           # nothing written past the end
            e_next, e_x0 = float((nxt.double() - want).abs().max()), float((buf0[off:off + n].double() - want0).abs().max())
            assert e_next <= R.rounding_bound(m) and e_x0 <= R.x0_bound(a), (n, off, e_next, R.rounding_bound(m), e_x0, R.x0_bound(a))
            worst['next'] = max(worst['next'], e_next / R.rounding_bound(m))
            worst['x0'] = max(worst['x0'], e_x0 / R.x0_bound(a))
            plain = ops.denoise_step(x, e, mode, coef, z=zz, out=torch.empty(n + 1, device=DEV)[off:off + n])
            assert torch.equal(plain, nxt)                                               # x0_out on / off
            xc = torch.empty(n + 1, device=DEV)[off:off + n].copy_(x)
            assert ops.denoise_step(xc, e, mode, coef, z=zz, out=xc) is xc and torch.equal(xc, nxt)    # in place
            mis = ops.denoise_step(x, e, mode, coef, z=zz, out=torch.empty(n + 2, device=DEV)[1 - off:1 - off + n])
            assert torch.equal(mis, nxt)                                                 # pointers of two alignments: all scalar
    _line(report, 'sizes/mode%d/n%d' % (mode, n), worst_next_over_bound=worst['next'], worst_x0_over_bound=worst['x0'])


def test_denoise_step_equals_the_torch_fp32_expression(seeded):
    """No contraction across the reference's separate roundings, a true division: torch's eager fp32 ops on the device, one
    rounding each, give the same bits."""
    ops = pkg('ops')
    x, e, z = (t[:4099] for t in seeded)
    f = lambda v: torch.tensor(v, dtype=torch.float32, device=DEV)
    s1, s2, s3, c1, c2 = (f(v) for v in _coefs('gen', 990, 980, 0.5))
    x0 = (x - e * s1) / s2
    want = s3 * x0 + c1 * z + c2 * e
    got0 = torch.empty_like(x)
    got = ops.denoise_step(x, e, 0, _coefs('gen', 990, 980, 0.5), z=z, x0_out=got0)
    assert torch.equal(got, want) and torch.equal(got0, x0)
    r1, r2, k0, kx, d, sig = (f(v) for v in _coefs('ddpm', 500, 490))
    x0 = torch.clamp(r1 * x - r2 * e, -1, 1)
    want = (k0 * x0 + kx * x) / d + sig * z
    got = ops.denoise_step(x, e, 1, _coefs('ddpm', 500, 490), z=z, x0_out=got0)
    assert torch.equal(got, want) and torch.equal(got0, x0)


# ---------------------------------------------------------------------------------------------- dp_image_to_u8
def _edge_values():
    """Every fp32 v whose v * 255 lies within 2 ulp of k + 0.5, k = 0 .. 254 (five neighbours of the fp32 nearest (k + 0.5) / 255),
    spread over [-1.3, 1.3] by the points between."""
    k = np.arange(255, dtype=np.float64)
    c = ((k + 0.5) / 255.0).astype(np.float32)
    v = [c]
    up, dn = c.copy(), c.copy()
    for _ in range(3):
        up, dn = np.nextafter(up, np.float32(2)), np.nextafter(dn, np.float32(-2))
        v += [up.copy(), dn.copy()]
    return np.concatenate(v + [np.linspace(-1.3, 1.3, 1021, dtype=np.float32), np.array([0.0, 1.0, -1.0, -0.0], np.float32)])


@pytest.mark.parametrize('rescaled', [True, False])
@pytest.mark.parametrize('shape,pad', [((1, 3, 1, 1), 0), ((2, 3, 5, 7), 0), ((3, 1, 32, 32), 0), ((2, 3, 8, 8), 4), ((2, 3, 8, 8), 1)])
def test_image_to_u8_equals_the_torch_fp32_expression(shape, pad, rescaled):
    ops, L = pkg('ops'), pkg('_lib')
    lib = L.load()
    v = _edge_values()
    vals = np.concatenate([v, 2 * v - 1]) if rescaled else v          # (x + 1) / 2 maps 2 v - 1 onto (nearly) v
    N, C, H, W = shape
    per = C * H * W
    reps = -(-len(vals) // (N * per))
    for r in range(reps):                                              # no value is left out
        chunk = np.resize(vals[r * N * per:] if r * N * per < len(vals) else vals, N * per).astype(np.float32)
        store = torch.zeros(N, per + pad, device=DEV)
        store[:, :per] = torch.from_numpy(chunk).view(N, per).to(DEV)
        x = store[:, :per].view(N, C, H, W) if N > 1 else store[:, :per].reshape(N, C, H, W)
        before = lib.dp_launch_count()
        got = ops.image_to_u8(x, rescaled)
        vec = C <= 4 and (H * W) % 4 == 0 and (pad % 4 == 0 or N == 1)
        assert _launched(lib, before) == ['image_to_u8_kernel<%s>' % ('true' if vec else 'false')]
        t = (x + 1.0) / 2.0 if rescaled else x
        want = torch.clamp(t, 0.0, 1.0).mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
        assert got.dtype == torch.uint8 and got.shape == (N, H, W, C) and torch.equal(got, want)


# ---------------------------------------------------------------------------------------------- chains on the HIP UNet
@pytest.fixture(scope='module')
def tiny():
    return make_model(gc.TINY_CFG, 5)


@pytest.mark.parametrize('skip', ['uniform', 'quad'])
def test_chains_on_the_hip_unet_against_the_reference(skip, tiny, report):
    S = pkg('ddpm_exp_sampler')
    g = R.load(R.CHAIN_FILES[skip])
    seq = S.timestep_sequence(1000, R.CHAIN_N, skip)
    assert seq == [int(v) for v in g['seq']]
    x_T = torch.from_numpy(g['x_T']).to(DEV)
    noise = torch.from_numpy(g['noise']).to(DEV)
    table = S.alpha_table(_betas())
    for kind, eta in R.CHAIN_KINDS:
        name = R.chain_name(kind, eta)
        runs = {}
        for replay in (True, False):
            fwd = tiny.sampling_forward(tuple(x_T.shape), len(seq), replay=replay)
            assert type(fwd).__name__ == ('_CapturedForward' if replay else '_EagerForward')
            try:
                runs[replay] = S._run(kind, x_T, seq, lambda x, i: fwd(x, int(i)), table, eta, 'all', None, lambda k, shape: noise[k])
            finally:
                fwd.close()
        for a, b in zip(runs[True][0] + runs[True][1], runs[False][0] + runs[False][1]):
            assert torch.equal(a, b)                                   # replayed and eager forwards: the same bits
        f = S.generalized_steps if kind == 'generalized' else S.ddpm_steps
        kw = dict(eta=eta) if kind == 'generalized' else {}
        last, _ = f(x_T, seq, tiny, _betas(), keep='last', noise_fn=lambda k, shape: noise[k], **kw)       # the public path
        assert torch.equal(last[0], runs[True][0][-1])
        xs, x0s = runs[True]
        assert xs[0] is x_T and len(xs) == len(seq) + 1 and len(x0s) == len(seq)
        for what, got, key, gkey in (('xs', xs, ':xs64', ':gap_xs'), ('x0s', x0s, ':x0s64', ':gap_x0s')):
            y64, gaps = g[name + key], g[name + gkey]
            errs = [float(np.abs(t.double().cpu().numpy() - y64[k]).max()) for k, t in enumerate(got)]
            bounds = [max(CHAIN_FACTOR * float(gaps[k]), 4 * R.U * float(np.abs(y64[k]).max())) for k in range(len(got))]
            _line(report, 'chain/%s/%s/%s' % (skip, name, what), worst_err=max(errs), worst_err_over_bound=max(e / b for e, b in zip(errs, bounds)),
                  errs=' '.join('%.1e' % v for v in errs), bounds=' '.join('%.1e' % v for v in bounds))
            assert all(e <= b for e, b in zip(errs, bounds)), (name, what, errs, bounds)


# ---------------------------------------------------------------------------------------------- sample_fid
def test_sample_fid_bytes_and_feature_stats(tiny, tmp_path, report):
    from PIL import Image
    S, ops, metrics = pkg('ddpm_exp_sampler'), pkg('ops'), pkg('metrics')
    ss = gc.TINY_CFG['sample_size']
    smp = S.Sampler(tiny, _betas(), (3, ss, ss), timesteps=5, eta=0.0)
    dims = 8
    proj = torch.randn(3 * ss * ss, dims, generator=torch.Generator().manual_seed(3)).to(DEV)

    def inception(batch):
        return ((batch.reshape(batch.shape[0], -1) @ proj)[:, :, None, None],)
    stats = metrics.FeatureStats(dims, torch.device(DEV))
    folder = str(tmp_path / 'fid')
    assert smp.sample_fid(folder, total_n_samples=9, batch_size=4, seed=5, rank=1, world=2, stats=stats, inception=inception) == 8
    files = sorted(os.listdir(folder), key=lambda f: int(f.split('.')[0]))
    assert files == ['%d.png' % i for i in range(8)]
    gen = torch.Generator(device=DEV).manual_seed(5 + 1)
    want = torch.cat([ops.image_to_u8(smp.sample_image(torch.randn((4, 3, ss, ss), device=DEV, generator=gen))) for _ in range(2)])
    got = np.stack([np.asarray(Image.open(os.path.join(folder, f)), dtype=np.uint8) for f in files])
    assert np.array_equal(got, want.cpu().numpy()) and got.min() != got.max()
    mu, sigma = stats.finalize()
    mu2, sigma2 = metrics.compute_statistics_of_path(folder, inception, 4, dims, DEV)
    e_mu, e_sg = float(np.abs(mu - mu2).max()), float(np.abs(sigma - sigma2).max())
    _line(report, 'sample_fid', mu_abs_diff=e_mu, sigma_abs_diff=e_sg)
    assert e_mu == 0.0 and e_sg == 0.0                  # the same bytes through the same kernels in the same batches
