"""The sampler of the ddpm_exp code base -- the one the paper's FID and SSIM numbers were drawn with.

  timestep_sequence            runners/diffusion.py:498-529   (the `seq` of sample_image, 'uniform' and 'quad')
  alpha_table                  functions/denoising.py:4-7     (compute_alpha: cumprod with a leading zero beta, alpha(-1) = 1)
  generalized_steps            functions/denoising.py:10-32   (HIP kernel dp_denoise_step, mode 0)
  ddpm_steps                   functions/denoising.py:35-67   (HIP kernel dp_denoise_step, mode 1)
  Sampler.sample_image         runners/diffusion.py:492-537
  Sampler.sample_fid           runners/diffusion.py:390-427   (bytes from dp_image_to_u8)
  Sampler.sample_sequence      runners/diffusion.py:429-450
  Sampler.sample_interpolation runners/diffusion.py:452-490

It is NOT diffusion.DDIMScheduler under another name: the timesteps are range(0, T, T // n) (n = 7 gives 8 steps) or the quad list
with its repeated entries, the "previous" alpha is the alpha of the next timestep actually visited (alpha(-1) = 1 after the last),
x0 is not clipped in generalized_steps, ddpm_steps uses beta_t = 1 - a_t / a_next of the SKIPPED schedule as its variance, and
every state and every x0 prediction is returned.

Per step: one UNet forward (the model's pinned / natively replayed `sampling_forward`) and ONE launch of dp_denoise_step, which
writes the next state and the x0 prediction in the same pass.  The per-step scalars are 0-d fp32 torch ops on the host, in the
reference's operation order, from the fp32 alpha table (a CPU cumprod, as the schedulers of diffusion.py compute theirs); only the
square roots go through `_sqrt`, so that they are the correctly rounded fp32 values on every host.

Noise: `torch.randn(shape, device=x.device, generator=generator)`, or `noise_fn(step_index, shape)` when given.  generalized_steps
with eta = 0 draws nothing (c1 is exactly 0, the result is unchanged); with eta != 0 it draws at every step; ddpm_steps draws at
every step but t = 0 (the reference's mask).  The reference draws `torch.randn_like` from the GLOBAL generator at every step, used
or not: draw-order parity with it beyond the first x_T is not claimed.

EMA weights are the caller's business (`with ft.ema_scope():`), as elsewhere in this package.
"""
import glob
import os

import numpy as np
import torch

from . import ops


def linear_betas(num_timesteps=1000, beta_start=1e-4, beta_end=0.02):
    """get_beta_schedule('linear') of runners/diffusion.py as the runner holds it: a float64 linspace cast to fp32."""
    return torch.from_numpy(np.linspace(beta_start, beta_end, num_timesteps, dtype=np.float64)).float()


def timestep_sequence(num_timesteps, timesteps, skip_type):
    """The timesteps sample_image visits, ascending (the loops walk them backwards).  'uniform': every (T // n)-th of 0 .. T - 1,
    which is n + 1 entries or more when n does not divide T; 'quad': the truncated squares of n equidistant points on
    [0, sqrt(0.8 T)], small ones repeated.  Anything else raises, as the reference does."""
    if skip_type == 'uniform':
        return list(range(0, num_timesteps, num_timesteps // timesteps))
    if skip_type == 'quad':
        return [int(s) for s in np.linspace(0, np.sqrt(num_timesteps * 0.8), timesteps) ** 2]
    raise NotImplementedError('skip_type %r (the reference knows "uniform" and "quad")' % (skip_type,))


def alpha_table(betas):
    """compute_alpha for every t at once: fp32 [T + 1] on the host, entry t + 1 = prod_{s <= t} (1 - beta_s), entry 0 = alpha(-1) = 1."""
    b = torch.as_tensor(betas).detach().to('cpu', torch.float32)
    return (1 - torch.cat([torch.zeros(1), b], dim=0)).cumprod(dim=0)


def _sqrt(t):
    """The correctly rounded fp32 square root of a 0-d fp32 tensor, on every host: taken in fp64 and rounded once more, which
    is innocuous for a square root (53 >= 2 * 24 + 2 bits) and equals IEEE sqrtf.  torch's own fp32 CPU sqrt is not correctly
    rounded everywhere -- one AVX512 host returned sqrt(alpha_990) and sqrt(1 / alpha_999) one ulp off, which moves an x0
    prediction at t = 999 (x / sqrt(alpha) with sqrt(alpha) = 6e-3) by 4e-5."""
    return t.double().sqrt().float()


def generalized_coefs(table, i, j, eta):
    """(s1, s2, s3, c1, c2) of denoising.py:23-29 for the step i -> j as 0-d fp32 tensors."""
    at, an = table[i + 1], table[j + 1]
    c1 = eta * _sqrt((1 - at / an) * (1 - an) / (1 - at))
    c2 = _sqrt((1 - an) - c1 ** 2)
    return _sqrt(1 - at), _sqrt(at), _sqrt(an), c1, c2


def ddpm_coefs(table, i, j):
    """(r1, r2, k0, kx, d, sigma) of denoising.py:45-65 for the step i -> j as 0-d fp32 tensors (sigma without the t = 0 mask)."""
    at, an = table[i + 1], table[j + 1]
    beta_t = 1 - at / an
    return (_sqrt(1.0 / at), _sqrt(1.0 / at - 1), _sqrt(an) * beta_t, _sqrt(1 - beta_t) * (1 - an), 1.0 - at,
            torch.exp(0.5 * beta_t.log()))


class _Forward:
    """`f(x, i) -> eps` plus close(): the model's own sampling forward, or a plain callable that is handed the timestep the way
    the reference hands it over -- one float per image, all equal to i."""

    def __init__(self, model, shape, n_calls):
        sf = getattr(model, 'sampling_forward', None)
        self.fwd = sf(tuple(shape), n_calls) if sf is not None else None
        self.model = model

    def __call__(self, x, i):
        if self.fwd is not None:
            return self.fwd(x, int(i))
        return self.model(x, torch.full((x.shape[0],), float(i), device=x.device))

    def close(self):
        if self.fwd is not None:
            self.fwd.close()


def _run(kind, x, seq, fwd, table, eta, keep, generator, noise_fn):
    if keep not in ('all', 'last'):
        raise ValueError("keep must be 'all' or 'last'")
    seq = [int(s) for s in seq]
    seq_next = [-1] + seq[:-1]
    shape = tuple(x.shape)
    xs, x0_preds = [x], []
    cur = x
    with torch.no_grad():
        for k, (i, j) in enumerate(zip(reversed(seq), reversed(seq_next))):
            eps = fwd(cur, i)
            if kind == 'generalized':
                mode, coef, noisy = ops.DENOISE_GENERALIZED, generalized_coefs(table, i, j, eta), eta != 0
            else:
                mode, coef, noisy = ops.DENOISE_DDPM, ddpm_coefs(table, i, j), i != 0
            z = None
            if noisy:
                z = noise_fn(k, shape) if noise_fn is not None else torch.randn(shape, device=x.device, generator=generator)
            coef = [float(c) for c in coef]
            if keep == 'all':
                x0 = torch.empty_like(x)
                cur = ops.denoise_step(cur, eps, mode, coef, z=z, x0_out=x0)
                xs.append(cur)
                x0_preds.append(x0)
            else:                                        # the caller's x stays as it is: the first step writes a new buffer
                cur = ops.denoise_step(cur, eps, mode, coef, z=z, out=None if cur is x else cur)
    return (xs, x0_preds) if keep == 'all' else ([cur], [])


def _steps(kind, x, seq, model, betas, eta, keep, generator, noise_fn):
    fwd = _Forward(model, x.shape, len(seq))
    try:
        return _run(kind, x.contiguous(), seq, fwd, alpha_table(betas), eta, keep, generator, noise_fn)
    finally:
        fwd.close()


def generalized_steps(x, seq, model, betas, eta=0.0, keep='all', generator=None, noise_fn=None):
    """denoising.py:10-32.  Returns (xs, x0_preds): xs[0] is the input, then one state per step; x0_preds holds the x0 prediction
    of every step (NOT clipped).  All on x's device.  keep='last': ([final state], []) -- nothing but the current state is held.
    `model`: this package's UNet2DModel (used through sampling_forward, closed in a finally) or any f(x, t) -> eps."""
    return _steps('generalized', x, seq, model, betas, float(eta), keep, generator, noise_fn)


def ddpm_steps(x, seq, model, betas, keep='all', generator=None, noise_fn=None):
    """denoising.py:35-67: x0 clamped to +-1, beta_t = 1 - a_t / a_next of the skipped schedule, variance beta_t, noise masked at
    t = 0.  Same return value as generalized_steps; keep='last' for the 1000-step run that needs no 1000 states."""
    return _steps('ddpm_noisy', x, seq, model, betas, 0.0, keep, generator, noise_fn)


SAMPLE_TYPES = ('generalized', 'ddpm_noisy')


def _write_pngs(u8, paths):
    """u8: host uint8 [N, H, W, C].  One-channel images are written as 8-bit greyscale."""
    from PIL import Image
    for a, p in zip(u8, paths):
        Image.fromarray(a[:, :, 0] if a.shape[2] == 1 else a).save(p)


class Sampler:
    """Runner.sample of runners/diffusion.py for `finetune.py --sample` (--fid / --sequence / --interpolation) and for the two
    image folders compute_ssim.py compares.  image_shape: (C, H, W).  `rescaled` is config.data.rescaled; logit_transform and
    image_mean are not implemented (no shipped config enables them; data.py refuses them too)."""

    def __init__(self, model, betas, image_shape, timesteps=100, sample_type='generalized', skip_type='uniform', eta=0.0,
                 rescaled=True, logit_transform=False, image_mean=False, device=None):
        if logit_transform or image_mean:
            raise NotImplementedError('logit_transform / image_mean are not implemented (no shipped config enables them)')
        if sample_type not in SAMPLE_TYPES:
            raise NotImplementedError('sample_type %r (the reference knows %s)' % (sample_type, ', '.join(SAMPLE_TYPES)))
        self.model, self.betas = model, torch.as_tensor(betas)
        self.num_timesteps = int(self.betas.shape[0])
        self.image_shape = tuple(int(s) for s in image_shape)
        self.sample_type, self.skip_type, self.timesteps, self.eta, self.rescaled = sample_type, skip_type, timesteps, float(eta), rescaled
        self.seq = timestep_sequence(self.num_timesteps, timesteps, skip_type)
        self.table = alpha_table(self.betas)
        self.device = torch.device(device if device is not None else getattr(model, 'device', 'cuda'))

    # ---- the loops ------------------------------------------------------------------------------------------------------------
    def _sample(self, x, fwd, last, generator=None, noise_fn=None):
        res = _run(self.sample_type, x.contiguous(), self.seq, fwd, self.table, self.eta if self.sample_type == 'generalized' else 0.0,
                   'last' if last else 'all', generator, noise_fn)
        return res[0][-1] if last else res

    def sample_image(self, x, last=True, generator=None, noise_fn=None):
        """runners/diffusion.py:492-537: the final state, or with last=False the pair (xs, x0_preds)."""
        fwd = _Forward(self.model, x.shape, len(self.seq))
        try:
            return self._sample(x, fwd, last, generator, noise_fn)
        finally:
            fwd.close()

    def _bytes(self, x):
        return ops.image_to_u8(x, self.rescaled)

    # ---- the jobs -------------------------------------------------------------------------------------------------------------
    def sample_fid(self, image_folder, total_n_samples=50000, batch_size=256, seed=1234, rank=None, world=None, stats=None,
                   inception=None, save=True):
        """runners/diffusion.py:390-427: `(total_n_samples - files already in the folder) // batch_size` rounds of batch_size images
        from a generator seeded seed + rank, x_T drawn on the device, files `{img_id}.png` continuing from the number of files
        already there.  The bytes of every file come from dp_image_to_u8; with `stats` (metrics.FeatureStats) and `inception` the
        FID features accumulate on the device from those same bytes, as metrics.sample_to_dir does.  As in the reference the
        number of rounds does not depend on `world`: ranks that share a folder would overwrite each other, so give each its own.
        save=False writes no file (timing).  Returns the number of images produced."""
        if rank is None or world is None:
            import torch.distributed as dist
            on = dist.is_available() and dist.is_initialized()
            rank, world = (dist.get_rank(), dist.get_world_size()) if on else (0, 1)
        generator = torch.Generator(device=self.device).manual_seed(seed + rank)
        os.makedirs(image_folder, exist_ok=True)
        img_id = len(glob.glob(os.path.join(image_folder, '*')))
        n_rounds = max((total_n_samples - img_id) // batch_size, 0)
        if n_rounds == 0:
            return 0
        shape = (batch_size,) + self.image_shape
        fwd = _Forward(self.model, shape, n_rounds * len(self.seq))          # one pinned / captured forward for the whole job
        try:
            for _ in range(n_rounds):
                x = torch.randn(shape, device=self.device, generator=generator)
                u8 = self._bytes(self._sample(x, fwd, True, generator))
                if save:
                    _write_pngs(u8.cpu().numpy(), [os.path.join(image_folder, '%d.png' % (img_id + i)) for i in range(batch_size)])
                img_id += batch_size
                if stats is not None:
                    from . import data, metrics
                    batch = data.to_device_batch(u8, True, u8.device, data.RAW, 0.0)      # what the FID reader sees: bytes / 255
                    metrics.get_activations([batch], inception, batch_size, stats.dims, stats.s1.device, stats=stats)
        finally:
            fwd.close()
        return n_rounds * batch_size

    def sample_sequence(self, image_folder, generator=None):
        """runners/diffusion.py:429-450: 8 images from one x_T; the files `{j}_{i}.png` hold the x0 PREDICTION of image j at step i
        (not the state).  Returns the number of files."""
        os.makedirs(image_folder, exist_ok=True)
        x = torch.randn((8,) + self.image_shape, device=self.device, generator=generator)
        _, x0_preds = self.sample_image(x, last=False, generator=generator)
        for i, y in enumerate(x0_preds):
            _write_pngs(self._bytes(y).cpu().numpy(), [os.path.join(image_folder, '%d_%d.png' % (j, i)) for j in range(y.shape[0])])
        return len(x0_preds) * 8

    def sample_interpolation(self, image_folder, generator=None):
        """runners/diffusion.py:452-490: the spherical interpolation of two x_T at alpha = 0, 0.1, ..., 1 (11 images), sampled in
        batches of 8, files `{i}.png`.  The slerp is a handful of torch ops on 11 images, once.  Returns the number of files."""
        os.makedirs(image_folder, exist_ok=True)
        z1 = torch.randn((1,) + self.image_shape, device=self.device, generator=generator)
        z2 = torch.randn((1,) + self.image_shape, device=self.device, generator=generator)

        def slerp(alpha):
            theta = torch.acos(torch.sum(z1 * z2) / (torch.norm(z1) * torch.norm(z2)))
            return torch.sin((1 - alpha) * theta) / torch.sin(theta) * z1 + torch.sin(alpha * theta) / torch.sin(theta) * z2
        alpha = torch.arange(0.0, 1.01, 0.1).to(self.device)
        x = torch.cat([slerp(alpha[i]) for i in range(alpha.shape[0])], dim=0)
        xs = [self.sample_image(x[i:i + 8], generator=generator) for i in range(0, x.shape[0], 8)]
        u8 = torch.cat([self._bytes(y) for y in xs], dim=0).cpu().numpy()
        _write_pngs(u8, [os.path.join(image_folder, '%d.png' % i) for i in range(u8.shape[0])])
        return u8.shape[0]
