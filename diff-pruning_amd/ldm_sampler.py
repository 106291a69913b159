"""The samplers of the ldm_exp code base -- the ones the paper's LDM numbers were drawn with.

  ddim_timesteps      ldm/modules/diffusionmodules/util.py:46-60    (make_ddim_timesteps, 'uniform' and 'quad')
  sampling_tables     util.py:63-74 + ddim.py:43-49,188-202         (the five fp32 scalars of every step, on the host)
  DDIMSampler         ldm/models/diffusion/ddim.py                  (guidance or none, any eta, temperature, intermediates)
  PLMSSampler         ldm/models/diffusion/plms.py                  (the same surface; eta must be 0)
  sample_classes      sample_for_FID.py:62-105                      (sample_pruned.py / sample_imagenet.py by its arguments)

Per model evaluation: one forward (`forward_cfg_pair` of this package's ldm.UNetModel under pin_weights + context_cache, or any
`f(x, t, context) -> eps`) and ONE launch of dp_cfg_denoise_step (csrc/ldm_sampler.hip), which reads both halves of the
[2B, C, H, W] eps in place and writes the next state, the x0 prediction and -- for PLMS -- the guided eps in the same pass.

It is NOT ldm_sweep.ddim_sample_cfg under another name.  That helper (eta = 0, guided, uniform, final state only; two launches
through dp_ddim_step, whose coefficients are formed in C) is what the C5 masks are pinned on and stays as it is; nothing here
calls it and it calls nothing here.

Scalars.  The reference reads `table[index]` into `torch.full((b, 1, 1, 1), ...)` and goes on in fp32; sampling_tables restates
that on the host value for value (see its docstring for where fp64 enters and leaves), except that the square roots go through
ddpm_exp_sampler._sqrt, which is correctly rounded on every host while torch's fp32 CPU sqrt is not.

Noise: `noise_fn(step, shape)` when given, else `torch.randn(shape, device=x.device, generator=generator)`; drawn only when
sigma != 0.  The reference draws from the GLOBAL generator at every step, used or not (ddim.py:199 multiplies it by sigma = 0):
draw-order parity with it beyond a given x_T is not claimed.

EMA weights are the caller's business (`with ft.ema_scope():`, checkpoint.load_ldm_finetuned), as elsewhere in this package.
"""
import contextlib
import os

import numpy as np
import torch

from . import ops
from .ddpm_exp_sampler import _sqrt, _write_pngs


def ddim_timesteps(discretize, S, T=1000):
    """make_ddim_timesteps: the timesteps a sampler of S steps visits, ascending, already shifted by the reference's + 1
    ('to get the final alpha values right').  'uniform': every (T // S)-th of 0 .. T - 1 -- more than S entries when S does not
    divide T; 'quad': the truncated squares of S equidistant points on [0, sqrt(0.8 T)].  Anything else raises, as there."""
    if discretize == 'uniform':
        steps = np.asarray(list(range(0, T, T // S)))
    elif discretize == 'quad':
        steps = ((np.linspace(0, np.sqrt(T * .8), S)) ** 2).astype(int)
    else:
        raise NotImplementedError('There is no ddim discretization method called "%s"' % (discretize,))
    return steps + 1


def sampling_tables(alphas_cumprod, steps, eta=0.0):
    """fp32 [len(steps), 5] on the host: (s1m, sqrt_a_t, sqrt_a_prev, c_dir, sigma) of every step, the values the reference's
    torch.full((b, 1, 1, 1), table[index]) and the fp32 ops behind it produce (ddim.py:188-202):
        a        = alphas_cumprod[steps]                         fp32 (ddim_alphas is an fp32 tensor)
        a_prev   = [alphas_cumprod[0]] + a[:-1]                  fp32 values (held in a float64 numpy array there: an exact cast)
        sigma    = fp32(eta * sqrt((reciprocal_fp32(1 - a) * (1 - a_prev)) * (1 - a / a_prev)))    everything else in fp64:
                   `(1 - a_prev) / (1 - a)` is numpy divided by a tensor, which torch answers through Tensor.__rtruediv__ --
                   an fp32 reciprocal times the float64 array; torch.full rounds the float64 result once
        s1m      = sqrt(1 - a)                                   ddim_sqrt_one_minus_alphas
        sqrt_a_t = sqrt(a),  sqrt_a_prev = sqrt(a_prev),  c_dir = sqrt((1 - a_prev) - sigma * sigma)   fp32 throughout
    with every square root correctly rounded (ddpm_exp_sampler._sqrt)."""
    acp = torch.as_tensor(alphas_cumprod).detach().to('cpu', torch.float32)
    idx = torch.as_tensor(np.asarray(steps), dtype=torch.long)
    a = acp[idx]
    a_prev = torch.cat([acp[:1], a[:-1]])
    r = (1 - a).reciprocal()
    sig64 = eta * ((r.double() * (1 - a_prev.double())) * (1 - a.double() / a_prev.double())).sqrt()
    sigma = sig64.float()
    c_dir = _sqrt((1. - a_prev) - sigma ** 2)
    return torch.stack([_sqrt(1. - a), _sqrt(a), _sqrt(a_prev), c_dir, sigma], dim=1)


_UNSUPPORTED = dict(mask=None, x0=None, quantize_x0=False, noise_dropout=0., score_corrector=None, corrector_kwargs=None,
                    ddim_use_original_steps=False, normals_sequence=None)


def _refuse(kw):
    for k, v in kw.items():
        if k not in _UNSUPPORTED:
            raise TypeError('sample() got an unexpected keyword argument %r' % (k,))
        if v is not None and v is not False and v != _UNSUPPORTED[k]:
            raise NotImplementedError('%s is not implemented (inpainting masks, x0 quantisation, noise dropout, the score corrector and '
                                      'the original-step schedule are left out)' % k)


class _Eval:
    """`f(x, t) -> (eps, scale)` plus close().  Guided (an unconditional conditioning and scale != 1, ddim.py:170): eps is
    [2B, ...], unconditional half first, contiguous, and scale the guidance scale; otherwise the model's one output and None.
    This package's ldm.UNetModel runs through forward_cfg_pair inside pin_weights + context_cache; any other callable is handed
    what the reference hands apply_model: cat([x, x]), cat([t, t]), cat([uncond, cond])."""

    def __init__(self, model, cond, uncond, scale):
        self.model = model
        self.guided = uncond is not None and scale != 1.
        self.scale = float(scale) if self.guided else None
        self.ctx = torch.cat([uncond, cond]).contiguous() if self.guided else cond
        self.pair = getattr(model, 'forward_cfg_pair', None) if self.guided else None
        self.stack = contextlib.ExitStack()
        if hasattr(model, 'pin_weights'):
            pinned = self.stack.enter_context(model.pin_weights())
            eng = getattr(pinned, '_engine', None)
            if self.ctx is not None and hasattr(eng, 'context_cache'):
                self.stack.enter_context(eng.context_cache(self.ctx))

    def __call__(self, x, step):
        t = torch.full((x.shape[0],), int(step), device=x.device, dtype=torch.long)
        if self.pair is not None:
            e = self.pair(x, t, self.ctx)
        elif self.guided:
            e = self.model(torch.cat([x, x]), torch.cat([t, t]), self.ctx)
        else:
            e = self.model(x, t, self.ctx)
        return e.contiguous(), self.scale

    def close(self):
        self.stack.close()


class DDIMSampler:
    """ddim.py's DDIMSampler.  `model`: this package's ldm.UNetModel, or any f(x, t, context) -> eps (what the CPU tests use).
    `schedule`: an ldm_sweep.LdmSchedule (default: the cin256-v2 one) or anything with `num_timesteps` and `alphas_cumprod`."""

    def __init__(self, model, schedule=None):
        if schedule is None:
            from .ldm_sweep import LdmSchedule
            schedule = LdmSchedule()
        self.model, self.schedule = model, schedule
        self.ddpm_num_timesteps = int(schedule.num_timesteps)

    def make_schedule(self, ddim_num_steps, ddim_discretize='uniform', ddim_eta=0.):
        self.ddim_timesteps = ddim_timesteps(ddim_discretize, ddim_num_steps, self.ddpm_num_timesteps)
        self.tables = sampling_tables(self.schedule.alphas_cumprod, self.ddim_timesteps, float(ddim_eta))
        self.coefs = [[float(v) for v in row] for row in self.tables]

    def _noise(self, k, sigma, x, generator, noise_fn):
        if sigma == 0.0:
            return None
        z = noise_fn(k, tuple(x.shape)) if noise_fn is not None else torch.randn(tuple(x.shape), device=x.device, generator=generator)
        return z.contiguous()

    def _step(self, fwd, img, i, step, step_next, index, temperature, generator, noise_fn):
        """One p_sample_ddim: (next state, x0 prediction), both new buffers."""
        e, scale = fwd(img, step)
        coef = self.coefs[index]
        x0 = torch.empty_like(img)
        nxt = ops.cfg_denoise_step(img, e, coef, scale=scale, z=self._noise(i, coef[4], img, generator, noise_fn),
                                   temperature=temperature, x0_out=x0)
        return nxt, x0

    def _begin(self):
        pass

    @torch.no_grad()
    def sample(self, S, batch_size, shape, conditioning=None, eta=0., temperature=1., x_T=None, log_every_t=100,
               unconditional_guidance_scale=1., unconditional_conditioning=None, callback=None, img_callback=None, verbose=False,
               generator=None, noise_fn=None, ddim_discretize='uniform', device=None, **unsupported):
        """DDIMSampler.sample (ddim.py:56-162).  Returns (samples, {'x_inter': [...], 'pred_x0': [...]}): both lists start with
        x_T (ddim.py:132) and gain the state / x0 prediction of every step whose index is a multiple of log_every_t, and of the
        first step (ddim.py:158-160).  ddim_discretize is make_schedule's argument, which the reference's sample() leaves at
        'uniform'.  mask / x0, quantize_x0, noise_dropout, score_corrector and ddim_use_original_steps raise NotImplementedError
        when set.  Noise: see the module docstring -- draw-order parity with the reference beyond a given x_T is not claimed."""
        _refuse(unsupported)
        self.make_schedule(S, ddim_discretize, eta)
        size = (batch_size,) + tuple(int(s) for s in shape)
        if x_T is None:
            dev = device if device is not None else (conditioning.device if conditioning is not None else getattr(self.model, 'device', 'cuda'))
            img = torch.randn(size, device=dev, generator=generator)
        else:
            img = x_T.contiguous()
            assert tuple(img.shape) == size and img.dtype == torch.float32
        time_range = np.flip(self.ddim_timesteps)
        total = time_range.shape[0]
        inter = {'x_inter': [img], 'pred_x0': [img]}
        fwd = _Eval(self.model, conditioning, unconditional_conditioning, unconditional_guidance_scale)
        try:
            self._begin()
            for i, step in enumerate(time_range):
                index = total - i - 1
                step_next = time_range[min(i + 1, total - 1)]
                img, pred_x0 = self._step(fwd, img, i, int(step), int(step_next), index, float(temperature), generator, noise_fn)
                if callback:
                    callback(i)
                if img_callback:
                    img_callback(pred_x0, i)
                if index % log_every_t == 0 or index == total - 1:
                    inter['x_inter'].append(img)
                    inter['pred_x0'].append(pred_x0)
        finally:
            fwd.close()
        return img, inter


class PLMSSampler(DDIMSampler):
    """plms.py's PLMSSampler: the DDIM update at eta = 0 with eps replaced by a linear multistep extrapolation over the last three
    GUIDED eps (plms.py:218-232).  The first step has no history and evaluates the model twice (pseudo improved Euler): once at
    (x, t) and once at (the plain DDIM update of x, t_next); it stores the FIRST of the two."""

    def make_schedule(self, ddim_num_steps, ddim_discretize='uniform', ddim_eta=0.):
        if ddim_eta != 0:
            raise ValueError('ddim_eta must be 0 for PLMS')
        super().make_schedule(ddim_num_steps, ddim_discretize, ddim_eta)

    def _begin(self):
        self.old_eps = []                                  # newest first, at most three

    def _step(self, fwd, img, i, step, step_next, index, temperature, generator, noise_fn):
        coef = self.coefs[index]                           # sigma is 0 in every row: no noise is drawn
        e, scale = fwd(img, step)
        x0 = torch.empty_like(img)
        eg = torch.empty_like(img)
        if not self.old_eps:
            x_prev = ops.cfg_denoise_step(img, e, coef, scale=scale, order=ops.CFG_ORDER_PLAIN, eg_out=eg)
            e2, _ = fwd(x_prev, step_next)
            nxt = ops.cfg_denoise_step(img, e2, coef, scale=scale, order=ops.CFG_ORDER_EULER, hist=[eg], out=x_prev, x0_out=x0)
        else:
            nxt = ops.cfg_denoise_step(img, e, coef, scale=scale, order=len(self.old_eps), hist=self.old_eps, x0_out=x0, eg_out=eg)
        self.old_eps = [eg] + self.old_eps[:2]
        return nxt, x0


# ---- the 2 GiB reach of the engine's 32-bit offsets -------------------------------------------------------------------------------
def forward_row_bytes(cfg, shape):
    """Upper bound, in bytes, of the largest buffer ONE row of a no-grad LdmEngine forward at latent `shape` (C, H, W) holds: the
    activations of every block at its widest (a decoder ResBlock reads its input and the skip tensor concatenated), the GEGLU
    projection of a transformer block (8 x its width) and, where the one-kernel attention does not take the shape, the
    [heads, T, T] scores of the self-attention."""
    from .ldm import ldm_blocks, st_heads
    inp, out, mid = ldm_blocks(cfg)
    H, W = int(shape[1]), int(shape[2])
    worst = max(int(shape[0]), cfg['out_channels']) * H * W

    def st(ch, hw):
        heads, d = st_heads(cfg, ch)
        fused = getattr(ops, 'FUSED_ATTN', False) and ops.attention_fused_ok(hw, d, d)
        return max(8 * ch * hw, 0 if fused else heads * hw * hw)
    h, w = H, W
    for items in inp:
        for it in items:
            if it[0] == 'down':
                h, w = (h + 1) // 2, (w + 1) // 2
                worst = max(worst, it[1] * h * w)
            elif it[0] == 'st':
                worst = max(worst, st(it[1], h * w))
            else:
                worst = max(worst, max(it[1], it[2]) * h * w)
    worst = max(worst, mid * h * w, st(mid, h * w))
    for items in out:
        for it in items:
            if it[0] == 'up':
                h, w = 2 * h, 2 * w
                worst = max(worst, it[1] * h * w)
            elif it[0] == 'st':
                worst = max(worst, st(it[1], h * w))
            else:
                worst = max(worst, max(it[1], it[2]) * h * w)
    return 4 * worst


def max_class_batch(model, shape):
    """The largest class batch whose guided forward (2 x batch rows) keeps every engine buffer below 2 GiB; None for a model
    that is not this package's UNet (a plain callable has no such reach)."""
    cfg = getattr(model, 'config', None)
    if cfg is None or not hasattr(model, 'forward_cfg_pair'):
        return None
    return max(1, (ops._MAX_BYTES - 1) // forward_row_bytes(cfg, shape) // 2)


def sample_classes(sampler, embedder, first_stage, out_dir, classes=range(1000), ipc=50, batch_size=50, ddim_steps=250, scale=3.0,
                   eta=0.0, seed=0, rank=None, world=None, stats=None, inception=None, save=True, latent_shape=(3, 64, 64),
                   uncond_class=1000, scale_factor=1.0):
    """The loop of sample_for_FID.py:62-105: ipc // batch_size rounds over `classes`; per (round, class) one guided sample of
    [batch_size, *latent_shape] against the unconditional context embedder([1000] * batch_size), ldm_sweep.decode_first_stage,
    bytes through ops.image_to_u8(rescaled=True) -- clamp((x + 1) / 2, 0, 1), then save_image's byte conversion -- and the files
    `{class}_{img_id}.png`, img_id = (round * len(classes) + class_position) * batch_size + i: the reference's running counter in
    closed form.  classes / ddim_steps / scale and save=False give sample_pruned.py and sample_imagenet.py without their grid.
    x_T of a (round, class) comes from a device generator seeded seed + round * len(classes) + class_position (and so does the
    noise of eta != 0), so the images do not depend on `world`; classes are dealt to ranks by position (position % world == rank).
    With `stats` (metrics.FeatureStats) and `inception` the FID features accumulate on the device from those same bytes, as
    ddpm_exp_sampler.Sampler.sample_fid does.  A class batch whose 2 * batch_size forward rows would pass the 2 GiB reach of the
    engine's 32-bit offsets is sampled in slices (max_class_batch), as vq.py does for its own; at eta = 0 the files are the same.
    EMA weights are the caller's business.  Returns the number of images this rank produced."""
    from . import ldm_sweep
    if rank is None or world is None:
        import torch.distributed as dist
        on = dist.is_available() and dist.is_initialized()
        rank, world = (dist.get_rank(), dist.get_world_size()) if on else (0, 1)
    classes = [int(c) for c in classes]
    dev = embedder.embedding.weight.device if hasattr(embedder, 'embedding') else torch.device(getattr(sampler.model, 'device', 'cuda'))
    if save:
        os.makedirs(out_dir, exist_ok=True)
    uc_all = embedder(torch.tensor(batch_size * [uncond_class], device=dev))
    limit = max_class_batch(sampler.model, latent_shape) or batch_size
    made = 0
    for rnd in range(ipc // batch_size):
        for pos, label in enumerate(classes):
            if pos % world != rank:
                continue
            k = rnd * len(classes) + pos
            generator = torch.Generator(device=dev).manual_seed(seed + k)
            x_T = torch.randn((batch_size,) + tuple(latent_shape), device=dev, generator=generator)
            c_all = embedder(torch.tensor(batch_size * [label], device=dev))
            parts = []
            for lo in range(0, batch_size, limit):
                hi = min(lo + limit, batch_size)
                z, _ = sampler.sample(S=ddim_steps, conditioning=c_all[lo:hi].contiguous(), batch_size=hi - lo, shape=latent_shape,
                                      unconditional_guidance_scale=scale, unconditional_conditioning=uc_all[lo:hi].contiguous(),
                                      eta=eta, x_T=x_T[lo:hi], generator=generator)
                parts.append(z)
            z = parts[0] if len(parts) == 1 else torch.cat(parts)
            u8 = ops.image_to_u8(ldm_sweep.decode_first_stage(first_stage, z, scale_factor))
            if save:
                _write_pngs(u8.cpu().numpy(), [os.path.join(out_dir, '%d_%d.png' % (label, k * batch_size + i)) for i in range(batch_size)])
            if stats is not None:
                from . import data, metrics
                batch = data.to_device_batch(u8, True, u8.device, data.RAW, 0.0)          # what the FID reader sees: bytes / 255
                metrics.get_activations([batch], inception, batch_size, stats.dims, stats.s1.device, stats=stats)
            made += batch_size
    return made
