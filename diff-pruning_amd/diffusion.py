"""DDPM / DDIM schedulers and pipelines with the Diffusers call surface used by the reference scripts.

  DDPMScheduler.add_noise      scheduling_ddpm.py:408-429   (HIP kernel dp_add_noise on device tensors)
  DDIMScheduler.set_timesteps  scheduling_ddim.py:239-268   (reference-modified: skip_type uniform|quad)
  DDIMScheduler.step           scheduling_ddim.py:270-390   (HIP kernel dp_ddim_step)
  DDIMPipeline.__call__        pipelines/ddim/pipeline_ddim.py:44-122
  DDPMScheduler.set_timesteps  scheduling_ddpm.py:185-236
  DDPMScheduler.step           scheduling_ddpm.py:312-406   (HIP kernel dp_ddpm_step; epsilon prediction)
  DDPMPipeline.__call__        pipelines/ddpm/pipeline_ddpm.py:24-105 (ancestral sampling loop)
  PNDMScheduler.step           scheduling_pndm.py:192-399   (HIP kernel dp_pndm_step)
  PNDMPipeline.__call__        pipelines/pndm/pipeline_pndm.py:47-99
  RePaintScheduler.step        scheduling_repaint.py:216-301 (HIP kernel dp_repaint_step), undo_step :303-318 (dp_repaint_undo)
  RePaintPipeline.__call__     pipelines/repaint/pipeline_repaint.py:82-171
  EulerDiscreteScheduler, EulerAncestralDiscreteScheduler, HeunDiscreteScheduler
                               scheduling_euler_discrete.py, scheduling_euler_ancestral_discrete.py, scheduling_heun_discrete.py
                               (HIP kernels dp_sigma_step, dp_sigma_scale, dp_sigma_add_noise; float64 timesteps, sample at scale sigma)
  LMSDiscreteScheduler, KDPM2DiscreteScheduler, KDPM2AncestralDiscreteScheduler
                               scheduling_lms_discrete.py, scheduling_k_dpm_2_discrete.py, scheduling_k_dpm_2_ancestral_discrete.py
                               (HIP kernels dp_lms_step, dp_kdpm2_step; the multistep coefficients by the reference's quadrature)
  randn_tensor                 utils/torch_utils.py:36-77   (CPU-generator semantics kept for seed parity)
Host-side table arithmetic (1000-entry alpha-bar table) is fp32 torch on the CPU, exactly as in the reference.
"""
from dataclasses import dataclass
from types import SimpleNamespace

import numpy as np
import torch

from . import ops


def randn_tensor(shape, generator=None, device=None, dtype=None):
    device = torch.device(device) if device is not None else torch.device('cpu')
    rand_device = device
    if generator is not None:
        gdev = generator.device.type if not isinstance(generator, list) else generator[0].device.type
        if gdev != device.type and gdev == 'cpu':
            rand_device = 'cpu'
        elif gdev != device.type and gdev == 'cuda':
            raise ValueError('Cannot generate a %s tensor from a generator of type %s.' % (device, gdev))
    if isinstance(generator, list):
        shape1 = (1,) + tuple(shape[1:])
        lat = [torch.randn(shape1, generator=generator[i], device=rand_device, dtype=dtype) for i in range(shape[0])]
        return torch.cat(lat, dim=0).to(device)
    return torch.randn(tuple(shape), generator=generator, device=rand_device, dtype=dtype).to(device)


def _betas(num_train_timesteps, beta_start, beta_end, beta_schedule):
    if beta_schedule == 'linear':
        return torch.linspace(beta_start, beta_end, num_train_timesteps, dtype=torch.float32)
    if beta_schedule == 'scaled_linear':
        return torch.linspace(beta_start ** 0.5, beta_end ** 0.5, num_train_timesteps, dtype=torch.float32) ** 2
    raise NotImplementedError('%s is not implemented' % beta_schedule)


class _SchedulerBase:
    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, subfolder=None, **kwargs):
        from . import checkpoint
        return checkpoint.load_scheduler(cls, pretrained_model_name_or_path, subfolder)

    def save_pretrained(self, save_directory):
        from . import checkpoint
        checkpoint.save_scheduler(self, save_directory)

    @classmethod
    def from_config(cls, config):
        d = vars(config) if not isinstance(config, dict) else config
        return cls(**{k: d[k] for k in cls._CONFIG_KEYS if k in d})

    def scale_model_input(self, sample, *args, **kwargs):
        return sample

    def host_timesteps(self):
        """The current timestep table as a host list, in the form `step` takes them: the list a scheduler keeps beside its
        `timesteps` tensor where it keeps one (ints for the multistep solvers and PNDM, floats -- mostly fractional -- for the
        sigma-space schedulers), else one read-back of `timesteps` as ints.  What a sampling loop walks instead of the tensor."""
        ts = getattr(self, '_ts', None)
        return list(ts) if ts is not None else [int(t) for t in self.timesteps.tolist()]

    def _init_tables(self, num_train_timesteps, beta_start, beta_end, beta_schedule, betas=None):
        self.betas = _betas(num_train_timesteps, beta_start, beta_end, beta_schedule) if betas is None else betas
        self.alphas = 1.0 - self.betas
        self.alphas_cumprod = torch.cumprod(self.alphas, dim=0)
        self.init_noise_sigma = 1.0
        self._acp_dev = {}

    def _acp_on(self, device):
        t = self._acp_dev.get(device)
        if t is None:
            t = self.alphas_cumprod.to(device)
            self._acp_dev[device] = t
        return t

    _PREDICTION_TYPES = ('epsilon', 'sample', 'v_prediction')

    def _x0_treatment(self):
        """(treat, host scalars) of step 3 / 4 of the reference's `step`: thresholding wins over clip_sample."""
        cfg = self.config
        if cfg.thresholding:
            return ops.X0_TREAT_THRESHOLD, dict(ratio=cfg.dynamic_thresholding_ratio, max_value=cfg.sample_max_value)
        if cfg.clip_sample:
            return ops.X0_TREAT_CLIP, dict(range=cfg.clip_sample_range)
        return ops.X0_TREAT_NONE, {}

    def _threshold_sample(self, sample):
        """scheduling_ddpm.py:278-310 for a caller's own [B, C, H, W] tensor (ops.dynamic_threshold)."""
        return ops.dynamic_threshold(sample.contiguous(), self.config.dynamic_thresholding_ratio, self.config.sample_max_value)

    def add_noise(self, original_samples, noise, timesteps):
        if original_samples.device.type != 'cuda':
            raise RuntimeError('add_noise runs on the HIP kernels: tensors must live on a cuda device')
        acp = self._acp_on(original_samples.device)
        return ops.add_noise(original_samples.contiguous(), noise.contiguous(), acp,
                             timesteps.to(device=original_samples.device, dtype=torch.long).contiguous())


@dataclass
class DDPMSchedulerOutput:
    prev_sample: torch.Tensor
    pred_original_sample: torch.Tensor = None


class DDPMScheduler(_SchedulerBase):
    """scheduling_ddpm.py:92-467 for epsilon, `sample` and `v_prediction` models, with clip_sample or dynamic thresholding
    (`thresholding`, `dynamic_thresholding_ratio`, `sample_max_value`: per image s = clamp(quantile(|x0|, ratio), min=1,
    max=sample_max_value), x0 = clamp(x0, -s, s) / s).  With the default sample_max_value = 1.0 the reference's clamp makes
    s == 1 for every image: thresholding is then a clip to [-1, 1], and the option only acts with sample_max_value > 1.
    Not carried (NotImplementedError): `trained_betas`, models that predict a variance, the learned variance types."""
    _CONFIG_KEYS = ('num_train_timesteps', 'beta_start', 'beta_end', 'beta_schedule', 'variance_type', 'clip_sample',
                    'prediction_type', 'clip_sample_range', 'thresholding', 'dynamic_thresholding_ratio', 'sample_max_value')

    def __init__(self, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule='linear',
                 variance_type='fixed_small', clip_sample=True, prediction_type='epsilon', clip_sample_range=1.0,
                 thresholding=False, dynamic_thresholding_ratio=0.995, sample_max_value=1.0):
        self.config = SimpleNamespace(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                                      beta_schedule=beta_schedule, variance_type=variance_type, clip_sample=clip_sample,
                                      prediction_type=prediction_type, clip_sample_range=clip_sample_range,
                                      thresholding=thresholding, dynamic_thresholding_ratio=dynamic_thresholding_ratio,
                                      sample_max_value=sample_max_value)
        self._init_tables(num_train_timesteps, beta_start, beta_end, beta_schedule)
        self.one = torch.tensor(1.0)
        self.variance_type = variance_type
        self.custom_timesteps = False
        self.num_inference_steps = None
        self.timesteps = torch.from_numpy(np.arange(0, num_train_timesteps)[::-1].copy())

    def set_timesteps(self, num_inference_steps=None, device=None, timesteps=None):
        """scheduling_ddpm.py:185-236."""
        T = self.config.num_train_timesteps
        if num_inference_steps is not None and timesteps is not None:
            raise ValueError('Can only pass one of `num_inference_steps` or `custom_timesteps`.')
        if timesteps is not None:
            for i in range(1, len(timesteps)):
                if timesteps[i] >= timesteps[i - 1]:
                    raise ValueError('`custom_timesteps` must be in descending order.')
            if timesteps[0] >= T:
                raise ValueError('`timesteps` must start before `self.config.train_timesteps`: %d.' % T)
            ts = np.array(timesteps, dtype=np.int64)
            self.custom_timesteps = True
        else:
            if num_inference_steps > T:
                raise ValueError('`num_inference_steps`: %d cannot be larger than `self.config.train_timesteps`: %d'
                                 % (num_inference_steps, T))
            self.num_inference_steps = num_inference_steps
            ts = (np.arange(0, num_inference_steps) * (T // num_inference_steps)).round()[::-1].copy().astype(np.int64)
            self.custom_timesteps = False
        self.timesteps = torch.from_numpy(ts).to(device)

    def previous_timestep(self, timestep):
        """scheduling_ddpm.py:454-467."""
        if self.custom_timesteps:
            index = (self.timesteps == timestep).nonzero(as_tuple=True)[0][0]
            return torch.tensor(-1) if index == self.timesteps.shape[0] - 1 else self.timesteps[index + 1]
        n = self.num_inference_steps if self.num_inference_steps else self.config.num_train_timesteps
        return timestep - self.config.num_train_timesteps // n

    def _get_variance(self, t, predicted_variance=None, variance_type=None):
        """scheduling_ddpm.py:238-280 (0-d fp32 tensor arithmetic on the host, as in the reference)."""
        prev_t = self.previous_timestep(t)
        a_t = self.alphas_cumprod[t]
        a_prev = self.alphas_cumprod[prev_t] if prev_t >= 0 else self.one
        cur_b = 1 - a_t / a_prev
        variance = torch.clamp((1 - a_prev) / (1 - a_t) * cur_b, min=1e-20)
        vt = variance_type if variance_type is not None else self.config.variance_type
        if vt == 'fixed_small':
            return variance
        if vt == 'fixed_small_log':
            return torch.exp(0.5 * torch.log(variance))
        if vt == 'fixed_large':
            return cur_b
        if vt == 'fixed_large_log':
            return torch.log(cur_b)
        raise NotImplementedError('variance_type %s needs a model that predicts the variance' % vt)

    def step(self, model_output, timestep, sample, generator=None, return_dict=True, variance_noise=None):
        """scheduling_ddpm.py:312-406.  The coefficients are 0-d fp32 tensors computed on the host in the reference's operation
        order.  An epsilon model without thresholding runs in one HIP kernel (dp_ddpm_step), as it always has; a `sample` or
        `v_prediction` model, or dynamic thresholding, goes through ops.x0_step (csrc/threshold.hip: one launch where an image's
        row fits in LDS) and returns the treated x0 as `pred_original_sample`.
        `variance_noise` (extension): caller-supplied noise instead of a draw from `generator` (parity tests)."""
        pt = self.config.prediction_type
        if pt not in self._PREDICTION_TYPES:
            raise ValueError('prediction_type given as %s must be one of `epsilon`, `sample` or `v_prediction`  for the DDPMScheduler.' % pt)
        if model_output.shape[1] != sample.shape[1]:
            raise NotImplementedError('learned-variance models are not part of this path')
        t = int(timestep)
        prev_t = int(self.previous_timestep(t))
        a_t = self.alphas_cumprod[t]
        a_prev = self.alphas_cumprod[prev_t] if prev_t >= 0 else self.one
        b_t = 1 - a_t
        b_prev = 1 - a_prev
        cur_a = a_t / a_prev
        cur_b = 1 - cur_a
        c_x0 = (a_prev ** 0.5 * cur_b) / b_t
        c_xt = cur_a ** 0.5 * b_prev / b_t
        sigma, noise = 0.0, None
        if t > 0:
            noise = variance_noise if variance_noise is not None else randn_tensor(
                model_output.shape, generator=generator, device=model_output.device, dtype=model_output.dtype)
            if self.variance_type == 'fixed_small_log':
                sigma = float(self._get_variance(t))
            elif self.variance_type in ('fixed_small', 'fixed_large'):
                sigma = float(self._get_variance(t) ** 0.5)
            else:
                raise NotImplementedError('variance_type %s' % self.variance_type)
        if pt != 'epsilon' or self.config.thresholding:
            treat, c = self._x0_treatment()
            c.update(sa=float(a_t ** 0.5), sb=float(b_t ** 0.5), c0=float(c_x0), c1=float(c_xt), cz=sigma)
            x0 = torch.empty_like(sample, memory_format=torch.contiguous_format)
            prev, x0, _ = ops.x0_step(sample.contiguous(), model_output.contiguous(), ops.X0_MODE_DDPM, ops.X0_PRED[pt], treat, c,
                                      z=None if noise is None else noise.contiguous(), x0_out=x0)
            if not return_dict:
                return (prev,)
            return DDPMSchedulerOutput(prev_sample=prev, pred_original_sample=x0)
        prev = ops.ddpm_step(sample.contiguous(), model_output.contiguous(), float(a_t ** 0.5), float(b_t ** 0.5),
                             float(c_x0), float(c_xt), sigma, None if noise is None else noise.contiguous(),
                             clip=self.config.clip_sample, clip_range=self.config.clip_sample_range)
        if not return_dict:
            return (prev,)
        return DDPMSchedulerOutput(prev_sample=prev)


@dataclass
class DDIMSchedulerOutput:
    prev_sample: torch.Tensor
    pred_original_sample: torch.Tensor = None


class DDIMScheduler(_SchedulerBase):
    """scheduling_ddim.py:78-440 (reference-modified: skip_type) for epsilon, `sample` and `v_prediction` models, with
    clip_sample or dynamic thresholding (`thresholding`, `dynamic_thresholding_ratio`, `sample_max_value`: per image
    s = clamp(quantile(|x0|, ratio), min=1, max=sample_max_value), x0 = clamp(x0, -s, s) / s) and `use_clipped_model_output`.
    With the default sample_max_value = 1.0 the reference's clamp makes s == 1 for every image: thresholding is then a clip to
    [-1, 1], and the option only acts with sample_max_value > 1.  Not carried (NotImplementedError): `trained_betas`."""
    _CONFIG_KEYS = ('num_train_timesteps', 'beta_start', 'beta_end', 'beta_schedule', 'clip_sample', 'set_alpha_to_one',
                    'steps_offset', 'prediction_type', 'skip_type', 'clip_sample_range', 'thresholding',
                    'dynamic_thresholding_ratio', 'sample_max_value')

    def __init__(self, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule='linear',
                 skip_type='uniform', clip_sample=True, set_alpha_to_one=True, steps_offset=0, prediction_type='epsilon',
                 clip_sample_range=1.0, thresholding=False, dynamic_thresholding_ratio=0.995, sample_max_value=1.0):
        if prediction_type not in self._PREDICTION_TYPES:
            raise ValueError('prediction_type given as %s must be one of `epsilon`, `sample`, or `v_prediction`' % prediction_type)
        self.config = SimpleNamespace(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                                      beta_schedule=beta_schedule, clip_sample=clip_sample,
                                      set_alpha_to_one=set_alpha_to_one, steps_offset=steps_offset,
                                      prediction_type=prediction_type, clip_sample_range=clip_sample_range,
                                      thresholding=thresholding, dynamic_thresholding_ratio=dynamic_thresholding_ratio,
                                      sample_max_value=sample_max_value)
        self.config.skip_type = skip_type            # the reference registers skip_type in the config (scheduling_ddim.py:122)
        self._init_tables(num_train_timesteps, beta_start, beta_end, beta_schedule)
        self.skip_type = skip_type
        self.final_alpha_cumprod = torch.tensor(1.0) if set_alpha_to_one else self.alphas_cumprod[0]
        self.num_inference_steps = None
        self.timesteps = torch.from_numpy(np.arange(0, num_train_timesteps)[::-1].copy().astype(np.int64))

    def set_timesteps(self, num_inference_steps, device=None):
        T = self.config.num_train_timesteps
        if num_inference_steps > T:
            raise ValueError('`num_inference_steps`: %d cannot be larger than `self.config.train_timesteps`: %d'
                             % (num_inference_steps, T))
        self.num_inference_steps = num_inference_steps
        n = num_inference_steps
        if self.skip_type == 'uniform':
            ratio = (T - 1) / (n - 1)
            ts = (np.arange(0, n) * ratio).round()[::-1].copy().astype(np.int64)
        elif self.skip_type == 'quad':
            ratio = (T - 1) / (n - 1) ** 2
            ts = (np.arange(0, n) ** 2 * ratio).round()[::-1].copy().astype(np.int64)
        else:
            raise NotImplementedError('skip_type %s is not implemented' % self.skip_type)
        self.timesteps = torch.from_numpy(ts).to(device)
        self.timesteps += self.config.steps_offset

    def _get_variance(self, timestep, prev_timestep):
        a_t = self.alphas_cumprod[timestep]
        a_prev = self.alphas_cumprod[prev_timestep] if prev_timestep >= 0 else self.final_alpha_cumprod
        return ((1 - a_prev) / (1 - a_t)) * (1 - a_t / a_prev)

    def step(self, model_output, timestep, sample, eta=0.0, use_clipped_model_output=False, generator=None,
             variance_noise=None, return_dict=True):
        """scheduling_ddim.py:270-390.  An epsilon model without thresholding and without `use_clipped_model_output` runs in one HIP
        kernel (dp_ddim_step), as it always has; every other step goes through ops.x0_step (csrc/threshold.hip: one launch where
        an image's row fits in LDS), with the host scalars as 0-d fp32 tensor arithmetic in the reference's order, and returns
        the treated x0 as `pred_original_sample`."""
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
        t = int(timestep)
        prev_t = t - self.config.num_train_timesteps // self.num_inference_steps      # reference quirk kept
        a_t = self.alphas_cumprod[t]
        a_prev = self.alphas_cumprod[prev_t] if prev_t >= 0 else self.final_alpha_cumprod
        std = 0.0
        if eta > 0:
            std = float(eta * self._get_variance(t, prev_t) ** 0.5)
            if variance_noise is None:
                variance_noise = randn_tensor(model_output.shape, generator=generator, device=model_output.device,
                                              dtype=model_output.dtype)
        pt = self.config.prediction_type
        if pt != 'epsilon' or self.config.thresholding or use_clipped_model_output:
            treat, c = self._x0_treatment()
            std_dev_t = eta * self._get_variance(t, prev_t) ** 0.5
            c.update(sa=float(a_t ** 0.5), sb=float((1 - a_t) ** 0.5), c0=float(a_prev ** 0.5),
                     c1=float((1 - a_prev - std_dev_t ** 2) ** 0.5), cz=std)
            x0 = torch.empty_like(sample, memory_format=torch.contiguous_format)
            prev, x0, _ = ops.x0_step(sample.contiguous(), model_output.contiguous(), ops.X0_MODE_DDIM, ops.X0_PRED[pt], treat, c,
                                      z=variance_noise.contiguous() if eta > 0 else None, x0_out=x0,
                                      reclip=bool(use_clipped_model_output))
            if not return_dict:
                return (prev,)
            return DDIMSchedulerOutput(prev_sample=prev, pred_original_sample=x0)
        prev = ops.ddim_step(sample.contiguous(), model_output.contiguous(), float(a_t), float(a_prev), std,
                             variance_noise if eta > 0 else None, clip=self.config.clip_sample,
                             clip_range=self.config.clip_sample_range)
        if not return_dict:
            return (prev,)
        return DDIMSchedulerOutput(prev_sample=prev)


@dataclass
class SchedulerOutput:
    prev_sample: torch.Tensor


def _betas_for_alpha_bar(num_diffusion_timesteps, max_beta=0.999):
    """The `squaredcos_cap_v2` table (scheduling_dpmsolver_multistep.py:29-55): Python doubles, one cast to fp32 at the end."""
    import math

    def alpha_bar(s):
        return math.cos((s + 0.008) / 1.008 * math.pi / 2) ** 2
    n = num_diffusion_timesteps
    return torch.tensor([min(1 - alpha_bar((i + 1) / n) / alpha_bar(i / n), max_beta) for i in range(n)], dtype=torch.float32)


def _rounded_once(fn, t):
    """fn(t) of an fp32 CPU tensor as the correctly rounded fp32 value: evaluated in fp64, rounded to fp32 once.  torch's fp32
    sqrt / log / exp on the CPU come from the host's vector math library: they are within an ulp, not correctly rounded, and two
    hosts with the same torch build return different last bits (measured: two x86 hosts of different vendors disagree on 5 of the 1000
    alpha_t entries).  The solver differences lambda values that are close together, so one such bit moves a third-order update by
    ten times its fp32 rounding error.  Rounded once from fp64, the tables and the per-step scalars are the same on every host."""
    return fn(t.double()).float()


class _MultistepBase(_SchedulerBase):
    """What the multistep solvers share, and where a new one starts: the alpha_t / sigma_t / lambda_t tables, the timesteps as a
    host list beside the `timesteps` tensor (so that `step` reads nothing back from the device), and the history: a ring of
    `solver_order` device buffers, newest last, that the steps write in turn."""
    order = 1

    def __len__(self):
        return self.config.num_train_timesteps

    def _init_solver_tables(self, num_train_timesteps, beta_start, beta_end, beta_schedule):
        """scheduling_dpmsolver_multistep.py:158-176, scheduling_unipc_multistep.py:144-167, sqrt and log correctly rounded
        (_rounded_once)."""
        self._init_tables(num_train_timesteps, beta_start, beta_end, beta_schedule,
                          _betas_for_alpha_bar(num_train_timesteps) if beta_schedule == 'squaredcos_cap_v2' else None)
        self.alpha_t = _rounded_once(torch.sqrt, self.alphas_cumprod)
        self.sigma_t = _rounded_once(torch.sqrt, 1 - self.alphas_cumprod)
        self.lambda_t = _rounded_once(torch.log, self.alpha_t) - _rounded_once(torch.log, self.sigma_t)

    def _reset_history(self):
        """Hook of _set_list: what a solver keeps between steps beside model_outputs and lower_order_nums."""

    def _set_list(self, ts, device=None):
        self.timesteps = torch.from_numpy(ts).to(device)
        self._ts = [int(v) for v in ts]                               # the host's copy: what `step` looks timesteps up in
        self._index = {}
        for i, v in enumerate(self._ts):
            self._index.setdefault(v, i)
        self.model_outputs = [None] * self.config.solver_order        # newest last, as the reference keeps them
        self.lower_order_nums = 0
        self._reset_history()

    def _rounded_linspace(self, top, num_inference_steps):
        return np.linspace(0, top, num_inference_steps + 1).round()[::-1][:-1].copy().astype(np.int64)

    def _set_unique(self, ts, device):
        """Duplicates removed in order of appearance, the history reset."""
        _, unique_indices = np.unique(ts, return_index=True)
        ts = ts[np.sort(unique_indices)]
        self._set_list(ts, device)
        self.num_inference_steps = len(ts)

    def _begin_step(self, timestep):
        """(ts, last, t, i, prev_t): the host's timestep list and its last index, this step's timestep, its index (the last one for
        a timestep that is not in the list) and the timestep after it (0 after the last)."""
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
        ts = self._ts
        last = len(ts) - 1
        t = int(timestep)
        i = self._index.get(t, last)
        return ts, last, t, i, 0 if i == last else ts[i + 1]

    def _oldest_buffer(self, sample):
        """The oldest buffer of the ring, which takes this step's converted output; a new one where it does not fit `sample`."""
        buf = self.model_outputs[0]
        if buf is None or buf.shape != sample.shape or buf.device != sample.device:
            buf = torch.empty_like(sample)
        return buf

    def _push_output(self, m):
        self.model_outputs = self.model_outputs[1:] + [m]
        if self.lower_order_nums < self.config.solver_order:
            self.lower_order_nums += 1


class DPMSolverMultistepScheduler(_MultistepBase):
    """scheduling_dpmsolver_multistep.py:58-707, the deterministic multistep DPM-Solver / DPM-Solver++ of orders 1 .. 3 for epsilon
    models.  The tables and every per-step scalar are 0-d fp32 torch arithmetic on the CPU in the reference's operation order
    (:420-423, :466-473, :557-572), with sqrt, log and exp correctly rounded (_rounded_once: the reference's bits on a host whose
    math library rounds them correctly, and the same bits on every host); the per-element work of a step -- convert_model_output
    and the update -- is ONE launch of dp_dpm_solver_step (ops.dpm_solver_step).  The timesteps are kept as a host list beside the `timesteps` tensor, so `step`
    reads nothing back from the device.  The history is a ring of `solver_order` device buffers that the steps write in turn.
    Not carried (NotImplementedError): the SDE variants, dynamic thresholding, `sample` / `v_prediction` models, models that
    predict a variance, `trained_betas`."""
    _CONFIG_KEYS = ('num_train_timesteps', 'beta_start', 'beta_end', 'beta_schedule', 'trained_betas', 'solver_order',
                    'prediction_type', 'thresholding', 'dynamic_thresholding_ratio', 'sample_max_value', 'algorithm_type',
                    'solver_type', 'lower_order_final', 'use_karras_sigmas', 'lambda_min_clipped', 'variance_type')

    def __init__(self, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule='linear', trained_betas=None,
                 solver_order=2, prediction_type='epsilon', thresholding=False, dynamic_thresholding_ratio=0.995,
                 sample_max_value=1.0, algorithm_type='dpmsolver++', solver_type='midpoint', lower_order_final=True,
                 use_karras_sigmas=False, lambda_min_clipped=-float('inf'), variance_type=None):
        if trained_betas is not None:
            raise NotImplementedError('trained_betas is not on the hot path')
        if prediction_type != 'epsilon':
            raise NotImplementedError('only epsilon prediction is on the hot path')
        if thresholding:
            raise NotImplementedError('dynamic thresholding is not on the hot path')
        if variance_type in ('learned', 'learned_range'):
            raise NotImplementedError('learned-variance models are not part of this path')
        if algorithm_type == 'deis':                                  # :188-198: the two rewrites of register_to_config
            algorithm_type = 'dpmsolver++'
        if algorithm_type not in ('dpmsolver', 'dpmsolver++'):
            raise NotImplementedError('algorithm_type %s is not implemented (the SDE variants are left out)' % algorithm_type)
        if solver_type in ('logrho', 'bh1', 'bh2'):
            solver_type = 'midpoint'
        if solver_type not in ('midpoint', 'heun'):
            raise NotImplementedError('solver_type %s is not implemented' % solver_type)
        if int(solver_order) < 1:
            raise ValueError('solver_order must be at least 1')
        self.config = SimpleNamespace(
            num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end, beta_schedule=beta_schedule,
            trained_betas=trained_betas, solver_order=solver_order, prediction_type=prediction_type, thresholding=thresholding,
            dynamic_thresholding_ratio=dynamic_thresholding_ratio, sample_max_value=sample_max_value,
            algorithm_type=algorithm_type, solver_type=solver_type, lower_order_final=lower_order_final,
            use_karras_sigmas=use_karras_sigmas, lambda_min_clipped=lambda_min_clipped, variance_type=variance_type)
        self._init_solver_tables(num_train_timesteps, beta_start, beta_end, beta_schedule)
        self.num_inference_steps = None
        self._set_list(np.linspace(0, num_train_timesteps - 1, num_train_timesteps, dtype=np.float32)[::-1].copy())
        self.use_karras_sigmas = use_karras_sigmas

    def _sigma_to_t(self, sigma, log_sigmas):
        """:285-306 for one sigma: the fractional index at which log sigma lies between two neighbours of the table."""
        log_sigma = np.log(sigma)
        dists = log_sigma - log_sigmas[:, np.newaxis]
        low_idx = np.cumsum((dists >= 0), axis=0).argmax(axis=0).clip(max=log_sigmas.shape[0] - 2)
        high_idx = low_idx + 1
        low, high = log_sigmas[low_idx], log_sigmas[high_idx]
        w = np.clip((low - log_sigma) / (low - high), 0, 1)
        t = (1 - w) * low_idx + w * high_idx
        return t.reshape(sigma.shape)

    def _convert_to_karras(self, in_sigmas, num_inference_steps):
        """:309-320, Karras et al. (2022) with rho = 7."""
        sigma_min, sigma_max = in_sigmas[-1].item(), in_sigmas[0].item()
        rho = 7.0
        ramp = np.linspace(0, 1, num_inference_steps)
        min_inv_rho, max_inv_rho = sigma_min ** (1 / rho), sigma_max ** (1 / rho)
        return (max_inv_rho + ramp * (min_inv_rho - max_inv_rho)) ** rho

    def set_timesteps(self, num_inference_steps=None, device=None):
        """:208-247: the lambda_min_clipped search, the rounded linspace (or the Karras sigmas mapped back to timesteps), duplicates
        removed in order of appearance, the history reset."""
        clipped_idx = int(torch.searchsorted(torch.flip(self.lambda_t, [0]), self.config.lambda_min_clipped))
        ts = self._rounded_linspace(self.config.num_train_timesteps - 1 - clipped_idx, num_inference_steps)
        if self.use_karras_sigmas:
            sigmas = (((1 - self.alphas_cumprod) / self.alphas_cumprod) ** 0.5).numpy()
            log_sigmas = np.log(sigmas)
            sigmas = self._convert_to_karras(in_sigmas=sigmas, num_inference_steps=num_inference_steps)
            ts = np.array([self._sigma_to_t(sigma, log_sigmas) for sigma in sigmas]).round()
            ts = np.flip(ts).copy().astype(np.int64)
        self._set_unique(ts, device)

    def step_coefs(self, order, timestep, prev_timestep, s1=None, s2=None):
        """The fp32 scalars of one update as ops.dpm_solver_step names them, formed as :351, :420-427, :466-501 and :557-588 form
        them.  `timestep` = s0, the step's own; s1 / s2: the two timesteps before it (orders 2 / 3)."""
        t, s0 = prev_timestep, timestep
        plus = self.config.algorithm_type == 'dpmsolver++'
        heun = self.config.solver_type == 'heun'
        lambda_t, lambda_s0 = self.lambda_t[t], self.lambda_t[s0]
        alpha_t, alpha_s0 = self.alpha_t[t], self.alpha_t[s0]
        sigma_t, sigma_s0 = self.sigma_t[t], self.sigma_t[s0]
        h = lambda_t - lambda_s0

        def exp(v):
            return _rounded_once(torch.exp, v)
        c = dict(sigma_s=sigma_s0, alpha_s=alpha_s0)
        if plus:
            c['kx'] = sigma_t / sigma_s0
            c['k0'] = alpha_t * (exp(-h) - 1.0)
        else:
            c['kx'] = alpha_t / alpha_s0
            c['k0'] = sigma_t * (exp(h) - 1.0)
        if order >= 2:
            h_0 = lambda_s0 - self.lambda_t[s1]
            r0 = h_0 / h
            c['ir0'] = 1.0 / r0
            if order == 2 and not heun:
                c['k1'] = 0.5 * c['k0']
            elif plus:                                                # the reference ADDS this term: k1 is its negative
                c['k1'] = -(alpha_t * ((exp(-h) - 1.0) / h + 1.0))
            else:
                c['k1'] = sigma_t * ((exp(h) - 1.0) / h - 1.0)
        if order == 3:
            h_1 = self.lambda_t[s1] - self.lambda_t[s2]
            r1 = h_1 / h
            c['ir1'] = 1.0 / r1
            c['q'] = r0 / (r0 + r1)
            c['iq'] = 1.0 / (r0 + r1)
            if plus:
                c['k2'] = alpha_t * ((exp(-h) - 1.0 + h) / h ** 2 - 0.5)
            else:
                c['k2'] = sigma_t * ((exp(h) - 1.0 - h) / h ** 2 - 0.5)
        return {k: float(v) for k, v in c.items()}

    def step(self, model_output, timestep, sample, generator=None, return_dict=True):
        """:591-667.  The order is the reference's choice (solver_order, the lower_order_nums warm-up, lower_order_final /
        lower_order_second below 15 steps); exactly one launch, nothing read back."""
        ts, last, t, i, prev_t = self._begin_step(timestep)
        if model_output.shape[1] != sample.shape[1]:
            raise NotImplementedError('learned-variance models are not part of this path')
        final = i == last and self.config.lower_order_final and len(ts) < 15
        second = i == last - 1 and self.config.lower_order_final and len(ts) < 15
        so = self.config.solver_order
        if so == 1 or self.lower_order_nums < 1 or final:
            order = 1
        elif so == 2 or self.lower_order_nums < 2 or second:
            order = 2
        else:
            order = 3
        coef = self.step_coefs(order, t, prev_t, ts[i - 1] if order >= 2 else None, ts[i - 2] if order == 3 else None)
        sample = sample.contiguous()
        hist = self.model_outputs
        prev, m0 = ops.dpm_solver_step(sample, model_output.contiguous(), coef, order=order,
                                       data_pred=self.config.algorithm_type == 'dpmsolver++',
                                       m1=hist[-1] if order >= 2 else None, m2=hist[-2] if order == 3 else None,
                                       m0_out=self._oldest_buffer(sample))
        self._push_output(m0)
        if not return_dict:
            return (prev,)
        return SchedulerOutput(prev_sample=prev)


class UniPCMultistepScheduler(_MultistepBase):
    """scheduling_unipc_multistep.py:60-641, the UniPC predictor-corrector of orders 1 .. 3 (B(h) forms bh1 / bh2) for epsilon
    models.  The corrector of a step reuses the model evaluation the next predictor needs, so `step` runs, in the reference's order,
    convert_model_output, the UniC update of the PREVIOUS step's order on the old history and `last_sample`, and the UniP update
    of this step's order on the new history -- ONE launch of dp_unipc_step (ops.unipc_step).  The tables and every per-step scalar
    are 0-d fp32 torch arithmetic on the CPU in the reference's operation order (:339-382, :443-497), with sqrt, log and expm1
    correctly rounded (_rounded_once) and the 2 x 2 / 3 x 3 systems of rhos_p / rhos_c solved in fp64 from the fp32 R and b and
    rounded once, for the same reason: every host forms the same bits.  The timesteps are kept as a host list beside the `timesteps`
    tensor, so `step` reads nothing back from the device.  The history is a ring of `solver_order` device buffers that the steps
    write in turn, and the corrected sample lives in a buffer of the scheduler's own: neither the caller's `sample` nor the
    model's output buffer is written.
    Not carried (NotImplementedError): dynamic thresholding, `solver_p`, `trained_betas`, `sample` / `v_prediction` models,
    solver_order above 3, models that predict a variance."""
    _CONFIG_KEYS = ('num_train_timesteps', 'beta_start', 'beta_end', 'beta_schedule', 'trained_betas', 'solver_order',
                    'prediction_type', 'thresholding', 'dynamic_thresholding_ratio', 'sample_max_value', 'predict_x0',
                    'solver_type', 'lower_order_final', 'disable_corrector', 'solver_p')

    def __init__(self, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule='linear', trained_betas=None,
                 solver_order=2, prediction_type='epsilon', thresholding=False, dynamic_thresholding_ratio=0.995,
                 sample_max_value=1.0, predict_x0=True, solver_type='bh2', lower_order_final=True, disable_corrector=[],
                 solver_p=None):
        if trained_betas is not None:
            raise NotImplementedError('trained_betas is not on the hot path')
        if prediction_type != 'epsilon':
            raise NotImplementedError('prediction_type %s: only epsilon prediction is on the hot path' % prediction_type)
        if thresholding:
            raise NotImplementedError('thresholding (dynamic thresholding) is not on the hot path')
        if solver_p is not None:
            raise NotImplementedError('solver_p (a foreign predictor) is not part of this path')
        if solver_type in ('midpoint', 'heun', 'logrho'):             # :169-173: the rewrite of register_to_config
            solver_type = 'bh1'
        if solver_type not in ('bh1', 'bh2'):
            raise NotImplementedError('solver_type %s is not implemented' % solver_type)
        if int(solver_order) < 1:
            raise ValueError('solver_order must be at least 1')
        if int(solver_order) > 3:
            raise NotImplementedError('solver_order %d: the kernel carries orders 1 to 3' % solver_order)
        self.config = SimpleNamespace(
            num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end, beta_schedule=beta_schedule,
            trained_betas=trained_betas, solver_order=solver_order, prediction_type=prediction_type, thresholding=thresholding,
            dynamic_thresholding_ratio=dynamic_thresholding_ratio, sample_max_value=sample_max_value, predict_x0=predict_x0,
            solver_type=solver_type, lower_order_final=lower_order_final, disable_corrector=list(disable_corrector),
            solver_p=solver_p)
        self._init_solver_tables(num_train_timesteps, beta_start, beta_end, beta_schedule)
        self.predict_x0 = predict_x0
        self.num_inference_steps = None
        self.disable_corrector = list(disable_corrector)
        self.solver_p = None
        self.timestep_list = [None] * solver_order
        self.this_order = None
        self._xc = None                                               # the corrected sample's buffer (last_sample after a corrector)
        self._set_list(np.linspace(0, num_train_timesteps - 1, num_train_timesteps, dtype=np.float32)[::-1].copy())

    def _reset_history(self):
        self.last_sample = None

    def set_timesteps(self, num_inference_steps, device=None):
        """:187-219: the rounded linspace, duplicates removed in order of appearance, the history reset (timestep_list is kept,
        as the reference keeps it)."""
        self._set_unique(self._rounded_linspace(self.config.num_train_timesteps - 1, num_inference_steps), device)

    def update_coefs(self, order, s0, t, sis, corrector):
        """The fp32 scalars of one UniP (:339-407) or UniC (:443-514) update of `order` from s0 to t, formed as the reference forms
        them: (cx, c0, cB, rks, rhos) with x' = (cx x - c0 m0) - cB (sum_i rhos[i] D_i), D_i = (m_i - m0) / rks[i].  `sis`: the
        order - 1 timesteps before s0, newest first.  The corrector's rhos carry one entry more, the factor of (m_t - m0)."""
        lambda_t, lambda_s0 = self.lambda_t[t], self.lambda_t[s0]
        alpha_t, alpha_s0 = self.alpha_t[t], self.alpha_t[s0]
        sigma_t, sigma_s0 = self.sigma_t[t], self.sigma_t[s0]
        h = lambda_t - lambda_s0
        rks = [(self.lambda_t[si] - lambda_s0) / h for si in sis]
        assert len(rks) == order - 1
        rk_all = torch.tensor(rks + [1.0])
        hh = -h if self.predict_x0 else h
        h_phi_1 = _rounded_once(torch.expm1, hh)
        h_phi_k = h_phi_1 / hh - 1
        factorial_i = 1
        B_h = hh if self.config.solver_type == 'bh1' else _rounded_once(torch.expm1, hh)
        R, b = [], []
        for i in range(1, order + 1):
            R.append(torch.pow(rk_all, i - 1))
            b.append(h_phi_k * factorial_i / B_h)
            factorial_i *= i + 1
            h_phi_k = h_phi_k / hh - 1 / factorial_i
        R = torch.stack(R)
        b = torch.tensor(b)

        def solve(A, y):                                              # fp64 from the fp32 system, rounded once
            return torch.linalg.solve(A.double(), y.double()).float()
        if corrector:
            rhos = torch.tensor([0.5]) if order == 1 else solve(R, b)
        elif order == 1:
            rhos = torch.zeros(0)
        elif order == 2:
            rhos = torch.tensor([0.5])
        else:
            rhos = solve(R[:-1, :-1], b[:-1])
        if self.predict_x0:
            cx, c0, cB = sigma_t / sigma_s0, alpha_t * h_phi_1, alpha_t * B_h
        else:
            cx, c0, cB = alpha_t / alpha_s0, sigma_t * h_phi_1, sigma_t * B_h
        return float(cx), float(c0), float(cB), [float(v) for v in rks], [float(v) for v in rhos]

    def step_coefs(self, pc, pp, timestep, prev_timestep, old_list):
        """The scalars of one launch as ops.unipc_step names them.  `old_list`: timestep_list before this step, newest last."""
        c = dict(sigma_s=float(self.sigma_t[timestep]), alpha_s=float(self.alpha_t[timestep]))
        if pc:
            sis = [old_list[-(i + 1)] for i in range(1, pc)]
            cx, c0, cB, rks, rhos = self.update_coefs(pc, old_list[-1], timestep, sis, True)
            c.update(c_cx=cx, c_c0=c0, c_cB=cB, c_rho_last=rhos[-1])
            c.update({'c_rk%d' % (i + 1): v for i, v in enumerate(rks)})
            c.update({'c_rho%d' % (i + 1): v for i, v in enumerate(rhos[:-1])})
        new_list = list(old_list[1:]) + [timestep]
        sis = [new_list[-(i + 1)] for i in range(1, pp)]
        cx, c0, cB, rks, rhos = self.update_coefs(pp, timestep, prev_timestep, sis, False)
        c.update(p_cx=cx, p_c0=c0, p_cB=cB)
        c.update({'p_rk%d' % (i + 1): v for i, v in enumerate(rks)})
        c.update({'p_rho%d' % (i + 1): v for i, v in enumerate(rhos)})
        return c

    def step(self, model_output, timestep, sample, return_dict=True):
        """:518-600.  The corrector's order is the previous step's `this_order`, the predictor's the reference's choice
        (solver_order, the steps that remain under lower_order_final, the lower_order_nums warm-up); exactly one launch, nothing
        read back."""
        ts, last, t, i, prev_t = self._begin_step(timestep)
        if model_output.shape[1] != sample.shape[1]:
            raise NotImplementedError('a model output of %d channels for a sample of %d (a predicted variance) is not part of this path'
                                      % (model_output.shape[1], sample.shape[1]))
        use_corrector = i > 0 and i - 1 not in self.disable_corrector and self.last_sample is not None
        pc = self.this_order if use_corrector else 0
        so = self.config.solver_order
        this_order = min(so, len(ts) - i) if self.config.lower_order_final else so
        pp = min(this_order, self.lower_order_nums + 1)
        assert pp > 0
        coef = self.step_coefs(pc, pp, t, prev_t, self.timestep_list)
        sample = sample.contiguous()
        hist = self.model_outputs
        buf = self._oldest_buffer(sample)
        if any(buf is h for h in hist[1:]):
            buf = torch.empty_like(sample)
        xc = None
        if pc:
            xc = self._xc
            if xc is None or xc.shape != sample.shape or xc.device != sample.device:
                xc = self._xc = torch.empty_like(sample)
        prev, xc, m_new = ops.unipc_step(model_output.contiguous(), sample, coef, pc=pc, pp=pp, predict_x0=self.predict_x0,
                                         x_last=self.last_sample if pc else None, hist=hist[::-1][:max(pc, pp - 1)],
                                         m_new=buf, x_c=xc)
        self._push_output(m_new)
        self.timestep_list = list(self.timestep_list[1:]) + [t]
        self.this_order = pp
        self.last_sample = xc if pc else sample
        if not return_dict:
            return (prev,)
        return SchedulerOutput(prev_sample=prev)


class _TreatedSolverBase(_MultistepBase):
    """What DEISMultistepScheduler and DPMSolverSinglestepScheduler share beyond _MultistepBase: the three model types and dynamic
    thresholding, whose per-image s is one launch of the exact quantile (ops.x0_abs_quantile) ahead of the step's own."""

    def _check_common(self, trained_betas, solver_order, prediction_type):
        if trained_betas is not None:
            raise NotImplementedError('trained_betas is not on the hot path')
        if prediction_type not in self._PREDICTION_TYPES:
            raise ValueError('prediction_type given as %s must be one of `epsilon`, `sample`, or `v_prediction` for the %s.'
                             % (prediction_type, type(self).__name__))
        if int(solver_order) < 1:
            raise ValueError('solver_order must be at least 1')
        if int(solver_order) > 3:
            raise NotImplementedError('solver_order %d: the kernel carries orders 1 to 3' % solver_order)

    def _begin_solver_step(self, model_output, timestep, sample):
        begun = self._begin_step(timestep)
        if model_output.shape[1] != sample.shape[1]:
            raise NotImplementedError('a model output of %d channels for a sample of %d (a predicted variance) is not part of this path'
                                      % (model_output.shape[1], sample.shape[1]))
        return begun

    def _stats(self, sample, model_output, coef):
        """The [B, 4] table of the thresholded x0's quantile: one launch, nothing read back."""
        return ops.x0_abs_quantile(sample, model_output, ops.X0_PRED[self.config.prediction_type], coef['sa'], coef['sb'],
                                   self.config.dynamic_thresholding_ratio, self.config.sample_max_value)


def _log_once(v):
    return _rounded_once(torch.log, v)


def _exp_once(v):
    return _rounded_once(torch.exp, v)


class DEISMultistepScheduler(_TreatedSolverBase):
    """scheduling_deis_multistep.py:58-513, the log-rho multistep DEIS of orders 1 .. 3 for epsilon, `sample` and `v_prediction`
    models, with dynamic thresholding (`thresholding`, `dynamic_thresholding_ratio`, `sample_max_value`; with the default
    sample_max_value = 1.0 every s is 1 and the option is a clip to [-1, 1]).  The tables and every per-step scalar are 0-d fp32 torch
    arithmetic on the CPU in the reference's operation order (:298-303, :329-345, :371-401), with sqrt, log and exp correctly rounded
    (_rounded_once) -- the log of the log-rho coefficients too, which the reference takes with numpy's fp32 log.  The per-element work
    of a step -- convert_model_output, which always converts to x0 and back to epsilon, and the update -- is ONE launch of dp_deis_step
    (ops.deis_step); a thresholded step is the quantile's launch (ops.x0_abs_quantile) and that one.  `step` reads nothing back.
    Not carried (NotImplementedError): `trained_betas`, solver_order above 3, models that predict a variance."""
    _CONFIG_KEYS = ('num_train_timesteps', 'beta_start', 'beta_end', 'beta_schedule', 'trained_betas', 'solver_order',
                    'prediction_type', 'thresholding', 'dynamic_thresholding_ratio', 'sample_max_value', 'algorithm_type',
                    'solver_type', 'lower_order_final')

    def __init__(self, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule='linear', trained_betas=None,
                 solver_order=2, prediction_type='epsilon', thresholding=False, dynamic_thresholding_ratio=0.995,
                 sample_max_value=1.0, algorithm_type='deis', solver_type='logrho', lower_order_final=True):
        self._check_common(trained_betas, solver_order, prediction_type)
        if algorithm_type in ('dpmsolver', 'dpmsolver++'):            # :155-165: the two rewrites of register_to_config
            algorithm_type = 'deis'
        if algorithm_type != 'deis':
            raise NotImplementedError('algorithm_type %s is not implemented' % algorithm_type)
        if solver_type in ('midpoint', 'heun', 'bh1', 'bh2'):
            solver_type = 'logrho'
        if solver_type != 'logrho':
            raise NotImplementedError('solver_type %s is not implemented' % solver_type)
        self.config = SimpleNamespace(
            num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end, beta_schedule=beta_schedule,
            trained_betas=trained_betas, solver_order=solver_order, prediction_type=prediction_type, thresholding=thresholding,
            dynamic_thresholding_ratio=dynamic_thresholding_ratio, sample_max_value=sample_max_value,
            algorithm_type=algorithm_type, solver_type=solver_type, lower_order_final=lower_order_final)
        self._init_solver_tables(num_train_timesteps, beta_start, beta_end, beta_schedule)
        self.num_inference_steps = None
        self._set_list(np.linspace(0, num_train_timesteps - 1, num_train_timesteps, dtype=np.float32)[::-1].copy())

    def set_timesteps(self, num_inference_steps, device=None):
        """:174-203: the rounded linspace, duplicates removed in order of appearance, the history reset."""
        self._set_unique(self._rounded_linspace(self.config.num_train_timesteps - 1, num_inference_steps), device)

    def step_coefs(self, order, timestep, prev_timestep, s1=None, s2=None):
        """The fp32 scalars of one update as ops.deis_step names them, formed as :298-303, :331-343 and :373-399 form them.
        `timestep` = s0, the step's own; s1 / s2: the two timesteps before it (orders 2 / 3)."""
        t, s0 = prev_timestep, timestep
        alpha_t, alpha_s0 = self.alpha_t[t], self.alpha_t[s0]
        sigma_t, sigma_s0 = self.sigma_t[t], self.sigma_t[s0]
        c = dict(sa=alpha_s0, sb=sigma_s0)
        log = _log_once
        if order == 1:
            h = self.lambda_t[t] - self.lambda_t[s0]
            c['kx'] = alpha_t / alpha_s0
            c['k0'] = sigma_t * (_exp_once(h) - 1.0)
        elif order == 2:
            rho_t, rho_s0, rho_s1 = sigma_t / alpha_t, sigma_s0 / alpha_s0, self.sigma_t[s1] / self.alpha_t[s1]

            def ind_fn(t, b, c):
                return t * (-log(c) + log(t) - 1) / (log(b) - log(c))
            c['c1'] = ind_fn(rho_t, rho_s0, rho_s1) - ind_fn(rho_s0, rho_s0, rho_s1)
            c['c2'] = ind_fn(rho_t, rho_s1, rho_s0) - ind_fn(rho_s0, rho_s1, rho_s0)
        else:
            rho_t, rho_s0 = sigma_t / alpha_t, sigma_s0 / alpha_s0
            rho_s1, rho_s2 = self.sigma_t[s1] / self.alpha_t[s1], self.sigma_t[s2] / self.alpha_t[s2]

            def ind_fn(t, b, c, d):
                numerator = t * (log(c) * (log(d) - log(t) + 1) - log(d) * log(t) + log(d) + log(t) ** 2 - 2 * log(t) + 2)
                denominator = (log(b) - log(c)) * (log(b) - log(d))
                return numerator / denominator
            c['c1'] = ind_fn(rho_t, rho_s0, rho_s1, rho_s2) - ind_fn(rho_s0, rho_s0, rho_s1, rho_s2)
            c['c2'] = ind_fn(rho_t, rho_s1, rho_s2, rho_s0) - ind_fn(rho_s0, rho_s1, rho_s2, rho_s0)
            c['c3'] = ind_fn(rho_t, rho_s2, rho_s0, rho_s1) - ind_fn(rho_s0, rho_s2, rho_s0, rho_s1)
        if order >= 2:
            c.update(at=alpha_t, as0=alpha_s0)
        return {k: float(v) for k, v in c.items()}

    def step(self, model_output, timestep, sample, return_dict=True):
        """:407-473.  The order is the reference's choice (solver_order, the lower_order_nums warm-up, lower_order_final /
        lower_order_second below 15 steps); exactly one launch, two with thresholding, nothing read back."""
        ts, last, t, i, prev_t = self._begin_solver_step(model_output, timestep, sample)
        final = i == last and self.config.lower_order_final and len(ts) < 15
        second = i == last - 1 and self.config.lower_order_final and len(ts) < 15
        so = self.config.solver_order
        if so == 1 or self.lower_order_nums < 1 or final:
            order = 1
        elif so == 2 or self.lower_order_nums < 2 or second:
            order = 2
        else:
            order = 3
        coef = self.step_coefs(order, t, prev_t, ts[i - 1] if order >= 2 else None, ts[i - 2] if order == 3 else None)
        sample, model_output = sample.contiguous(), model_output.contiguous()
        hist = self.model_outputs
        prev, m0 = ops.deis_step(sample, model_output, coef, order=order, pred=ops.X0_PRED[self.config.prediction_type],
                                 m1=hist[-1] if order >= 2 else None, m2=hist[-2] if order == 3 else None,
                                 stats=self._stats(sample, model_output, coef) if self.config.thresholding else None,
                                 m0_out=self._oldest_buffer(sample))
        self._push_output(m0)
        if not return_dict:
            return (prev,)
        return SchedulerOutput(prev_sample=prev)


class DPMSolverSinglestepScheduler(_TreatedSolverBase):
    """scheduling_dpmsolver_singlestep.py:60-658, the singlestep DPM-Solver / DPM-Solver++ of orders 1 .. 3 (midpoint / heun) for
    epsilon, `sample` and `v_prediction` models, with dynamic thresholding on the dpmsolver++ branch (the reference applies none under
    `dpmsolver`, and neither does this class).  A solver step of order k spans k model evaluations: the first is a first-order step
    from the sample it is handed, which the scheduler keeps (`self.sample`, a reference -- no copy launch; every `step` writes into a
    buffer of its own, so nothing lands in it); the k-th restarts from that saved sample with the k converted outputs.  The tables and
    every per-step scalar are 0-d fp32 torch arithmetic on the CPU in the reference's operation order (:379-386, :414-446, :475-518),
    with sqrt, log and exp correctly rounded (_rounded_once); the per-element work of a step is ONE launch of dp_dpm_single_step
    (ops.dpm_single_step), two with thresholding.  `step` reads nothing back.
    A reference oddity, reproduced: `step` takes its order from `order_list`, which __init__ builds once for num_train_timesteps steps
    (:195, :599), and not from `orders`, which set_timesteps builds for the steps asked for.  With solver_order = 3 and 9 steps the
    last step is therefore a third-order one, where `orders` says 1.
    Unlike the multistep classes the reference does not remove duplicate timesteps here, and its `step` then fails on the duplicate;
    set_timesteps raises ValueError for such a step count.
    Not carried (NotImplementedError): `trained_betas`, solver_order above 3, models that predict a variance."""
    _CONFIG_KEYS = ('num_train_timesteps', 'beta_start', 'beta_end', 'beta_schedule', 'trained_betas', 'solver_order',
                    'prediction_type', 'thresholding', 'dynamic_thresholding_ratio', 'sample_max_value', 'algorithm_type',
                    'solver_type', 'lower_order_final', 'lambda_min_clipped', 'variance_type')

    def __init__(self, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule='linear', trained_betas=None,
                 solver_order=2, prediction_type='epsilon', thresholding=False, dynamic_thresholding_ratio=0.995,
                 sample_max_value=1.0, algorithm_type='dpmsolver++', solver_type='midpoint', lower_order_final=True,
                 lambda_min_clipped=-float('inf'), variance_type=None):
        self._check_common(trained_betas, solver_order, prediction_type)
        if variance_type in ('learned', 'learned_range'):
            raise NotImplementedError('learned-variance models are not part of this path')
        if algorithm_type == 'deis':                                  # :178-187: the two rewrites of register_to_config
            algorithm_type = 'dpmsolver++'
        if algorithm_type not in ('dpmsolver', 'dpmsolver++'):
            raise NotImplementedError('algorithm_type %s is not implemented' % algorithm_type)
        if solver_type in ('logrho', 'bh1', 'bh2'):
            solver_type = 'midpoint'
        if solver_type not in ('midpoint', 'heun'):
            raise NotImplementedError('solver_type %s is not implemented' % solver_type)
        self.config = SimpleNamespace(
            num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end, beta_schedule=beta_schedule,
            trained_betas=trained_betas, solver_order=solver_order, prediction_type=prediction_type, thresholding=thresholding,
            dynamic_thresholding_ratio=dynamic_thresholding_ratio, sample_max_value=sample_max_value,
            algorithm_type=algorithm_type, solver_type=solver_type, lower_order_final=lower_order_final,
            lambda_min_clipped=lambda_min_clipped, variance_type=variance_type)
        self._init_solver_tables(num_train_timesteps, beta_start, beta_end, beta_schedule)
        self.num_inference_steps = None
        self._set_list(np.linspace(0, num_train_timesteps - 1, num_train_timesteps, dtype=np.float32)[::-1].copy())
        self.order_list = self.get_order_list(num_train_timesteps)

    def _reset_history(self):
        self.sample = None

    def get_order_list(self, num_inference_steps):
        """:197-229: the solver order at each step."""
        steps, order = num_inference_steps, self.config.solver_order
        if not self.config.lower_order_final:
            return list(range(1, order + 1)) * (steps // order)
        if order == 3:
            if steps % 3 == 0:
                return [1, 2, 3] * (steps // 3 - 1) + [1, 2] + [1]
            return [1, 2, 3] * (steps // 3) + [1, 2][:steps % 3]
        if order == 2:
            return [1, 2] * (steps // 2) + [1] * (steps % 2)
        return [1] * steps

    def set_timesteps(self, num_inference_steps, device=None):
        """:231-254: the lambda_min_clipped search and the rounded linspace; duplicates are NOT removed (see the class), `orders`."""
        clipped_idx = int(torch.searchsorted(torch.flip(self.lambda_t, [0]), self.config.lambda_min_clipped))
        ts = self._rounded_linspace(self.config.num_train_timesteps - 1 - clipped_idx, num_inference_steps)
        if len(set(ts.tolist())) != len(ts):
            raise ValueError('%d inference steps give a timestep table with duplicates, which the singlestep solver cannot step through'
                             % num_inference_steps)
        self._set_list(ts, device)
        self.num_inference_steps = num_inference_steps
        self.orders = self.get_order_list(num_inference_steps)

    def step_coefs(self, order, timestep, prev_timestep, s1=None, s2=None):
        """The fp32 scalars of one update as ops.dpm_single_step names them, formed as :379-386, :414-446 and :475-518 form them.
        `timestep` = s0, the step's own; s1 / s2: the two timesteps before it (orders 2 / 3).  The update starts at the oldest."""
        t, s0 = prev_timestep, timestep
        plus = self.config.algorithm_type == 'dpmsolver++'
        heun = self.config.solver_type == 'heun'
        base = (s0, s1, s2)[order - 1]
        lambda_t, lambda_b = self.lambda_t[t], self.lambda_t[base]
        alpha_t, sigma_t = self.alpha_t[t], self.sigma_t[t]
        h = lambda_t - lambda_b
        exp = _exp_once
        c = dict(sa=self.alpha_t[s0], sb=self.sigma_t[s0])
        if plus:
            c['kx'] = sigma_t / self.sigma_t[base]
            c['k0'] = alpha_t * (exp(-h) - 1.0)
        else:
            c['kx'] = alpha_t / self.alpha_t[base]
            c['k0'] = sigma_t * (exp(h) - 1.0)
        if order >= 2:
            r0 = (self.lambda_t[s0] - lambda_b) / h
            c['ir0'] = 1.0 / r0
            if order == 2 and not heun:
                c['k1'] = 0.5 * c['k0']
            elif plus:                                                # the reference ADDS this term: k1 is its negative
                c['k1'] = -(alpha_t * ((exp(-h) - 1.0) / h + 1.0))
            else:
                c['k1'] = sigma_t * ((exp(h) - 1.0) / h - 1.0)
        if order == 3:
            r1 = (self.lambda_t[s1] - lambda_b) / h
            c['ir1'] = 1.0 / r1
            if heun:
                c.update(r0=r0, r1=r1, dr=r0 - r1)
                if plus:
                    c['k2'] = alpha_t * ((exp(-h) - 1.0 + h) / h ** 2 - 0.5)
                else:
                    c['k2'] = sigma_t * ((exp(h) - 1.0 - h) / h ** 2 - 0.5)
        return {k: float(v) for k, v in c.items()}

    def step(self, model_output, timestep, sample, return_dict=True):
        """:558-612.  The order is order_list's at this step's index (see the class); exactly one launch, two with thresholding on
        the dpmsolver++ branch, nothing read back."""
        ts, last, t, i, prev_t = self._begin_solver_step(model_output, timestep, sample)
        order = self.order_list[i]
        sample, model_output = sample.contiguous(), model_output.contiguous()
        if order == 1:
            self.sample = sample                                      # a reference: the step of order 2 / 3 restarts from it
        elif self.sample is None or i < order - 1 or any(h is None for h in self.model_outputs[-(order - 1):]):
            raise ValueError('step %d is of order %d, and the steps it completes have not been taken' % (i, order))
        coef = self.step_coefs(order, t, prev_t, ts[i - 1] if order >= 2 else None, ts[i - 2] if order == 3 else None)
        plus = self.config.algorithm_type == 'dpmsolver++'
        hist = self.model_outputs
        prev, m0 = ops.dpm_single_step(sample, model_output, coef, order=order, pred=ops.X0_PRED[self.config.prediction_type],
                                       data_pred=plus, heun=self.config.solver_type == 'heun',
                                       xs=self.sample if order >= 2 else None,
                                       m1=hist[-1] if order >= 2 else None, m2=hist[-2] if order == 3 else None,
                                       stats=self._stats(sample, model_output, coef) if plus and self.config.thresholding else None,
                                       m0_out=self._oldest_buffer(sample))
        self._push_output(m0)
        if not return_dict:
            return (prev,)
        return SchedulerOutput(prev_sample=prev)


class PNDMScheduler(_SchedulerBase):
    """scheduling_pndm.py:58-427, F-PNDM: twelve Runge-Kutta calls (step_prk) and then the linear multistep method (step_plms), or
    the multistep method alone (`skip_prk_steps`), for epsilon and `v_prediction` models.  The counter logic is the reference's, its
    oddities included: the Runge-Kutta stages 1 .. 3 start from `cur_sample`, not from the `sample` they are handed; the second call
    with `skip_prk_steps` shifts its timesteps and goes back to `cur_sample`; a negative previous timestep selects
    `final_alpha_cumprod`.  The scalars of a step are 0-d fp32 torch arithmetic on the CPU in the reference's operation order, each
    `** 0.5` correctly rounded (_rounded_once: the reference's bits on a host whose math library rounds sqrt correctly, and the same
    bits on every host); the per-element work -- the accumulation or the multistep combination, the v-conversion and formula (9) --
    is ONE launch of dp_pndm_step (ops.pndm_step).  The timesteps are kept as host lists beside the `timesteps` tensor, so `step`
    reads nothing back from the device.  The history `ets` is a ring of four device buffers that the steps write in turn (the model's
    own tensor is not kept: a captured forward reuses its output buffer); `cur_sample` is held by reference, as the reference holds it.
    Not carried: `trained_betas` (NotImplementedError); `sample`-prediction models (ValueError in `step`, as in the reference);
    models that predict a variance (NotImplementedError)."""
    _CONFIG_KEYS = ('num_train_timesteps', 'beta_start', 'beta_end', 'beta_schedule', 'trained_betas', 'skip_prk_steps',
                    'set_alpha_to_one', 'prediction_type', 'steps_offset')
    order = 1
    pndm_order = 4

    def __init__(self, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule='linear', trained_betas=None,
                 skip_prk_steps=False, set_alpha_to_one=False, prediction_type='epsilon', steps_offset=0):
        if trained_betas is not None:
            raise NotImplementedError('trained_betas is not on the hot path')
        self.config = SimpleNamespace(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                                      beta_schedule=beta_schedule, trained_betas=trained_betas, skip_prk_steps=skip_prk_steps,
                                      set_alpha_to_one=set_alpha_to_one, prediction_type=prediction_type, steps_offset=steps_offset)
        self._init_tables(num_train_timesteps, beta_start, beta_end, beta_schedule,
                          _betas_for_alpha_bar(num_train_timesteps) if beta_schedule == 'squaredcos_cap_v2' else None)
        self.final_alpha_cumprod = torch.tensor(1.0) if set_alpha_to_one else self.alphas_cumprod[0]
        self.num_inference_steps = None
        self._timesteps = np.arange(0, num_train_timesteps)[::-1].copy()
        self.prk_timesteps = self.plms_timesteps = self.timesteps = None
        self._reset()

    def __len__(self):
        return self.config.num_train_timesteps

    def _reset(self):
        self.counter = 0
        self.cur_sample = None
        self.ets = []                                 # the history: up to four buffers of this scheduler's own, newest last
        self._acc = None                              # cur_model_output, the Runge-Kutta accumulator: written by stage 0, read by 1 .. 3

    def set_timesteps(self, num_inference_steps, device=None):
        """:152-190 with the reference's numpy expressions, repeats included; the running values reset."""
        T = self.config.num_train_timesteps
        if not self.config.skip_prk_steps and num_inference_steps < self.pndm_order:
            raise ValueError('num_inference_steps = %d: without skip_prk_steps the Runge-Kutta timesteps need at least %d inference '
                             'steps (the reference fails to broadcast its arrays there)' % (num_inference_steps, self.pndm_order))
        self.num_inference_steps = num_inference_steps
        step_ratio = T // num_inference_steps
        self._timesteps = (np.arange(0, num_inference_steps) * step_ratio).round()
        self._timesteps += self.config.steps_offset
        if self.config.skip_prk_steps:
            self.prk_timesteps = np.array([])
            self.plms_timesteps = np.concatenate([self._timesteps[:-1], self._timesteps[-2:-1], self._timesteps[-1:]])[::-1].copy()
        else:
            prk = np.array(self._timesteps[-self.pndm_order:]).repeat(2) + np.tile(
                np.array([0, T // num_inference_steps // 2]), self.pndm_order)
            self.prk_timesteps = (prk[:-1].repeat(2)[1:-1])[::-1].copy()
            self.plms_timesteps = self._timesteps[:-3][::-1].copy()
        ts = np.concatenate([self.prk_timesteps, self.plms_timesteps]).astype(np.int64)
        self.timesteps = torch.from_numpy(ts).to(device)
        self._ts = [int(v) for v in ts]                               # the host's copies: what `step` looks timesteps up in
        self._prk = [int(v) for v in self.prk_timesteps]
        self._reset()

    def step_coefs(self, timestep, prev_timestep):
        """The fp32 scalars of _get_prev_sample (:371-397) as ops.pndm_step names them: sa = alpha_prod_t ** 0.5 and
        sb = beta_prod_t ** 0.5 (the v-conversion; v_prediction only), sc = sample_coeff, d = alpha_prod_t_prev - alpha_prod_t,
        den = model_output_denom_coeff."""
        pt = self.config.prediction_type
        if pt not in ('epsilon', 'v_prediction'):
            raise ValueError('prediction_type given as %s must be one of `epsilon` or `v_prediction`' % pt)

        def sqrt(v):
            return _rounded_once(torch.sqrt, v)
        alpha_prod_t = self.alphas_cumprod[timestep]
        alpha_prod_t_prev = self.alphas_cumprod[prev_timestep] if prev_timestep >= 0 else self.final_alpha_cumprod
        beta_prod_t = 1 - alpha_prod_t
        beta_prod_t_prev = 1 - alpha_prod_t_prev
        c = {}
        if pt == 'v_prediction':
            c['sa'], c['sb'] = sqrt(alpha_prod_t), sqrt(beta_prod_t)
        c['sc'] = sqrt(alpha_prod_t_prev / alpha_prod_t)
        c['den'] = alpha_prod_t * sqrt(beta_prod_t_prev) + sqrt(alpha_prod_t * beta_prod_t * alpha_prod_t_prev)
        c['d'] = alpha_prod_t_prev - alpha_prod_t
        return {k: float(v) for k, v in c.items()}

    def _fits(self, buf, sample):
        return buf is not None and buf.shape == sample.shape and buf.device == sample.device

    def step(self, model_output, timestep, sample, return_dict=True, out=None):
        """:192-343: step_prk while the counter is inside prk_timesteps (and the Runge-Kutta calls are not skipped), step_plms after
        that; exactly one launch, nothing read back.  `out` (extension): the buffer that takes prev_sample, which may be `sample`
        itself; without it a step writes none of its inputs."""
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
        if model_output.shape[1] != sample.shape[1]:
            raise NotImplementedError('learned-variance models are not part of this path')
        cfg = self.config
        if cfg.prediction_type not in ('epsilon', 'v_prediction'):
            raise ValueError('prediction_type given as %s must be one of `epsilon` or `v_prediction`' % cfg.prediction_type)
        t = int(timestep)
        stride = cfg.num_train_timesteps // self.num_inference_steps
        acc, hist, hist_out = None, (), None
        if self.counter < len(self._prk) and not cfg.skip_prk_steps:                                  # step_prk, :251-270
            prev_t = t - (0 if self.counter % 2 else stride // 2)
            t = self._prk[self.counter // 4 * 4]
            mode = ops.PNDM_PRK0 + self.counter % 4
            if mode == ops.PNDM_PRK0:
                if not self._fits(self._acc, sample):
                    self._acc = torch.empty_like(sample, memory_format=torch.contiguous_format)
                hist_out = torch.empty_like(sample, memory_format=torch.contiguous_format)
                self.cur_sample = sample
            acc = self._acc
            x = self.cur_sample if self.cur_sample is not None else sample
            keep = self.ets
        else:                                                                                         # step_plms, :306-337
            if not cfg.skip_prk_steps and len(self.ets) < 3:
                raise ValueError('%s can only be run AFTER scheduler has been run in \'prk\' mode for at least 12 iterations'
                                 % type(self).__name__)
            prev_t = t - stride
            x = sample
            if self.counter != 1:
                keep = self.ets[-3:]
                old = self.ets[:-3]
                hist_out = old[0] if old and self._fits(old[0], sample) else torch.empty_like(sample, memory_format=torch.contiguous_format)
                if keep:
                    mode = (ops.PNDM_PLMS2, ops.PNDM_PLMS3, ops.PNDM_PLMS4)[len(keep) - 1]
                elif self.counter == 0:
                    mode = ops.PNDM_PLMS1
                    self.cur_sample = sample
                else:
                    raise RuntimeError('step_plms without history at counter %d: not a state that `step` reaches' % self.counter)
            else:
                if len(self.ets) != 1:
                    raise RuntimeError('step_plms at counter 1 with %d history entries: not a state that `step` reaches' % len(self.ets))
                prev_t, t = t, t + stride                                                             # :319-321
                keep = self.ets
                mode = ops.PNDM_PLMS_AVG
                x = self.cur_sample
                self.cur_sample = None
            hist = keep[::-1]
        prev, appended = ops.pndm_step(x.contiguous(), model_output.contiguous(), self.step_coefs(t, prev_t), mode,
                                       v_pred=cfg.prediction_type == 'v_prediction', acc=acc, hist=hist, out=out, hist_out=hist_out)
        self.ets = keep + [appended] if appended is not None else keep
        self.counter += 1                             # (cur_model_output = 0 after stage 3: stage 0 of the next round overwrites _acc)
        if not return_dict:
            return (prev,)
        return SchedulerOutput(prev_sample=prev)


@dataclass
class RePaintSchedulerOutput:
    prev_sample: torch.Tensor
    pred_original_sample: torch.Tensor = None


class RePaintScheduler(_SchedulerBase):
    """scheduling_repaint.py:75-329, RePaint inpainting with an unconditional epsilon model: `step` is the DDIM update of the unknown
    region, the re-noised original image of the known region and the blend by the mask; `undo_step` re-noises a state by
    num_train_timesteps // num_inference_steps steps of the forward process.  The timestep list walks down and jumps back up
    (`jump_length`, `jump_n_sample`).  The scalars are 0-d fp32 torch arithmetic on the CPU in the reference's operation order, each
    `** 0.5` correctly rounded (_rounded_once); the per-element work of `step` is ONE launch of dp_repaint_step (ops.repaint_step) and
    that of `undo_step` one launch of dp_repaint_undo per eight re-noising steps (ops.repaint_undo).  The timesteps are kept as a
    host list beside the `timesteps` tensor, so neither reads anything back from the device.  The noise is drawn as the reference
    draws it: one randn_tensor per `step`, always, and one per re-noising step.  `eta` is an attribute that the pipeline
    overwrites, as in the reference.  Not carried: `trained_betas` and models that predict a variance (NotImplementedError)."""
    _CONFIG_KEYS = ('num_train_timesteps', 'beta_start', 'beta_end', 'beta_schedule', 'eta', 'trained_betas', 'clip_sample')
    order = 1

    def __init__(self, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule='linear', eta=0.0,
                 trained_betas=None, clip_sample=True):
        if trained_betas is not None:
            raise NotImplementedError('trained_betas is not on the hot path')
        self.config = SimpleNamespace(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                                      beta_schedule=beta_schedule, eta=eta, trained_betas=trained_betas, clip_sample=clip_sample)
        betas = None
        if beta_schedule == 'squaredcos_cap_v2':
            betas = _betas_for_alpha_bar(num_train_timesteps)
        elif beta_schedule == 'sigmoid':                                         # :131-134, GeoDiff's schedule
            betas = _rounded_once(torch.sigmoid, torch.linspace(-6, 6, num_train_timesteps)) * (beta_end - beta_start) + beta_start
        self._init_tables(num_train_timesteps, beta_start, beta_end, beta_schedule, betas)
        self.one = torch.tensor(1.0)
        self.final_alpha_cumprod = torch.tensor(1.0)
        self.num_inference_steps = None
        self.timesteps = torch.from_numpy(np.arange(0, num_train_timesteps)[::-1].copy())
        self._ts = [int(v) for v in self.timesteps]
        self.eta = eta
        self._coefs, self._mask = {}, None

    def __len__(self):
        return self.config.num_train_timesteps

    def set_timesteps(self, num_inference_steps, jump_length=10, jump_n_sample=10, device=None):
        """:174-195: down one step at a time; at every `jump_length`-th step, `jump_n_sample - 1` times, back up `jump_length`
        steps (the entries that `undo_step` serves)."""
        num_inference_steps = min(self.config.num_train_timesteps, num_inference_steps)
        self.num_inference_steps = num_inference_steps
        timesteps = []
        jumps = {}
        for j in range(0, num_inference_steps - jump_length, jump_length):
            jumps[j] = jump_n_sample - 1
        t = num_inference_steps
        while t >= 1:
            t = t - 1
            timesteps.append(t)
            if jumps.get(t, 0) > 0:
                jumps[t] = jumps[t] - 1
                for _ in range(jump_length):
                    t = t + 1
                    timesteps.append(t)
        timesteps = np.array(timesteps) * (self.config.num_train_timesteps // self.num_inference_steps)
        self.timesteps = torch.from_numpy(timesteps).to(device)
        self._ts = [int(v) for v in timesteps]                        # the host's copy: what the pipeline iterates over
        self._coefs = {}

    def _get_variance(self, t):
        """:197-214."""
        prev_timestep = t - self.config.num_train_timesteps // self.num_inference_steps
        alpha_prod_t = self.alphas_cumprod[t]
        alpha_prod_t_prev = self.alphas_cumprod[prev_timestep] if prev_timestep >= 0 else self.final_alpha_cumprod
        beta_prod_t = 1 - alpha_prod_t
        beta_prod_t_prev = 1 - alpha_prod_t_prev
        return (beta_prod_t_prev / beta_prod_t) * (1 - alpha_prod_t / alpha_prod_t_prev)

    def step_coefs(self, timestep):
        """The fp32 scalars of `step` (:251-290) as ops.repaint_step names them: sa = alpha_prod_t ** 0.5, sb = beta_prod_t ** 0.5,
        sap = alpha_prod_t_prev ** 0.5, s1 = (1 - alpha_prod_t_prev) ** 0.5, sd = std_dev_t = eta * variance ** 0.5,
        cd = (1 - alpha_prod_t_prev - std_dev_t ** 2) ** 0.5.  Kept per (timestep, eta): the list revisits its timesteps."""
        key = ('step', timestep, self.eta)
        c = self._coefs.get(key)
        if c is not None:
            return c

        def sqrt(v):
            return _rounded_once(torch.sqrt, v)
        prev_timestep = timestep - self.config.num_train_timesteps // self.num_inference_steps
        alpha_prod_t = self.alphas_cumprod[timestep]
        alpha_prod_t_prev = self.alphas_cumprod[prev_timestep] if prev_timestep >= 0 else self.final_alpha_cumprod
        beta_prod_t = 1 - alpha_prod_t
        std_dev_t = self.eta * sqrt(self._get_variance(timestep))
        c = dict(sa=sqrt(alpha_prod_t), sb=sqrt(beta_prod_t), sap=sqrt(alpha_prod_t_prev), s1=sqrt(1 - alpha_prod_t_prev),
                 cd=sqrt(1 - alpha_prod_t_prev - std_dev_t ** 2), sd=std_dev_t)
        c = self._coefs[key] = {k: float(v) for k, v in c.items()}
        return c

    def undo_coefs(self, timestep):
        """[(a_i, b_i)] of `undo_step` (:304-316): a_i = (1 - beta) ** 0.5, b_i = beta ** 0.5 at timestep + i."""
        key = ('undo', timestep)
        c = self._coefs.get(key)
        if c is None:
            n = self.config.num_train_timesteps // self.num_inference_steps
            betas = [self.betas[timestep + i] for i in range(n)]
            c = self._coefs[key] = [(float(_rounded_once(torch.sqrt, 1 - b)), float(_rounded_once(torch.sqrt, b))) for b in betas]
        return c

    def _mask_for(self, mask, sample):
        """The mask as ops.repaint_step reads it: itself where the kernel indexes its shape in place, otherwise expanded to the
        sample's shape, once per mask."""
        if ops.repaint_mask_geometry(sample.shape, mask.shape) is not None:
            return mask.contiguous()
        if self._mask is None or self._mask[0] is not mask or self._mask[1].shape != sample.shape:
            self._mask = (mask, mask.expand(sample.shape).contiguous())
        return self._mask[1]

    def step(self, model_output, timestep, sample, original_image, mask, generator=None, return_dict=True, out=None, need_x0=True):
        """:216-301: exactly one launch, nothing read back; one randn_tensor draw per call, also where the noise is not added.
        `out` (extension): the buffer that takes prev_sample, which may be `sample` itself; without it a step writes none of its
        inputs.  `need_x0=False` (extension): pred_original_sample is not written and is None in the result."""
        if self.num_inference_steps is None:
            raise ValueError("Number of inference steps is 'None', you need to run 'set_timesteps' after creating the scheduler")
        if model_output.shape[1] != sample.shape[1]:
            raise NotImplementedError('learned-variance models are not part of this path')
        t = int(timestep)
        noise = randn_tensor(model_output.shape, generator=generator, device=model_output.device, dtype=model_output.dtype)
        prev, x0 = ops.repaint_step(sample.contiguous(), model_output.contiguous(), noise, original_image.contiguous(),
                                    self._mask_for(mask, sample), self.step_coefs(t), clip=self.config.clip_sample,
                                    add_noise=t > 0 and self.eta > 0, out=out, x0_out=True if need_x0 else None)
        if not return_dict:
            return (prev, x0)
        return RePaintSchedulerOutput(prev_sample=prev, pred_original_sample=x0)

    def undo_step(self, sample, timestep, generator=None, out=None):
        """:303-318: num_train_timesteps // num_inference_steps re-noising steps from `timestep`, each with a randn_tensor draw of
        its own, in ceil(n / 8) launches.  `out` (extension) may be `sample` itself."""
        coefs = self.undo_coefs(int(timestep))
        noises = [randn_tensor(sample.shape, generator=generator, device=sample.device, dtype=sample.dtype) for _ in coefs]
        return ops.repaint_undo(sample.contiguous(), noises, coefs, out=out)

    def add_noise(self, original_samples, noise, timesteps):
        raise NotImplementedError('Use `DDPMScheduler.add_noise()` to train for sampling with RePaint.')


@dataclass
class EulerDiscreteSchedulerOutput:
    prev_sample: torch.Tensor
    pred_original_sample: torch.Tensor = None


@dataclass
class EulerAncestralDiscreteSchedulerOutput:
    prev_sample: torch.Tensor
    pred_original_sample: torch.Tensor = None


class _SigmaSchedulerBase(_SchedulerBase):
    """What the sigma-space (k-diffusion) schedulers share, and where a new one starts: the sample is carried at scale sigma
    (`init_noise_sigma`, up to 157 for the CIFAR schedule), the model input is rescaled every step (`scale_model_input`, one launch of
    dp_sigma_scale), the timesteps are float64 and mostly fractional, and `add_noise` is x0 + sigma * noise (dp_sigma_add_noise).
    The timestep and sigma tables live as host lists (`_ts`, `_sig`) beside the `timesteps` / `sigmas` tensors: `step` and
    `scale_model_input` look the index up on the host and read nothing back from the device.  The scalars of a step are 0-d fp32
    torch arithmetic on the CPU in the reference's operation order, each `** 0.5`, log and exp correctly rounded (_rounded_once).
    Outputs go into buffers of the scheduler's own, written in turn, so that a returned `prev_sample` stays valid while it is the
    next step's input; the caller's `sample` and the model's output buffer are never written.
    `sigma_space` is what a pipeline that neither scales its input nor starts from `init_noise_sigma` refuses by."""
    sigma_space = True
    order = 1
    _WARNS_UNSCALED = True            # `step` before any `scale_model_input` warns once (the two Euler classes; Heun has no such warning)
    _PRED = {'epsilon': ops.SIGMA_EPSILON, 'v_prediction': ops.SIGMA_V}
    _sigma_to_t = DPMSolverMultistepScheduler._sigma_to_t
    _convert_to_karras = DPMSolverMultistepScheduler._convert_to_karras

    def __len__(self):
        return self.config.num_train_timesteps

    def _init_sigma_tables(self):
        cfg = self.config
        if cfg.trained_betas is not None:
            raise NotImplementedError('trained_betas is not on the hot path')
        T = cfg.num_train_timesteps
        self._init_tables(T, cfg.beta_start, cfg.beta_end, cfg.beta_schedule,
                          _betas_for_alpha_bar(T) if cfg.beta_schedule == 'squaredcos_cap_v2' else None)
        self.num_inference_steps = None
        self.is_scale_input_called = False
        self._warned = False
        self._ring, self._turn = [None] * (self.order + 1), 0
        self._x0 = self._scaled = self._deriv = None

    def _train_sigmas(self):
        """((1 - alphas_cumprod) / alphas_cumprod) ** 0.5 as an fp32 numpy array, ascending."""
        return _rounded_once(torch.sqrt, (1 - self.alphas_cumprod) / self.alphas_cumprod).numpy()

    def _log(self, a):
        """np.log of an fp32 array or scalar, rounded once from fp64."""
        return np.log(np.asarray(a, np.float64)).astype(np.float32)

    def _karras(self, sigmas, log_sigmas, num_inference_steps):
        sigmas = self._convert_to_karras(in_sigmas=sigmas, num_inference_steps=num_inference_steps)
        return sigmas, np.array([self._sigma_to_t(sigma, log_sigmas) for sigma in sigmas])

    def _set_tables(self, timesteps, sigmas, device=None):
        """timesteps: float64, sigmas: fp32 with the trailing 0 (numpy); the host's copies and the index beside the tensors."""
        assert timesteps.dtype == np.float64 and sigmas.dtype == np.float32
        self._sig = torch.from_numpy(sigmas)                          # on the host: a step's scalars are 0-d views of it
        self.sigmas = self._sig.to(device=device)
        self.timesteps = torch.from_numpy(timesteps).to(device=device)
        self._ts = [float(v) for v in timesteps]                      # what `step` and `scale_model_input` look timesteps up in
        self._index = {}
        for i, v in enumerate(self._ts):
            self._index.setdefault(v, []).append(i)

    def _matches(self, timestep):
        """The table indices of a timestep: a Python number or a 0-d / 1-element tensor."""
        if torch.is_tensor(timestep) and timestep.numel() != 1:
            raise ValueError('timestep must be a number or a tensor with one element, got shape %s' % (tuple(timestep.shape),))
        at = self._index.get(float(timestep))
        if not at:
            raise ValueError('timestep %r is not one of `scheduler.timesteps`' % (float(timestep),))
        return at

    def index_for_timestep(self, timestep):
        at = self._matches(timestep)
        if len(at) != 1:
            raise ValueError('timestep %r is in `scheduler.timesteps` %d times' % (float(timestep), len(at)))
        return at[0]

    def _refuse_integers(self, timestep):
        if isinstance(timestep, int) or (torch.is_tensor(timestep) and timestep.dtype in (torch.int32, torch.int64)):
            raise ValueError('Passing integer indices (e.g. from `enumerate(timesteps)`) as timesteps to `EulerDiscreteScheduler.step()` '
                             'is not supported. Make sure to pass one of the `scheduler.timesteps` as a timestep.')

    def _prediction(self):
        pt = self.config.prediction_type
        if pt == 'sample':
            raise NotImplementedError('prediction_type not implemented yet: sample')
        if pt not in self._PRED:
            raise ValueError('prediction_type given as %s must be one of `epsilon`, or `v_prediction`' % pt)
        return self._PRED[pt]

    def _begin_step(self, model_output, sample):
        if model_output.shape[1] != sample.shape[1]:
            raise NotImplementedError('learned-variance models are not part of this path')
        if self._WARNS_UNSCALED and not self.is_scale_input_called and not self._warned:
            import warnings
            self._warned = True
            warnings.warn('The `scale_model_input` function should be called before `step` to ensure correct denoising.')

    @staticmethod
    def _sqrt(v):
        return _rounded_once(torch.sqrt, v)

    def _v_coefs(self, c, sigma):
        if self.config.prediction_type == 'v_prediction':
            c['c_out'], c['c_den'] = -sigma / self._sqrt(sigma ** 2 + 1), sigma ** 2 + 1
        return c

    @staticmethod
    def _fits(buf, like):
        return buf is not None and buf.shape == like.shape and buf.device == like.device and buf.dtype == like.dtype

    def _own(self, name, like):
        buf = getattr(self, name)
        if not self._fits(buf, like):
            buf = torch.empty_like(like, memory_format=torch.contiguous_format)
            setattr(self, name, buf)
        return buf

    def _next_buffer(self, like, *keep):
        """The ring buffer that takes this step's prev_sample: never one that `keep` (the sample, Heun's saved sample) lives in."""
        held = {t.data_ptr() for t in keep if t is not None}
        for _ in range(len(self._ring)):
            self._turn = (self._turn + 1) % len(self._ring)
            buf = self._ring[self._turn]
            if not self._fits(buf, like):
                buf = self._ring[self._turn] = torch.empty_like(like, memory_format=torch.contiguous_format)
            if buf.data_ptr() not in held:
                return buf
        raise RuntimeError('no free output buffer: not a state that `step` reaches')

    def _draw(self, model_output, generator, needed):
        """The reference's randn_tensor(model_output.shape, dtype, device, generator), so that a generator's stream advances as the
        reference's does; a draw that no kernel reads is made where the generator lives and not uploaded."""
        e = model_output
        if not needed and generator is not None and e.device.type != 'cpu':
            g = generator[0] if isinstance(generator, list) else generator
            if g.device.type == 'cpu':
                randn_tensor(e.shape, generator=generator, device='cpu', dtype=e.dtype)
                return None
        z = randn_tensor(e.shape, generator=generator, device=e.device, dtype=e.dtype)
        return z.contiguous() if needed else None

    def scale_model_input(self, sample, timestep):
        """sample / ((sigma**2 + 1) ** 0.5) into a buffer of this scheduler's own: one launch."""
        sigma = self._sig[self.index_for_timestep(timestep)]
        out = ops.sigma_scale(sample.contiguous(), float(self._sqrt(sigma ** 2 + 1)), out=self._own('_scaled', sample))
        self.is_scale_input_called = True
        return out

    def add_noise(self, original_samples, noise, timesteps):
        """original_samples + noise * sigma, one sigma per image looked up on the host."""
        if original_samples.device.type != 'cuda':
            raise RuntimeError('add_noise runs on the HIP kernels: tensors must live on a cuda device')
        sig = self.noise_sigmas(timesteps)
        if len(sig) != original_samples.shape[0]:
            raise ValueError('add_noise: %d timesteps for %d images' % (len(sig), original_samples.shape[0]))
        return ops.sigma_add_noise(original_samples.contiguous(), noise.contiguous(), sig.to(original_samples.device))

    def noise_sigmas(self, timesteps):
        """The sigma of every timestep of `timesteps` (a tensor or a list), looked up on the host: an fp32 host tensor."""
        ts = timesteps.reshape(-1).tolist() if torch.is_tensor(timesteps) else list(timesteps)
        return self._sig[[self.index_for_timestep(t) for t in ts]].contiguous()


class _EulerTables(_SigmaSchedulerBase):
    """The tables the two Euler classes share: the constructor's (all training timesteps, `init_noise_sigma` from them and not
    updated afterwards) and `set_timesteps` (the ancestral class has neither `interpolation_type` nor `use_karras_sigmas`)."""

    def _init_euler(self):
        self._init_sigma_tables()
        T = self.config.num_train_timesteps
        sigmas = np.concatenate([self._train_sigmas()[::-1], [0.0]]).astype(np.float32)
        self._set_tables(np.linspace(0, T - 1, T, dtype=float)[::-1].copy(), sigmas)
        self.init_noise_sigma = self.sigmas.max()
        self.use_karras_sigmas = getattr(self.config, 'use_karras_sigmas', False)

    def set_timesteps(self, num_inference_steps, device=None):
        """scheduling_euler_discrete.py:182-218 with the reference's numpy expressions."""
        cfg = self.config
        interpolation = getattr(cfg, 'interpolation_type', 'linear')
        if interpolation not in ('linear', 'log_linear'):
            raise ValueError("%s is not implemented. Please specify interpolation_type to either 'linear' or 'log_linear'" % interpolation)
        self.num_inference_steps = num_inference_steps
        timesteps = np.linspace(0, cfg.num_train_timesteps - 1, num_inference_steps, dtype=float)[::-1].copy()
        sigmas = self._train_sigmas()
        log_sigmas = self._log(sigmas)
        if interpolation == 'linear':
            sigmas = np.interp(timesteps, np.arange(0, len(sigmas)), sigmas)
        else:                                                         # n + 1 sigmas for n timesteps, as the reference has it
            ramp = torch.linspace(float(self._log(sigmas[-1])), float(self._log(sigmas[0])), num_inference_steps + 1)
            sigmas = _rounded_once(torch.exp, ramp).numpy()
        if self.use_karras_sigmas:
            sigmas, timesteps = self._karras(sigmas, log_sigmas, num_inference_steps)
        self._set_tables(timesteps, np.concatenate([sigmas, [0.0]]).astype(np.float32), device)


class EulerDiscreteScheduler(_EulerTables):
    """scheduling_euler_discrete.py:79-383, Algorithm 2 of Karras et al. (2022) with its churn, for epsilon, `v_prediction` and `sample`
    models, `interpolation_type` linear / log_linear (whose table has n + 2 entries for n timesteps, as the reference's has) and
    `use_karras_sigmas`.  One launch of dp_sigma_step per `step`.  `init_noise_sigma` is the training table's maximum and is not
    updated by `set_timesteps`.  The noise is drawn on every step, as the reference draws it; without churn it is not used.
    With churn and `v_prediction` the conversion uses sigma, not sigma_hat, as the reference does.
    Not carried (NotImplementedError): `trained_betas`, models that predict a variance."""
    _CONFIG_KEYS = ('num_train_timesteps', 'beta_start', 'beta_end', 'beta_schedule', 'trained_betas', 'prediction_type',
                    'interpolation_type', 'use_karras_sigmas')
    _PRED = dict(_SigmaSchedulerBase._PRED, sample=ops.SIGMA_SAMPLE, original_sample=ops.SIGMA_SAMPLE)

    def __init__(self, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule='linear', trained_betas=None,
                 prediction_type='epsilon', interpolation_type='linear', use_karras_sigmas=False):
        self.config = SimpleNamespace(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                                      beta_schedule=beta_schedule, trained_betas=trained_betas, prediction_type=prediction_type,
                                      interpolation_type=interpolation_type, use_karras_sigmas=use_karras_sigmas)
        self._init_euler()

    def step_coefs(self, index, gamma=0.0, s_noise=1.0):
        """The fp32 scalars of :317-347 as ops.sigma_step names them, for table index `index`."""
        sigma = self._sig[index]
        sigma_hat = sigma * (gamma + 1)
        c = dict(sig=sigma_hat, dt=self._sig[index + 1] - sigma_hat)
        if gamma > 0:
            c['k'], c['s_noise'] = self._sqrt(sigma_hat ** 2 - sigma ** 2), torch.tensor(s_noise, dtype=torch.float32)
        return {k: float(v) for k, v in self._v_coefs(c, sigma).items()}

    def step(self, model_output, timestep, sample, s_churn=0.0, s_tmin=0.0, s_tmax=float('inf'), s_noise=1.0, generator=None,
             return_dict=True):
        self._refuse_integers(timestep)
        pt = self.config.prediction_type
        if pt not in self._PRED:
            raise ValueError('prediction_type given as %s must be one of `epsilon`, or `v_prediction`' % pt)
        self._begin_step(model_output, sample)
        i = self.index_for_timestep(timestep)
        sigma = self._sig[i]
        gamma = min(s_churn / (len(self._sig) - 1), 2 ** 0.5 - 1) if s_tmin <= sigma <= s_tmax else 0.0
        noise = self._draw(model_output, generator, gamma > 0)
        prev, x0 = ops.sigma_step(sample.contiguous(), model_output.contiguous(), self.step_coefs(i, gamma, s_noise), ops.SIGMA_EULER,
                                  self._PRED[pt], noise=noise, out=self._next_buffer(sample, sample), aux_out=self._own('_x0', sample))
        if not return_dict:
            return (prev,)
        return EulerDiscreteSchedulerOutput(prev_sample=prev, pred_original_sample=x0)


class EulerAncestralDiscreteScheduler(_EulerTables):
    """scheduling_euler_ancestral_discrete.py:79-309: ancestral sampling with Euler steps for epsilon and `v_prediction` models; the
    noise is drawn after the update, as the reference draws it.  One launch of dp_sigma_step per `step`.
    Not carried: `trained_betas`, models that predict a variance (NotImplementedError); `sample` models (the reference's
    NotImplementedError from `step`)."""
    _CONFIG_KEYS = ('num_train_timesteps', 'beta_start', 'beta_end', 'beta_schedule', 'trained_betas', 'prediction_type')

    def __init__(self, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule='linear', trained_betas=None,
                 prediction_type='epsilon'):
        self.config = SimpleNamespace(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                                      beta_schedule=beta_schedule, trained_betas=trained_betas, prediction_type=prediction_type)
        self._init_euler()

    def step_coefs(self, index):
        """The fp32 scalars of :243-266 as ops.sigma_step names them, and `sigma_down`, which only the host reads."""
        sigma_from, sigma_to = self._sig[index], self._sig[index + 1]
        sigma_up = self._sqrt(sigma_to ** 2 * (sigma_from ** 2 - sigma_to ** 2) / sigma_from ** 2)
        sigma_down = self._sqrt(sigma_to ** 2 - sigma_up ** 2)
        c = dict(sig=sigma_from, dt=sigma_down - sigma_from, sigma_up=sigma_up, sigma_down=sigma_down)
        return {k: float(v) for k, v in self._v_coefs(c, sigma_from).items()}

    def step(self, model_output, timestep, sample, generator=None, return_dict=True):
        self._refuse_integers(timestep)
        pred = self._prediction()
        self._begin_step(model_output, sample)
        c = self.step_coefs(self.index_for_timestep(timestep))
        del c['sigma_down']
        noise = self._draw(model_output, generator, True)
        prev, x0 = ops.sigma_step(sample.contiguous(), model_output.contiguous(), c, ops.SIGMA_ANCESTRAL, pred, noise=noise,
                                  out=self._next_buffer(sample, sample), aux_out=self._own('_x0', sample))
        if not return_dict:
            return (prev,)
        return EulerAncestralDiscreteSchedulerOutput(prev_sample=prev, pred_original_sample=x0)


class HeunDiscreteScheduler(_SigmaSchedulerBase):
    """scheduling_heun_discrete.py:53-351, Algorithm 1 of Karras et al. (2022) without churn, for epsilon and `v_prediction` models:
    two model calls per step but the last, so both tables are doubled (2n - 1 timesteps, 2n sigmas).  `state_in_first_order`,
    `prev_derivative`, `dt` and `sample` are kept as the reference keeps them; the sample of the first call is held by reference, not
    copied.  One launch of dp_sigma_step per `step`.  `init_noise_sigma` follows `set_timesteps`.
    Not carried: `trained_betas`, models that predict a variance (NotImplementedError); `sample` models (the reference's
    NotImplementedError from `step`)."""
    _CONFIG_KEYS = ('num_train_timesteps', 'beta_start', 'beta_end', 'beta_schedule', 'trained_betas', 'prediction_type',
                    'use_karras_sigmas')
    order = 2
    _WARNS_UNSCALED = False

    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule='linear', trained_betas=None,
                 prediction_type='epsilon', use_karras_sigmas=False):
        self.config = SimpleNamespace(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                                      beta_schedule=beta_schedule, trained_betas=trained_betas, prediction_type=prediction_type,
                                      use_karras_sigmas=use_karras_sigmas)
        self._init_sigma_tables()
        self.use_karras_sigmas = use_karras_sigmas    # (the reference's constructor reads it from the config before it is set)
        self.set_timesteps(num_train_timesteps)

    def set_timesteps(self, num_inference_steps, device=None):
        """:150-197 with the reference's numpy expressions; the running values reset."""
        self.num_inference_steps = num_inference_steps
        timesteps = np.linspace(0, self.config.num_train_timesteps - 1, num_inference_steps, dtype=float)[::-1].copy()
        sigmas = self._train_sigmas()
        log_sigmas = self._log(sigmas)
        sigmas = np.interp(timesteps, np.arange(0, len(sigmas)), sigmas)
        if self.use_karras_sigmas:
            sigmas, timesteps = self._karras(sigmas, log_sigmas, num_inference_steps)
        sigmas = np.concatenate([sigmas, [0.0]]).astype(np.float32)
        sigmas = np.concatenate([sigmas[:1], sigmas[1:-1].repeat(2), sigmas[-1:]])
        timesteps = np.concatenate([timesteps[:1], timesteps[1:].repeat(2)])
        self._set_tables(timesteps, sigmas, device)
        self.init_noise_sigma = self.sigmas.max()
        self.prev_derivative = self.dt = self.sample = None

    @property
    def state_in_first_order(self):
        return self.dt is None

    def index_for_timestep(self, timestep):
        """The last match in first-order state, the first otherwise (:119-129)."""
        return self._matches(timestep)[-1 if self.state_in_first_order else 0]

    def step_coefs(self, index):
        """The fp32 scalars of :263-309 as ops.sigma_step names them, for the state the scheduler is in."""
        if self.state_in_first_order:
            sigma, sigma_next = self._sig[index], self._sig[index + 1]
        else:
            sigma, sigma_next = self._sig[index - 1], self._sig[index]
        sigma_hat = sigma * (0 + 1)
        sigma_input = sigma_hat if self.state_in_first_order else sigma_next
        c = dict(sig=sigma_input, dt=sigma_next - sigma_hat if self.state_in_first_order else self.dt)
        return {k: float(v) for k, v in self._v_coefs(c, sigma_input).items()}

    def step(self, model_output, timestep, sample, return_dict=True):
        pred = self._prediction()
        self._begin_step(model_output, sample)
        c = self.step_coefs(self.index_for_timestep(timestep))
        x, e = sample.contiguous(), model_output.contiguous()
        if self.state_in_first_order:
            prev, d = ops.sigma_step(x, e, c, ops.SIGMA_HEUN1, pred, out=self._next_buffer(sample, sample), aux_out=self._own('_deriv', sample))
            self.prev_derivative, self.dt, self.sample = d, torch.tensor(c['dt'], dtype=torch.float32), sample
        else:
            prev, _ = ops.sigma_step(x, e, c, ops.SIGMA_HEUN2, pred, d1=self.prev_derivative, saved=self.sample.contiguous(),
                                     out=self._next_buffer(sample, sample, self.sample))
            self.prev_derivative = self.dt = self.sample = None
        if not return_dict:
            return (prev,)
        return SchedulerOutput(prev_sample=prev)


@dataclass
class LMSDiscreteSchedulerOutput:
    prev_sample: torch.Tensor
    pred_original_sample: torch.Tensor = None


class LMSDiscreteScheduler(_SigmaSchedulerBase):
    """scheduling_lms_discrete.py:77-364: the linear multistep method of k-diffusion for epsilon, `v_prediction` and `sample` models,
    with `use_karras_sigmas`.  One launch of dp_lms_step per `step`: the conversion, the derivative, the sum over up to `order`
    derivatives and the update.  `derivatives` is the reference's list, oldest first, over at most four buffers of the scheduler's
    own: the new derivative takes the slot of the one dropped.  `init_noise_sigma` is the training table's maximum and is not updated
    by `set_timesteps`.
    The coefficients are the reference's in bits: the same `scipy.integrate.quad(..., epsrel=1e-4)` over the same integrand of 0-d
    fp32 tensors (which is not the exact integral of the polynomial: it differs around the eighth digit), each rounded to fp32 once,
    as torch rounds a Python float that multiplies an fp32 tensor.  They are kept per (order, index) until the next `set_timesteps`;
    the reference integrates again on every step.
    Not carried (NotImplementedError): `trained_betas`, models that predict a variance, `order` above 4."""
    _CONFIG_KEYS = ('num_train_timesteps', 'beta_start', 'beta_end', 'beta_schedule', 'trained_betas', 'use_karras_sigmas',
                    'prediction_type')
    _PRED = {'epsilon': ops.KDIFF_EPSILON, 'v_prediction': ops.KDIFF_V, 'sample': ops.KDIFF_SAMPLE}
    MAX_ORDER = 4

    def __init__(self, num_train_timesteps=1000, beta_start=0.0001, beta_end=0.02, beta_schedule='linear', trained_betas=None,
                 use_karras_sigmas=False, prediction_type='epsilon'):
        self.config = SimpleNamespace(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                                      beta_schedule=beta_schedule, trained_betas=trained_betas, use_karras_sigmas=use_karras_sigmas,
                                      prediction_type=prediction_type)
        self._init_sigma_tables()
        self.init_noise_sigma = torch.from_numpy(self._train_sigmas()).max()
        self.use_karras_sigmas = use_karras_sigmas
        self.set_timesteps(num_train_timesteps, None)

    def set_timesteps(self, num_inference_steps, device=None):
        """:196-227 with the reference's numpy expressions; the derivatives and the kept coefficients reset."""
        self.num_inference_steps = num_inference_steps
        timesteps = np.linspace(0, self.config.num_train_timesteps - 1, num_inference_steps, dtype=float)[::-1].copy()
        sigmas = self._train_sigmas()
        log_sigmas = self._log(sigmas)
        sigmas = np.interp(timesteps, np.arange(0, len(sigmas)), sigmas)
        if self.use_karras_sigmas:
            sigmas, timesteps = self._karras(sigmas, log_sigmas, num_inference_steps)
        self._set_tables(timesteps, np.concatenate([sigmas, [0.0]]).astype(np.float32), device)
        self.derivatives = []
        self._lms = {}

    def get_lms_coefficient(self, order, t, current_order):
        """:174-194: the integral of the Lagrange basis polynomial `current_order` of `order` nodes over [sigma_t, sigma_t+1], as
        the reference's adaptive quadrature returns it (a Python float).  tau - sigma rounds tau to fp32: the integrand is fp32."""
        from scipy import integrate
        sig = self._sig

        def lms_derivative(tau):
            prod = 1.0
            for k in range(order):
                if current_order == k:
                    continue
                prod *= (tau - sig[t - k]) / (sig[t - current_order] - sig[t - k])
            return prod
        return integrate.quad(lms_derivative, sig[t], sig[t + 1], epsrel=1e-4)[0]

    def lms_coefficients(self, order, index):
        """The `order` coefficients of table index `index`, newest derivative first, each rounded to fp32 once; integrated once."""
        got = self._lms.get((order, index))
        if got is None:
            got = self._lms[(order, index)] = tuple(float(np.float32(self.get_lms_coefficient(order, index, k))) for k in range(order))
        return got

    def step_coefs(self, index, order=4, terms=None):
        """The fp32 scalars of :302-330 as ops.lms_step names them: the first `terms` coefficients of order min(index + 1, order)."""
        sigma = self._sig[index]
        c = {k: float(v) for k, v in self._v_coefs(dict(sig=sigma), sigma).items()}
        coefs = self.lms_coefficients(min(index + 1, order), index)
        for k, v in enumerate(coefs[:len(coefs) if terms is None else terms]):
            c['c%d' % k] = v
        return c

    def step(self, model_output, timestep, sample, order=4, return_dict=True):
        pt = self.config.prediction_type
        if pt not in self._PRED:
            raise ValueError('prediction_type given as %s must be one of `epsilon`, or `v_prediction`' % pt)
        if order > self.MAX_ORDER:
            raise NotImplementedError('order %d: the step kernel carries at most %d derivatives' % (order, self.MAX_ORDER))
        if order < 1:
            raise ValueError('order must be at least 1, got %r' % (order,))
        self._begin_step(model_output, sample)
        i = self.index_for_timestep(timestep)
        history = self.derivatives[::-1]                              # newest first
        # the reference appends the new derivative and then drops the oldest of more than `order`: the kernel does not read that one
        slot = self.derivatives.pop(0) if len(self.derivatives) + 1 > order else None
        if not self._fits(slot, sample):
            slot = torch.empty_like(sample, memory_format=torch.contiguous_format)
        terms = min(i + 1, order, len(self.derivatives) + 1)          # zip() in the reference stops at the shorter list
        prev, d, x0 = ops.lms_step(sample.contiguous(), model_output.contiguous(), self.step_coefs(i, order, terms), terms, self._PRED[pt],
                                   history=history[:terms - 1], out=self._next_buffer(sample, sample), d_out=slot,
                                   x0_out=self._own('_x0', sample))
        self.derivatives.append(d)
        if not return_dict:
            return (prev,)
        return LMSDiscreteSchedulerOutput(prev_sample=prev, pred_original_sample=x0)


class _KDPM2Tables(_SigmaSchedulerBase):
    """What the two KDPM2 classes share: two model calls per step but the last, so the tables are doubled (2n - 1 timesteps, 2n + 2
    sigmas); every second timestep is the fractional time of an interpolated sigma (`sigmas_interpol`, the geometric mean of two
    neighbours: log, lerp at 0.5 and exp in fp32 torch as the reference has them, log and exp rounded once), found by `sigma_to_t`,
    the reference's fp32 torch search of the training table.  `sample` is the sample of the first-order call, held by reference;
    `state_in_first_order` is `sample is None`.  One launch of dp_kdpm2_step per `step`.  `init_noise_sigma` follows
    `set_timesteps`.  The tables keep the reference's entries that are never read (a NaN among them)."""
    order = 2
    _WARNS_UNSCALED = False
    _PRED = {'epsilon': ops.KDIFF_EPSILON, 'v_prediction': ops.KDIFF_V}
    _CONFIG_KEYS = ('num_train_timesteps', 'beta_start', 'beta_end', 'beta_schedule', 'trained_betas', 'prediction_type')

    def __init__(self, num_train_timesteps=1000, beta_start=0.00085, beta_end=0.012, beta_schedule='linear', trained_betas=None,
                 prediction_type='epsilon'):
        self.config = SimpleNamespace(num_train_timesteps=num_train_timesteps, beta_start=beta_start, beta_end=beta_end,
                                      beta_schedule=beta_schedule, trained_betas=trained_betas, prediction_type=prediction_type)
        self._init_sigma_tables()
        self.set_timesteps(num_train_timesteps, None, num_train_timesteps)

    @staticmethod
    def _tlog(t):
        return _rounded_once(torch.log, t)

    @staticmethod
    def _geometric_mean(a, b):
        """a.log().lerp(b.log(), 0.5).exp(): at weight 0.5 torch's lerp takes its `b - (b - a) * (1 - w)` branch."""
        la, lb = _KDPM2Tables._tlog(a), _KDPM2Tables._tlog(b)
        return _rounded_once(torch.exp, lb - (lb - la) * 0.5)

    @staticmethod
    def _doubled(t):
        return torch.cat([t[:1], t[1:].repeat_interleave(2), t[-1:]])

    def sigma_to_t(self, sigma):
        """The reference's fp32 torch search: the fractional index at which log sigma lies between two neighbours of the table."""
        log_sigmas = self._log_sigmas
        log_sigma = self._tlog(sigma)
        dists = log_sigma - log_sigmas[:, None]
        low_idx = dists.ge(0).cumsum(dim=0).argmax(dim=0).clamp(max=log_sigmas.shape[0] - 2)
        high_idx = low_idx + 1
        low, high = log_sigmas[low_idx], log_sigmas[high_idx]
        w = ((low - log_sigma) / (low - high)).clamp(0, 1)
        t = (1 - w) * low_idx + w * high_idx
        return t.view(sigma.shape)

    def set_timesteps(self, num_inference_steps, device=None, num_train_timesteps=None):
        self.num_inference_steps = num_inference_steps
        T = num_train_timesteps or self.config.num_train_timesteps
        timesteps = np.linspace(0, T - 1, num_inference_steps, dtype=float)[::-1].copy()
        sigmas = self._train_sigmas()
        self._log_sigmas = torch.from_numpy(self._log(sigmas))
        self.log_sigmas = self._log_sigmas.to(device)
        sigmas = np.interp(timesteps, np.arange(0, len(sigmas)), sigmas)
        sigmas = torch.from_numpy(np.concatenate([sigmas, [0.0]]).astype(np.float32))
        sigmas_interpol, used = self._interpolate(sigmas, device)
        self._interpol = self._doubled(sigmas_interpol)               # on the host, as `_sig`
        self.sigmas_interpol = self._interpol.to(device=device)
        timesteps = torch.from_numpy(timesteps)
        timesteps_interpol = self.sigma_to_t(sigmas_interpol).to(dtype=timesteps.dtype)
        interleaved = torch.stack((timesteps_interpol[used, None], timesteps[1:, None]), dim=-1).flatten()
        self._set_tables(torch.cat([timesteps[:1], interleaved]).numpy(), self._doubled(sigmas).numpy(), device)
        self.init_noise_sigma = self.sigmas.max()
        self.sample = None

    @property
    def state_in_first_order(self):
        return self.sample is None

    def index_for_timestep(self, timestep):
        """The last match in first-order state, the first otherwise: the timestep table holds equal pairs."""
        return self._matches(timestep)[-1 if self.state_in_first_order else 0]

    def scale_model_input(self, sample, timestep):
        i = self.index_for_timestep(timestep)
        sigma = self._sig[i] if self.state_in_first_order else self._interpol[i + self._SCALE_AT]
        return ops.sigma_scale(sample.contiguous(), float(self._sqrt(sigma ** 2 + 1)), out=self._own('_scaled', sample))

    def _step(self, model_output, timestep, sample, noise_of, return_dict):
        pred = self._prediction()
        self._begin_step(model_output, sample)
        i = self.index_for_timestep(timestep)
        first = self.state_in_first_order
        noise = noise_of(not first)
        c = self.step_coefs(i)
        x, e = sample.contiguous(), model_output.contiguous()
        if first:
            prev = ops.kdpm2_step(x, e, c, pred, out=self._next_buffer(sample, sample))
            self.sample = sample
        else:
            prev = ops.kdpm2_step(x, e, c, pred, saved=self.sample.contiguous(), noise=noise,
                                  out=self._next_buffer(sample, sample, self.sample))
            self.sample = None
        if not return_dict:
            return (prev,)
        return SchedulerOutput(prev_sample=prev)


class KDPM2DiscreteScheduler(_KDPM2Tables):
    """scheduling_k_dpm_2_discrete.py:53-340: DPM-Solver-2 in the form of Algorithm 2 of Karras et al. (2022) without churn, for
    epsilon and `v_prediction` models.  The first call of a pair steps to the interpolated sigma, the second from the saved sample
    to the next sigma with the derivative taken there.  `sigmas_interpol[0]` is NaN, as the reference's is (a lerp towards log 0);
    it is never read.
    Not carried: `trained_betas`, models that predict a variance (NotImplementedError); `sample` models (the reference's
    NotImplementedError from `step`)."""
    _SCALE_AT = 0

    def _interpolate(self, sigmas, device):
        """:180-201: (sigmas_interpol, the entries of it whose times are interleaved into `timesteps`)."""
        return self._geometric_mean(sigmas, sigmas.roll(1)), slice(1, -1)

    def step_coefs(self, index):
        """The fp32 scalars of :254-305 as ops.kdpm2_step names them, for the state the scheduler is in."""
        if self.state_in_first_order:
            sigma, sigma_interpol = self._sig[index], self._interpol[index + 1]
            sigma_input, dt = sigma * (0 + 1), sigma_interpol - sigma * (0 + 1)
        else:
            sigma, sigma_interpol, sigma_next = self._sig[index - 1], self._interpol[index], self._sig[index]
            sigma_input, dt = sigma_interpol, sigma_next - sigma * (0 + 1)
        return {k: float(v) for k, v in self._v_coefs(dict(sig=sigma_input, dt=dt), sigma_input).items()}

    def step(self, model_output, timestep, sample, return_dict=True):
        return self._step(model_output, timestep, sample, lambda needed: None, return_dict)


class KDPM2AncestralDiscreteScheduler(_KDPM2Tables):
    """scheduling_k_dpm_2_ancestral_discrete.py:54-358: KDPM2 with ancestral noise, for epsilon and `v_prediction` models.  The
    interpolated sigma lies between sigma and `sigmas_down`; the second call of a pair steps from the saved sample to sigma_down and
    adds noise * sigma_up.  The noise is drawn on every call, as the reference draws it, and uploaded for the second call of a pair
    only.  The timestep table holds equal or nearly equal pairs, so the lookup goes by the state.
    Not carried: `trained_betas`, models that predict a variance (NotImplementedError); `sample` models (the reference's
    NotImplementedError from `step`)."""
    _SCALE_AT = -1

    def _interpolate(self, sigmas, device):
        """:181-210: sigmas_up and sigmas_down beside sigmas_interpol."""
        sigmas_next = sigmas.roll(-1)
        sigmas_next[-1] = 0.0
        sigmas_up = self._sqrt(sigmas_next ** 2 * (sigmas ** 2 - sigmas_next ** 2) / sigmas ** 2)
        sigmas_down = self._sqrt(sigmas_next ** 2 - sigmas_up ** 2)
        sigmas_down[-1] = 0.0
        sigmas_interpol = self._geometric_mean(sigmas, sigmas_down)
        sigmas_interpol[-2:] = 0.0
        self._up, self._down = self._doubled(sigmas_up), self._doubled(sigmas_down)
        self.sigmas_up, self.sigmas_down = self._up.to(device=device), self._down.to(device=device)
        return sigmas_interpol, slice(None, -2)

    def step_coefs(self, index):
        """The fp32 scalars of :266-324 as ops.kdpm2_step names them, for the state the scheduler is in."""
        if self.state_in_first_order:
            sigma, sigma_interpol = self._sig[index], self._interpol[index]
            c = dict(sig=sigma * (0 + 1), dt=sigma_interpol - sigma * (0 + 1))
        else:
            sigma, sigma_interpol = self._sig[index - 1], self._interpol[index - 1]
            c = dict(sig=sigma_interpol, dt=self._down[index - 1] - sigma * (0 + 1), sigma_up=self._up[index - 1])
        return {k: float(v) for k, v in self._v_coefs(c, c['sig']).items()}

    def step(self, model_output, timestep, sample, generator=None, return_dict=True):
        return self._step(model_output, timestep, sample, lambda needed: self._draw(model_output, generator, needed), return_dict)


@dataclass
class ImagePipelineOutput:
    images: object


class _PipelineBase:
    def __init__(self, unet, scheduler):
        self.unet, self.scheduler = unet, scheduler
        self._progress_bar_config = {}

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, **kwargs):
        """A local Diffusers pipeline directory (model_index.json, unet/, scheduler/); there is no hub access."""
        from . import checkpoint
        return checkpoint.load_pipeline(cls, pretrained_model_name_or_path)

    def save_pretrained(self, save_directory, safe_serialization=False):
        from . import checkpoint
        checkpoint.save_pipeline(self, save_directory, safe_serialization)

    def set_progress_bar_config(self, **kwargs):
        self._progress_bar_config = kwargs

    @property
    def device(self):
        return self.unet.device

    def to(self, device):
        self.unet.to(device)
        return self

    def progress_bar(self, it):
        cfg = getattr(self, '_progress_bar_config', {})
        if cfg.get('disable', True):               # quiet unless asked for (pipeline_utils.py progress_bar + tqdm)
            return it
        from tqdm import tqdm
        return tqdm(it, **cfg)

    @staticmethod
    def numpy_to_pil(images):
        from PIL import Image
        arr = (images * 255).round().astype('uint8')
        return [Image.fromarray(a) for a in arr]


def _sampling_forward(unet, shape, n_calls):
    """`f(sample, t) -> eps` for a sampling loop: the model's own captured / pinned forward (UNet2DModel.sampling_forward) or, for
    a foreign model object, a plain call."""
    sf = getattr(unet, 'sampling_forward', None)
    if sf is not None:
        return sf(shape, n_calls)

    class _Plain:
        def __call__(self, sample, t):
            return unet(sample, t).sample

        def close(self):
            pass
    return _Plain()


def _image_shape(unet, batch_size):
    ss = unet.config.sample_size
    return (batch_size, unet.config.in_channels) + ((ss, ss) if isinstance(ss, int) else tuple(ss))


def _to_output(pipe, image, output_type, return_dict):
    image = (image / 2 + 0.5).clamp(0, 1)
    image = image.cpu().permute(0, 2, 3, 1).numpy()
    if output_type == 'pil':
        image = pipe.numpy_to_pil(image)
    if not return_dict:
        return (image,)
    return ImagePipelineOutput(images=image)


class DDPMPipeline(_PipelineBase):
    """pipelines/ddpm/pipeline_ddpm.py:24-105: ancestral sampling, one UNet forward + one dp_ddpm_step per timestep.
    Also the holder the prune / finetune scripts read `pipeline.unet` / `pipeline.scheduler` from (ddpm_prune.py:50-52)."""

    @torch.no_grad()
    def __call__(self, batch_size=1, generator=None, num_inference_steps=1000, output_type='pil', return_dict=True):
        if getattr(self.scheduler, 'sigma_space', False):
            # the reference would sample without scale_model_input and without init_noise_sigma here, and only warn
            raise ValueError('%s carries the sample at scale sigma: DDPMPipeline neither scales the model input nor starts from '
                             'init_noise_sigma.  Use LDMPipeline, or the explicit loop over unet.sampling_forward: '
                             'scale_model_input, the model, step (README.md)' % type(self.scheduler).__name__)
        shape = _image_shape(self.unet, batch_size)
        image = randn_tensor(shape, generator=generator, device=self.device)
        self.scheduler.set_timesteps(num_inference_steps)
        ts = [int(t) for t in self.scheduler.timesteps.tolist()]              # one read-back instead of one per step
        import inspect                                      # a deterministic scheduler's step (UniPC) takes no generator
        params = inspect.signature(self.scheduler.step).parameters
        takes = 'generator' in params or any(p.kind is p.VAR_KEYWORD for p in params.values())
        extra = {'generator': generator} if takes else {}
        fwd = _sampling_forward(self.unet, shape, len(ts))  # weights pinned; the forward replayed natively where it pays
        try:
            for t in self.progress_bar(ts):
                model_output = fwd(image, t)
                image = self.scheduler.step(model_output, t, image, **extra).prev_sample
        finally:
            fwd.close()
        return _to_output(self, image, output_type, return_dict)


class DDIMPipeline(_PipelineBase):
    def __init__(self, unet, scheduler):
        # pipeline_ddim.py:40: the scheduler is re-created from its config, so skip_type must be set afterwards
        if not isinstance(scheduler, DDIMScheduler):
            scheduler = DDIMScheduler.from_config(scheduler.config)
        super().__init__(unet, scheduler)

    @torch.no_grad()
    def __call__(self, batch_size=1, generator=None, eta=0.0, num_inference_steps=50, use_clipped_model_output=None,
                 output_type='pil', return_dict=True):
        shape = _image_shape(self.unet, batch_size)
        if isinstance(generator, list) and len(generator) != batch_size:
            raise ValueError('You have passed a list of generators of length %d, but requested an effective batch size of %d.'
                             % (len(generator), batch_size))
        image = randn_tensor(shape, generator=generator, device=self.device, dtype=self.unet.dtype)
        self.scheduler.set_timesteps(num_inference_steps)
        ts = [int(t) for t in self.scheduler.timesteps.tolist()]
        extra = {'use_clipped_model_output': True} if use_clipped_model_output else {}      # pipeline_ddim.py:113-115
        fwd = _sampling_forward(self.unet, shape, len(ts))
        try:
            for t in self.progress_bar(ts):
                model_output = fwd(image, t)
                image = self.scheduler.step(model_output, t, image, eta=eta, generator=generator, **extra).prev_sample
        finally:
            fwd.close()
        return _to_output(self, image, output_type, return_dict)


class PNDMPipeline(_PipelineBase):
    """pipelines/pndm/pipeline_pndm.py:26-99: one UNet forward + one dp_pndm_step per entry of the scheduler's timestep list, which
    is longer than `num_inference_steps` (the Runge-Kutta calls, the repeated timestep of `skip_prk_steps`)."""

    def __init__(self, unet, scheduler):
        super().__init__(unet, PNDMScheduler.from_config(scheduler.config))                      # pipeline_pndm.py:43

    @torch.no_grad()
    def __call__(self, batch_size=1, num_inference_steps=50, generator=None, output_type='pil', return_dict=True, **kwargs):
        shape = _image_shape(self.unet, batch_size)
        image = randn_tensor(shape, generator=generator, device=self.device)
        self.scheduler.set_timesteps(num_inference_steps)
        ts = self.scheduler._ts                                               # the host's list: nothing is read back
        fwd = _sampling_forward(self.unet, shape, len(ts))
        try:
            for t in self.progress_bar(ts):
                model_output = fwd(image, t)
                image = self.scheduler.step(model_output, t, image).prev_sample
        finally:
            fwd.close()
        return _to_output(self, image, output_type, return_dict)


def _pil_resample(name):
    from PIL import Image
    return getattr(getattr(Image, 'Resampling', Image), name)


def _preprocess_image(image):
    """pipeline_repaint.py:32-50: a tensor as it is; PIL images resized down to a multiple of 8 (Lanczos), scaled to [-1, 1], NCHW."""
    from PIL import Image
    if isinstance(image, torch.Tensor):
        return image
    if isinstance(image, Image.Image):
        image = [image]
    if isinstance(image[0], Image.Image):
        w, h = image[0].size
        w, h = (x - x % 8 for x in (w, h))
        image = [np.array(i.resize((w, h), resample=_pil_resample('LANCZOS')))[None, :] for i in image]
        image = np.concatenate(image, axis=0)
        image = np.array(image).astype(np.float32) / 255.0
        image = image.transpose(0, 3, 1, 2)
        image = 2.0 * image - 1.0
        image = torch.from_numpy(image)
    elif isinstance(image[0], torch.Tensor):
        image = torch.cat(image, dim=0)
    return image


def _preprocess_mask(mask):
    """pipeline_repaint.py:53-70: a tensor as it is; PIL masks to grey, resized down to a multiple of 32 (nearest), made 0 / 1:
    [N, H, W], which broadcasts against the image batch as [1, N, H, W]."""
    from PIL import Image
    if isinstance(mask, torch.Tensor):
        return mask
    if isinstance(mask, Image.Image):
        mask = [mask]
    if isinstance(mask[0], Image.Image):
        w, h = mask[0].size
        w, h = (x - x % 32 for x in (w, h))
        mask = [np.array(m.convert('L').resize((w, h), resample=_pil_resample('NEAREST')))[None, :] for m in mask]
        mask = np.concatenate(mask, axis=0)
        mask = mask.astype(np.float32) / 255.0
        mask[mask < 0.5] = 0
        mask[mask >= 0.5] = 1
        mask = torch.from_numpy(mask)
    elif isinstance(mask[0], torch.Tensor):
        mask = torch.cat(mask, dim=0)
    return mask


class RePaintPipeline(_PipelineBase):
    """pipelines/repaint/pipeline_repaint.py:73-171: inpainting with an unconditional UNet.  Per entry of the scheduler's timestep
    list either one UNet forward + one dp_repaint_step (the entry lies below the one before it) or one dp_repaint_undo (it lies
    above: a jump back).  The loop runs over the scheduler's host list and reads nothing back; the state is updated in place."""

    @torch.no_grad()
    def __call__(self, image, mask_image, num_inference_steps=250, eta=0.0, jump_length=10, jump_n_sample=10, generator=None,
                 output_type='pil', return_dict=True):
        original_image = _preprocess_image(image).to(device=self.device, dtype=self.unet.dtype).contiguous()
        mask_image = _preprocess_mask(mask_image).to(device=self.device, dtype=self.unet.dtype).contiguous()
        batch_size = original_image.shape[0]
        if isinstance(generator, list) and len(generator) != batch_size:
            raise ValueError('You have passed a list of generators of length %d, but requested an effective batch size of %d. '
                             'Make sure the batch size matches the length of the generators.' % (len(generator), batch_size))
        shape = tuple(original_image.shape)
        image = randn_tensor(shape, generator=generator, device=self.device, dtype=self.unet.dtype)
        self.scheduler.set_timesteps(num_inference_steps, jump_length, jump_n_sample, self.device)
        self.scheduler.eta = eta
        ts = self.scheduler._ts                                               # the host's list: nothing is read back
        n_calls = sum(1 for prev, t in zip([ts[0] + 1] + ts[:-1], ts) if t < prev)
        t_last = ts[0] + 1
        generator = generator[0] if isinstance(generator, list) else generator
        fwd = _sampling_forward(self.unet, shape, n_calls)
        try:
            for t in self.progress_bar(ts):
                if t < t_last:
                    model_output = fwd(image, t)
                    image = self.scheduler.step(model_output, t, image, original_image, mask_image, generator, out=image,
                                                need_x0=False).prev_sample
                else:
                    image = self.scheduler.undo_step(image, t_last, generator, out=image)
                t_last = t
        finally:
            fwd.close()
        return _to_output(self, image, output_type, return_dict)


class LDMPipeline(_PipelineBase):
    """pipelines/latent_diffusion_uncond/pipeline_latent_diffusion_uncond.py:44-111: unconditional latent diffusion -- the
    scheduler loop over the UNet's latents (the captured / pinned forward of `_sampling_forward`), then the VQ first stage's
    decode (vq.VQModel) and the usual [0, 1] image output."""

    def __init__(self, vqvae, unet, scheduler):
        super().__init__(unet, scheduler)
        self.vqvae = vqvae

    def to(self, device):
        self.unet.to(device)
        self.vqvae.to(device)
        return self

    @torch.no_grad()
    def __call__(self, batch_size=1, generator=None, eta=0.0, num_inference_steps=50, output_type='pil', return_dict=True,
                 **kwargs):
        import inspect
        ss = self.unet.config.sample_size
        shape = (batch_size, self.unet.config.in_channels, ss, ss)
        latents = randn_tensor(shape, generator=generator)              # drawn on the host, as the reference does, then moved
        latents = latents.to(self.device)
        if self.scheduler.init_noise_sigma != 1.0:                    # (x 1.0 is the identity)
            latents = latents * self.scheduler.init_noise_sigma
        self.scheduler.set_timesteps(num_inference_steps)
        extra = {'eta': eta} if 'eta' in inspect.signature(self.scheduler.step).parameters else {}
        ts = self.scheduler.host_timesteps()                          # ints as before; the sigma-space schedulers' floats as they are
        fwd = _sampling_forward(self.unet, shape, len(ts))
        try:
            for t in self.progress_bar(ts):
                noise_prediction = fwd(self.scheduler.scale_model_input(latents, t), t)
                latents = self.scheduler.step(noise_prediction, t, latents, **extra).prev_sample
        finally:
            fwd.close()
        image = self.vqvae.decode(latents).sample
        return _to_output(self, image, output_type, return_dict)
