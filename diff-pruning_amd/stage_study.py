"""The stage study of Diff-Pruning (ddpm_exp/prune_ssim.py + compute_pruned_ssim_curve.py + draw_ssim_pruned_curve.py): for every
stage s the Taylor gradients of the timesteps 0 .. s - 1, a prune from them, samples from one fixed x_T, and the SSIM of those
samples against the unpruned model's -- the curve the method's threshold is read from, beside the relative loss.

The reference runs one process per stage, each with a fresh s-step sweep (10 500 timesteps for the 20 stages of the figure).  The
gradient after s timesteps is a prefix of the gradient after the last stage's, so ONE sweep with a snapshot at every stage boundary
(sweep.taylor_sweep(stages=...), csrc/stage.hip) yields all of them, bit for bit.  The snapshots are consumed after the sweep: each
stage builds a new model, prunes it at its snapshot, samples, and is dropped before the next.  The caller's model is never sliced."""
import os

import torch

from . import data, ddpm_exp_sampler, metrics, ops, pruning, sweep


def prune_at_stage(model, flat_grad, pruning_ratio, importance=None, **prune_args):
    """A new model of `model`'s configuration with `model`'s weights (copied device to device) and the gradients `flat_grad`
    (a flat buffer laid out like sweep.flatten_grads': named_parameters() order), pruned by sweep.prune_model.
    Returns (pruned_model, pruner).  `model` and `flat_grad` are left as they are."""
    params = dict(model.named_parameters())
    if flat_grad.dim() != 1 or flat_grad.numel() != sum(p.numel() for p in params.values()):
        raise ValueError('flat_grad does not lay out the gradients of this model (%d elements)' % flat_grad.numel())
    dev = next(iter(params.values())).device
    new = type(model).from_config(model.config).to(dev)
    new.train(model.training)
    new.dropout_seed = getattr(model, 'dropout_seed', 0)
    if getattr(model, 'attention_scale_from_width', False):      # an original-DDPM model: the pruned q width scales its attention
        new.attention_scale_from_width = True
    mine = dict(new.named_parameters())
    if {n: p.shape for n, p in mine.items()} != {n: p.shape for n, p in params.items()}:
        raise ValueError('the model does not have the shapes of its configuration (already pruned?)')
    _, views = sweep.grad_views(mine)
    off = 0
    with torch.no_grad():
        for n, p in mine.items():
            p.copy_(params[n])
            views[n].copy_(flat_grad[off:off + p.numel()].view_as(p))
            p.grad = views[n]
            off += p.numel()
    pruner = sweep.prune_model(new, pruning_ratio, importance, **prune_args)
    return new, pruner


def steps_for_threshold(losses, thr):
    """The first k with loss_k < max(loss_0 .. loss_k) * thr, compared in fp32 as the sweep compares (sweep._f32_lt_prod): the stage
    at which a Diff-Pruning sweep with that threshold stops (ddpm_exp/prune.py:249-256).  None when no step is below."""
    loss_max = 0.0
    for k, l in enumerate(losses):
        loss_max = max(loss_max, float(l))
        if sweep._f32_lt_prod(float(l), loss_max, thr):
            return k
    return None


def _to_unit(u8, device):
    """uint8 [N, H, W, C] -> fp32 [N, C, H, W] in [0, 1]: ToTensor of the PNG (compute_pruned_ssim_curve.py:17-21)."""
    return data.to_device_batch(u8, True, torch.device(device), data.RAW, 0.0)


def _mean(per_image):
    """sum(list) / len(list) over the per-image values on the host, as compute_pruned_ssim_curve.py:24 forms it."""
    vals = [float(v) for v in per_image.cpu()]
    return sum(vals) / len(vals)


def _ssim_mse(base_u8, u8, device):
    a, b = _to_unit(base_u8, device), _to_unit(u8, device)
    return metrics.ssim(a, b, 1.0), metrics.mse_per_image(a, b)


def run(model, scheduler, clean_images, noise, x_T, stages, pruning_ratio=0.3, loss_kind='sum', importance=None, sampler_args=None,
        out_dir=None, n_ssim=32, group=None, **sweep_args):
    """One staged sweep of `model` (sweep.taylor_sweep(stages=the stages > 0)), then per stage in ascending order: prune a copy at
    the stage's snapshot (stage 0: the unpruned model, prune_ssim.py:236), sample from `x_T` with ddpm_exp_sampler.Sampler
    (`sampler_args`: its keyword arguments; betas default to the scheduler's), convert to bytes (ops.image_to_u8), write
    `{out_dir}/{stage}/{i}.png` when out_dir is given, and compare the first n_ssim images with stage 0's bytes.
    Returns dict(stages, losses, relative_loss, per_stage=[dict(stage, pruned_idxs, params, macs, ssim, ssim_per_image, mse)]):
    losses per timestep of the sweep, relative_loss = losses / max(losses) (draw_ssim_pruned_curve.py), pruned_idxs = {root:
    indices} from the pruner's records, ssim / mse = means over the compared images.  The memory of the snapshots is
    taylor_sweep's: len(stages) x 4 B x parameters.  A `timings` dict among the sweep arguments also receives the wall-clock split
    of the stages ('prune_s', 'sample_s', 'ssim_s'; each part then ends in a device synchronise)."""
    import time
    stages = sorted(int(s) for s in stages)
    if not stages or stages[0] != 0:
        raise ValueError('stage 0, the unpruned model every other stage is compared with, must be among the stages')
    num_steps = sweep_args.pop('num_steps', stages[-1])
    res = sweep.taylor_sweep(model, scheduler, clean_images, noise, num_steps=num_steps, loss_kind=loss_kind, group=group,
                             stages=[s for s in stages if s > 0], **sweep_args)
    losses = list(res['losses'])
    top = max(losses) if losses else 1.0
    sargs = dict(sampler_args or {})
    betas = sargs.pop('betas', None)
    if betas is None:
        betas = scheduler.betas
    dev = x_T.device
    per_stage, base_u8 = [], None
    timings = sweep_args.get('timings')
    if timings is not None:
        timings.update(prune_s=0.0, sample_s=0.0, ssim_s=0.0)

    def mark(key, t0):
        if timings is not None:
            torch.cuda.synchronize()
            timings[key] += time.perf_counter() - t0
        return time.perf_counter()
    for s in stages:
        t0 = time.perf_counter()
        if s == 0:
            m, idxs = model, {}
        else:
            m, pruner = prune_at_stage(model, res['stage_grads'][s], pruning_ratio, importance)
            idxs = {root: [int(i) for i in pruned] for root, _, _, pruned in pruner.records}
            del pruner
        t0 = mark('prune_s', t0)
        sampler = ddpm_exp_sampler.Sampler(m, betas, tuple(x_T.shape[1:]), **sargs)
        with torch.no_grad():
            u8 = ops.image_to_u8(sampler.sample_image(x_T), sampler.rescaled)
        t0 = mark('sample_s', t0)
        macs, nparams = pruning.count_ops_and_params(m, x_T[:1])
        del sampler, m                                    # each stage's model is dropped before the next is built
        if out_dir is not None:
            folder = os.path.join(out_dir, str(s))
            os.makedirs(folder, exist_ok=True)
            ddpm_exp_sampler._write_pngs(u8.cpu().numpy(), [os.path.join(folder, '%d.png' % i) for i in range(u8.shape[0])])
        if base_u8 is None:
            base_u8 = u8
        k = min(int(n_ssim), u8.shape[0])
        t0 = time.perf_counter()
        ss, ms = _ssim_mse(base_u8[:k], u8[:k], dev)
        mark('ssim_s', t0)
        per_stage.append(dict(stage=s, pruned_idxs=idxs, params=int(nparams), macs=int(macs), ssim=_mean(ss),
                              ssim_per_image=[float(v) for v in ss.cpu()], mse=_mean(ms)))
    return dict(stages=stages, losses=losses, relative_loss=[l / top for l in losses], per_stage=per_stage)


def ssim_curve(root, stages, base=0, n_samples=32, device='cuda'):
    """compute_pruned_ssim_curve.py over folders that are already written: per stage the mean over the images 0 .. n_samples - 1 of
    the SSIM of `{root}/{stage}/{i}.png` against `{root}/{base}/{i}.png`."""
    def files(s):
        return [os.path.join(root, str(s), '%d.png' % i) for i in range(n_samples)]
    ref = next(metrics._image_batches(files(base), n_samples, device))
    return [_mean(metrics.ssim(ref, next(metrics._image_batches(files(s), n_samples, device)), 1.0)) for s in stages]
