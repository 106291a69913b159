"""Post-prune finetune step of the latent-diffusion recipe (ldm_exp/run.sh: `main.py -t --load_pruned_model ...`) on the HIP engine.

One step = LatentDiffusion.training_step (ldm/models/diffusion/ddpm.py:342-356 -> shared_step :865 -> forward :870-879 ->
p_losses :1022-1056) + `torch.optim.AdamW(params, lr=lr)` over `list(unet.parameters()) + list(cond_stage_model.parameters())`
(:1372-1381; cin256-v2.yaml sets cond_stage_trainable) + LitEma when use_ema (ldm/modules/ema.py):

    t ~ randint(0, T, (B,)) per image; c = embedding[class_ids][:, None]; x_t = q_sample(x_start, t, noise);
    loss = mean_B mean_CHW (noise - unet(x_t, t, c))^2      (eps parameterisation, logvar 0, l_simple_weight 1, elbo weight 0)
    backward through the UNet INTO the context (LdmEngine.backward(want_context_grad=True)) and from there into the embedding rows
    (ops.embedding_bwd: repeated ids added in ascending b, no atomics);  AdamW with decoupled weight decay on EVERY parameter --
    the 1001 embedding rows and the exactly-zero-gradient attn2.to_q / to_k / norm2 included -- and the LitEma shadow of the UNet.

Parameters, gradients and moments live in flat fp32 buffers (UNet first, embedder last; train_state.TrainState, the core shared
with train.FinetuneEngine: flat state, accumulation window, exchange ranges, EMA swap), so the update is ONE launch of
dp_adamw_ema (two with the EMA: the shadow covers the UNet only, LitEma(self.model)) and the data-parallel exchange a handful of
all-reduces over contiguous ranges.  Gradient accumulation (accumulate_grad_batches, main.py:707-722): a window of k calls is one
optimizer step; LitEma runs at the end of EVERY batch (ddpm.py:366-368), so the k-1 calls that do not step update the shadow alone
(dp_ema_update).  The training state (train_state.TrainState) makes a run resumable bit for bit.  No LR scheduler (use_scheduler
is off in the config), no learn_logvar, no native replay of the step.
"""
import contextlib

import numpy as np
import torch

from . import ops
from .ldm_sweep import LdmSchedule, encode_first_stage
from .sweep import dist_active
from .train_state import TrainState, flat_views, segment_ranges

# the exchange order of the data-parallel step = the order the backward pass finishes the segments: output path + head, middle,
# input path, time embedding, embedder
_SEGMENT_ORDER = {'output_blocks': 0, 'middle_block': 1, 'input_blocks': 2, 'time_embed': 3, 'cond_stage_model': 4}


def learning_rate(base_lr, batch_size, n_gpus, accumulate_grad_batches=1):
    """main.py:707-722 with --scale_lr (the reference's default): accumulate_grad_batches * ngpu * bs * base_lr
    (run.sh: 2e-6 x 16 x 4 GPUs = 1.28e-4)."""
    return accumulate_grad_batches * n_gpus * batch_size * base_lr


def lit_ema_decay(decay, num_updates):
    """LitEma.forward (ema.py:33-38) in its own fp32 tensor arithmetic: `num_updates` is the counter AFTER this update's
    increment (1 at the first update); decay = min(decay, (1 + n) / (10 + n)) -> 2/11, 3/12, 4/13, ... capped at `decay`."""
    n = np.float32(num_updates)
    return float(min(np.float32(decay), (np.float32(1) + n) / (np.float32(10) + n)))


def _require_hip_device(dev):
    if dev.type != 'cuda':
        raise RuntimeError('the LDM finetune step runs on the MI355X HIP kernels only')


class LdmFinetuneEngine(TrainState):
    TORCH_OPTIMIZER = 'AdamW'

    def __init__(self, model, embedder, schedule=None, lr=1.28e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2,
                 use_ema=False, ema_decay=0.9999, group=None, first_stage=None, scale_factor=1.0,
                 accumulate_grad_batches=1):
        """model: an ldm.UNetModel (pruned or not); embedder: an ldm_sweep.ClassEmbedder, trained with it.
        lr: see learning_rate().  use_ema: keep LitEma's shadow of the UNet (cin256-v2 has use_ema False).
        group: torch.distributed process group of the data-parallel step (None = the default group when initialised): every rank
        steps on its shard of the batch, the gradients (UNet and embedder) are summed over ranks before the update, and the loss
        and gradient of a rank are its share of the mean over the GLOBAL batch.
        first_stage / scale_factor: the VQModel and latent scale step_images() encodes with.
        accumulate_grad_batches = k: a window of k step() calls is one optimizer step on k * B latents per rank (see step()).
        The flat buffers, the window and state_dict() / load_state_dict() come from train_state.TrainState; the data-loader
        position and host generators are not part of the training state and stay with the caller."""
        self._init_window(accumulate_grad_batches, 'accumulate_grad_batches')
        from .ldm import UNetModel
        from .ldm_sweep import ClassEmbedder
        if not isinstance(model, UNetModel):
            raise TypeError('model must be an ldm.UNetModel, got %s' % type(model).__name__)
        if not isinstance(embedder, ClassEmbedder):
            raise TypeError('embedder must be an ldm_sweep.ClassEmbedder, got %s' % type(embedder).__name__)
        self.model, self.embedder = model, embedder
        self.schedule = schedule or LdmSchedule()
        self.lr, self.betas, self.eps, self.weight_decay = float(lr), tuple(betas), float(eps), float(weight_decay)
        self.ema_decay, self.group = float(ema_decay), group
        self.first_stage, self.scale_factor = first_stage, scale_factor
        params = list(model.parameters()) + list(embedder.parameters())  # ddpm.py:1374-1377
        dev = params[0].device
        _require_hip_device(dev)
        if any(p.device != dev for p in params):
            raise ValueError('the UNet and the embedder must be on the same device')
        self.n_unet = sum(p.numel() for p in model.parameters())
        self._init_flat(use_ema, self.n_unet)                            # LitEma(self.model): the shadow covers the UNet only
        self._buckets = sorted(segment_ranges(self._state_named(), self._segment), key=lambda b: (_SEGMENT_ORDER.get(b[0], 5), b[1]))
        self.num_updates = 0                 # LitEma.num_updates
        self.last_loss = None

    # ---- train_state.TrainState
    def _state_named(self):
        from .checkpoint import LDM_UNET_PREFIX, LDM_EMBEDDER_PREFIX
        return ([(LDM_UNET_PREFIX + n, p) for n, p in self.model.named_parameters()] +
                [(LDM_EMBEDDER_PREFIX + n, p) for n, p in self.embedder.named_parameters()])

    def _state_hyper(self):
        return dict(lr=self.lr, betas=list(self.betas), eps=self.eps, weight_decay=self.weight_decay, ema_decay=self.ema_decay,
                    max_grad_norm=None, dropout_seed=None, accumulation=int(self.accum), kd_weights=None, use_ema=self.ema is not None)

    def _state_counters(self):
        return dict(step_count=int(self.step_count), num_updates=int(self.num_updates))

    def _load_counters(self, sd):
        self.step_count, self.num_updates = int(sd['step_count']), int(sd['num_updates'])

    @staticmethod
    def _segment(name):
        from .checkpoint import LDM_UNET_PREFIX
        seg = (name[len(LDM_UNET_PREFIX):] if name.startswith(LDM_UNET_PREFIX) else name).split('.')[0]
        return {'out': 'output_blocks'}.get(seg, seg)

    # ---- LitEma (ema.py) -----------------------------------------------------------------------------------------
    def ema_state(self):
        """The shadow as a {UNet parameter name: tensor} dict (views of the flat shadow buffer)."""
        if self.ema is None:
            raise RuntimeError('LdmFinetuneEngine was built with use_ema=False')
        return flat_views(self.ema, self.model.named_parameters())

    @contextlib.contextmanager
    def ema_scope(self):
        """ddpm.py:172-186: store the live UNet weights, copy the shadow in, restore on exit (TrainState._live_*).  Without EMA: a
        no-op scope."""
        if self.ema is None:
            yield
            return
        self._live_store()                                               # LitEma.store
        self._live_from_shadow()                                         # LitEma.copy_to
        try:
            yield
        finally:
            self._live_restore()                                         # LitEma.restore

    # ---- the step ------------------------------------------------------------------------------------------------
    def _reduce_grads(self, dist):
        pending = [dist.all_reduce(self.flat_g[lo:hi], group=self.group, async_op=True) for _, lo, hi in self._buckets]
        for w in pending:                                                # stream-ordered under RCCL (blocks the host for gloo)
            w.wait()

    def step(self, x_start, class_ids, noise=None, timesteps=None, generator=None, global_batch=None):
        """One optimizer step on latents x_start [B, C, H, W] with class ids [B].  timesteps default to randint(0, T, (B,)) per
        image (ddpm.py:871), noise to randn_like (both from `generator`, a CPU generator, when given).  Returns nothing that forces a
        host synchronisation: `last_loss` is a [1] device tensor (this rank's share of the global mean under a process group).
        With accumulate_grad_batches = k a window is k calls: call 0 zeroes the gradient, every call adds its share of the mean over
        the B * world * k latents of the window, calls 0 .. k-2 leave parameters and moments alone (no collective, packed operands
        kept) and update the LitEma shadow only -- num_updates and the warm-up decay advance per BATCH -- and call k-1 reduces and
        runs the fused update."""
        import torch.distributed as dist
        use_dist = dist_active(self.group)
        model, emb_w = self.model, self.embedder.embedding.weight
        dev = self.flat_p.device
        B = x_start.shape[0]
        ids = ops.check_class_ids(class_ids, emb_w.shape[0])             # host-side: a ValueError, never a device fault
        if ids.numel() != B:
            raise ValueError('%d class ids for %d latents' % (ids.numel(), B))
        k, j = self.accum, self._micro
        gb = global_batch if global_batch is not None else (B * dist.get_world_size(self.group) if use_dist else B) * k
        T = self.schedule.num_timesteps
        if timesteps is None:
            timesteps = torch.randint(0, T, (B,), generator=generator)
        if noise is None:
            noise = (torch.randn(tuple(x_start.shape), generator=generator) if generator is not None
                     else torch.randn(tuple(x_start.shape), dtype=torch.float32, device=dev))
        x_start = x_start.detach().to(dev, torch.float32).contiguous()
        noise = noise.to(dev, torch.float32).contiguous()
        t = timesteps.to(device=dev, dtype=torch.long).contiguous()
        ids = ids.to(dev).contiguous()
        model.train()
        eng = self._window_engine(ops)
        c = emb_w.detach().index_select(0, ids)[:, None, :]              # ClassEmbedder.forward, differentiated below
        sa, sb = self.schedule.tables(dev)
        x_noisy = ops.q_sample(x_start, noise, sa, sb, t)
        if j == 0:
            self.flat_g.zero_()                                          # optimizer.zero_grad()
        out = eng.forward(x_noisy, t, c, save=True)
        n_glob = gb * (out.numel() // B)                                 # mean_B(mean_CHW) == mean over every element
        loss, dout = ops.mse_fwd_bwd(out, noise, 2.0 / n_glob, 1.0 / n_glob)
        dctx = eng.backward(dout, want_context_grad=True)                # [B, 1, D]
        if dctx.shape[1] != 1:
            raise NotImplementedError('the class embedder yields one context token per image')
        ops.embedding_bwd(ids, dctx.reshape(B, dctx.shape[2]).contiguous(), emb_w.grad)
        if j < k - 1:                                                    # the gradient stays in flat_g: LitEma alone (on_train_batch_end)
            if self.ema is not None:
                self.num_updates += 1
                ops.ema_update(self.ema, self.flat_p[:self.n_unet], lit_ema_decay(self.ema_decay, self.num_updates))
            self.last_loss = loss
            self._end_call(last=False)
            return loss
        if use_dist:
            self._reduce_grads(dist)
        self.step_count += 1
        b1, b2 = self.betas
        if self.ema is None:
            ops.adamw_ema(self.flat_p, self.flat_g, self.m, self.v, None, self.lr, b1, b2, self.eps, self.weight_decay, self.step_count)
        else:
            self.num_updates += 1
            decay = lit_ema_decay(self.ema_decay, self.num_updates)
            nu = self.n_unet
            ops.adamw_ema(self.flat_p[:nu], self.flat_g[:nu], self.m[:nu], self.v[:nu], self.ema, self.lr, b1, b2, self.eps,
                          self.weight_decay, self.step_count, decay)
            ops.adamw_ema(self.flat_p[nu:], self.flat_g[nu:], self.m[nu:], self.v[nu:], None, self.lr, b1, b2, self.eps,
                          self.weight_decay, self.step_count)
        eng.packs.clear()                                                # weights changed: packed operands are stale
        self.last_loss = loss
        self._end_call(last=True)
        return loss

    def step_images(self, images, class_ids, **kw):
        """step() on the first stage's pre-quantisation latents of `images` (ddpm.py:826-863: get_input -> encode_first_stage ->
        get_first_stage_encoding), times scale_factor."""
        if self.first_stage is None:
            raise RuntimeError('step_images needs LdmFinetuneEngine(first_stage=VQModel)')
        return self.step(encode_first_stage(self.first_stage, images, self.scale_factor), class_ids, **kw)
