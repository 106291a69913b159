"""Post-prune finetune step (ddpm_train.py:426-471) on the HIP engine, data-parallel over ranks.

One step = add_noise -> UNet forward -> eps-loss (sum over C,H,W, mean over the batch) -> hand-written backward
-> gradient all-reduce (one flat buffer; RCCL over xGMI) -> global-norm clip (1.0) -> Adam -> EMA (constant decay).
Parameters, gradients, Adam moments and the EMA copy live in flat fp32 buffers (train_state.TrainState: the core shared with
ldm_train -- flat state, accumulation window, exchange ranges, EMA swap) so that the optimizer is ONE HBM-bound kernel launch
(csrc/optim.hip) and the all-reduce a few collectives over contiguous ranges.  Here: what only this engine has.
Dropout: the reference finetunes with dropout 0.1 (scripts/finetune_ddpm_cifar10.sh:16 -> utils.set_dropout, utils.py:26-29,
ddpm_train.py:380-382: EVERY nn.Dropout of the model, i.e. ResnetBlock2D.dropout and Attention.to_out[1]).  The masks are
Philox functions of (seed, layer, optimizer step, global element index): fused into the GroupNorm+SiLU kernels, regenerated
in the backward pass, independent of how the batch is sharded over ranks (csrc/dp_common.h).
LR schedule: diffusers/optimization.py:282 `get_scheduler` (LambdaLR multipliers), stepped once per optimizer step
(ddpm_train.py:340-346,464).
Distillation (ddpm_exp/finetune.py --kd, runners/diffusion.py:197-217,301-302, functions/losses.py:17-31): with a frozen
`teacher` the loss is w_kd * mean_b sum_chw (T - S)^2 + w_eps * mean_b sum_chw (e - S)^2 (0.7 / 0.3), T the teacher's no-grad
forward of the same noisy input -- on the side stream, concurrently with the student's forward, when DP_KD_OVERLAP says so.
"""
import math
import numbers
import os

import torch

from . import ops
from .sweep import dist_active
from .train_state import TrainState, flat_views, segment_ranges


def antithetic_timesteps(bsz, num_train_timesteps, generator=None):
    """ddpm_train.py:446-449 -- generated on the CPU (RNG-stream parity), then moved by the caller."""
    t = torch.randint(low=0, high=num_train_timesteps, size=(bsz // 2 + 1,), generator=generator)
    return torch.cat([t, num_train_timesteps - t - 1], dim=0)[:bsz]


class LambdaLR:
    """torch.optim.lr_scheduler.LambdaLR semantics for ONE parameter group (host scalar arithmetic): the lr in force is
    base_lr * f(last_epoch); construction evaluates f(0), every step() advances last_epoch by one."""

    def __init__(self, base_lr, lr_lambda, last_epoch=-1):
        self.base_lr, self.lr_lambda = float(base_lr), lr_lambda
        self.last_epoch = last_epoch
        self.step()

    def step(self):
        self.last_epoch += 1
        self._last_lr = [self.base_lr * self.lr_lambda(self.last_epoch)]

    def get_last_lr(self):
        return self._last_lr

    def state_dict(self):
        return dict(base_lr=self.base_lr, last_epoch=self.last_epoch)

    def load_state_dict(self, sd):
        self.base_lr, self.last_epoch = sd['base_lr'], sd['last_epoch'] - 1
        self.step()


SCHEDULER_TYPES = ('linear', 'cosine', 'cosine_with_restarts', 'polynomial', 'constant', 'constant_with_warmup',
                   'piecewise_constant')


def get_scheduler(name, base_lr, step_rules=None, num_warmup_steps=None, num_training_steps=None, num_cycles=1, power=1.0,
                  last_epoch=-1, lr_end=1e-7):
    """diffusers/optimization.py:282-354 with the optimizer replaced by its learning rate (one parameter group)."""
    if name not in SCHEDULER_TYPES:
        raise ValueError('%r is not a valid SchedulerType' % (name,))
    if name == 'constant':                                        # optimization.py:40-53
        return LambdaLR(base_lr, lambda _: 1, last_epoch)
    if name == 'piecewise_constant':
        # reference behaviour kept: optimization.py:321 calls get_piecewise_constant_schedule(optimizer, rules=...) whose
        # parameter is named step_rules, so this branch of get_scheduler raises; the schedule itself is reachable directly
        raise TypeError("get_piecewise_constant_schedule() got an unexpected keyword argument 'rules'")
    if num_warmup_steps is None:
        raise ValueError('%s requires `num_warmup_steps`, please provide that argument.' % name)
    W = num_warmup_steps
    if name == 'constant_with_warmup':                            # optimization.py:56-78
        return LambdaLR(base_lr, lambda k: float(k) / float(max(1.0, W)) if k < W else 1.0, last_epoch)
    if num_training_steps is None:
        raise ValueError('%s requires `num_training_steps`, please provide that argument.' % name)
    T = num_training_steps
    if name == 'linear':                                          # optimization.py:123-149
        def f(k):
            if k < W:
                return float(k) / float(max(1, W))
            return max(0.0, float(T - k) / float(max(1, T - W)))
    elif name == 'cosine':                                        # optimization.py:152-183 (num_cycles = 0.5)
        def f(k):
            if k < W:
                return float(k) / float(max(1, W))
            progress = float(k - W) / float(max(1, T - W))
            return max(0.0, 0.5 * (1.0 + math.cos(math.pi * float(0.5) * 2.0 * progress)))
    elif name == 'cosine_with_restarts':                          # optimization.py:186-218
        def f(k):
            if k < W:
                return float(k) / float(max(1, W))
            progress = float(k - W) / float(max(1, T - W))
            if progress >= 1.0:
                return 0.0
            return max(0.0, 0.5 * (1.0 + math.cos(math.pi * ((float(num_cycles) * progress) % 1.0))))
    else:                                                         # polynomial, optimization.py:221-268
        lr_init = base_lr
        if not (lr_init > lr_end):
            raise ValueError('lr_end (%s) must be be smaller than initial lr (%s)' % (lr_end, lr_init))

        def f(k):
            if k < W:
                return float(k) / float(max(1, W))
            if k > T:
                return lr_end / lr_init
            pct_remaining = 1 - (k - W) / (T - W)
            return ((lr_init - lr_end) * pct_remaining ** power + lr_end) / lr_init
    return LambdaLR(base_lr, f, last_epoch)


def get_piecewise_constant_schedule(base_lr, step_rules, last_epoch=-1):
    """optimization.py:81-120: step_rules = "1:10,0.1:20,0.01:30,0.005" -> multiplier 1 before step 10, 0.1 before 20, ..."""
    rules, rule_list = {}, step_rules.split(',')
    for rule in rule_list[:-1]:
        value, steps = rule.split(':')
        rules[int(steps)] = float(value)
    last = float(rule_list[-1])

    def piecewise(step):
        for s in sorted(rules):
            if step < s:
                return rules[s]
        return last
    return LambdaLR(base_lr, piecewise, last_epoch)


def set_dropout(model, p):
    """utils.py:26-29."""
    for m in model.modules():
        if isinstance(m, torch.nn.Dropout):
            m.p = p


def _require_hip_device(dev):
    if dev.type != 'cuda':
        raise RuntimeError('finetune runs on the MI355X HIP kernels only')


def _check_kd_weights(kd_weights):
    try:
        w = tuple(kd_weights)
    except TypeError:
        w = None
    if w is None or len(w) != 2 or not all(isinstance(x, numbers.Real) and not isinstance(x, bool) and math.isfinite(x) for x in w):
        raise ValueError('kd_weights must be two finite numbers (w_kd, w_eps), got %r' % (kd_weights,))
    return float(w[0]), float(w[1])


def _check_teacher(teacher, student, dev):
    from .unet import UNet2DModel
    if not isinstance(teacher, UNet2DModel):
        raise TypeError('teacher must be a UNet2DModel (train.load_teacher converts checkpoints), got %s' % type(teacher).__name__)
    if teacher is student:
        raise ValueError('the teacher must not be the student model itself')
    tdev = next(teacher.parameters()).device
    if tdev != dev:
        raise ValueError('the teacher is on %s, the student on %s' % (tdev, dev))
    for k in ('in_channels', 'out_channels', 'sample_size'):
        if teacher.config[k] != student.config[k]:
            raise ValueError('teacher %s = %r does not match the student\'s %r' % (k, teacher.config[k], student.config[k]))


def load_teacher(src, device, ch=None, ch_mult=None, num_res_blocks=None, attn_resolutions=None, image_size=None,
                 in_channels=3, out_ch=3):
    """The frozen teacher of a distillation finetune as a UNet2DModel on `device` (eval mode, parameters frozen).
    src: a UNet2DModel; a Diffusers model / pipeline directory (checkpoint.load_unet); or an original-DDPM checkpoint -- a
    `Model` state dict, the `[state_dict, ...]` list the reference unpacks with `states[0]` (runners/diffusion.py:207-211), or
    a file holding either -- together with that model's ch / ch_mult / num_res_blocks / attn_resolutions / image_size
    (ddpm_exp/configs/*.yml), converted with checkpoint.convert_ddpm_original."""
    from . import checkpoint
    from .unet import UNet2DModel
    if isinstance(src, UNet2DModel):
        model = src
    elif isinstance(src, (str, os.PathLike)) and os.path.isdir(src):
        model = checkpoint.load_unet(os.fspath(src))
    else:
        states = torch.load(os.fspath(src), map_location='cpu', weights_only=True) if isinstance(src, (str, os.PathLike)) else src
        sd = states[0] if isinstance(states, (list, tuple)) else states
        if not isinstance(sd, dict):
            raise TypeError('load_teacher: expected a UNet2DModel, a model directory, an original-DDPM state dict or a '
                            '[state_dict, ...] list, got %s' % type(sd).__name__)
        arch = (ch, ch_mult, num_res_blocks, attn_resolutions, image_size)
        if any(a is None for a in arch):
            raise ValueError('load_teacher: an original-DDPM checkpoint needs ch, ch_mult, num_res_blocks, attn_resolutions and '
                             'image_size (ddpm_exp/configs/*.yml)')
        cfg = checkpoint.unet2d_config_from_ddpm_original(ch, list(ch_mult), num_res_blocks, list(attn_resolutions), image_size,
                                                          in_channels, out_ch)
        model = UNet2DModel(**cfg)
        model.load_state_dict(checkpoint.convert_ddpm_original(sd), strict=True)
        model.attention_scale_from_width = True            # AttnBlock's `int(c) ** -0.5`: the same number until the model is pruned
    model = model.to(device).eval()
    for p in model.parameters():
        p.requires_grad_(False)
    return model


class FinetuneEngine(TrainState):
    def __init__(self, model, scheduler, lr=2e-4, betas=(0.9, 0.999), eps=1e-8, ema_decay=0.9999, max_grad_norm=1.0,
                 use_ema=True, group=None, dropout=None, lr_scheduler=None, dropout_seed=0, replay=None, teacher=None,
                 kd_weights=(0.7, 0.3), gradient_accumulation_steps=1):
        """dropout: None keeps whatever `set_dropout(model, p)` has set on the nn.Dropout holders; a float sets it.
        lr_scheduler: a `LambdaLR` from `get_scheduler` (its base_lr is the learning rate) or None (constant `lr`).
        replay: True / False / None (automatic: single-process steps on a cuda device, DP_FINETUNE_REPLAY=0 disables) -- the step is
        stream-captured ONCE (second call; the first runs eagerly) and afterwards re-issued from the library's C loop
        (ops.CapturedCall): ~750 launches without Python / ctypes per launch.  What changes from step to step lives on the device:
        inputs and timesteps in static buffers, {lr, Adam bias corrections, optimizer step (= the dropout masks' step)} in a
        4-word buffer written by ONE by-value launch per step (ops.set_step_scalars); the weight re-packing is part of the
        captured step.  Same kernels, arguments and order as the eager step -> the same bits.
        teacher: None (the eps loss), or a frozen UNet2DModel on the model's device whose no-grad forward of the same noisy input
        enters the distillation loss with weights kd_weights = (w_kd, w_eps) (functions/losses.py:17-31).  It runs in eval mode
        without dropout; its packed operands are built once and kept (it is never written); EMA and the optimizer see the student
        only.  `last_loss_terms` holds the [kd, eps] device tensor of the last step.
        gradient_accumulation_steps = k: a window of k step() calls is ONE optimizer step on a batch of k * B images per rank,
        sharded in time (see step()).  With k > 1 the step runs eagerly (replay=None resolves to eager, replay=True raises).
        The flat buffers, the window and state_dict() / load_state_dict() come from train_state.TrainState; the teacher, the
        data-loader position and host generators are not part of the training state and stay with the caller."""
        self._init_window(gradient_accumulation_steps, 'gradient_accumulation_steps')
        if self.accum > 1 and replay:
            raise ValueError('replay=True with gradient_accumulation_steps = %d: an accumulating step runs eagerly' % self.accum)
        if teacher is not None:
            kd_weights = _check_kd_weights(kd_weights)
            _check_teacher(teacher, model, next(model.parameters()).device)
        self.replay = replay
        self._caps = None            # {capture key: captured step} (_step_replayed)
        self._seen = {}              # {batch shape: eager steps run at it}
        if dropout is not None:
            set_dropout(model, float(dropout))
        self.model, self.scheduler = model, scheduler
        self.lr_scheduler = lr_scheduler
        self.dropout_seed = dropout_seed
        self.lr, self.betas, self.eps = lr, betas, eps
        self.ema_decay, self.max_grad_norm, self.group = ema_decay, max_grad_norm, group
        dev = next(model.parameters()).device
        _require_hip_device(dev)
        self._init_flat(use_ema)
        # gradient buckets of the data-parallel step: contiguous ranges of the flat gradient buffer that become final at the three
        # milestones of the backward pass (output head + up blocks, mid block, down blocks) and at its end (conv_in, time embedding)
        self._buckets = {'up': [], 'mid': [], 'down': [], 'rest': []}
        for seg, lo, hi in segment_ranges(self._state_named(), self._segment):
            self._buckets[seg].append([lo, hi])
        self.acp = scheduler._acp_on(dev)
        self.last_grad_norm = None
        self.teacher, self.kd_weights, self.last_loss_terms = None, None, None
        if teacher is not None:
            teacher.eval()
            for p in teacher.parameters():
                p.requires_grad_(False)
            self._teacher_pin = teacher.pin_weights()     # frozen for the engine's lifetime: its operands are packed once
            self._teacher_pin.__enter__()
            self._teacher_eng = self._teacher_pin.eng
            self.teacher, self.kd_weights = teacher, kd_weights

    # ---- train_state.TrainState
    def _state_named(self):
        return list(self.model.named_parameters())

    def _state_hyper(self):
        return dict(lr=float(self.lr), betas=[float(b) for b in self.betas], eps=float(self.eps), weight_decay=0.0,
                    ema_decay=float(self.ema_decay), max_grad_norm=float(self.max_grad_norm), dropout_seed=int(self.dropout_seed),
                    accumulation=int(self.accum), kd_weights=None if self.kd_weights is None else [float(w) for w in self.kd_weights],
                    use_ema=self.ema is not None)

    @staticmethod
    def _segment(name):
        return ('up' if name.startswith(('up_blocks.', 'conv_norm_out.', 'conv_out.')) else
                'mid' if name.startswith('mid_block.') else 'down' if name.startswith('down_blocks.') else 'rest')

    def ema_state(self):
        """EMA parameters as a {name: tensor} dict (views of the flat EMA buffer)."""
        return flat_views(self.ema, self._state_named())

    # ---- EMAModel.store / copy_to / restore (training_utils.py:220-262) as used around checkpoints and evaluation
    #      (ddpm_train.py:387-401,489-514): swap the EMA weights into the live model and back (TrainState._live_*)
    def ema_store(self):
        self._live_store()

    def ema_copy_to(self):
        if self.ema is None:
            raise RuntimeError('FinetuneEngine was built with use_ema=False')
        self._live_from_shadow()

    def ema_restore(self):
        if self._stash is None:
            raise RuntimeError('This ExponentialMovingAverage has no `store()`ed weights to `restore()`')
        self._live_restore()

    REPLAY_OVERLAP = None        # weight-gradient side stream inside the captured step: None = the engine's own rule (by step size)
    # teacher forward on the side stream, beside the student's forward (DP_KD_OVERLAP=0 / 1 overrides).  [measured, C4 shapes,
    # tools/bench_kd.py, replayed, one box] 31.13 ms per KD step serial, 29.40 overlapped: 5.6 % on each of three rounds
    KD_OVERLAP = True
    MAX_CAPTURES = 2             # captured steps kept alive at once (full batch + the partial last batch of an epoch)

    @property
    def _cap(self):
        """The most recently built captured step, or None."""
        return next(reversed(self._caps.values())) if self._caps else None

    def _kd_overlap(self, dev):
        ov = os.environ.get('DP_KD_OVERLAP')
        return dev.type == 'cuda' and (self.KD_OVERLAP if ov is None else ov != '0')

    def _teacher_forward(self, noisy, t, overlap, slot):
        """The frozen teacher's no-grad forward of the student's input (eval mode: no dropout, packed operands pinned).
        overlap: fork onto the engine's process-lifetime side stream (idle during the forward; the student's forward goes on on
        the current stream) -- the caller joins with _teacher_join before anything reads the result.  `noisy` and `t` are
        alive until that join (the caller holds them); what the side stream allocates goes back to its own pool, whose next
        user (the next fork) is ordered after the join."""
        teng = self._teacher_eng
        teng.set_dropout(None)
        if not overlap:
            return teng.forward(noisy, t, save=False), None
        from .engine import shared_stream, _low_priority_stream
        side = shared_stream(noisy.device, 'wgrad', slot, _low_priority_stream)
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            out = teng.forward(noisy, t, save=False)
        return out, side

    @staticmethod
    def _teacher_join(side):
        if side is not None:
            torch.cuda.current_stream().wait_stream(side)

    def _replay_wanted(self, use_dist, dev):
        if use_dist or dev.type != 'cuda' or getattr(ops, 'IS_MOCK', False) or not hasattr(ops, 'CapturedCall') or self.accum > 1:
            return False                                 # the data-parallel step interleaves collectives with the backward pass
        if self.replay is None:
            return os.environ.get('DP_FINETUNE_REPLAY', '1') != '0'
        return bool(self.replay)

    def _step_replayed(self, clean, noise, timesteps, gb, image_offset):
        """One optimizer step through the captured step (built on first use for this batch shape)."""
        model, dev = self.model, self.flat_p.device
        table = getattr(model, 'dropout_table', dict)()
        # everything the captured launches carry as immediate arguments: a change of any of them builds a new capture
        key = (tuple(clean.shape), int(image_offset), int(gb), tuple(sorted(table.items())), int(self.dropout_seed),
               self.max_grad_norm, self.eps, self.ema_decay, tuple(self.betas))
        kd_overlap = self._kd_overlap(dev) if self.teacher is not None else False
        if self.teacher is not None:
            key = key + (('kd', id(self.teacher), self.kd_weights, kd_overlap),)
        if self._caps is None:
            self._caps = {}
        cap = self._caps.get(key)
        if cap is None:
            # One capture per key, at most MAX_CAPTURES alive (the partial last batch of an epoch is a second shape: with
            # drop_last=False it alternates with the full one, and re-capturing at every epoch boundary would hold the old pool, the
            # new pool and the eager step's cache at once).  Each capture's private pool pins every activation of a training
            # step, so the oldest goes -- and its pool is returned to the device -- BEFORE the new one is built.
            while len(self._caps) >= self.MAX_CAPTURES:
                old_key = next(iter(self._caps))
                torch.cuda.synchronize(dev)               # nothing of the old capture may still be in flight when its pool goes
                del self._caps[old_key]
                import gc
                gc.collect()
                torch.cuda.empty_cache()
            hyper = torch.zeros(4, dtype=torch.float32, device=dev)
            st = dict(key=key, hyper=hyper, clean=ops.empty_act(tuple(clean.shape), dev), noise=ops.empty_act(tuple(noise.shape), dev),
                      t=torch.zeros(clean.shape[0], dtype=torch.long, device=dev))
            eng = model.engine()
            P = {n: p.detach() for n, p in model.named_parameters()}
            G = {n: p.grad for n, p in model.named_parameters()}
            ov = os.environ.get('DP_FINETUNE_REPLAY_OVERLAP')
            overlap = self.REPLAY_OVERLAP if ov is None else (ov != '0')

            def body():
                eng.bind(P, G)
                eng.set_dropout(table, self.dropout_seed, 0, image_offset, step_dev=hyper.data_ptr() + 12)
                if overlap is not None:
                    eng.overlap_wgrad = overlap
                eng.prepare_packs()                       # the optimizer update of the previous replay invalidated every operand
                noisy = ops.add_noise(st['clean'], st['noise'], self.acp, st['t'])
                if self.teacher is not None:
                    t_out, side = self._teacher_forward(noisy, st['t'], kd_overlap, eng.stream_slot)
                self.flat_g.zero_()
                out = eng.forward(noisy, st['t'], save=True)
                if self.teacher is None:
                    loss, dout = ops.mse_fwd_bwd(out, st['noise'], 2.0 / gb, 1.0 / gb)
                else:
                    self._teacher_join(side)
                    loss, dout = ops.kd_fwd_bwd(out, t_out, st['noise'], self.kd_weights[0], self.kd_weights[1], 2.0 / gb, 1.0 / gb)
                    del t_out
                eng.backward(dout)
                nc = ops.clip_coef(ops.sumsq_partials(self.flat_g), self.max_grad_norm)
                ops.adam_ema_dev(self.flat_p, self.flat_g, self.m, self.v, self.ema, nc[1:2], hyper, self.betas[0], self.betas[1],
                                 self.eps, self.ema_decay)
                eng.packs.clear()                         # host bookkeeping: nothing packed here outlives the step
                return loss, nc
            saved_overlap = eng.overlap_wgrad
            packs_before = self._teacher_packs() if self.teacher is not None else None
            try:
                st['call'] = ops.CapturedCall(body, side_stream=eng.replay_side_stream(dev))
            finally:
                eng.overlap_wgrad = saved_overlap
                eng.set_dropout(None)
            if packs_before is not None and not self._same_packs(packs_before, self._teacher_packs()):
                # the eager step before every capture packed all of them: a pack recorded into the capture would be re-run by
                # every replay into a buffer the capture's pool owns
                raise RuntimeError('the teacher\'s packed operands changed inside the captured step')
            self._caps[key] = cap = st
        if clean.data_ptr() != cap['clean'].data_ptr():
            cap['clean'].copy_(clean)
        if noise.data_ptr() != cap['noise'].data_ptr():
            cap['noise'].copy_(noise)
        cap['t'].copy_(timesteps)
        self.step_count += 1
        lr = self.lr_scheduler.get_last_lr()[0] if self.lr_scheduler is not None else self.lr
        self.last_lr = lr
        ops.set_step_scalars(cap['hyper'], lr, self.betas[0], self.betas[1], self.step_count)
        loss, nc = cap['call'].launch()
        self.last_grad_norm = nc[0:1].clone()              # (the captured tensors are overwritten by the next step)
        if self.lr_scheduler is not None:
            self.lr_scheduler.step()                       # ddpm_train.py:464
        eng = getattr(model, '_engine', None)
        if eng is not None:
            eng.packs.clear()
        if self.teacher is not None:
            terms = loss.clone()                           # [loss, kd, eps]
            loss, self.last_loss_terms = terms[0:1], terms[1:3]
        else:
            loss = loss.clone()                            # the captured tensor is overwritten by the next step
        self._throttle.mark()
        return loss

    def _teacher_packs(self):
        """A snapshot of the teacher's operand cache (pinned: filled by its first forward, then never rebuilt)."""
        return dict(self._teacher_eng.packs._c)

    @staticmethod
    def _same_packs(a, b):
        return a.keys() == b.keys() and all(a[k] is b[k] for k in a)

    def step(self, clean, noise, timesteps, global_batch=None, image_offset=None):
        """Returns the (local share of the) loss as a [1] device tensor; no host synchronisation.
        image_offset: global index of this rank's first image (default rank * B): the dropout masks are functions of the
        GLOBAL element index, so a sharded step draws the masks of the un-sharded one.
        With gradient_accumulation_steps = k a window is k calls: one batch of k * B images per rank sharded in time.  Call 0
        zeroes the gradient; every call runs forward, loss and backward at the global batch B * world * k and the dropout-mask step
        step_count + 1 (default image_offset (rank * k + j) * B: the masks of the un-split batch) and accumulates; calls 0 .. k-2
        touch neither parameters, moments, step_count nor the LR schedule, issue no collective and keep the packed operands; call
        k-1 all-reduces, clips the ACCUMULATED gradient, updates and steps the LR schedule once.  Every call returns its share of
        the global mean."""
        import torch.distributed as dist
        use_dist = dist_active(self.group)
        B = clean.shape[0]
        k, j = self.accum, self._micro
        gb = global_batch if global_batch is not None else (B * dist.get_world_size(self.group) if use_dist else B) * k
        if image_offset is None:
            image_offset = ((dist.get_rank(self.group) if use_dist else 0) * k + j) * B
        model = self.model
        model.train()                                     # ddpm_train.py:430
        dev = self.flat_p.device
        # a batch shape runs eagerly the first time it is seen (lazy operands, streams, code objects: CapturedCall's precondition)
        shape_key = tuple(clean.shape)
        seen = self._seen.get(shape_key, 0)
        self._seen[shape_key] = seen + 1
        if seen >= 1 and self.step_count >= 1 and self._replay_wanted(use_dist, dev):
            return self._step_replayed(clean.to(dev, torch.float32).contiguous(), noise.to(dev, torch.float32).contiguous(),
                                       timesteps.to(device=dev, dtype=torch.long).contiguous(), gb, image_offset)
        clean = clean.to(dev, torch.float32).contiguous()
        noise = noise.to(dev, torch.float32).contiguous()
        eng = self._window_engine(ops)
        eng.set_dropout(getattr(model, 'dropout_table', dict)(), self.dropout_seed, self.step_count + 1, image_offset)
        # the batched time-embedding backward finalises the time_emb_proj gradients only at the END of the backward pass: it is
        # switched off when gradient buckets are all-reduced at the segment milestones
        eng.temb_batch = eng.temb_batch and not use_dist
        t = timesteps.to(device=dev, dtype=torch.long).contiguous()
        noisy = ops.add_noise(clean, noise, self.acp, t)
        if self.teacher is not None:
            t_out, side = self._teacher_forward(noisy, t, self._kd_overlap(dev), eng.stream_slot)
        if j == 0:
            self.flat_g.zero_()                           # optimizer.zero_grad()
        out = eng.forward(noisy, t, save=True)
        if self.teacher is None:
            loss, dout = ops.mse_fwd_bwd(out, noise, 2.0 / gb, 1.0 / gb)
        else:
            self._teacher_join(side)
            terms, dout = ops.kd_fwd_bwd(out, t_out, noise, self.kd_weights[0], self.kd_weights[1], 2.0 / gb, 1.0 / gb)
            loss, self.last_loss_terms = terms[0:1], terms[1:3]
            del t_out
        pending = []
        if j < k - 1:                                     # the gradient stays in flat_g: no collective, no update, no LR step
            eng.backward(dout)
            self._end_call(last=False)
            return loss
        if use_dist:
            # bucketed all-reduce overlapped with the backward pass: each bucket's collective (RCCL over xGMI) is enqueued as
            # soon as its gradients are final and runs while the remaining layers' MFMA kernels execute
            def reduce_segment(seg):
                for lo, hi in self._buckets[seg]:
                    pending.append(dist.all_reduce(self.flat_g[lo:hi], group=self.group, async_op=True))
            eng.segment_hook = reduce_segment
        try:
            eng.backward(dout)
        finally:
            eng.segment_hook = None
        if use_dist:
            reduce_segment('rest')
            for w in pending:                                   # stream-ordered wait for RCCL (blocks the host for gloo)
                w.wait()
        partial = ops.sumsq_partials(self.flat_g)
        nc = ops.clip_coef(partial, self.max_grad_norm)
        self.last_grad_norm = nc[0:1]
        self.step_count += 1
        lr = self.lr_scheduler.get_last_lr()[0] if self.lr_scheduler is not None else self.lr
        self.last_lr = lr
        ops.adam_ema(self.flat_p, self.flat_g, self.m, self.v, self.ema, nc[1:2], lr, self.betas[0], self.betas[1],
                     self.eps, self.step_count, self.ema_decay)
        if self.lr_scheduler is not None:
            self.lr_scheduler.step()                       # ddpm_train.py:464
        eng.packs.clear()                                  # weights changed: packed operands are stale
        self._end_call(last=True)
        return loss
