"""The flat-buffer core both finetune engines (train.FinetuneEngine, ldm_train.LdmFinetuneEngine) are built on, and their training
state.  The core: parameters and gradients re-homed into `flat_p` / `flat_g` with the moments and the EMA shadow beside them, the
accumulation window and the engine a call of it runs on, the ranges of `flat_g` a data-parallel step exchanges (segment_ranges),
the swap of the live weights against the shadow -- all over ONE offset walk (_offsets).  An engine adds what differs: its step,
hyper-parameters, segment function, exchange order and EMA rule.  The state: what a stopped run needs to go on bit for bit --
Adam's moments, the EMA shadow, the step counters and the LR schedule -- and the same moments in torch's optimizer layout
(ddpm_exp/runners/diffusion.py:236-248 `--resume_training`; Lightning's `optimizer_states`).

The state holds plain tensors, numbers, strings and lists only, so a file of it loads under `weights_only=True`.  NOT part of it:
the weights themselves (checkpoint.save_training_state writes them beside the state), the frozen teacher of a distillation
engine, the position of the data loader and every host generator -- they stay with the caller.  Under a process group the state
is identical on every rank (the gradients are summed before the update), so rank 0 writes and every rank loads.

Loading copies INTO the engine's flat buffers: the parameters are views of `flat_p` and captured steps hold these pointers, so
nothing is rebound; packed operands are invalidated as `ema_copy_to` does."""
import itertools

import torch

from .sweep import StepThrottle

FORMAT_VERSION = 1


def _offsets(named):
    """(name, parameter, lo, hi) of every parameter in a flat buffer: the one offset walk of the package."""
    off = 0
    for n, p in named:
        yield n, p, off, off + p.numel()
        off += p.numel()


def flat_views(buf, named):
    """{name: view of `buf` in the parameter's shape}, `named` = [(name, parameter), ...] in the order of the flat buffer."""
    return {n: buf[lo:hi].view(p.shape) for n, p, lo, hi in _offsets(named)}


def param_layout(named):
    """[[name, shape, offset into the flat buffer], ...] in the engine's parameter order."""
    return [[n, [int(s) for s in p.shape], lo] for n, p, lo, _ in _offsets(named)]


def segment_ranges(named, segment):
    """[[segment(name), lo, hi], ...] in parameter order, adjacent parameters of one segment merged; the engine orders them."""
    out = []
    for n, _, lo, hi in _offsets(named):
        seg = segment(n)
        if out and out[-1][0] == seg:
            out[-1][2] = hi
        else:
            out.append([seg, lo, hi])
    return out


def check_layout(own, got):
    for i, (a, b) in enumerate(itertools.zip_longest(own, got)):
        a = None if a is None else [a[0], [int(s) for s in a[1]], int(a[2])]
        b = None if b is None else [b[0], [int(s) for s in b[1]], int(b[2])]
        if a != b:
            def show(x):
                return 'nothing' if x is None else '%s %s at offset %d' % (x[0], tuple(x[1]), x[2])
            raise ValueError('the parameter layout of the state differs from the engine\'s at tensor %d: the engine has %s, the state '
                             'has %s (a state belongs to the pruned shapes it was taken at)' % (i, show(a), show(b)))


def _plain(x):
    if isinstance(x, (tuple, list)):
        return [_plain(y) for y in x]
    return x


def _int_step(x):
    """torch stores `step` as a 0-d fp32 tensor; older files and other writers hold integers."""
    v = float(x)
    if v != int(v) or v < 0:
        raise ValueError('optimizer step %r is not a non-negative whole number' % (x,))
    return int(v)


class TrainState:
    """Base of the finetune engines: the flat state, the accumulation window and state_dict / load_state_dict with their
    torch-layout pair.  A subclass sets `model`, implements the two hooks below and calls _init_window and _init_flat from its
    constructor; everything else it reads (flat_p, flat_g, m, v, ema, step_count, accum, _micro) is set up here."""

    TORCH_OPTIMIZER = 'Adam'

    def _state_named(self):
        """[(name, parameter), ...] in the order of the flat buffers."""
        raise NotImplementedError

    def _state_hyper(self):
        """The hyper-parameters the arithmetic depends on, as plain numbers / lists / None."""
        raise NotImplementedError

    # ---- construction ----------------------------------------------------------------------------------------------------
    def _init_window(self, k, arg):
        """accum = k calls of step() are one optimizer step, _micro the position inside the window; `arg` names k in the error."""
        if int(k) < 1 or int(k) != k:
            raise ValueError('%s must be a positive integer, got %r' % (arg, k))
        self.accum, self._micro = int(k), 0

    def _init_flat(self, use_ema, n_shadow=None):
        """Re-home the parameters of _state_named() into flat_p and bind their gradients to views of flat_g (views keep nn.Module
        semantics); zeroed moments; with use_ema the shadow of the leading n_shadow elements (default: all of them)."""
        named = self._state_named()
        dev = named[0][1].device
        total = sum(p.numel() for _, p in named)
        self.flat_p = torch.empty(total, dtype=torch.float32, device=dev)
        self.flat_g = torch.zeros(total, dtype=torch.float32, device=dev)
        for _, p, lo, hi in _offsets(named):
            self.flat_p[lo:hi].copy_(p.data.reshape(-1))
            p.data = self.flat_p[lo:hi].view_as(p)
            p.grad = self.flat_g[lo:hi].view_as(p)
        self.m = torch.zeros_like(self.flat_p)
        self.v = torch.zeros_like(self.flat_p)
        self._n_shadow = total if n_shadow is None else n_shadow
        self.ema = self.flat_p[:self._n_shadow].clone() if use_ema else None
        self.step_count = 0
        self._stash = None
        self._throttle = StepThrottle()

    # ---- the window ------------------------------------------------------------------------------------------------------
    def _window_engine(self, ops):
        """The model's engine for this call, bound to the flat views.  Inside a window the weights did not change: the engine of
        call 0 and its packed operands are kept (model.engine() drops them); call 0 follows an update that invalidated every
        operand and re-packs in a few launches.  ops: the engine module's kernel module (a CPU mock has no pack_weight_batch)."""
        model, first = self.model, self._micro == 0
        eng = model.engine() if first or getattr(model, '_engine', None) is None else model._engine
        eng.bind({n: p.detach() for n, p in model.named_parameters()}, {n: p.grad for n, p in model.named_parameters()})
        if hasattr(ops, 'pack_weight_batch') and first:
            eng.prepare_packs()
        return eng

    def _end_call(self, last):
        """Close a step() call: advance the window; a step reads nothing back, so bound how far the host runs ahead."""
        self._micro = 0 if last else self._micro + 1
        self._throttle.mark()

    def _weights_changed(self):
        eng = getattr(self.model, '_engine', None)
        if eng is not None:
            eng.packs.clear()                              # packed operands are stale

    # ---- live weights against the shadow, over the shadow's range (EMAModel / LitEma store, copy_to, restore) ------------------
    def _live_store(self):
        self._stash = self.flat_p[:self._n_shadow].clone()

    def _live_from_shadow(self):
        self.flat_p[:self._n_shadow].copy_(self.ema)
        self._weights_changed()

    def _live_restore(self):
        self.flat_p[:self._n_shadow].copy_(self._stash)
        self._stash = None
        self._weights_changed()

    def _state_counters(self):
        return dict(step_count=int(self.step_count))

    def _load_counters(self, sd):
        self.step_count = int(sd['step_count'])

    def _check_window(self, what):
        if self._micro != 0:
            raise ValueError('%s in the middle of an accumulation window (call %d of %d): the accumulated gradient is not part of '
                             'the state' % (what, self._micro, self.accum))

    # ---- the native state ------------------------------------------------------------------------------------------------
    def state_dict(self, device=None):
        """The training state (module docstring).  The tensors are copies (on `device`; default: where the buffers live): a step
        taken afterwards does not change them.  Raises ValueError in the middle of an accumulation window."""
        self._check_window('state_dict()')
        sched = getattr(self, 'lr_scheduler', None)

        def copy(t):
            return None if t is None else t.detach().to(device if device is not None else t.device, copy=True)
        sd = dict(format_version=FORMAT_VERSION, engine=type(self).__name__, micro_step=int(self._micro),
                  m=copy(self.m), v=copy(self.v), ema=copy(self.ema),
                  lr_scheduler=None if sched is None else _plain(dict(sched.state_dict())),
                  layout=param_layout(self._state_named()), hyper=_plain(self._state_hyper()))
        sd.update(self._state_counters())
        return sd

    def check_state_dict(self, sd, strict=True):
        """Every check load_state_dict makes, and no write: format, engine class, parameter layout (ValueError naming the first
        differing tensor), window position, hyper-parameters under `strict`, EMA presence, dtypes and sizes."""
        if sd.get('format_version') != FORMAT_VERSION:
            raise ValueError('unsupported training-state format %r' % (sd.get('format_version'),))
        if sd.get('engine') != type(self).__name__:
            raise ValueError('a %s state cannot be loaded into a %s' % (sd.get('engine'), type(self).__name__))
        check_layout(param_layout(self._state_named()), sd['layout'])
        if int(sd.get('micro_step', 0)) != 0:
            raise ValueError('the state was taken in the middle of an accumulation window')
        sched = getattr(self, 'lr_scheduler', None)
        own = _plain(self._state_hyper())
        own['lr_scheduler_base_lr'] = None if sched is None else float(sched.base_lr)
        got = dict(sd['hyper'])
        got['lr_scheduler_base_lr'] = None if sd['lr_scheduler'] is None else float(sd['lr_scheduler']['base_lr'])
        if strict:
            for k in own:
                if k not in got or own[k] != got[k]:
                    raise ValueError('hyper-parameter %s: the engine has %r, the state %r (strict=False keeps the engine\'s)'
                                     % (k, own[k], got.get(k)))
        if (self.ema is None) != (sd['ema'] is None):
            raise ValueError('the state %s an EMA shadow, the engine %s' % ('has' if sd['ema'] is not None else 'has not',
                                                                           'keeps one' if self.ema is not None else 'keeps none'))
        for name, t, buf in (('m', sd['m'], self.m), ('v', sd['v'], self.v), ('ema', sd['ema'], self.ema)):
            if buf is not None and (t.dtype != torch.float32 or t.numel() != buf.numel()):
                raise ValueError('state tensor %s: %s of %d elements, the engine holds fp32 of %d' % (name, t.dtype, t.numel(), buf.numel()))

    def load_state_dict(self, sd, strict=True):
        """Take a state_dict() (of this engine class, at this parameter layout) into the existing flat buffers.
        strict: a recorded hyper-parameter that differs from the engine's raises ValueError; with strict=False the state is taken and
        the constructor's values stay in force (what runners/diffusion.py:243 does with eps).  A differing layout always raises
        ValueError naming the first differing tensor.  Nothing is written before every check (check_state_dict) has passed."""
        self.check_state_dict(sd, strict=strict)
        sched = getattr(self, 'lr_scheduler', None)
        for t, buf in ((sd['m'], self.m), (sd['v'], self.v), (sd['ema'], self.ema)):
            if buf is not None:
                buf.copy_(t.reshape(-1))
        self._load_counters(sd)
        self._micro = 0
        if sched is not None and sd['lr_scheduler'] is not None:
            sched.load_state_dict(dict(base_lr=sched.base_lr, last_epoch=int(sd['lr_scheduler']['last_epoch'])))
        self._weights_changed()

    # ---- torch's optimizer layout ----------------------------------------------------------------------------------------
    def _torch_param_group(self, n):
        """The param_groups entry torch.optim.Adam / AdamW of the running torch writes for this engine's hyper-parameters."""
        h = self._state_hyper()
        dummies = [torch.nn.Parameter(torch.empty(0)) for _ in range(n)]
        sched = getattr(self, 'lr_scheduler', None)
        lr = float(sched.get_last_lr()[0]) if sched is not None else float(h['lr'])
        opt = getattr(torch.optim, self.TORCH_OPTIMIZER)(dummies, lr=lr, betas=tuple(h['betas']), eps=h['eps'],
                                                         weight_decay=h['weight_decay'])
        group = opt.state_dict()['param_groups'][0]
        if sched is not None:
            group['initial_lr'] = float(sched.base_lr)
        return group

    def optimizer_state_dict(self):
        """{'state': {i: {'step', 'exp_avg', 'exp_avg_sq'}}, 'param_groups': [...]} as torch.optim.Adam (AdamW for the LDM engine)
        writes it: indices in the order of the optimizer's parameter list, `step` a 0-d fp32 tensor, the moments as CPU copies."""
        self._check_window('optimizer_state_dict()')
        named = self._state_named()
        m, v = flat_views(self.m.detach().cpu(), named), flat_views(self.v.detach().cpu(), named)
        state = {i: dict(step=torch.tensor(float(self.step_count), dtype=torch.float32), exp_avg=m[n].clone(), exp_avg_sq=v[n].clone())
                 for i, (n, _) in enumerate(named)}
        return dict(state=state, param_groups=[self._torch_param_group(len(named))])

    def load_optimizer_state_dict(self, sd):
        """Take the moments and the step of a torch-layout optimizer state (indices in this engine's parameter order).  The
        hyper-parameters stay the engine's; the file's param_groups are not read beyond their parameter count."""
        self._check_window('load_optimizer_state_dict()')
        named = self._state_named()
        state = sd['state']
        ids = [i for g in sd['param_groups'] for i in g['params']]
        if len(ids) != len(named) or (state and sorted(state) != sorted(ids)):
            raise ValueError('the optimizer state covers %d parameters (%d with moments), the engine has %d'
                             % (len(ids), len(state), len(named)))
        if not state:                                        # torch creates the per-parameter state at the first step
            self.m.zero_()
            self.v.zero_()
            self.step_count = 0
            return
        steps = {_int_step(state[i]['step']) for i in ids}
        if len(steps) != 1:
            raise ValueError('the parameters are at different optimizer steps: %s' % sorted(steps))
        for (name, p), i in zip(named, ids):
            for key in ('exp_avg', 'exp_avg_sq'):
                if tuple(state[i][key].shape) != tuple(p.shape):
                    raise ValueError('%s of parameter %d (%s): shape %s, the engine has %s'
                                     % (key, i, name, tuple(state[i][key].shape), tuple(p.shape)))
        dev = self.m.device
        self.m.copy_(torch.cat([state[i]['exp_avg'].detach().reshape(-1).to(torch.float32) for i in ids]).to(dev))
        self.v.copy_(torch.cat([state[i]['exp_avg_sq'].detach().reshape(-1).to(torch.float32) for i in ids]).to(dev))
        self.step_count = steps.pop()
