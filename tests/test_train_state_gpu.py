"""Training state and gradient accumulation of the finetune engines on the MI355X: a stopped run continues bit for bit from the
one-file state (eager, natively replayed, without EMA, with a teacher, with accumulation; both engines), accumulation equals the
full batch, dp_ema_update against fp64 and bit for bit against the EMA half of dp_adamw_ema, torch's optimizer layout against torch
itself, and the reference's own states (tests/golden/train_state.json + train_state_*.npz, written by the DDIM code base's model /
optimizer / EMAHelper and by LatentDiffusion + AdamW + LitEma).  Every measured figure is printed beside its bound and kept in the
session report under 'train_state/...'."""
import ctypes
import os

import numpy as np
import pytest
import torch

import golden_common as gc
import ldm_finetune_ref as R
from helpers import load_json, load_npz, make_model, pkg, relerr
from kd_ref import original_state_dict

pytestmark = pytest.mark.gpu
DEV = 'cuda'
B = 4


def note(report, key, **vals):
    print('train_state/%s: %s' % (key, '  '.join('%s %s' % (k, ('%.3e' % v) if isinstance(v, float) else v) for k, v in vals.items())))
    report['train_state/' + key] = vals


# ---- builders ------------------------------------------------------------------------------------------------------------
def _ddpm(teacher=False, cfg=None, **kw):
    train, diffusion = pkg('train'), pkg('diffusion')
    model = make_model(cfg or gc.TINY_CFG, 5)
    kw.setdefault('lr_scheduler', train.get_scheduler('cosine', 2e-4, num_warmup_steps=2, num_training_steps=10))
    if teacher:
        kw['teacher'] = make_model(gc.TINY_CFG, 9)
    return model, train.FinetuneEngine(model, diffusion.DDPMScheduler(), dropout=0.1, dropout_seed=7, **kw)


def _batch(k, b=B):
    train = pkg('train')
    return (torch.from_numpy(gc.det_clean((b, 3, 16, 16), 30 + k)).to(DEV), torch.from_numpy(gc.det_noise((b, 3, 16, 16), 40 + k)).to(DEV),
            train.antithetic_timesteps(b, 1000, torch.Generator().manual_seed(100 + k)))


def _ldm(cfg=None, unet_seed=9, **kw):
    ldm, ldm_sweep, ldm_train = pkg('ldm'), pkg('ldm_sweep'), pkg('ldm_train')
    cfg = cfg or gc.LDM_TINY_CFG
    model = ldm.UNetModel(**cfg)
    gc.det_init_(model, unet_seed)
    embedder = ldm_sweep.ClassEmbedder(cfg['context_dim'], 1001)
    with torch.no_grad():
        embedder.embedding.weight.copy_(torch.from_numpy(gc.det_param('embedding.weight', (1001, cfg['context_dim']), 61)))
    model, embedder = model.to(DEV), embedder.to(DEV)
    return model, embedder, ldm_train.LdmFinetuneEngine(model, embedder, lr=1.28e-4, **kw)


LDM_IDS = [3, 500, 3, 1000]


def _ldm_batch(k, sl=slice(None), x_seed=None, noise_seed=60):
    H = gc.LDM_TINY_CFG['image_size']
    x = torch.from_numpy(gc.det_noise((B, 3, H, H), (50 + k) if x_seed is None else x_seed))
    noise = torch.from_numpy(gc.det_noise((B, 3, H, H), noise_seed + k))
    return dict(x_start=x[sl].to(DEV), class_ids=torch.tensor(LDM_IDS)[sl], noise=noise[sl].to(DEV), timesteps=torch.tensor([0, 250, 999, 17 + k])[sl])


def _same(a, b):
    torch.cuda.synchronize()
    return (torch.equal(a.flat_p, b.flat_p) and torch.equal(a.m, b.m) and torch.equal(a.v, b.v) and
            (a.ema is None) == (b.ema is None) and (a.ema is None or torch.equal(a.ema, b.ema)) and
            a.step_count == b.step_count and getattr(a, 'last_lr', None) == getattr(b, 'last_lr', None) and
            getattr(a, 'num_updates', 0) == getattr(b, 'num_updates', 0))


# ---- resume is bit-identical -----------------------------------------------------------------------------------------
@pytest.mark.parametrize('mode,kw,a,n', [
    ('eager', dict(replay=False), 3, 6),
    ('replay', dict(replay=True), 2, 6),                  # on both sides the first step at a shape is eager, the rest captured
    ('no_ema', dict(replay=False, use_ema=False), 3, 6),
    ('kd', dict(replay=False, teacher=True), 3, 6),
    ('k2', dict(gradient_accumulation_steps=2), 4, 8),    # 2 + 2 windows against 4
])
def test_ddpm_resume_is_bit_identical(report, tmp_path, mode, kw, a, n):
    """n steps in one go against a steps, save_training_state, a NEW model and engine built from the file alone, n - a steps:
    flat_p, m, v, ema, step_count, last_lr and every post-resume loss, bit for bit (dropout 0.1 seed 7: the Philox masks are keyed
    by the step; cosine schedule with warm-up 2 of 10)."""
    ckpt = pkg('checkpoint')
    _, whole = _ddpm(**kw)
    l_whole = [float(whole.step(*_batch(k))) for k in range(n)]
    _, first = _ddpm(**kw)
    l_first = [float(first.step(*_batch(k))) for k in range(a)]
    path = str(tmp_path / 'state.pt')
    ckpt.save_training_state(path, first)
    del first
    _, second = _ddpm(**kw)                                    # (a KD engine's teacher stays with the caller: built again here)
    ckpt.load_training_state(path, second)
    l_second = [float(second.step(*_batch(k))) for k in range(a, n)]
    if mode == 'replay':
        assert whole._cap is not None and second._cap is not None and second._cap['call'].replay is not None
    else:
        assert whole._cap is None and second._cap is None
    note(report, 'resume_' + mode, losses=l_whole, resumed_equal=l_first + l_second == l_whole)
    assert l_first + l_second == l_whole and _same(whole, second)
    assert whole.step_count == (n // 2 if mode == 'k2' else n)


@pytest.mark.parametrize('use_ema', [True, False])
@pytest.mark.parametrize('k', [1, 2])
def test_ldm_resume_is_bit_identical(report, tmp_path, use_ema, k):
    """The LDM engine, 2 + 2 windows against 4, with and without LitEma, k = 1 and k = 2 (B = 4 with a repeated class id): the
    UNet, the embedder, moments, shadow, step_count and num_updates from the one file; and through the `last.ckpt` additions."""
    ckpt = pkg('checkpoint')
    kw = dict(use_ema=use_ema, accumulate_grad_batches=k)
    *_, whole = _ldm(**kw)
    l_whole = [float(whole.step(**_ldm_batch(i))) for i in range(4 * k)]
    m1, e1, first = _ldm(**kw)
    [first.step(**_ldm_batch(i)) for i in range(2 * k)]
    native, last = str(tmp_path / 'state.pt'), str(tmp_path / 'last.ckpt')
    ckpt.save_training_state(native, first)
    ckpt.save_ldm_finetuned(last, m1, e1, ema=first if use_ema else None, training_state=first)
    assert first.num_updates == (2 * k if use_ema else 0) and first.step_count == 2
    for how in ('native', 'last.ckpt'):
        m2, e2, second = _ldm(**kw)
        if how == 'native':
            ckpt.load_training_state(native, second)
        else:
            assert ckpt.load_ldm_finetuned(last, m2, e2, engine=second)['global_step'] == 2
        l_second = [float(second.step(**_ldm_batch(i))) for i in range(2 * k, 4 * k)]
        assert l_second == l_whole[2 * k:] and _same(whole, second), how
    note(report, 'resume_ldm_ema%d_k%d' % (use_ema, k), losses=l_whole, num_updates=whole.num_updates)


def test_state_is_a_copy_and_loading_rewinds(tmp_path):
    """A state taken earlier is unchanged by later steps; loading it into the engine that has stepped on rewinds it exactly."""
    ckpt = pkg('checkpoint')
    _, ft = _ddpm(replay=True)
    [ft.step(*_batch(k)) for k in range(3)]                    # eager, eager-free capture, replay: the capture holds the pointers
    path = str(tmp_path / 'state.pt')
    ckpt.save_training_state(path, ft)
    sd = ft.state_dict()
    torch.cuda.synchronize()
    keep = {k: v.clone() for k, v in sd.items() if torch.is_tensor(v)}
    p3, ptr = ft.flat_p.clone(), ft.flat_p.data_ptr()
    l_a = [float(ft.step(*_batch(k))) for k in (3, 4)]
    end = [t.clone() for t in (ft.flat_p, ft.m, ft.v, ft.ema)]
    assert all(torch.equal(sd[k], v) for k, v in keep.items()) and not torch.equal(ft.m, sd['m'])
    ckpt.load_training_state(path, ft)
    assert ft.flat_p.data_ptr() == ptr and torch.equal(ft.flat_p, p3) and ft.step_count == 3 and torch.equal(ft.m, keep['m'])
    l_b = [float(ft.step(*_batch(k))) for k in (3, 4)]
    torch.cuda.synchronize()
    assert l_a == l_b and all(torch.equal(a, b) for a, b in zip(end, (ft.flat_p, ft.m, ft.v, ft.ema)))


def test_error_cases(tmp_path):
    """ValueError: an un-pruned state into the ratio-0.3 pruned tiny model (first differing tensor named, nothing written), differing
    betas under strict=True (strict=False takes it), a save in mid-window, replay=True with k = 2."""
    train, ckpt, diffusion, sweep = pkg('train'), pkg('checkpoint'), pkg('diffusion'), pkg('sweep')
    _, ft = _ddpm()
    ft.step(*_batch(0))
    path = str(tmp_path / 'state.pt')
    ckpt.save_training_state(path, ft)
    sd = ft.state_dict()
    pruned = make_model(gc.TINY_CFG, 5)
    c, n, _ = _batch(0, 2)
    sweep.taylor_sweep(pruned, diffusion.DDPMScheduler(), c, n, num_steps=2)
    sweep.prune_model(pruned, 0.3)
    for p in pruned.parameters():
        p.grad = None
    fp = train.FinetuneEngine(pruned, diffusion.DDPMScheduler(), dropout=0.1, dropout_seed=7,
                              lr_scheduler=train.get_scheduler('cosine', 2e-4, num_warmup_steps=2, num_training_steps=10))
    first_diff = next(a for (a, p), (_, q) in zip(pruned.named_parameters(), ft.model.named_parameters()) if p.shape != q.shape)
    before = fp.flat_p.clone()
    for load in (lambda: fp.load_state_dict(sd), lambda: ckpt.load_training_state(path, fp)):
        with pytest.raises(ValueError, match=first_diff.replace('.', r'\.')):
            load()
    assert torch.equal(fp.flat_p, before) and fp.step_count == 0 and not bool(fp.m.any())
    _, other = _ddpm(betas=(0.8, 0.999))
    with pytest.raises(ValueError, match='betas'):
        other.load_state_dict(sd)
    other.load_state_dict(sd, strict=False)
    assert other.step_count == 1 and tuple(other.betas) == (0.8, 0.999) and torch.equal(other.m, sd['m'])
    _, acc = _ddpm(gradient_accumulation_steps=2)
    acc.step(*_batch(0))
    with pytest.raises(ValueError, match='window'):
        acc.state_dict()
    with pytest.raises(ValueError, match='window'):
        ckpt.save_training_state(path, acc)
    with pytest.raises(ValueError):
        _ddpm(gradient_accumulation_steps=2, replay=True)


# ---- accumulation equals the full batch ------------------------------------------------------------------------------
NOISE = 1e-6


def _per_tensor_rel_l2(named, g, g_ref):
    """(worst per-tensor relative L2, its name, flat max-abs error relative to the largest gradient element, tensors left out).
    A tensor whose exact gradient is zero -- the key bias of an attention (softmax is invariant to a shift per query), a bias in
    front of a GroupNorm with one channel per group -- holds only the rounding residue of terms that cancel, ~2^-24 of those
    terms: a relative error OF that residue measures nothing.  Such tensors (largest element below NOISE = 1e-6 of the largest
    gradient element, in the full batch) are left out of the per-tensor figure and bounded in absolute terms by the flat one, which
    is the measure tests/test_e2e_gpu.py applies to micro-batched against un-batched gradients.  A full-batch gradient that is
    exactly zero must be exactly zero accumulated."""
    worst, name, off, left_out = 0.0, None, 0, []
    top = float(g_ref.abs().max())
    for n, p in named:
        a, r = g[off:off + p.numel()].double(), g_ref[off:off + p.numel()].double()
        off += p.numel()
        if float(r.abs().max()) == 0.0:
            assert float(a.abs().max()) == 0.0, n
            continue
        if float(r.abs().max()) < NOISE * top:
            left_out.append(n)
            continue
        e = float((a - r).norm() / r.norm())
        if e > worst:
            worst, name = e, n
    return worst, name, float((g.double() - g_ref.double()).abs().max()) / top, left_out


@pytest.mark.parametrize('k', [2, 4])
def test_ddpm_accumulation_equals_the_full_batch(report, k):
    """B = 8 in one call against k calls of 8 / k (dropout 0.1): calls 0 .. k-2 leave flat_p, m, v, ema, step_count and the schedule
    bit-unchanged; after the window flat_g is the full-batch gradient per tensor within 1e-5 relative L2 (fp32 re-association only:
    the bound of test_e2e_gpu for micro-batched against un-batched gradients; a wrong mask offset or scale is off by orders of
    magnitude); the returned losses sum to the full-batch loss; the clip coefficient comes from the accumulated norm; one LR step."""
    full_b = 8
    c, n, t = _batch(0, full_b)
    _, full = _ddpm(replay=False)
    _, acc = _ddpm(gradient_accumulation_steps=k)
    for window in range(2):                                   # the second window runs at lr > 0 and with non-zero moments
        c, n, t = _batch(window, full_b)
        l_full = float(full.step(c, n, t))
        before = [x.clone() for x in (acc.flat_p, acc.m, acc.v, acc.ema)]
        ep0, losses, per = acc.lr_scheduler.last_epoch, [], full_b // k
        for j in range(k):
            losses.append(float(acc.step(c[j * per:(j + 1) * per], n[j * per:(j + 1) * per], t[j * per:(j + 1) * per])))
            if j < k - 1:
                torch.cuda.synchronize()
                assert all(torch.equal(a, b) for a, b in zip(before, (acc.flat_p, acc.m, acc.v, acc.ema)))
                assert acc.step_count == window and acc.lr_scheduler.last_epoch == ep0
        torch.cuda.synchronize()
        assert acc.step_count == window + 1 == full.step_count and acc.lr_scheduler.last_epoch == ep0 + 1 and acc.last_lr == full.last_lr
        e_g, name, e_flat, left_out = _per_tensor_rel_l2(list(acc.model.named_parameters()), acc.flat_g, full.flat_g)
        assert all(x.endswith('to_k.bias') for x in left_out), left_out
        e_l = abs(sum(losses) - l_full) / l_full
        norm_acc = float(acc.flat_g.double().norm())
        e_norm = abs(float(acc.last_grad_norm) - norm_acc) / norm_acc
        e_norm_full = abs(float(acc.last_grad_norm) - float(full.last_grad_norm)) / float(full.last_grad_norm)
        note(report, 'accum_k%d_window%d' % (k, window), grad_rel_l2_worst=e_g, worst_tensor=name, grad_flat_rel=e_flat, noise_only=len(left_out), loss_rel=e_l,
             clip_norm_rel=e_norm, clip_norm_vs_full_rel=e_norm_full, grad_norm=norm_acc, bound=1e-5)
        assert e_g <= 1e-5 and e_flat <= 1e-5 and e_l <= 1e-5 and e_norm <= 1e-5 and e_norm_full <= 1e-5
        assert norm_acc > 1.0                                 # the clip is active: max_grad_norm = 1


# One channel per GroupNorm group at LDM_TINY_CFG's width, so a constant per channel in front of a GroupNorm has an exactly-zero
# gradient in exact arithmetic.  These, and only these, add one: inside a ResBlock the first conv's bias and the time-embedding
# projection (in front of out_layers.0); on the residual stream, whose readers are GroupNorms (through 1x1 skips at most), the
# stem's bias, a ResBlock's last conv and 1x1 skip, a transformer's output projection, and inside it (in front of proj_out, which
# is linear per pixel) the attention output and the feed-forward's last bias.  Not: norm affines, the time MLP, proj_in, the
# feed-forward's first layer, resampling convs (zero padding breaks the constant), the output conv.
LDM_ZERO_GRAD = ('.in_layers.2.bias', '.emb_layers.1.weight', '.emb_layers.1.bias', '.out_layers.3.bias', '.skip_connection.bias',
                 'input_blocks.0.0.bias', '.proj_out.bias', '.to_out.0.bias', '.ff.net.2.bias')


def _shadow_chain(dtype, s0, weights, decays):
    """k-1 EMA-only updates on the old weights, then the update's EMA on the new ones, per window: weights = [(old, new, k)]."""
    s = s0.to(dtype).clone()
    it = iter(decays)
    for old, new, k in weights:
        for j in range(k):
            d = next(it)
            omd = 1.0 - d if dtype == torch.float64 else float(np.float32(1) - np.float32(d))
            s.sub_(omd * (s - (new if j == k - 1 else old).to(dtype)))
    return s


def test_ldm_accumulation_equals_the_full_batch(report):
    """B = 4 in one call against 2 x 2 (id 3 in both micro-batches): gradients per tensor as above, embedding rows included;
    num_updates advances by k per window; the shadow against an fp64 restatement of "k-1 EMA-only updates on the old weights, then
    the update and its EMA" over the engine's own weights, within max(4 e_ref32, 2^-23 max|shadow|) (e_ref32: the same chain in
    fp32 torch) -- the rule of test_ldm_finetune_gpu for the shadow."""
    *_, full = _ldm(use_ema=True)
    *_, acc = _ldm(use_ema=True, accumulate_grad_batches=2)
    s0, chain = acc.ema.detach().cpu().clone(), []
    named = acc._state_named()
    for window in range(2):
        for dst, src in ((acc.flat_p, full.flat_p), (acc.m, full.m), (acc.v, full.v)):
            dst.copy_(src)                                    # both sides enter the window at the same weights and moments: what is
        acc._weights_changed()                                # compared is the association of one batch, not two diverging runs
        l_full = float(full.step(**_ldm_batch(window)))
        old = acc.flat_p[:acc.n_unet].detach().cpu().clone()
        before = [x.clone() for x in (acc.flat_p, acc.m, acc.v)]
        l0 = float(acc.step(**_ldm_batch(window, slice(0, 2))))
        torch.cuda.synchronize()
        assert all(torch.equal(a, b) for a, b in zip(before, (acc.flat_p, acc.m, acc.v)))
        assert acc.num_updates == 2 * window + 1 and acc.step_count == window
        l1 = float(acc.step(**_ldm_batch(window, slice(2, 4))))
        torch.cuda.synchronize()
        assert acc.num_updates == 2 * window + 2 and acc.step_count == window + 1
        chain.append((old, acc.flat_p[:acc.n_unet].detach().cpu().clone(), 2))
        e_g, name, e_flat, left_out = _per_tensor_rel_l2(named, acc.flat_g, full.flat_g)
        rows = sorted(set(LDM_IDS))
        ge, gf = acc.embedder.embedding.weight.grad, full.embedder.embedding.weight.grad
        e_rows = R.rel_l2(ge[rows], gf[rows])
        untouched = [i for i in range(1001) if i not in rows]
        assert float(ge[untouched].abs().max()) == 0.0
        e_l = abs(l0 + l1 - l_full) / l_full
        note(report, 'accum_ldm_window%d' % window, grad_rel_l2_worst=e_g, worst_tensor=name, grad_flat_rel=e_flat, noise_only=len(left_out), emb_rows_rel_l2=e_rows,
             loss_rel=e_l, bound=1e-5, noise_names=','.join(left_out))
        assert all(x.endswith(LDM_ZERO_GRAD) for x in left_out), left_out
        assert e_g <= 1e-5 and e_flat <= 1e-5 and e_rows <= 1e-5 and e_l <= 1e-5
    decays = R.lit_ema_decays(0.9999, 4)
    s64, s32 = _shadow_chain(torch.float64, s0, chain, decays), _shadow_chain(torch.float32, s0, chain, decays)
    e_hip = float((acc.ema.detach().cpu().double() - s64).abs().max())
    e_ref = float((s32.double() - s64).abs().max())
    bound = max(4 * e_ref, 2.0 ** -23 * float(s64.abs().max()))
    note(report, 'accum_ldm_shadow', e_hip=e_hip, e_ref32=e_ref, bound=bound)
    assert e_hip <= bound
    # a shadow that skipped the non-stepping batches (what a per-step EMA would give) is far outside the bound
    skipped = _shadow_chain(torch.float64, s0, [(o, n_, 1) for o, n_, _ in chain], decays[1::2])
    assert float((skipped - s64).abs().max()) > 10 * bound


# ---- dp_ema_update ---------------------------------------------------------------------------------------------------
def _launched(ops, fn):
    lib = ops._lib()
    c0 = lib.dp_launch_count()
    fn()
    n = lib.dp_launch_count() - c0
    arr = (ctypes.c_char_p * 256)()
    k = lib.dp_recent_launches(arr, 256)
    names = [arr[i].decode() for i in range(k - n, k)]
    return [s[1:-1] if s.startswith('(') else s for s in names]


@pytest.mark.parametrize('offset', [0, 1])
@pytest.mark.parametrize('n', [1, 5, 1027, 8388613])
def test_ema_update_kernel(report, n, offset):
    """Three chained updates at LitEma's warm-up decays: against fp64 within max(4 e_ref32, 2^-23 max|shadow|), e_ref32 the fp32
    torch expression's own error; BIT-equal to dp_adamw_ema run with zero gradient, zero moments and zero weight decay on the same
    buffers (which leaves p unchanged and applies only its EMA half); a view at element offset 1 takes the 4-byte path; the launch
    ring shows the kernel."""
    ops = pkg('ops')
    g_ = torch.Generator().manual_seed(n)
    p0, s0 = torch.randn(n, generator=g_), torch.randn(n, generator=g_)
    decays = R.lit_ema_decays(0.9999, 3)
    bufs = [torch.full((n + 5,), 777.0, device=DEV) for _ in range(6)]
    s, p, s2, p2, m, v = (b[offset:offset + n] for b in bufs)
    g = torch.zeros(n + 5, device=DEV)[offset:offset + n]
    for t, src in ((s, s0), (p, p0), (s2, s0), (p2, p0)):
        t.copy_(src)
    m.zero_(); v.zero_()
    s64, s32 = s0.double(), s0.clone()
    want = 'ema_update_kernel<%s>' % ('true' if offset == 0 and n >= 4 else 'false')
    for k, d in enumerate(decays):
        names = _launched(ops, lambda: ops.ema_update(s, p, d))
        assert names == [want], names
        ops.adamw_ema(p2, g, m, v, s2, 1e-3, 0.9, 0.999, 1e-8, 0.0, k + 1, d)
        s64.sub_((1.0 - d) * (s64 - p0.double()))
        s32.sub_(float(np.float32(1) - np.float32(d)) * (s32 - p0))
    torch.cuda.synchronize()
    assert torch.equal(p2.cpu(), p0) and torch.equal(p.cpu(), p0) and not bool(m.any()) and not bool(v.any())
    assert torch.equal(s, s2)                                   # the EMA half of dp_adamw_ema, bit for bit
    for b in bufs[:2]:                                          # nothing outside the view is written
        assert bool((b[:offset] == 777.0).all()) and bool((b[offset + n:] == 777.0).all())
    e_hip = float((s.double().cpu() - s64).abs().max())
    e_ref = float((s32.double() - s64).abs().max())
    bound = max(4 * e_ref, 2.0 ** -23 * float(s64.abs().max()))
    note(report, 'ema_update_n%d_off%d' % (n, offset), e_hip=e_hip, e_ref32=e_ref, bound=bound, kernel=want)
    assert e_hip <= bound


def test_ema_update_mixed_alignment_takes_the_scalar_path():
    ops = pkg('ops')
    n = 1027
    a, b = torch.randn(n + 1, device=DEV), torch.randn(n + 1, device=DEV)
    ref = a[1:].clone()
    ops.ema_update(ref, b[:n].clone(), 0.25)
    s = a[1:].clone()                                           # (an aligned copy of the same values)
    names = _launched(ops, lambda: ops.ema_update(a[1:], b[:n], 0.25))
    assert names == ['ema_update_kernel<false>'] and torch.equal(a[1:], ref) and not torch.equal(a[1:], s)


def _optimizer_operands(n, seed, pad=0, offset=0):
    """Seeded p, g, m, v (>= 0), shadow as views at element `offset` of device buffers of n + pad elements."""
    g_ = torch.Generator().manual_seed(seed)
    host = [torch.randn(n, generator=g_), torch.randn(n, generator=g_), 0.1 * torch.randn(n, generator=g_),
            torch.rand(n, generator=g_), torch.randn(n, generator=g_)]
    out = []
    for h in host:
        t = torch.full((n + pad,), 777.0, device=DEV)[offset:offset + n]
        t.copy_(h)
        out.append(t)
    return out


@pytest.mark.parametrize('n', [1, 255, 257, 1027, 8192 * 256 + 77])
def test_adam_ema_host_and_device_scalars_agree_bitwise(n):
    """adam_ema_kernel (lr and the bias corrections by value) and adam_ema_dev_kernel (the same three read from the buffer
    set_step_scalars fills: the replayed step) run ONE shared device function: the same seeded operands give the same bits in p, m,
    v and the shadow -- with and without shadow, with and without clip coefficient, at step 1 and 1000.  n: the one-thread grid, both
    sides of the block edge, a ragged end over several blocks, and a grid-stride turn past the 8192-block cap."""
    ops = pkg('ops')
    lr, b1, b2, eps, decay = 2e-4, 0.9, 0.999, 1e-8, 0.9999
    coef_t = torch.tensor([0.37], device=DEV)
    hyper = torch.zeros(4, device=DEV)
    for use_ema in (True, False):
        for coef in (coef_t, None):
            for step in (1, 1000):
                p, g, m, v, s = _optimizer_operands(n, n + step)
                p2, m2, v2, s2 = p.clone(), m.clone(), v.clone(), s.clone()
                ops.adam_ema(p, g, m, v, s if use_ema else None, coef, lr, b1, b2, eps, step, decay)
                ops.set_step_scalars(hyper, lr, b1, b2, step)
                ops.adam_ema_dev(p2, g, m2, v2, s2 if use_ema else None, coef, hyper, b1, b2, eps, decay)
                torch.cuda.synchronize()
                assert int(hyper.view(torch.int32)[3]) == step
                for name, a, b in (('p', p, p2), ('m', m, m2), ('v', v, v2), ('ema', s, s2)):
                    assert torch.equal(a, b), (name, use_ema, coef is not None, step)
                assert bool(torch.isfinite(p).all())


@pytest.mark.parametrize('d', ['warmup', 0.9999])
@pytest.mark.parametrize('offset', [0, 1])
@pytest.mark.parametrize('n', [1, 3, 4, 1027])
def test_fused_and_standalone_litema_agree_bitwise(n, offset, d):
    """One AdamW step with the LitEma shadow fused in == the same step without a shadow followed by dp_ema_update, bit for bit in
    the shadow and in p, m, v: both kernels call the one dp_lit_ema of csrc/dp_common.h (the guarantee the header of csrc/ema.hip
    states).  Element offset 0 with n >= 4 takes the 16-byte path of both kernels, everything else the 4-byte path; d: the first
    warm-up decay of lit_ema_decay (2/11 in fp32) and the cap."""
    ops = pkg('ops')
    d = pkg('ldm_train').lit_ema_decay(0.9999, 1) if d == 'warmup' else d
    args = (1.28e-4, 0.9, 0.999, 1e-8, 1e-2, 3)
    p, g, m, v, s = _optimizer_operands(n, 17 * n + offset, pad=5, offset=offset)
    p2, g2, m2, v2, s2 = _optimizer_operands(n, 17 * n + offset, pad=5, offset=offset)
    assert torch.equal(p, p2) and torch.equal(s, s2)
    vec = 'true' if offset == 0 and n >= 4 else 'false'
    assert _launched(ops, lambda: ops.adamw_ema(p, g, m, v, s, *args, ema_decay=d)) == ['adamw_ema_kernel<%s>' % vec]
    names = _launched(ops, lambda: (ops.adamw_ema(p2, g2, m2, v2, None, *args), ops.ema_update(s2, p2, d)))
    assert names == ['adamw_ema_kernel<%s>' % vec, 'ema_update_kernel<%s>' % vec]
    torch.cuda.synchronize()
    for name, a, b in (('shadow', s, s2), ('p', p, p2), ('m', m, m2), ('v', v, v2)):
        assert torch.equal(a, b), name
    p0, _, _, _, s0 = _optimizer_operands(n, 17 * n + offset)
    assert not torch.equal(p, p0) and not torch.equal(s, s0)          # both moved


# ---- torch's optimizer layout ----------------------------------------------------------------------------------------
def test_torch_adam_loads_the_exported_state_and_steps_alike(report):
    """torch.optim.Adam loads optimizer_state_dict(); one torch step on clones with the engine's next (clipped) gradient lands within
    1e-5 relative of the engine's parameters (the project's bound for its update on identical gradients); export -> import gives the
    same bits."""
    model, ft = _ddpm(replay=False, lr_scheduler=None, lr=2e-4)
    [ft.step(*_batch(k)) for k in range(2)]
    sd = ft.optimizer_state_dict()
    clones = [torch.nn.Parameter(p.detach().cpu().clone()) for p in model.parameters()]
    opt = torch.optim.Adam(clones, lr=2e-4, betas=(0.9, 0.999), eps=1e-8)
    assert set(sd['param_groups'][0]) == set(opt.state_dict()['param_groups'][0])
    opt.load_state_dict(sd)
    assert all(float(opt.state[p]['step']) == 2.0 and opt.state[p]['step'].dtype == torch.float32 for p in clones)
    m, v = ft.m.clone(), ft.v.clone()
    ft.load_optimizer_state_dict(opt.state_dict())
    assert torch.equal(ft.m, m) and torch.equal(ft.v, v) and ft.step_count == 2
    ft.step(*_batch(2))
    torch.cuda.synchronize()
    for c, p in zip(clones, model.parameters()):
        c.grad = p.grad.detach().cpu().clone()
    torch.nn.utils.clip_grad_norm_(clones, 1.0)
    opt.step()
    e = max(relerr(p.detach(), c.detach()) for c, p in zip(clones, model.parameters()))
    note(report, 'torch_adam_step', param_rel_worst=e, bound=1e-5)
    assert e <= 1e-5


def test_torch_adamw_loads_the_exported_ldm_state_and_steps_alike(report):
    m_, e_, ft = _ldm(use_ema=False)
    [ft.step(**_ldm_batch(k)) for k in range(2)]
    sd = ft.optimizer_state_dict()
    params = list(m_.parameters()) + list(e_.parameters())       # UNet, then the embedder (ddpm.py:1372-1381)
    clones = [torch.nn.Parameter(p.detach().cpu().clone()) for p in params]
    opt = torch.optim.AdamW(clones, lr=1.28e-4)
    assert set(sd['param_groups'][0]) == set(opt.state_dict()['param_groups'][0])
    opt.load_state_dict(sd)
    m, v = ft.m.clone(), ft.v.clone()
    ft.load_optimizer_state_dict(opt.state_dict())
    assert torch.equal(ft.m, m) and torch.equal(ft.v, v) and ft.step_count == 2
    ft.step(**_ldm_batch(2))
    torch.cuda.synchronize()
    for c, p in zip(clones, params):
        c.grad = p.grad.detach().cpu().clone()
    opt.step()
    e = max(relerr(p.detach(), c.detach()) for c, p in zip(clones, params))
    note(report, 'torch_adamw_step', param_rel_worst=e, bound=1e-5)
    assert e <= 1e-5


# ---- the reference's own states ----------------------------------------------------------------------------------------
def _fixture_arrays(tag):
    out = {}
    for k in ('exp_avg', 'exp_avg_sq', 'shadow', 'params_final'):
        z = load_npz('train_state_%s_%s.npz' % (tag, k))
        out[k] = (z['fp32'].astype(np.float64), z['fp32'].astype(np.float64) + z['delta64'].astype(np.float64))
    return out


def _samples(names, tensors):
    return np.concatenate([t.detach().reshape(-1).double().cpu().numpy()[R.sample_index(t.numel(), name=n, row=t.shape[-1] if t.dim() else 1)]
                           for n, t in zip(names, tensors)])


def _sizes(names, tensors):
    return [len(R.sample_index(t.numel(), name=n, row=t.shape[-1] if t.dim() else 1)) for n, t in zip(names, tensors)]


def _check_rule(report, key, got, pair, floor, per_tensor=None):
    """max |got - fp64| over all samples / max |fp64| <= max(4 e_ref32, floor), e_ref32 the reference's fp32 run in that measure.
    per_tensor = (names, sample counts): the same rule tensor by tensor, in the same scale -- max |got_i - fp64_i| <=
    max(4 max |fp32_i - fp64_i|, floor * max |fp64|) -- so that a tensor put in another's place (the `ckpt.pth` permutation) shows
    even where the worst tensor's reference error would cover it.  Applied to the moments, whose rounding noise (a gradient that is
    zero in exact arithmetic) lies below the floor, and to a shadow at decay 0.9999, which takes 1e-4 of any parameter difference; not
    to the parameters after a step or a warm-up shadow that follows them: Adam's update of a noise gradient is +-lr per element
    whichever way the rounding fell, so there the reference's fp32 error of ONE tensor's samples says nothing about another fp32 run's."""
    f32, f64 = pair
    scale = float(np.abs(f64).max())
    e_hip, e_ref = float(np.abs(got - f64).max()) / scale, float(np.abs(f32 - f64).max()) / scale
    bound = max(4 * e_ref, floor)
    vals = dict(e_hip=e_hip, e_ref32=e_ref, bound=bound)
    worst = None
    if per_tensor is not None:
        off = 0
        for n, k in zip(*per_tensor):
            sl = slice(off, off + k)
            off += k
            e_i, b_i = float(np.abs(got[sl] - f64[sl]).max()) / scale, max(4 * float(np.abs(f32[sl] - f64[sl]).max()) / scale, floor)
            if worst is None or e_i / b_i > worst[0] / worst[1]:
                worst = (e_i, b_i, n)
        assert off == len(got) == len(f64)
        vals.update(per_tensor_worst=worst[0], its_bound=worst[1], its_name=worst[2])
    note(report, key, **vals)
    assert e_hip <= bound, (key, e_hip, bound)
    assert worst is None or worst[0] <= worst[1], (key, worst)


def test_ddpm_exp_states_against_the_reference(report, tmp_path):
    """The DDIM code base's model / get_optimizer / EMAHelper ran 3 + 2 steps (fixture); the engine runs the same steps (dropout 0).
    At step 3 its `ckpt.pth` list has the fixture's structure, `step` values and parameter order; exp_avg within
    max(4 e_ref32, 2e-5) and exp_avg_sq within max(4 e_ref32, 4e-5) of the reference's fp64 run (the gradient floor: exp_avg is
    linear in g, exp_avg_sq quadratic), the shadow within max(4 e_ref32, 2^-23); reloading the file continues bit for bit, and the
    later steps follow the reference: losses within max(4 e_ref32, 1e-5) (the loss floor of tests/ldm_finetune_ref.py), the parameters
    after step 5 within max(4 e_ref32, 1e-5) (the project's bound for its update on identical gradients).  Measure of every array
    figure: max |a - fp64| over the stored samples of all tensors / max |fp64| -- Adam's moments of a gradient that is zero in
    exact arithmetic (one channel per GroupNorm group at this width) are rounding noise, which only an absolute measure bounds."""
    train, diffusion, ckpt, unet = pkg('train'), pkg('diffusion'), pkg('checkpoint'), pkg('unet')
    fx = load_json('train_state.json')['ddpm']
    arr = _fixture_arrays('ddpm')
    cfg, orig = original_state_dict(ckpt, fx['arch'], fx['seed'], unet.UNet2DModel)
    g = fx['param_groups'][0]

    def build():
        model = unet.UNet2DModel(**cfg)
        model.load_state_dict(ckpt.convert_ddpm_original(orig), strict=True)
        model = model.to(DEV)
        return model, train.FinetuneEngine(model, diffusion.DDPMScheduler(), lr=g['lr'], betas=tuple(g['betas']), eps=g['eps'],
                                           ema_decay=fx['ema_rate'], max_grad_norm=fx['grad_clip'], dropout=0.0, replay=False)

    def steps(ft, ks):
        out = []
        for k in ks:
            c = torch.from_numpy(gc.det_clean((fx['batch'], 3, 16, 16), fx['clean_seed'] + k)).to(DEV)
            n = torch.from_numpy(gc.det_noise((fx['batch'], 3, 16, 16), fx['noise_seed'] + k)).to(DEV)
            t = train.antithetic_timesteps(fx['batch'], 1000, torch.Generator().manual_seed(fx['t_seed'] + k))
            assert t.tolist() == fx['timesteps'][k]
            out.append(float(ft.step(c, n, t)))
        return out
    a, n = fx['save_at'], fx['save_at'] + fx['further']
    model, ft = build()
    losses = steps(ft, range(a))
    path = str(tmp_path / 'ckpt.pth')
    ckpt.save_ddpm_exp_states(path, ft, epoch=fx['epoch'])
    states = torch.load(path, weights_only=True)
    names = fx['param_names']
    assert len(states) == fx['states_len'] and list(states[0]) == names and states[2:4] == [fx['epoch'], fx['step']]
    assert list(states[1]) == fx['optimizer_keys'] and sorted(states[1]['state'][0]) == sorted(fx['state_keys'])
    assert set(states[1]['param_groups'][0]) == set(g) and states[1]['param_groups'][0]['params'] == g['params']
    assert {k: v for k, v in states[1]['param_groups'][0].items() if k != 'betas'} == {k: v for k, v in g.items() if k != 'betas'}
    assert list(states[1]['param_groups'][0]['betas']) == g['betas']
    assert type(states[4]).__name__ == fx['ema_type'] and len(states[4]) == fx['ema_len']
    st = states[1]['state']
    assert [float(st[i]['step']) for i in range(len(names))] == fx['steps']
    assert all(str(st[i]['step'].dtype) == fx['step_dtype'] and st[i]['step'].dim() == fx['step_dim'] for i in range(len(names)))
    assert all(list(st[i]['exp_avg'].shape) == fx['shapes'][n_] == list(states[4][i].shape) == list(states[0][n_].shape)
               for i, n_ in enumerate(names))
    per = (names, _sizes(names, list(states[4])))
    _check_rule(report, 'ddpm_ref_exp_avg', _samples(names, [st[i]['exp_avg'] for i in range(len(names))]), arr['exp_avg'], 2e-5, per)
    _check_rule(report, 'ddpm_ref_exp_avg_sq', _samples(names, [st[i]['exp_avg_sq'] for i in range(len(names))]), arr['exp_avg_sq'], 4e-5, per)
    _check_rule(report, 'ddpm_ref_shadow', _samples(names, list(states[4])), arr['shadow'], 2.0 ** -23, per)
    # reloading the file continues bit for bit; the later steps follow the reference
    losses += steps(ft, range(a, n))
    _, second = build()
    assert ckpt.load_ddpm_exp_states(path, second) == (fx['epoch'], fx['step'])
    assert steps(second, range(a, n)) == losses[a:] and _same(ft, second)
    e_l = max(abs(x - y) / abs(y) for x, y in zip(losses, fx['losses_fp64']))
    bound_l = max(4 * fx['e_ref32']['loss'], 1e-5)
    note(report, 'ddpm_ref_losses', e_hip=e_l, e_ref32=fx['e_ref32']['loss'], bound=bound_l, losses=losses)
    assert e_l <= bound_l
    final = ckpt.convert_to_ddpm_original({k: v.detach() for k, v in model.named_parameters()})
    _check_rule(report, 'ddpm_ref_params_final', _samples(names, [final[n_] for n_ in names]), arr['params_final'], 1e-5)


def test_ldm_optimizer_state_against_the_reference(report, tmp_path):
    """LatentDiffusion + AdamW + LitEma ran 2 + 1 steps at LDM_TINY_CFG (fixture); the engine's exported AdamW state has the
    reference's keys, `step` values and parameter order (UNet, then the embedder), its moments and shadow obey the same rule, and
    the `last.ckpt` form written from it continues bit for bit."""
    ckpt = pkg('checkpoint')
    fx = load_json('train_state.json')['ldm']
    arr = _fixture_arrays('ldm')
    assert fx['config'] == {k: (list(v) if isinstance(v, tuple) else v) for k, v in gc.LDM_TINY_CFG.items()} and fx['class_ids'] == LDM_IDS
    a, n = fx['save_at'], fx['save_at'] + fx['further']
    kw = dict(use_ema=True, ema_decay=fx['ema_decay'])
    m1, e1, ft = _ldm(**kw)

    def steps(eng, ks):
        return [float(eng.step(**_ldm_batch(k, x_seed=fx['x_seed'], noise_seed=fx['noise_seed']))) for k in ks]
    losses = steps(ft, range(a))
    sd = ft.optimizer_state_dict()
    names = fx['param_names']
    ours = [n_ for n_, _ in ft._state_named()]
    assert ours == [ckpt.LDM_UNET_PREFIX + n_ for n_ in names[:-1]] + [ckpt.LDM_EMBEDDER_PREFIX + names[-1]]
    g = fx['param_groups'][0]
    assert list(sd) == fx['optimizer_keys'] and sorted(sd['state'][0]) == sorted(fx['state_keys'])
    assert {k: v for k, v in sd['param_groups'][0].items() if k != 'betas'} == {k: v for k, v in g.items() if k != 'betas'}
    assert list(sd['param_groups'][0]['betas']) == g['betas']
    assert [float(sd['state'][i]['step']) for i in range(len(names))] == fx['steps'] and str(sd['state'][0]['step'].dtype) == fx['step_dtype']
    assert [list(sd['state'][i]['exp_avg'].shape) for i in range(len(names))] == fx['shapes'] and ft.num_updates == fx['num_updates']
    per = (names, _sizes(names, [sd['state'][i]['exp_avg'] for i in range(len(names))]))
    _check_rule(report, 'ldm_ref_exp_avg', _samples(names, [sd['state'][i]['exp_avg'] for i in range(len(names))]), arr['exp_avg'], 2e-5, per)
    _check_rule(report, 'ldm_ref_exp_avg_sq', _samples(names, [sd['state'][i]['exp_avg_sq'] for i in range(len(names))]), arr['exp_avg_sq'], 4e-5, per)
    es = ft.ema_state()
    _check_rule(report, 'ldm_ref_shadow', _samples(names[:-1], [es[n_] for n_ in names[:-1]]), arr['shadow'], 2.0 ** -23)
    path = str(tmp_path / 'last.ckpt')
    ckpt.save_ldm_finetuned(path, m1, e1, ema=ft, training_state=ft)
    losses += steps(ft, range(a, n))
    m2, e2, second = _ldm(**kw)
    ckpt.load_ldm_finetuned(path, m2, e2, engine=second)
    assert steps(second, range(a, n)) == losses[a:] and _same(ft, second)
    e_l = max(abs(x - y) / abs(y) for x, y in zip(losses, fx['losses_fp64']))
    bound_l = max(4 * fx['e_ref32']['loss'], 1e-5)
    note(report, 'ldm_ref_losses', e_hip=e_l, e_ref32=fx['e_ref32']['loss'], bound=bound_l, losses=losses)
    assert e_l <= bound_l
    final = [p for _, p in ft._state_named()]
    _check_rule(report, 'ldm_ref_params_final', _samples(names, final), arr['params_final'], 1e-5)
