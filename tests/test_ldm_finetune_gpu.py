"""LDM finetune step on the MI355X: dp_adamw_ema against fp64 AdamW, dp_embedding_bwd bit for bit against the ascending-b loop,
the context gradient of LdmEngine.backward against the reference's stored embedding-row gradients and the fp64 restatement, the
reference's own K = 3 training steps (tests/golden/ldm_finetune.{npz,json}) end to end on ldm_train.LdmFinetuneEngine, a pruned
model, cin256-v2 at full size in a child interpreter, and the step under a one-rank RCCL group.

Rule of every comparison (README, "max(4 e_ref32, floor)"): e_hip and e_ref32 are distances from the fp64 restatement of
tests/ldm_finetune_ref.py; the HIP path may be 4 times as far from fp64 as the reference's fp32 is, and a floor keeps a luckily
small e_ref32 from asking for more than fp32 can give.  Every measured figure is printed next to its bound."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import golden_common as gc
import ldm_finetune_ref as R
from conftest import isolated
from helpers import load_json, load_npz, pkg, relerr

pytestmark = pytest.mark.gpu
DEV = 'cuda'
HERE = os.path.dirname(os.path.abspath(__file__))


# ---- dp_adamw_ema ---------------------------------------------------------------------------------------------------
def _adamw_case(n, seed):
    """Seeded buffers with three regions: gradients exactly 0 (pure decay), denormal-small, and ordinary."""
    g_ = torch.Generator().manual_seed(seed)
    p = torch.randn(n, generator=g_)
    grads = []
    for _ in range(5):
        g = torch.randn(n, generator=g_) * 0.1
        g[: n // 4] = 0.0
        g[n // 4: n // 2] *= 1e-39
        grads.append(g)
    return p, grads


def _adamw_cpu(p0, grads, lr, wd, dtype, decays):
    """torch.optim.AdamW (single tensor) + the LitEma formula on the CPU in `dtype`: (p, m, v, shadow)."""
    p = p0.to(dtype).clone().requires_grad_(True)
    opt = torch.optim.AdamW([p], lr=lr, betas=R.BETAS, eps=R.EPS, weight_decay=wd, foreach=False)
    s = p.detach().clone()
    for g, d in zip(grads, decays):
        p.grad = g.to(dtype)
        opt.step()
        omd = 1.0 - d if dtype == torch.float64 else float(np.float32(1) - np.float32(d))
        with torch.no_grad():
            s.sub_(omd * (s - p))
    st = opt.state[p]
    return p.detach(), st['exp_avg'], st['exp_avg_sq'], s


@pytest.mark.parametrize('use_ema', [False, True])
@pytest.mark.parametrize('n', [1, 3, 4, 1023, 2 ** 20 + 5, 2 ** 24 + 3])
def test_adamw_ema_kernel_matches_fp64_adamw(report, n, use_ema):
    """5 chained steps (bias corrections) for wd 0 / 1e-2 / 0.1: every buffer within max(4 e_ref32, 2^-23 max|buffer|) of fp64 AdamW,
    e_ref32 from torch.optim.AdamW in fp32 on the CPU; where the gradient is exactly 0, p equals fl(p fl(1 - lr wd)) per step bit
    for bit; with wd = 0 and no EMA, within the same bound of dp_adam_ema."""
    ops = pkg('ops')
    lr = 1.28e-4
    decays = R.lit_ema_decays(0.9999, 5)
    p0, grads = _adamw_case(n, 1000 + n)
    for wd in (0.0, 1e-2, 0.1):
        ref64 = _adamw_cpu(p0, grads, lr, wd, torch.float64, decays)
        ref32 = _adamw_cpu(p0, grads, lr, wd, torch.float32, decays)
        p, m, v = p0.to(DEV).clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
        s = p.clone() if use_ema else None
        for k, g in enumerate(grads):
            ops.adamw_ema(p, g.to(DEV), m, v, s, lr, R.BETAS[0], R.BETAS[1], R.EPS, wd, k + 1, decays[k])
        torch.cuda.synchronize()
        bufs = (('p', p), ('m', m), ('v', v)) + ((('ema', s),) if use_ema else ())
        for (name, got), a64, a32 in zip(bufs, ref64, ref32):
            e_hip = float((got.double().cpu() - a64).abs().max())
            e_ref = float((a32.double() - a64).abs().max())
            bound = max(4 * e_ref, 2.0 ** -23 * float(a64.abs().max()))
            print('adamw n=%d ema=%d wd=%g %-3s e_hip %.3e e_ref32 %.3e bound %.3e' % (n, use_ema, wd, name, e_hip, e_ref, bound))
            report.setdefault('ldm_finetune/adamw', {})['n%d_ema%d_wd%g_%s' % (n, use_ema, wd, name)] = [e_hip, e_ref, bound]
            assert e_hip <= bound, (name, wd, e_hip, bound)
        if n >= 4:                                       # pure decay: one fp32 multiplication by fl(1 - lr wd) per step
            f = np.float32(1.0 - lr * wd)
            want = p0[: n // 4].numpy()
            for _ in grads:
                want = want * f
            assert np.array_equal(p[: n // 4].cpu().numpy(), want)
            assert torch.equal(m[: n // 4].cpu(), torch.zeros(n // 4)) and torch.equal(v[: n // 4].cpu(), torch.zeros(n // 4))
        if wd == 0.0 and not use_ema:                    # the same mathematics as dp_adam_ema
            p2, m2, v2 = p0.to(DEV).clone(), torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
            for k, g in enumerate(grads):
                ops.adam_ema(p2, g.to(DEV), m2, v2, None, None, lr, R.BETAS[0], R.BETAS[1], R.EPS, k + 1, 0.0)
            torch.cuda.synchronize()
            e_ref = float((ref32[0].double() - ref64[0]).abs().max())
            bound = max(4 * e_ref, 2.0 ** -23 * float(ref64[0].abs().max()))
            d = float((p.double() - p2.double()).abs().max())
            print('adamw n=%d vs dp_adam_ema: %.3e bound %.3e' % (n, d, bound))
            assert d <= bound


def test_adamw_ema_kernel_unaligned_views_take_the_scalar_path():
    """Slices that start 4 bytes into an allocation (the embedder's range of a flat buffer whose UNet part is odd) give the same
    bits as aligned buffers."""
    ops = pkg('ops')
    n = 4099
    p0, grads = _adamw_case(n, 7)
    outs = []
    for off in (0, 1):
        bufs = [torch.zeros(n + 1, device=DEV) for _ in range(5)]
        p, g, m, v, s = (b[off:off + n] for b in bufs)
        p.copy_(p0)
        s.copy_(p0)
        for k, gk in enumerate(grads[:2]):
            g.copy_(gk)
            ops.adamw_ema(p, g, m, v, s, 1e-3, 0.9, 0.999, 1e-8, 1e-2, k + 1, 0.25)
        outs.append([t.clone() for t in (p, m, v, s)])
    torch.cuda.synchronize()
    assert all(torch.equal(a, b) for a, b in zip(*outs))


# ---- dp_embedding_bwd -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('D', [16, 512])
@pytest.mark.parametrize('B', [1, 6, 16, 256, 4096])
def test_embedding_bwd_is_the_ascending_b_sum_bit_for_bit(B, D):
    ops = pkg('ops')
    n_classes = 5000
    g_ = torch.Generator().manual_seed(B * 1000 + D)
    for kind in ('distinct', 'repeats', 'equal'):
        if kind == 'distinct':
            ids = torch.randperm(n_classes, generator=g_)[:B]
        elif kind == 'repeats':
            ids = torch.randint(0, max(2, B // 3), (B,), generator=g_) * 7 % n_classes
        else:
            ids = torch.full((B,), 1000, dtype=torch.long)
        dctx = torch.randn(B, D, generator=g_)
        dW0 = torch.randn(n_classes, D, generator=g_)
        want = dW0.clone()
        for b in range(B):                               # fp32, ascending b
            want[int(ids[b])] += dctx[b]
        ids = ops.check_class_ids(ids, n_classes)
        runs = []
        for _ in range(2):
            dW = dW0.to(DEV).clone()
            ops.embedding_bwd(ids.to(DEV), dctx.to(DEV), dW)
            runs.append(dW)
        torch.cuda.synchronize()
        assert torch.equal(runs[0], runs[1]), kind
        assert torch.equal(runs[0].cpu(), want), (kind, float((runs[0].cpu() - want).abs().max()))
        touched = torch.zeros(n_classes, dtype=torch.bool)
        touched[ids] = True
        assert torch.equal(runs[0].cpu()[~touched], dW0[~touched])
    with pytest.raises(ValueError):
        ops.embedding_bwd(torch.zeros(4097, dtype=torch.long, device=DEV), torch.zeros(4097, D, device=DEV),
                          torch.zeros(n_classes, D, device=DEV))


# ---- context gradient -----------------------------------------------------------------------------------------------
def _ldm_model(cfg, seed=R.UNET_SEED):
    m = pkg('ldm').UNetModel(**cfg)
    gc.det_init_(m, seed)
    return m.to(DEV).eval()


def _engine_grads(model, x, t, ctx, noise, want):
    """One scored forward / backward at timesteps t (q_sample, eps loss) on the engine: ({name: grad}, d context | None, loss)."""
    ops = pkg('ops')
    eng = model.engine()
    grads = {n: torch.zeros_like(p) for n, p in model.named_parameters()}
    eng.bind(eng.P, grads)
    sa, sb = pkg('ldm_sweep').LdmSchedule().tables(torch.device(DEV, 0))
    x_noisy = ops.q_sample(x.to(DEV).contiguous(), noise.to(DEV).contiguous(), sa, sb, t.to(DEV))
    y = eng.forward(x_noisy, t.to(DEV), ctx.to(DEV), save=True)
    n = y.numel()
    loss, dout = ops.mse_fwd_bwd(y, noise.to(DEV), 2.0 / n, 1.0 / n)
    dctx = eng.backward(dout, want_context_grad=True) if want else eng.backward(dout)
    torch.cuda.synchronize()
    return grads, dctx, loss


def test_context_gradient_matches_reference_embedding_rows(report):
    """LDM_TINY_CFG at t = 250, ids [3, 500, 1000]: d loss / d context scattered into the embedding rows against
    `grad_embedding_rows` of ldm_loss_at_t.npz (written by the reference's LatentDiffusion + ClassEmbedder under autograd), by the
    rule with a floor of 2e-5 relative; with the switch off every parameter gradient is bit-identical and nothing is returned."""
    ops = pkg('ops')
    g = load_npz('ldm_loss_at_t.npz')
    cfg = gc.LDM_TINY_CFG
    ids = torch.from_numpy(g['class_ids']).long()
    k = list(g['ts']).index(250)
    B, H = len(ids), cfg['image_size']
    x = torch.from_numpy(gc.det_noise((B, cfg['in_channels'], H, H), 62))
    noise = torch.from_numpy(gc.det_noise((B, cfg['in_channels'], H, H), 70 + k))
    t = torch.full((B,), 250, dtype=torch.long)
    P, E = R.initial_weights(cfg, torch.float64)
    _, _, dE64 = R.loss_and_grads(P, E, cfg, x, ids, t, noise)
    rows64 = dE64[ids]
    model = _ldm_model(cfg)
    emb = torch.from_numpy(gc.det_param('embedding.weight', (R.N_CLASSES, cfg['context_dim']), R.EMB_SEED))
    ctx = emb[ids][:, None, :]
    grads_on, dctx, _ = _engine_grads(model, x, t, ctx, noise, True)
    grads_off, none, _ = _engine_grads(model, x, t, ctx, noise, False)
    assert none is None and tuple(dctx.shape) == (B, 1, cfg['context_dim'])
    assert all(torch.equal(grads_on[n], grads_off[n]) for n in grads_on)
    dW = torch.zeros(R.N_CLASSES, cfg['context_dim'], device=DEV)
    ops.embedding_bwd(ids.to(DEV), dctx.reshape(B, -1).contiguous(), dW)
    e_hip, e_ref = R.rel_l2(dW[ids.to(DEV)], rows64), R.rel_l2(g['grad_embedding_rows'], rows64)
    bound = max(4 * e_ref, 2e-5)
    print('context gradient rows: e_hip %.3e e_ref32 %.3e bound %.3e' % (e_hip, e_ref, bound))
    report['ldm_finetune/context_rows'] = dict(e_hip=e_hip, e_ref32=e_ref, bound=bound)
    assert e_hip <= bound
    assert float(dW.abs().sum(dim=1).cpu()[[i for i in range(R.N_CLASSES) if i not in ids.tolist()]].max()) == 0.0


def test_context_gradient_over_three_tokens_and_several_heads(report):
    """hc16_L3 (heads of 16 channels, L = 3 context tokens): the input gradients of attn2.to_k and attn2.to_v, accumulated over the
    blocks, against the fp64 restatement with context.requires_grad_(); e_ref32 is the fp32 restatement's; switch off: bit-identical
    parameter gradients."""
    rec = load_json('ldm_heads.json')['hc16_L3']
    cfg = rec['cfg']
    x = torch.from_numpy(gc.det_noise((2, 3, 16, 16), 31))
    ctx = torch.from_numpy(gc.det_noise((2, rec['context_tokens'], cfg['context_dim']), 32))
    noise = torch.from_numpy(gc.det_noise((2, 3, 16, 16), 33))
    t = torch.tensor([7, 640])
    shapes = {n: tuple(s) for n, s in rec['shapes'].items()}
    ref = {}
    for dtype in (torch.float64, torch.float32):
        P, E = R.initial_weights(cfg, dtype, shapes=shapes)
        _, _, ref[dtype] = R.loss_and_grads(P, E, cfg, x, None, t, noise, context=ctx.to(dtype).clone())
    model = _ldm_model(cfg)
    grads_on, dctx, _ = _engine_grads(model, x, t, ctx, noise, True)
    grads_off, none, _ = _engine_grads(model, x, t, ctx, noise, False)
    assert none is None and tuple(dctx.shape) == tuple(ctx.shape)
    assert all(torch.equal(grads_on[n], grads_off[n]) for n in grads_on)
    e_hip, e_ref = R.rel_l2(dctx, ref[torch.float64]), R.rel_l2(ref[torch.float32], ref[torch.float64])
    bound = max(4 * e_ref, 2e-5)
    print('context gradient L=3: e_hip %.3e e_ref32 %.3e bound %.3e' % (e_hip, e_ref, bound))
    report['ldm_finetune/context_L3'] = dict(e_hip=e_hip, e_ref32=e_ref, bound=bound)
    assert e_hip <= bound


# ---- the step, end to end -------------------------------------------------------------------------------------------
def _build(cfg, use_ema, model=None, **kw):
    ldm_sweep, ldm_train = pkg('ldm_sweep'), pkg('ldm_train')
    model = model if model is not None else _ldm_model(cfg)
    embedder = ldm_sweep.ClassEmbedder(cfg['context_dim'], R.N_CLASSES)
    with torch.no_grad():
        embedder.embedding.weight.copy_(torch.from_numpy(gc.det_param('embedding.weight', (R.N_CLASSES, cfg['context_dim']), R.EMB_SEED)))
    embedder = embedder.to(DEV)
    return model, embedder, ldm_train.LdmFinetuneEngine(model, embedder, lr=R.LR, use_ema=use_ema, **kw)


def _run_steps(model, embedder, ft, x, ids, ts, noises):
    losses, g1, dE1 = [], None, None
    for k in range(len(ts)):
        ft.step(x, ids, noise=noises[k], timesteps=ts[k])
        losses.append(ft.last_loss.clone())
        if k == 0:
            g1 = {n: p.grad.clone() for n, p in model.named_parameters()}
            dE1 = embedder.embedding.weight.grad.clone()
    torch.cuda.synchronize()
    return R.run_view([float(v) for v in losses], g1, dE1, dict(model.named_parameters()), embedder.embedding.weight,
                      ft.ema_state() if ft.ema is not None else None)


@pytest.mark.parametrize('use_ema', [False, True])
def test_reference_training_steps_end_to_end(report, use_ema):
    """The reference's K = 3 steps (LatentDiffusion.p_losses + AdamW + LitEma, B = 4, ids [3, 500, 3, 1000], per-image timesteps) on
    LdmFinetuneEngine: losses, step-1 gradients per tensor, the exactly-zero set, global update L2, decay-only tensors, EMA shadow."""
    fx, gold = load_json('ldm_finetune.json'), load_npz('ldm_finetune.npz')
    cfg = fx['config']
    x, ids, ts, noises = R.fixture_inputs(fx, cfg)
    P, E = R.initial_weights(cfg, torch.float64)
    run = R.finetune(P, E, cfg, x, ids, ts, noises, lr=fx['lr'], ema_decay=fx['ema_decay'])
    ref64 = R.run_view(run['losses'], run['grads1'], run['dE1'], run['params'], run['emb'], run['ema'])
    ref32, init = R.fixture_view(fx, gold), R.initial_view(cfg)
    model, embedder, ft = _build(cfg, use_ema)
    view = _run_steps(model, embedder, ft, x, ids, ts, noises)
    zero64 = sorted(n for n, g in ref64['grad1'].items() if not np.any(g))
    e_hip, e_ref = R.errors(view, ref64, init), R.errors(ref32, ref64, init)
    report['ldm_finetune/reference_steps_ema%d' % use_ema] = dict(e_hip={k: v for k, v in e_hip.items() if k != 'zero'},
                                                                   e_ref32={k: v for k, v in e_ref.items() if k != 'zero'})
    R.check(e_hip, e_ref, zero64, what='hip ema=%d' % use_ema)
    assert len(zero64) == 64 and ft.num_updates == (3 if use_ema else 0)


def test_pruned_model_steps_against_the_restatement(report):
    """A model pruned at ratio 0.3 by the LDM prune path: three steps against the fp64 restatement on the same pruned shapes;
    e_ref32 is the fp32 restatement's (no reference fixture at these shapes)."""
    fx = load_json('ldm_finetune.json')
    cfg = fx['config']
    x, ids, ts, noises = R.fixture_inputs(fx, cfg)
    model = R.prune_ldm(_ldm_model(cfg), 0.3)
    shapes = {n: tuple(p.shape) for n, p in model.named_parameters()}
    assert sum(p.numel() for p in model.parameters()) < 0.6 * 43.53e6
    W0 = {n: p.detach().cpu().clone() for n, p in model.named_parameters()}
    E0 = torch.from_numpy(gc.det_param('embedding.weight', (R.N_CLASSES, cfg['context_dim']), R.EMB_SEED))
    views = {}
    for dtype in (torch.float64, torch.float32):
        P = {n: w.to(dtype).clone() for n, w in W0.items()}
        run = R.finetune(P, E0.to(dtype).clone(), cfg, x, ids, ts, noises, lr=fx['lr'], ema_decay=fx['ema_decay'])
        views[dtype] = R.run_view(run['losses'], run['grads1'], run['dE1'], run['params'], run['emb'], run['ema'])
    init = R.run_view([], W0, E0, W0, E0, None)['final']
    init['__weight__'] = dict({n: R.sample_weight(n, w.numel()) for n, w in W0.items()}, **{'embedding.weight': 1.0})
    _, embedder, ft = _build(cfg, True, model=model)
    view = _run_steps(model, embedder, ft, x, ids, ts, noises)
    assert {n: tuple(p.shape) for n, p in model.named_parameters()} == shapes
    zero64 = sorted(n for n, g in views[torch.float64]['grad1'].items() if not np.any(g))
    e_hip, e_ref = R.errors(view, views[torch.float64], init), R.errors(views[torch.float32], views[torch.float64], init)
    report['ldm_finetune/pruned_steps'] = dict(e_hip={k: v for k, v in e_hip.items() if k != 'zero'},
                                               e_ref32={k: v for k, v in e_ref.items() if k != 'zero'})
    R.check(e_hip, e_ref, zero64, what='hip pruned')


def test_ema_scope_and_checkpoint_round_trip_on_the_device(tmp_path):
    """ema_scope() swaps the shadow in and back bit for bit; a saved checkpoint loads into a fresh engine's flat buffers."""
    ckpt = pkg('checkpoint')
    cfg = gc.LDM_TINY_CFG
    model, embedder, ft = _build(cfg, True)
    x = torch.from_numpy(gc.det_noise((2, 3, 16, 16), 1))
    ft.step(x, torch.tensor([3, 1000]), noise=torch.from_numpy(gc.det_noise((2, 3, 16, 16), 2)), timesteps=torch.tensor([5, 700]))
    live = ft.flat_p.clone()
    with ft.ema_scope():
        assert torch.equal(ft.flat_p[:ft.n_unet], ft.ema) and not torch.equal(ft.flat_p, live)
        with torch.no_grad():
            y_ema = model(x.to(DEV), torch.tensor([5, 700], device=DEV), context=embedder(torch.tensor([3, 1000], device=DEV)))
    assert torch.equal(ft.flat_p, live)
    with torch.no_grad():
        y_live = model(x.to(DEV), torch.tensor([5, 700], device=DEV), context=embedder(torch.tensor([3, 1000], device=DEV)))
    assert not torch.equal(y_ema, y_live)
    path = str(tmp_path / 'last.ckpt')
    ckpt.save_ldm_finetuned(path, model, embedder, ft)
    m2, e2, ft2 = _build(cfg, False, model=_ldm_model(cfg, seed=10))
    res = ckpt.load_ldm_finetuned(path, m2, e2)
    assert res['missing'] == [] and torch.equal(ft2.flat_p, ft.flat_p)
    assert m2.out[2].bias.data_ptr() == ft2.flat_p[ft2.n_unet - 3:].data_ptr()            # still views of the flat buffer


@isolated()
def test_cin256_full_size_step(report):
    """Un-pruned cin256-v2 (400 920 579 + 512 512 parameters), B = 2 with two timesteps and ids, one step: loss, gradients of eleven
    named tensors and the embedding rows against the fp32 restatement on the host cores, with the tolerances
    test_c5_ldm_cin256_full_size applies to its one-image oracle leg (loss 1e-5, gradients 5e-5 of the tensor's largest element);
    every parameter moved or decayed; reserved memory reported."""
    cfg = gc.LDM_CIN256_CFG
    torch.cuda.reset_peak_memory_stats()
    model, embedder, ft = _build(cfg, False)
    assert ft.flat_p.numel() == 400920579 + 1001 * 512
    ids, t = torch.tensor([417, 1000]), torch.tensor([250, 901])
    x = torch.from_numpy(gc.det_noise((2, 3, 64, 64), 301))
    noise = torch.from_numpy(gc.det_noise((2, 3, 64, 64), 302))
    before = ft.flat_p.clone()
    ft.step(x, ids, noise=noise, timesteps=t)
    torch.cuda.synchronize()
    reserved = torch.cuda.max_memory_reserved()
    names = ['input_blocks.0.0.weight', 'input_blocks.4.1.transformer_blocks.0.attn2.to_v.weight',
             'input_blocks.4.1.transformer_blocks.0.attn1.to_q.weight', 'input_blocks.7.1.transformer_blocks.0.ff.net.0.proj.weight',
             'middle_block.1.transformer_blocks.0.attn2.to_out.0.weight', 'middle_block.0.emb_layers.1.weight',
             'output_blocks.2.2.conv.weight', 'input_blocks.3.0.op.weight', 'output_blocks.5.0.skip_connection.weight', 'time_embed.0.weight', 'out.2.bias']
    P, E = R.initial_weights(cfg, torch.float32)
    loss, grads, dE = R.loss_and_grads(P, E, cfg, x, ids, t, noise)
    e_l = abs(float(ft.last_loss) - float(loss)) / float(loss)
    G = {n: p.grad for n, p in model.named_parameters()}
    worst = {n: relerr(G[n], grads[n]) for n in names}
    e_rows = relerr(embedder.embedding.weight.grad[ids.to(DEV)], dE[ids])
    moved = float((ft.flat_p != before).float().mean())
    report['ldm_finetune/cin256_full_size'] = dict(loss_rel=e_l, grad_rel=worst, emb_rows_rel=e_rows, moved_fraction=moved,
                                                   reserved_gb=reserved / 2 ** 30)
    print('cin256 step: loss rel %.2e, worst grad rel %.2e, rows %.2e, reserved %.1f GiB' % (e_l, max(worst.values()), e_rows,
                                                                                          reserved / 2 ** 30))
    assert e_l < 1e-5 and max(worst.values()) < 5e-5 and e_rows < 5e-5
    assert float(embedder.embedding.weight.grad.abs().sum(dim=1).ne(0).sum()) == 2
    assert moved > 0.99


def test_step_under_a_one_rank_rccl_group(tmp_path, report):
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    out = str(tmp_path / 'rccl_ldm_finetune.json')
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY='0', MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    p = subprocess.run([sys.executable, os.path.join(HERE, '_rccl_worker_ldm_finetune.py'), out, str(port)], env=env, timeout=600,
                       capture_output=True, text=True)
    assert p.returncode == 0, (p.stdout[-3000:], p.stderr[-3000:])
    rep = json.load(open(out))
    report['ldm_finetune/rccl_one_rank'] = rep
    assert rep['ok'] is True and rep['params_equal'] and rep['ema_equal'] and rep['losses_equal']
