"""Distillation finetune (ddpm_exp/finetune.py --kd) on the MI355X: the fused KD loss kernel against fp64, one eager KD step
against the reference's golden step (tests/golden/kd.npz / kd.json), the degenerate weights (0, 1) against today's step, the
captured and natively replayed KD step against the eager one, and the full-size C4 student with the unpruned CIFAR teacher against
the restatement of tests/kd_ref.py."""
import numpy as np
import pytest
import torch

import golden_common as gc
from conftest import isolated
from helpers import load_json, load_npz, make_model, pkg, relerr
from kd_ref import kd_loss, original_state_dict

pytestmark = pytest.mark.gpu
DEV = 'cuda'


@pytest.mark.parametrize('nblocks', [1, 512])
@pytest.mark.parametrize('n', [1, 255, 257, 393216, 3 * 2 ** 20 + 7])
def test_kd_loss_kernel_matches_fp64(report, monkeypatch, n, nblocks):
    """ops.kd_fwd_bwd: loss terms and dout <= 1e-6 relative to fp64 torch for several weight pairs, two runs bit-identical, and
    (w_kd, w_eps) = (0, 1) bit-identical to ops.mse_fwd_bwd (dout and loss) at the same grid."""
    ops = pkg('ops')
    g = torch.Generator().manual_seed(n + nblocks)
    S, T, E = (torch.randn(n, generator=g).to(DEV) for _ in range(3))
    T = S + 0.3 * T                                     # a teacher near the student, as after the prune
    gscale, lscale = 2.0 / 4, 1.0 / 4
    S64, T64, E64 = S.double().cpu(), T.double().cpu(), E.double().cpu()
    kd_ref, eps_ref = lscale * float((S64 - T64).square().sum()), lscale * float((S64 - E64).square().sum())
    worst = 0.0
    for wk, we in ((0.7, 0.3), (1.0, 0.0), (0.25, 2.0), (0.0, 1.0)):
        terms, dout = ops.kd_fwd_bwd(S, T, E, wk, we, gscale, lscale, nblocks=nblocks)
        terms2, dout2 = ops.kd_fwd_bwd(S, T, E, wk, we, gscale, lscale, nblocks=nblocks)
        torch.cuda.synchronize()
        assert torch.equal(terms, terms2) and torch.equal(dout, dout2)
        got = terms.double().cpu()
        want = [wk * kd_ref + we * eps_ref, kd_ref, eps_ref]
        for a, b in zip(got.tolist(), want):
            e = abs(a - b) / max(abs(b), 1e-30) if b != 0.0 else abs(a)
            worst = max(worst, e)
            assert e <= 1e-6, (wk, we, got.tolist(), want)
        d_ref = gscale * (wk * (S64 - T64) + we * (S64 - E64))
        e_d = relerr(dout, d_ref) if float(d_ref.abs().max()) > 0 else float(dout.abs().max())
        assert e_d <= 1e-6, (wk, we, e_d)
    monkeypatch.setattr(ops, 'MSE_BLOCKS', nblocks)
    loss_m, dout_m = ops.mse_fwd_bwd(S, E, gscale, lscale)
    terms, dout = ops.kd_fwd_bwd(S, T, E, 0.0, 1.0, gscale, lscale, nblocks=nblocks)
    torch.cuda.synchronize()
    assert torch.equal(dout, dout_m) and torch.equal(terms[0:1], loss_m) and torch.equal(terms[2:3], loss_m)
    report.setdefault('kd/kernel', {})['n%d_b%d' % (n, nblocks)] = worst


def _fixture_models():
    ckpt, unet, train = pkg('checkpoint'), pkg('unet'), pkg('train')
    fx = load_json('kd.json')
    cfg_s, orig_s = original_state_dict(ckpt, fx['student'], fx['student_seed'], unet.UNet2DModel)
    _, orig_t = original_state_dict(ckpt, fx['teacher'], fx['teacher_seed'], unet.UNet2DModel)
    student = unet.UNet2DModel(**cfg_s)
    student.load_state_dict(ckpt.convert_ddpm_original(orig_s), strict=True)
    a = fx['teacher']
    teacher = train.load_teacher([orig_t, None], DEV, ch=a['ch'], ch_mult=a['ch_mult'], num_res_blocks=a['num_res_blocks'],
                                 attn_resolutions=a['attn_resolutions'], image_size=a['image_size'])
    return fx, student.to(DEV), teacher, ckpt.ddpm_original_key_map(orig_s.keys())


def test_kd_step_matches_reference_step(report):
    """One eager KD step of the engine (teacher and student converted from the original-DDPM layout) against the reference's own
    step: loss and both terms <= 1e-5, gradient statistics and three full gradients <= 2e-5, parameters and EMA weights after
    clip + Adam + EMA <= 1e-5 (those with a real gradient); the teacher's parameters are bit-unchanged."""
    train, diffusion = pkg('train'), pkg('diffusion')
    fx, student, teacher, kmap = _fixture_models()
    gold = load_npz('kd.npz')
    t_before = {n: p.detach().clone() for n, p in teacher.named_parameters()}
    ft = train.FinetuneEngine(student, diffusion.DDPMScheduler(), lr=2e-4, dropout=0.0, teacher=teacher,
                              kd_weights=tuple(fx['weights']), replay=False)
    B = fx['batch']
    clean = torch.from_numpy(gc.det_clean((B, 3, 16, 16), fx['clean_seed'])).to(DEV)
    noise = torch.from_numpy(gc.det_noise((B, 3, 16, 16), fx['noise_seed'])).to(DEV)
    loss = ft.step(clean, noise, torch.tensor(fx['timesteps']))
    torch.cuda.synchronize()
    assert loss.shape == (1,) and loss.is_cuda and ft.last_loss_terms.shape == (2,)
    got = dict(loss=float(loss), kd=float(ft.last_loss_terms[0]), eps=float(ft.last_loss_terms[1]))
    e_terms = max(abs(got[k] - fx[k]) / abs(fx[k]) for k in got)
    pm = dict(student.named_parameters())
    scale = max(a for _, a in fx['grad_stats'].values())
    for on, (s_ref, a_ref) in fx['grad_stats'].items():
        g = pm[kmap[on]].grad.double()
        a, s = float(g.abs().sum()), float(g.sum())
        # (zero in exact arithmetic in front of a one-channel-per-group GroupNorm: absolute floor, see test_kd_cpu.py)
        assert abs(a - a_ref) <= 2e-5 * a_ref + 1e-7 * scale and abs(s - s_ref) <= 2e-5 * a_ref + 1e-7 * scale, (on, a, a_ref)
    e_full = max(relerr(pm[kmap[on]].grad, torch.from_numpy(gold['grad:' + on]).reshape(pm[kmap[on]].shape))
                 for on in fx['full_grads'])
    ema = ft.ema_state()
    e_p = 0.0
    # parameters whose gradient is zero in exact arithmetic (the k biases, and the 32-channel level's biases and time projections in
    # front of a one-channel-per-group GroupNorm: <= 6e-9 of the largest statistic, the next is 3.5e-5) hold rounding noise on both
    # sides, and Adam's first step turns noise of either sign into a full +-lr update: they are not compared after the step
    noise_only = {on for on, (_, a_ref) in fx['grad_stats'].items() if a_ref <= 1e-6 * scale}
    for on, (s_ref, a_ref) in fx['param_stats'].items():
        if on in noise_only:
            continue
        for t_, (s2, a2) in ((pm[kmap[on]].detach(), (s_ref, a_ref)), (ema[kmap[on]], fx['ema_stats'][on])):
            a, s = float(t_.double().abs().sum()), float(t_.double().sum())
            e_p = max(e_p, abs(a - a2) / a2, abs(s - s2) / a2)
    unchanged = all(torch.equal(p, t_before[n]) for n, p in teacher.named_parameters())
    report['kd/fixture_step'] = dict(terms_rel=e_terms, full_grad_rel=e_full, param_rel=e_p, loss=got, noise_only=len(noise_only))
    assert e_terms <= 1e-5 and e_full <= 2e-5 and e_p <= 1e-5 and unchanged


def _tiny_pair():
    return make_model(gc.TINY_CFG, 5), make_model(gc.TINY_CFG, 9)


def _batches(n, B=8):
    train = pkg('train')
    gen = torch.Generator().manual_seed(3)
    return [(torch.from_numpy(gc.det_clean((B, 3, 16, 16), 20 + k)), torch.from_numpy(gc.det_noise((B, 3, 16, 16), 30 + k)),
             train.antithetic_timesteps(B, 1000, gen)) for k in range(n)]


@pytest.mark.parametrize('replay', [False, True])
def test_kd_zero_weight_step_equals_plain_step(report, replay):
    """kd_weights = (0, 1) with a teacher: three steps bit-identical to today's step without one (losses, gradient norms,
    parameters, Adam moments, EMA weights), eager and natively replayed."""
    train, diffusion = pkg('train'), pkg('diffusion')
    batches = _batches(3)

    def run(with_teacher):
        student, teacher = _tiny_pair()
        kw = dict(teacher=teacher, kd_weights=(0.0, 1.0)) if with_teacher else {}
        ft = train.FinetuneEngine(student, diffusion.DDPMScheduler(), lr=2e-4, dropout=0.1, dropout_seed=7, replay=replay, **kw)
        out = []
        for c, n, t in batches:
            loss = ft.step(c.to(DEV), n.to(DEV), t)
            out.append((float(loss), float(ft.last_grad_norm)))
        torch.cuda.synchronize()
        return ft, out

    fp, op = run(False)
    fk, ok = run(True)
    assert (fk._cap is not None) == replay and (fp._cap is not None) == replay
    assert op == ok, (op, ok)
    assert torch.equal(fp.flat_p, fk.flat_p) and torch.equal(fp.ema, fk.ema) and torch.equal(fp.m, fk.m) and torch.equal(fp.v, fk.v)
    report['kd/zero_weight_%s' % ('replayed' if replay else 'eager')] = [a[0] for a in ok]


@pytest.mark.parametrize('wgrad_overlap', [False, True])
@pytest.mark.parametrize('kd_overlap', [False, True])
def test_kd_step_replayed_natively_equals_eager(report, monkeypatch, kd_overlap, wgrad_overlap):
    """Five KD steps with dropout 0.1 and a cosine warm-up schedule, captured once and replayed natively, against the eager engine:
    losses, terms, gradient norms, parameters, Adam moments and EMA weights BIT-identical -- with the teacher's forward on the side
    stream (DP_KD_OVERLAP=1) or not, with and without the weight-gradient side stream.  The teacher's packed operands are built by
    its first forward and never again."""
    train, diffusion = pkg('train'), pkg('diffusion')
    monkeypatch.setenv('DP_KD_OVERLAP', '1' if kd_overlap else '0')
    batches = _batches(5)

    def run(replay):
        student, teacher = _tiny_pair()
        t_before = [p.detach().clone() for p in teacher.parameters()]
        sched = train.get_scheduler('cosine', 2e-4, num_warmup_steps=2, num_training_steps=10)
        ft = train.FinetuneEngine(student, diffusion.DDPMScheduler(), lr=2e-4, dropout=0.1, dropout_seed=7, lr_scheduler=sched,
                                  replay=replay, teacher=teacher)
        ft.REPLAY_OVERLAP = wgrad_overlap
        student.engine().overlap_wgrad = wgrad_overlap
        out, packs = [], None
        for c, n, t in batches:
            loss = ft.step(c.to(DEV), n.to(DEV), t.to(DEV))
            out.append((float(loss), ft.last_loss_terms.tolist(), float(ft.last_grad_norm), ft.last_lr))
            student._engine.overlap_wgrad = wgrad_overlap
            if packs is None:
                packs = ft._teacher_packs()
            assert ft._same_packs(packs, ft._teacher_packs()), 'the teacher was re-packed'
        torch.cuda.synchronize()
        assert all(torch.equal(a, p) for a, p in zip(t_before, teacher.parameters()))
        return ft, out

    fe, oe = run(False)
    fr, orr = run(True)
    assert fe._cap is None and fr._cap is not None and fr._cap['call'].replay is not None
    info = fr._cap['call'].info
    report['kd/replay_%s_%s' % ('kd_overlap' if kd_overlap else 'kd_serial', 'wgrad_side' if wgrad_overlap else 'wgrad_main')] = dict(
        losses=[a[0] for a in orr], replay=info)
    assert oe == orr, (oe, orr)
    assert torch.equal(fe.flat_p, fr.flat_p) and torch.equal(fe.ema, fr.ema) and torch.equal(fe.m, fr.m) and torch.equal(fe.v, fr.v)
    assert (info['side_nodes'] > 0) == (kd_overlap or wgrad_overlap)


@isolated()
def test_kd_c4_student_with_unpruned_teacher(report):
    """The C4 finetune with a teacher: the ratio-0.3 pruned CIFAR-10 UNet (19 851 157 parameters, masks of the C4 sweep) as the
    student, the unpruned CIFAR-10 UNet it was pruned from as the teacher, batch 128, dropout 0.1 on the student, two steps:
    loss and raw gradients against the restatement of tests/kd_ref.py with the same Philox masks (1e-5 / 5e-5, the C4 tolerances;
    the restatement runs in fp32 on the host like the C4 test's), clip + Adam + EMA on identical gradients (1e-5)."""
    from oracle import diffusion_ref as D, philox_ref as PH
    train, diffusion, sweep = pkg('train'), pkg('diffusion'), pkg('sweep')
    cfg, B = gc.CIFAR_CFG, 128
    teacher = make_model(cfg, 0)
    model = make_model(cfg, 0)
    clean = torch.from_numpy(gc.det_clean((4, 3, 32, 32), 1))
    noise = torch.from_numpy(gc.det_noise((4, 3, 32, 32), 2))
    sweep.taylor_sweep(model, diffusion.DDPMScheduler(), clean.to(DEV), noise.to(DEV), num_steps=8)
    sweep.prune_model(model, 0.3)
    assert sum(p.numel() for p in model.parameters()) == 19851157
    for p in model.parameters():
        p.grad = None
    P = {n: p.detach().cpu().clone().requires_grad_(True) for n, p in model.named_parameters()}
    Pt = {n: p.detach().cpu().clone() for n, p in teacher.named_parameters()}
    names = list(P)
    ft = train.FinetuneEngine(model, diffusion.DDPMScheduler(), dropout=0.1, dropout_seed=31, ema_decay=0.9999,
                              lr_scheduler=train.get_scheduler('constant', 2e-4), teacher=teacher)
    table = model.dropout_table()
    m = [torch.zeros_like(P[n]) for n in names]
    v = [torch.zeros_like(P[n]) for n in names]
    ema = [P[n].detach().clone() for n in names]
    gen = torch.Generator().manual_seed(17)
    worst_g, e_loss, e_terms = 0.0, 0.0, 0.0
    for step in (1, 2):
        fc = torch.from_numpy(gc.det_clean((B, 3, 32, 32), 50 + step))
        fn = torch.from_numpy(gc.det_noise((B, 3, 32, 32), 60 + step))
        t = train.antithetic_timesteps(B, 1000, gen)
        l_gpu = float(ft.step(fc.to(DEV), fn.to(DEV), t))
        terms = ft.last_loss_terms.tolist()
        for n in names:
            P[n].grad = None
        l_cpu, kd, eps, _, _ = kd_loss(P, cfg, Pt, cfg, fc, fn, t, (0.7, 0.3), PH.DropSpec(table, 31, step, 0))
        l_cpu.backward()
        e_loss = max(e_loss, abs(l_gpu - float(l_cpu.detach())) / float(l_cpu.detach()))
        e_terms = max(e_terms, abs(terms[0] - float(kd)) / float(kd), abs(terms[1] - float(eps)) / float(eps))
        gpu_g = {n: p.grad.detach().cpu().clone() for n, p in model.named_parameters()}
        for n in names:
            if float(P[n].grad.abs().max()) > 1e-6:
                worst_g = max(worst_g, relerr(gpu_g[n], P[n].grad))
        with torch.no_grad():
            D.adam_ema_step([P[n] for n in names], [gpu_g[n] for n in names], m, v, ema, step)
    pm = dict(model.named_parameters())
    e_p = max(relerr(pm[n], P[n].detach()) for n in names)
    es = ft.ema_state()
    e_e = max(relerr(es[n], e) for n, e in zip(names, ema))
    report['kd/c4_with_teacher'] = dict(loss_rel=e_loss, terms_rel=e_terms, grad_rel_worst=worst_g, param_rel_after2=e_p,
                                        ema_rel_after2=e_e, teacher_params=sum(x.numel() for x in teacher.parameters()))
    assert e_loss < 1e-5 and e_terms < 1e-5 and worst_g < 5e-5
    assert e_p < 1e-5 and e_e < 1e-5
