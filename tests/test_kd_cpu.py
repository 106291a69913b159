"""Distillation finetune (ddpm_exp/finetune.py --kd), CPU part: the restatement of the KD loss on the oracle UNet against the
reference's own golden step (tests/golden/kd.npz / kd.json), the API of FinetuneEngine(teacher=...) and train.load_teacher,
and the data-parallel KD step's shard invariance (world_size 2, gloo, mocked kernels)."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import golden_common as gc
from helpers import load_json, load_npz, pkg, relerr
from kd_ref import kd_loss, original_state_dict, reference_acp

HERE = os.path.dirname(os.path.abspath(__file__))


def _fixture_weights(dtype=torch.float64):
    """(student cfg, student P, teacher cfg, teacher P, key map original -> ours) of kd.json, converted to this package's names."""
    ckpt, unet = pkg('checkpoint'), pkg('unet')
    fx = load_json('kd.json')
    cfg_s, orig_s = original_state_dict(ckpt, fx['student'], fx['student_seed'], unet.UNet2DModel)
    cfg_t, orig_t = original_state_dict(ckpt, fx['teacher'], fx['teacher_seed'], unet.UNet2DModel)
    Ps = {k: v.to(dtype) for k, v in ckpt.convert_ddpm_original(orig_s).items()}
    Pt = {k: v.to(dtype) for k, v in ckpt.convert_ddpm_original(orig_t).items()}
    return fx, cfg_s, Ps, cfg_t, Pt, ckpt.ddpm_original_key_map(orig_s.keys()), orig_s


def test_kd_restatement_matches_reference_step():
    """fp64 restatement of noise_estimation_kd_loss on the oracle UNet, weights converted from the original-DDPM layout: loss and
    both terms <= 1e-6 relative to the reference's fp32 step, S and T, and every parameter gradient (statistics and the three
    full tensors) <= 1e-5."""
    fx, cfg_s, Ps, cfg_t, Pt, kmap, _ = _fixture_weights()
    gold = load_npz('kd.npz')
    B = fx['batch']
    clean = torch.from_numpy(gc.det_clean((B, 3, 16, 16), fx['clean_seed'])).double()
    noise = torch.from_numpy(gc.det_noise((B, 3, 16, 16), fx['noise_seed'])).double()
    t = torch.tensor(fx['timesteps'])
    for p in Ps.values():
        p.requires_grad_(True)
    loss, kd, eps, S, T = kd_loss(Ps, cfg_s, Pt, cfg_t, clean, noise, t, fx['weights'], acp=reference_acp().double())
    loss.backward()
    for name, got in (('loss', loss.detach()), ('kd', kd.detach()), ('eps', eps.detach())):
        assert abs(float(got) - fx[name]) <= 1e-6 * abs(fx[name]), (name, float(got), fx[name])
    assert relerr(S.detach(), gold['S']) <= 1e-5 and relerr(T, gold['T']) <= 1e-5
    scale = max(a for _, a in fx['grad_stats'].values())
    for on, (s_ref, a_ref) in fx['grad_stats'].items():
        g = Ps[kmap[on]].grad.double()
        a, s = float(g.abs().sum()), float(g.sum())
        # (parameters in front of a one-channel-per-group GroupNorm -- the 32-channel student's first-level biases and time
        # projections -- have zero gradient in exact arithmetic; the reference's fp32 holds rounding noise there: an absolute
        # floor of one fp32 ulp of the largest statistic)
        assert abs(a - a_ref) <= 1e-5 * a_ref + 6e-8 * scale, (on, a, a_ref)
        assert abs(s - s_ref) <= 1e-5 * a_ref + 6e-8 * scale, (on, s, s_ref)
    for on in fx['full_grads']:
        g = Ps[kmap[on]].grad
        ref = torch.from_numpy(gold['grad:' + on]).double().reshape(g.shape)
        assert relerr(g, ref) <= 1e-5, on


def _tiny(seed, **over):
    unet = pkg('unet')
    cfg = dict(gc.TINY_CFG, **over)
    m = unet.UNet2DModel(**cfg)
    gc.det_init_(m, seed)
    return m


def test_finetune_engine_rejects_bad_teachers_and_weights():
    """Teacher validation happens before anything is built: not a UNet2DModel, the student itself, mismatched in / out channels or
    sample size, another device; kd_weights must be two finite numbers."""
    train, diffusion = pkg('train'), pkg('diffusion')
    sched = diffusion.DDPMScheduler()
    student = _tiny(5)
    good = _tiny(9)
    bad = [(ValueError, dict(teacher=student)),
           (TypeError, dict(teacher=torch.nn.Conv2d(3, 3, 3))),
           (ValueError, dict(teacher=_tiny(9, in_channels=4))),
           (ValueError, dict(teacher=_tiny(9, out_channels=6))),
           (ValueError, dict(teacher=_tiny(9, sample_size=32))),
           (ValueError, dict(teacher=good.to(torch.device('meta')))),
           (ValueError, dict(teacher=_tiny(9), kd_weights=(0.7,))),
           (ValueError, dict(teacher=_tiny(9), kd_weights=(0.7, 0.3, 0.0))),
           (ValueError, dict(teacher=_tiny(9), kd_weights=(float('nan'), 0.3))),
           (ValueError, dict(teacher=_tiny(9), kd_weights=(0.7, float('inf')))),
           (ValueError, dict(teacher=_tiny(9), kd_weights=('0.7', 0.3))),
           (ValueError, dict(teacher=_tiny(9), kd_weights=0.7))]
    before = [p.detach().clone() for p in student.parameters()]
    for exc, kw in bad:
        with pytest.raises(exc):
            train.FinetuneEngine(student, sched, **kw)
    # nothing of the student was touched by a rejected construction
    assert all(torch.equal(a, p.detach()) and p.grad is None for a, p in zip(before, student.parameters()))


def test_load_teacher_from_original_ddpm_checkpoints(tmp_path):
    """train.load_teacher: an original-DDPM state dict, the [state_dict, ...] list the reference unpacks with states[0], a file
    holding that list, a Diffusers model directory and a UNet2DModel all give the same frozen eval-mode model; a checkpoint
    without its architecture is refused."""
    train, unet, ckpt = pkg('train'), pkg('unet'), pkg('checkpoint')
    fx = load_json('kd.json')
    arch = fx['teacher']
    cfg, orig = original_state_dict(ckpt, arch, fx['teacher_seed'], unet.UNet2DModel)
    want = ckpt.convert_ddpm_original(orig)
    kw = dict(ch=arch['ch'], ch_mult=arch['ch_mult'], num_res_blocks=arch['num_res_blocks'],
              attn_resolutions=arch['attn_resolutions'], image_size=arch['image_size'])
    path = str(tmp_path / 'ema_teacher.pth')
    torch.save([orig, {'state': 'optimizer'}, 3, 100], path)
    made = [train.load_teacher(orig, 'cpu', **kw), train.load_teacher([orig, None], 'cpu', **kw),
            train.load_teacher(path, 'cpu', **kw)]
    d = str(tmp_path / 'teacher_dir')
    made[0].save_pretrained(d)
    made.append(train.load_teacher(d, 'cpu'))
    made.append(train.load_teacher(made[0], 'cpu'))
    for m in made:
        assert isinstance(m, unet.UNet2DModel) and not m.training
        assert dict(m.config) == dict(made[0].config) and m.config['block_out_channels'] == (64, 128, 128, 128)
        sd = m.state_dict()
        assert sd.keys() == want.keys() and all(torch.equal(sd[k], want[k]) for k in want)
        assert not any(p.requires_grad for p in m.parameters())
    assert sum(p.numel() for p in made[0].parameters()) == 8952067
    with pytest.raises(ValueError):
        train.load_teacher(orig, 'cpu')                                   # no architecture
    with pytest.raises(TypeError):
        train.load_teacher([42], 'cpu', **kw)


def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _run(world, outdir):
    port = str(_free_port())
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, '_dist_worker_kd.py'), str(r), str(world), port, outdir])
             for r in range(world)]
    for p in procs:
        assert p.wait(timeout=600) == 0


def test_two_rank_kd_step_equals_single_process(tmp_path):
    """world_size 2 (gloo, mocked kernels): each rank runs the teacher on its own shard, the loss terms are normalised by the global
    batch, the dropout masks follow the global element index -- two KD steps give the single process's losses, terms, parameters
    and EMA weights; the teacher is never written."""
    out = str(tmp_path)
    _run(1, out)
    _run(2, out)
    one = torch.load(os.path.join(out, 'kd_r0_w1.pt'))
    r0 = torch.load(os.path.join(out, 'kd_r0_w2.pt'))
    r1 = torch.load(os.path.join(out, 'kd_r1_w2.pt'))
    assert one['teacher_unchanged'] and r0['teacher_unchanged'] and r1['teacher_unchanged']
    for a, b, c in zip(one['losses'], r0['losses'], r1['losses']):
        assert abs(a - b) <= 1e-5 * abs(a) and b == c
    for k, (a, b, c) in enumerate(zip(one['terms'], r0['terms'], r1['terms'])):
        assert np.allclose(a, b, rtol=1e-5) and b == c
        assert abs(0.7 * a[0] + 0.3 * a[1] - one['losses'][k]) <= 1e-5 * one['losses'][k]
    assert abs(one['norm'] - r0['norm']) <= 1e-4 * one['norm'] and r0['norm'] == r1['norm']
    for n, p in one['params'].items():
        assert torch.equal(r0['params'][n], r1['params'][n]) and torch.equal(r0['ema'][n], r1['ema'][n])
        assert float((r0['params'][n] - p).abs().max()) <= 2e-4 * float(p.abs().max()) + 1e-7, n
        assert float((r0['ema'][n] - one['ema'][n]).abs().max()) <= 2e-4 * float(p.abs().max()) + 1e-7, n
