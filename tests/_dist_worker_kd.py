"""Worker for tests/test_kd_cpu.py: one rank of a world_size-2 gloo job running the PRODUCT's data-parallel distillation finetune
step (train.FinetuneEngine with a frozen teacher) with the kernel wrappers replaced by the CPU stand-ins of tests/mock_ops.py
plus a stand-in of ops.kd_fwd_bwd installed here at run time."""
import os
import sys

import torch
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import _dist_worker as W     # noqa: E402  (patch(): mock ops, CPU engine binding)
import golden_common as gc   # noqa: E402
import mock_ops              # noqa: E402


def kd_fwd_bwd(out, teacher_out, noise, w_kd, w_eps, gscale, loss_scale, nblocks=512):
    """csrc/elementwise.hip kd_kernel + kd_terms_kernel in fp32 torch: ([loss, kd, eps], dout)."""
    dk, de = out - teacher_out, out - noise
    kd, eps = loss_scale * dk.square().sum(), loss_scale * de.square().sum()
    return torch.stack([w_kd * kd + w_eps * eps, kd, eps]), gscale * (w_kd * dk + w_eps * de)


def main():
    rank, world, port, outdir = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
    torch.set_num_threads(2)
    setattr(mock_ops, 'kd_fwd_bwd', kd_fwd_bwd)
    W.patch()
    if world > 1:
        dist.init_process_group('gloo', init_method='tcp://127.0.0.1:%s' % port, rank=rank, world_size=world)
    unet, train, diffusion = W.pkg('unet'), W.pkg('train'), W.pkg('diffusion')
    cfg = gc.TINY_CFG
    student, teacher = unet.UNet2DModel(**cfg), unet.UNet2DModel(**cfg)
    gc.det_init_(student, 5)
    gc.det_init_(teacher, 9)
    teacher_before = {n: p.detach().clone() for n, p in teacher.named_parameters()}
    B = 4
    per = B // world
    sl = slice(rank * per, (rank + 1) * per)
    ft = train.FinetuneEngine(student, diffusion.DDPMScheduler(), dropout=0.1, dropout_seed=7, teacher=teacher,
                              kd_weights=(0.7, 0.3), lr_scheduler=train.get_scheduler('constant_with_warmup', 2e-4, num_warmup_steps=2))
    gen = torch.Generator().manual_seed(13)
    losses, terms = [], []
    for step in range(2):
        fc = torch.from_numpy(gc.det_clean((B, 3, 16, 16), 50 + step))
        fn = torch.from_numpy(gc.det_noise((B, 3, 16, 16), 60 + step))
        t = train.antithetic_timesteps(B, 1000, gen)
        loss = ft.step(fc[sl], fn[sl], t[sl])
        lt = ft.last_loss_terms.clone()
        if world > 1:
            dist.all_reduce(loss)
            dist.all_reduce(lt)
        losses.append(float(loss))
        terms.append([float(v) for v in lt])
    torch.save(dict(losses=losses, terms=terms, norm=float(ft.last_grad_norm),
                    params={n: p.detach().clone() for n, p in student.named_parameters()},
                    ema={n: e.clone() for n, e in ft.ema_state().items()},
                    teacher_unchanged=all(torch.equal(p, teacher_before[n]) for n, p in teacher.named_parameters())),
               os.path.join(outdir, 'kd_r%d_w%d.pt' % (rank, world)))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
