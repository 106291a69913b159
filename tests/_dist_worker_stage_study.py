"""Worker for tests/test_stage_study_cpu.py: one rank of a gloo job running the PRODUCT's staged sweep (sweep.taylor_sweep(stages=...))
on its shard of the batch with the kernel wrappers replaced by CPU stand-ins -- once with reduce_grads=False (the snapshots stay the
rank's local sums) and once with the exchange (every snapshot all-reduced after the sweep, before the final gradient's)."""
import os
import sys

import torch
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)
import _dist_worker as W     # noqa: E402  (sys.path, the CPU engine and step constructor)
import golden_common as gc   # noqa: E402
import mock_ops_stage_study  # noqa: E402

NUM_STEPS, STAGES = 6, [0, 2, 5, 6]


def main():
    rank, world, port, outdir = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
    torch.set_num_threads(2)
    W.patch()
    W.pkg('sweep').ops = mock_ops_stage_study
    if world > 1:
        dist.init_process_group('gloo', init_method='tcp://127.0.0.1:%s' % port, rank=rank, world_size=world)
    B = 4
    clean = torch.from_numpy(gc.det_clean((B, 3, 16, 16), 1))
    noise = torch.from_numpy(gc.det_noise((B, 3, 16, 16), 2))
    per = B // world
    sl = slice(rank * per, (rank + 1) * per)
    sched = W.pkg('diffusion').DDPMScheduler()
    out = {}
    for key, reduce_grads in (('local', False), ('reduced', True)):
        model = W.pkg('unet').UNet2DModel(**gc.TINY_CFG)
        gc.det_init_(model, 5)
        model.eval()
        res = W.pkg('sweep').taylor_sweep(model, sched, clean[sl], noise[sl], num_steps=NUM_STEPS, stages=STAGES,
                                          reduce_grads=reduce_grads)
        out[key] = dict(stage_grads={s: g.clone() for s, g in res['stage_grads'].items()}, losses=res['losses'],
                        final=torch.cat([p.grad.reshape(-1) for p in model.parameters()]))
    out['sizes'] = [p.numel() for p in model.parameters()]
    torch.save(out, os.path.join(outdir, 'stage_r%d_w%d.pt' % (rank, world)))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
