"""Worker for tests/test_train_state_cpu.py: one rank of a world_size-2 gloo job (mocked kernels, as tests/_dist_worker.py).  Three
finetune steps in one go; separately two steps, checkpoint.save_training_state (rank 0 writes), a NEW model and engine on every
rank loaded from that one file, one more step.  Each rank writes its state after step 2, its final buffers and its losses."""
import os
import sys

import torch
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import _dist_worker as W     # noqa: E402  (patch(): mock ops, CPU engine binding)
import golden_common as gc   # noqa: E402

pkg = W.pkg
B = 4


def build():
    train = pkg('train')
    model = pkg('unet').UNet2DModel(**gc.TINY_CFG)
    gc.det_init_(model, 5)
    sched = train.get_scheduler('cosine', 2e-4, num_warmup_steps=2, num_training_steps=10)
    return model, train.FinetuneEngine(model, pkg('diffusion').DDPMScheduler(), dropout=0.1, dropout_seed=7, lr_scheduler=sched)


def steps(ft, ks, sl):
    train = pkg('train')
    out = []
    for k in ks:
        c = torch.from_numpy(gc.det_clean((B, 3, 16, 16), 30 + k))
        n = torch.from_numpy(gc.det_noise((B, 3, 16, 16), 40 + k))
        t = train.antithetic_timesteps(B, 1000, torch.Generator().manual_seed(100 + k))
        out.append(float(ft.step(c[sl], n[sl], t[sl])))
    return out


def main():
    rank, world, port, outdir = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
    torch.set_num_threads(2)
    W.patch()
    dist.init_process_group('gloo', init_method='tcp://127.0.0.1:%s' % port, rank=rank, world_size=world)
    checkpoint = pkg('checkpoint')
    per = B // world
    sl = slice(rank * per, (rank + 1) * per)
    _, whole = build()
    l_whole = steps(whole, range(3), sl)
    _, first = build()
    l_first = steps(first, range(2), sl)
    state = first.state_dict()
    path = os.path.join(outdir, 'shared_state.pt')
    checkpoint.save_training_state(path, first)              # rank 0 writes; returns on every rank once the file is there
    assert os.path.exists(path)
    _, second = build()
    checkpoint.load_training_state(path, second)
    l_second = steps(second, [2], sl)
    torch.save(dict(state=state, whole=dict(p=whole.flat_p, m=whole.m, v=whole.v, ema=whole.ema, step=whole.step_count, lr=whole.last_lr),
                    resumed=dict(p=second.flat_p, m=second.m, v=second.v, ema=second.ema, step=second.step_count, lr=second.last_lr),
                    l_whole=l_whole, l_resumed=l_first + l_second), os.path.join(outdir, 'ts_r%d.pt' % rank))
    dist.barrier()
    dist.destroy_process_group()


if __name__ == '__main__':
    main()
