"""Worker for tests/test_ldm_finetune_cpu.py: one rank of a world_size-2 gloo job running the PRODUCT's data-parallel LDM finetune
step (ldm_train.LdmFinetuneEngine) with the kernel wrappers replaced by the CPU stand-ins of tests/mock_ops_ldm.py."""
import importlib
import os
import sys

import torch
import torch.distributed as dist

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for p in (ROOT, HERE, os.path.join(HERE, 'golden')):
    if p not in sys.path:
        sys.path.insert(0, p)
import golden_common as gc   # noqa: E402
import mock_ops_ldm          # noqa: E402


def pkg(sub):
    return importlib.import_module('diff-pruning_amd.' + sub)


def patch():
    """Mock ops everywhere the step reaches, a CPU engine binding, no device requirement."""
    for sub in ('engine', 'ldm', 'ldm_sweep', 'ldm_train'):
        pkg(sub).ops = mock_ops_ldm
    ldm, ldm_train = pkg('ldm'), pkg('ldm_train')

    def cpu_engine(self):
        if self._engine is None:
            self._engine = ldm.LdmEngine(self.config)
        self._engine.packs.rebind()
        self._engine.bind({n: p.detach() for n, p in self.named_parameters()}, None)
        return self._engine
    ldm.UNetModel.engine = cpu_engine
    ldm_train._require_hip_device = lambda dev: None


def build(use_ema=True, group=None):
    ldm, ldm_sweep, ldm_train = pkg('ldm'), pkg('ldm_sweep'), pkg('ldm_train')
    cfg = gc.LDM_TINY_CFG
    model = ldm.UNetModel(**cfg)
    gc.det_init_(model, 9)
    embedder = ldm_sweep.ClassEmbedder(cfg['context_dim'], 1001)
    with torch.no_grad():
        embedder.embedding.weight.copy_(torch.from_numpy(gc.det_param('embedding.weight', (1001, cfg['context_dim']), 61)))
    return cfg, model, embedder, ldm_train.LdmFinetuneEngine(model, embedder, lr=1.28e-4, use_ema=use_ema, group=group)


def main():
    rank, world, port, outdir = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
    torch.set_num_threads(2)
    patch()
    if world > 1:
        dist.init_process_group('gloo', init_method='tcp://127.0.0.1:%s' % port, rank=rank, world_size=world)
    cfg, model, embedder, ft = build()
    B, H = 4, cfg['image_size']
    per = B // world
    sl = slice(rank * per, (rank + 1) * per)
    ids = torch.tensor([3, 500, 3, 1000])               # id 3 on both ranks of the two-rank run
    losses = []
    for step in range(2):
        x = torch.from_numpy(gc.det_noise((B, 3, H, H), 50 + step))
        noise = torch.from_numpy(gc.det_noise((B, 3, H, H), 60 + step))
        t = torch.tensor([0, 250, 999, 17 + step])
        loss = ft.step(x[sl], ids[sl], noise=noise[sl], timesteps=t[sl]).clone()
        if world > 1:
            dist.all_reduce(loss)
        losses.append(float(loss))
    torch.save(dict(losses=losses, params={n: p.detach().clone() for n, p in model.named_parameters()},
                    emb=embedder.embedding.weight.detach().clone(), ema={n: e.clone() for n, e in ft.ema_state().items()}),
               os.path.join(outdir, 'ldmft_r%d_w%d.pt' % (rank, world)))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == '__main__':
    main()
