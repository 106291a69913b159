"""Training state and gradient accumulation of the finetune engines, CPU part (mocked kernels, as the other CPU finetune tests): the
state round trip through the one-file form, the error cases, window bookkeeping, torch's optimizer layout against torch itself, the
`ckpt.pth` list with its parameter permutation against the reference's recorded name order (tests/golden/train_state.json), the
`last.ckpt` additions, and a two-rank gloo run whose rank-0 file resumes both ranks."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import golden_common as gc
from helpers import load_json, pkg

HERE = os.path.dirname(os.path.abspath(__file__))
B = 4


# ---- DDPM engine on mocked kernels ---------------------------------------------------------------------------------------
@pytest.fixture()
def mocked(monkeypatch):
    import mock_ops
    for sub in ('engine', 'sweep', 'train', 'diffusion', 'pruning'):
        monkeypatch.setattr(pkg(sub), 'ops', mock_ops)
    unet, engine, train = pkg('unet'), pkg('engine'), pkg('train')

    def cpu_engine(self):
        if self._engine is None:
            self._engine = engine.UNetEngine(self.config)
        self._engine.packs.rebind()
        self._engine.bind({n: p.detach() for n, p in self.named_parameters()}, None)
        self._engine.set_dropout(self.dropout_table() if self.training else None, getattr(self, 'dropout_seed', 0),
                                 getattr(self, '_dropout_step', 0))
        return self._engine
    monkeypatch.setattr(unet.UNet2DModel, 'engine', cpu_engine)
    monkeypatch.setattr(train, '_require_hip_device', lambda dev: None)
    monkeypatch.setattr(pkg('diffusion').DDPMScheduler, '_acp_on', lambda self, dev: self.alphas_cumprod, raising=False)
    return mock_ops


def _engine(cfg=None, **kw):
    train = pkg('train')
    model = pkg('unet').UNet2DModel(**(cfg or gc.TINY_CFG))
    gc.det_init_(model, 5)
    kw.setdefault('lr_scheduler', train.get_scheduler('cosine', 2e-4, num_warmup_steps=2, num_training_steps=10))
    return model, train.FinetuneEngine(model, pkg('diffusion').DDPMScheduler(), dropout=0.1, dropout_seed=7, **kw)


def _batch(k, b=B):
    train = pkg('train')
    return (torch.from_numpy(gc.det_clean((b, 3, 16, 16), 30 + k)), torch.from_numpy(gc.det_noise((b, 3, 16, 16), 40 + k)),
            train.antithetic_timesteps(b, 1000, torch.Generator().manual_seed(100 + k)))


def _same(a, b):
    return (torch.equal(a.flat_p, b.flat_p) and torch.equal(a.m, b.m) and torch.equal(a.v, b.v) and
            (a.ema is None) == (b.ema is None) and (a.ema is None or torch.equal(a.ema, b.ema)) and
            a.step_count == b.step_count and getattr(a, 'last_lr', None) == getattr(b, 'last_lr', None) and
            getattr(a, 'num_updates', 0) == getattr(b, 'num_updates', 0))


def test_state_round_trip_through_one_file(mocked, tmp_path):
    """4 steps in one go == 2 steps, save, a NEW model and engine from the file alone, 2 steps: parameters, moments, shadow,
    counters, learning rate and every post-resume loss, bit for bit.  The file loads under weights_only=True; a state taken earlier
    is not changed by later steps; loading into an engine that has stepped on rewinds it exactly."""
    ckpt = pkg('checkpoint')
    _, whole = _engine()
    l_whole = [float(whole.step(*_batch(k))) for k in range(4)]
    _, first = _engine()
    [first.step(*_batch(k)) for k in range(2)]
    path = str(tmp_path / 'state.pt')
    ckpt.save_training_state(path, first)
    early = first.state_dict()
    keep = {k: v.clone() for k, v in early.items() if torch.is_tensor(v)}
    snapshot = first.flat_p.clone()
    blob = torch.load(path, weights_only=True)
    assert set(blob) == {'format_version', 'engine', 'weights', 'training_state'}
    ts = blob['training_state']
    assert ts['step_count'] == 2 and ts['micro_step'] == 0 and ts['lr_scheduler']['last_epoch'] == 2
    assert [r[0] for r in ts['layout']] == [n for n, _ in first.model.named_parameters()]
    assert ts['hyper']['betas'] == [0.9, 0.999] and ts['hyper']['dropout_seed'] == 7 and ts['hyper']['accumulation'] == 1
    _, second = _engine()
    ckpt.load_training_state(path, second)
    assert torch.equal(second.flat_p, snapshot) and second.step_count == 2
    assert all(p.data_ptr() >= second.flat_p.data_ptr() for p in second.model.parameters())      # still views of flat_p
    l_second = [float(second.step(*_batch(k))) for k in (2, 3)]
    assert l_second == l_whole[2:] and _same(whole, second)
    # no aliasing: `first` steps on, the state taken at step 2 stays
    [first.step(*_batch(k)) for k in (2, 3)]
    assert _same(whole, first) and all(torch.equal(early[k], v) for k, v in keep.items())
    # rewind: the file again, into the engine that is now at step 4
    ckpt.load_training_state(path, first)
    assert torch.equal(first.flat_p, snapshot) and first.step_count == 2 and torch.equal(first.m, keep['m'])
    assert [float(first.step(*_batch(k))) for k in (2, 3)] == l_whole[2:] and _same(whole, first)


def _pruned_tiny():
    model = pkg('unet').UNet2DModel(**gc.TINY_CFG)
    gc.det_init_(model, 5)
    pruning = pkg('pruning')
    pruning.DependencyGraph(model).load_pruning_history([['down_blocks.0.resnets.0.conv1', True, [0, 3, 5, 7, 9, 11, 13, 15]]])
    pruning.fix_static_attributes(model)
    return model


def test_error_cases(mocked, tmp_path):
    """ValueError: a state of the un-pruned model for a pruned one (the first differing tensor is named, nothing is written), differing
    betas under strict=True (strict=False takes the state and keeps the engine's), a save in mid-window, replay=True with k = 2."""
    train, ckpt, diffusion = pkg('train'), pkg('checkpoint'), pkg('diffusion')
    _, ft = _engine()
    ft.step(*_batch(0))
    sd = ft.state_dict()
    path = str(tmp_path / 'state.pt')
    ckpt.save_training_state(path, ft)
    pruned = _pruned_tiny()
    fp = train.FinetuneEngine(pruned, diffusion.DDPMScheduler(), dropout=0.1, dropout_seed=7,
                              lr_scheduler=train.get_scheduler('cosine', 2e-4, num_warmup_steps=2, num_training_steps=10))
    first_diff = next(n for (n, p), (_, q) in zip(pruned.named_parameters(), ft.model.named_parameters()) if p.shape != q.shape)
    before = fp.flat_p.clone()
    for load in (lambda: fp.load_state_dict(sd), lambda: ckpt.load_training_state(path, fp)):
        with pytest.raises(ValueError, match=first_diff.replace('.', r'\.')):
            load()
    assert torch.equal(fp.flat_p, before) and fp.step_count == 0 and not fp.m.any()
    _, other = _engine(betas=(0.8, 0.999))
    with pytest.raises(ValueError, match='betas'):
        other.load_state_dict(sd)
    assert other.step_count == 0
    other.load_state_dict(sd, strict=False)
    assert other.step_count == 1 and tuple(other.betas) == (0.8, 0.999) and torch.equal(other.m, sd['m'])
    _, acc = _engine(gradient_accumulation_steps=2)
    acc.step(*_batch(0))
    for save in (acc.state_dict, acc.optimizer_state_dict, lambda: ckpt.save_training_state(path, acc)):
        with pytest.raises(ValueError, match='window'):
            save()
    acc.step(*_batch(1))
    assert acc.state_dict()['step_count'] == 1
    with pytest.raises(ValueError):
        _engine(gradient_accumulation_steps=2, replay=True)
    with pytest.raises(ValueError):
        _engine(gradient_accumulation_steps=0)
    assert _engine(gradient_accumulation_steps=2, replay=None)[1]._replay_wanted(False, torch.device('cuda')) is False


def test_window_bookkeeping_k3(mocked):
    """k = 3: calls 0 and 1 leave parameters, moments, shadow, step_count and the LR schedule bit-unchanged, keep the packed operands
    and use the dropout-mask step of the coming update at image offsets 0, B, 2B; call 2 updates once and steps the schedule once."""
    model, ft = _engine(gradient_accumulation_steps=3)
    seen = []
    eng0 = model.engine()
    real = type(eng0).set_dropout

    def spy(self, table, seed=0, step=0, n_off=0, step_dev=None):
        if table:
            seen.append((step, n_off))
        return real(self, table, seed, step, n_off, step_dev)
    type(eng0).set_dropout = spy
    try:
        for window in range(2):
            before = [t.clone() for t in (ft.flat_p, ft.m, ft.v, ft.ema)]
            lr0, ep0 = ft.lr_scheduler.get_last_lr()[0], ft.lr_scheduler.last_epoch
            for j in range(2):
                ft.step(*_batch(3 * window + j))
                assert all(torch.equal(a, b) for a, b in zip(before, (ft.flat_p, ft.m, ft.v, ft.ema)))
                assert ft.step_count == window and ft._micro == j + 1 and ft.lr_scheduler.last_epoch == ep0
                assert len(model._engine.packs._c) > 0                      # operands of call 0 are kept inside the window
            g_before = ft.flat_g.clone()
            ft.step(*_batch(3 * window + 2))
            assert ft.step_count == window + 1 and ft._micro == 0 and ft.lr_scheduler.last_epoch == ep0 + 1
            assert ft.last_lr == lr0 and not torch.equal(ft.flat_g, g_before) and not torch.equal(ft.m, before[1])
            assert torch.equal(ft.flat_p, before[0]) == (lr0 == 0.0)        # (the warm-up schedule starts at lr 0)
    finally:
        type(eng0).set_dropout = real
    assert [s for s in seen if s[0] > 0] == [(1, 0), (1, B), (1, 2 * B), (2, 0), (2, B), (2, 2 * B)]


def test_torch_layout_loads_into_torch_adam(mocked):
    """optimizer_state_dict() is what torch.optim.Adam of the running torch takes without complaint: same param_groups keys as its
    own, `step` a 0-d fp32 tensor, indices in model.parameters() order; export -> import gives the same bits; integers as `step` are
    accepted."""
    model, ft = _engine(lr_scheduler=None, lr=2e-4)
    [ft.step(*_batch(k)) for k in range(2)]
    sd = ft.optimizer_state_dict()
    clones = [torch.nn.Parameter(p.detach().clone()) for p in model.parameters()]
    opt = torch.optim.Adam(clones, lr=2e-4, betas=(0.9, 0.999), eps=1e-8)
    assert set(sd['param_groups'][0]) == set(opt.state_dict()['param_groups'][0])
    opt.load_state_dict(sd)
    for i, p in enumerate(clones):
        st = opt.state[p]
        assert st['step'].dtype == torch.float32 and st['step'].dim() == 0 and float(st['step']) == 2.0
        assert st['exp_avg'].shape == p.shape and torch.equal(st['exp_avg'], sd['state'][i]['exp_avg'])
    m, v = ft.m.clone(), ft.v.clone()
    _, other = _engine(lr_scheduler=None, lr=2e-4)
    other.load_optimizer_state_dict(opt.state_dict())
    assert torch.equal(other.m, m) and torch.equal(other.v, v) and other.step_count == 2
    for s in sd['state'].values():
        s['step'] = 2
    other.step_count = 0
    other.load_optimizer_state_dict(sd)
    assert other.step_count == 2
    sd['state'][3]['step'] = 5
    with pytest.raises(ValueError):
        other.load_optimizer_state_dict(sd)


def test_ddpm_exp_states_permutation_against_the_reference_order(mocked, tmp_path):
    """The `ckpt.pth` list: element 0 in the DDIM code base's key names, Adam's indices and the EMA LIST positional in the order of
    THAT model's parameters() -- the name order recorded from the reference (train_state.json), which is not UNet2DModel's.  The
    written file has the fixture's structure; reading it back continues bit for bit; a pickled module as element 0 is refused."""
    ckpt = pkg('checkpoint')
    fx = load_json('train_state.json')['ddpm']
    model, ft = _engine(lr_scheduler=None, lr=2e-4)
    ours = [n for n, _ in model.named_parameters()]
    o_names = list(ckpt.convert_to_ddpm_original({n: torch.empty(0) for n in ours}))
    assert ckpt.ddpm_original_parameter_order(sorted(o_names)) == fx['param_names']
    assert o_names != fx['param_names']                                        # a permutation is needed
    [ft.step(*_batch(k)) for k in range(2)]
    path = str(tmp_path / 'ckpt.pth')
    ckpt.save_ddpm_exp_states(path, ft, epoch=1)
    states = torch.load(path, weights_only=True)
    assert len(states) == fx['states_len'] == 5 and list(states[0]) == fx['param_names'] and states[2:4] == [1, 2]
    assert sorted(states[1]) == sorted(fx['optimizer_keys']) and sorted(states[1]['state'][0]) == sorted(fx['state_keys'])
    assert states[1]['param_groups'][0]['params'] == list(range(len(ours))) == fx['param_groups'][0]['params']
    assert set(states[1]['param_groups'][0]) == set(fx['param_groups'][0])
    assert isinstance(states[4], list) and len(states[4]) == len(ours)
    o2d = ckpt.ddpm_original_key_map(fx['param_names'])
    named, es, off = dict(model.named_parameters()), ft.ema_state(), {r[0]: r[2] for r in ft.state_dict()['layout']}
    for i, on in enumerate(fx['param_names']):
        n = o2d[on]
        st = states[1]['state'][i]
        assert list(states[0][on].shape) == fx['shapes'][on] == list(st['exp_avg'].shape) == list(states[4][i].shape)
        assert str(st['step'].dtype) == fx['step_dtype'] and st['step'].dim() == 0
        sl = slice(off[n], off[n] + named[n].numel())
        assert torch.equal(st['exp_avg'].reshape(-1), ft.m[sl]) and torch.equal(st['exp_avg_sq'].reshape(-1), ft.v[sl])
        assert torch.equal(states[4][i].reshape(-1), es[n].reshape(-1)) and torch.equal(states[0][on].reshape(-1), named[n].reshape(-1))
    _, whole = _engine(lr_scheduler=None, lr=2e-4)
    l_whole = [float(whole.step(*_batch(k))) for k in range(3)]
    _, second = _engine(lr_scheduler=None, lr=2e-4, eps=1e-8)
    states[1]['param_groups'][0]['eps'] = 1.0                                   # the engine's hyper-parameters hold, not the file's
    assert ckpt.load_ddpm_exp_states(states, second) == (1, 2)
    assert float(second.step(*_batch(2))) == l_whole[2] and _same(whole, second)
    torch.save([torch.nn.Conv2d(1, 1, 1)] + states[1:], path)
    with pytest.raises(ValueError, match='pickled module'):
        ckpt.load_ddpm_exp_states(path, second)
    with pytest.raises(ValueError, match='pickled module'):
        ckpt.load_ddpm_exp_states([torch.nn.Conv2d(1, 1, 1)] + states[1:], second)


# ---- LDM engine on mocked kernels ----------------------------------------------------------------------------------------
@pytest.fixture()
def mocked_ldm(monkeypatch):
    import mock_ops_train_state
    ldm, ldm_train = pkg('ldm'), pkg('ldm_train')
    for sub in ('engine', 'ldm', 'ldm_sweep', 'ldm_train', 'pruning'):
        monkeypatch.setattr(pkg(sub), 'ops', mock_ops_train_state)

    def cpu_engine(self):
        if self._engine is None:
            self._engine = ldm.LdmEngine(self.config)
        self._engine.packs.rebind()
        self._engine.bind({n: p.detach() for n, p in self.named_parameters()}, None)
        return self._engine
    monkeypatch.setattr(ldm.UNetModel, 'engine', cpu_engine)
    monkeypatch.setattr(ldm_train, '_require_hip_device', lambda dev: None)


def _ldm_engine(**kw):
    ldm, ldm_sweep, ldm_train = pkg('ldm'), pkg('ldm_sweep'), pkg('ldm_train')
    cfg = gc.LDM_TINY_CFG
    model = ldm.UNetModel(**cfg)
    gc.det_init_(model, 9)
    embedder = ldm_sweep.ClassEmbedder(cfg['context_dim'], 1001)
    with torch.no_grad():
        embedder.embedding.weight.copy_(torch.from_numpy(gc.det_param('embedding.weight', (1001, cfg['context_dim']), 61)))
    return model, embedder, ldm_train.LdmFinetuneEngine(model, embedder, lr=1.28e-4, **kw)


def _ldm_batch(k, b=B):
    H = gc.LDM_TINY_CFG['image_size']
    return dict(x_start=torch.from_numpy(gc.det_noise((b, 3, H, H), 50 + k)), class_ids=torch.tensor([3, 500, 3, 1000][:b]),
                noise=torch.from_numpy(gc.det_noise((b, 3, H, H), 60 + k)), timesteps=torch.tensor([0, 250, 999, 17 + k][:b]))


@pytest.mark.parametrize('use_ema,k', [(True, 1), (False, 1), (True, 2)])
def test_ldm_state_round_trip_and_last_ckpt(mocked_ldm, tmp_path, use_ema, k):
    """The LDM engine: 2 + 2 windows against 4 through the one-file form (UNet, embedder, moments, shadow, step_count, num_updates)
    and through save_ldm_finetuned(training_state=) / load_ldm_finetuned(engine=); torch.optim.AdamW loads the exported state; with
    k = 2 num_updates advances by 2 per window and a save in mid-window raises."""
    ckpt = pkg('checkpoint')
    kw = dict(use_ema=use_ema, accumulate_grad_batches=k)
    *_, whole = _ldm_engine(**kw)
    l_whole = [float(whole.step(**_ldm_batch(i))) for i in range(4 * k)]
    m1, e1, first = _ldm_engine(**kw)
    [first.step(**_ldm_batch(i)) for i in range(2 * k)]
    assert first.step_count == 2 and first.num_updates == (2 * k if use_ema else 0)
    native, last = str(tmp_path / 'native.pt'), str(tmp_path / 'last.ckpt')
    ckpt.save_training_state(native, first)
    ckpt.save_ldm_finetuned(last, m1, e1, ema=first if use_ema else None, training_state=first, epoch=3)
    blob = torch.load(native, weights_only=True)
    assert set(blob) == {'format_version', 'engine', 'weights', 'embedder', 'training_state'} and blob['training_state']['num_updates'] == first.num_updates
    for how in ('native', 'last'):
        m2, e2, second = _ldm_engine(**kw)
        if how == 'native':
            ckpt.load_training_state(native, second)
        else:
            got = ckpt.load_ldm_finetuned(last, m2, e2, engine=second)
            assert got['global_step'] == 2 and got['epoch'] == 3 and not got['missing']
        l_second = [float(second.step(**_ldm_batch(i))) for i in range(2 * k, 4 * k)]
        assert l_second == l_whole[2 * k:] and _same(whole, second), how
    sd = first.optimizer_state_dict()
    clones = [torch.nn.Parameter(p.detach().clone()) for p in list(m1.parameters()) + list(e1.parameters())]
    opt = torch.optim.AdamW(clones, lr=1.28e-4)
    assert set(sd['param_groups'][0]) == set(opt.state_dict()['param_groups'][0]) and sd['param_groups'][0]['weight_decay'] == 1e-2
    opt.load_state_dict(sd)
    assert float(opt.state[clones[-1]]['step']) == 2.0 and opt.state[clones[-1]]['exp_avg'].shape == e1.embedding.weight.shape
    if k > 1:
        first.step(**_ldm_batch(0))
        with pytest.raises(ValueError, match='window'):
            first.state_dict()
    with pytest.raises(ValueError):
        ckpt.load_training_state(native, _ldm_engine(use_ema=use_ema, accumulate_grad_batches=k, betas=(0.8, 0.999))[2])
    with pytest.raises(ValueError):
        _ldm_engine(use_ema=not use_ema, accumulate_grad_batches=k)[2].load_state_dict(first.state_dict() if k == 1 else blob['training_state'])


def test_refused_files_write_nothing(mocked, mocked_ldm, tmp_path):
    """load_training_state makes every check of the state (here: betas under strict=True) before it writes a weight;
    load_ldm_finetuned(engine=) refuses a file without model_ema.* when the engine keeps a LitEma shadow -- the stale shadow would
    go on silently -- and a file without optimizer_states, both before anything is written; an engine without EMA ignores the
    file's shadow."""
    ckpt = pkg('checkpoint')
    _, ft = _engine()
    ft.step(*_batch(0))
    path = str(tmp_path / 'state.pt')
    ckpt.save_training_state(path, ft)
    _, other = _engine(betas=(0.8, 0.999))
    other.step(*_batch(1))
    keep = [t.clone() for t in (other.flat_p, other.m, other.v, other.ema)]
    with pytest.raises(ValueError, match='betas'):
        ckpt.load_training_state(path, other)
    assert all(torch.equal(a, b) for a, b in zip(keep, (other.flat_p, other.m, other.v, other.ema))) and other.step_count == 1
    ckpt.load_training_state(path, other, strict=False)
    assert torch.equal(other.flat_p, ft.flat_p) and torch.equal(other.m, ft.m)

    m1, e1, first = _ldm_engine(use_ema=True)
    first.step(**_ldm_batch(0))
    no_ema, no_opt, full = (str(tmp_path / n) for n in ('no_ema.ckpt', 'no_opt.ckpt', 'full.ckpt'))
    ckpt.save_ldm_finetuned(no_ema, m1, e1, ema=None, training_state=first)
    ckpt.save_ldm_finetuned(no_opt, m1, e1, ema=first)
    ckpt.save_ldm_finetuned(full, m1, e1, ema=first, training_state=first)
    m2, e2, second = _ldm_engine(use_ema=True)
    second.step(**_ldm_batch(1))
    keep = [t.clone() for t in (second.flat_p, second.m, second.v, second.ema)]
    for bad, what in ((no_ema, 'LitEma'), (no_opt, 'optimizer_states')):
        with pytest.raises(ValueError, match=what):
            ckpt.load_ldm_finetuned(bad, m2, e2, engine=second)
        assert all(torch.equal(a, b) for a, b in zip(keep, (second.flat_p, second.m, second.v, second.ema))) and second.num_updates == 1
    m3, e3, third = _ldm_engine(use_ema=False)
    ckpt.load_ldm_finetuned(full, m3, e3, engine=third)
    assert third.ema is None and third.num_updates == 0 and torch.equal(third.m, first.m) and torch.equal(third.flat_p, first.flat_p)


def test_ldm_window_shadow_is_updated_every_batch(mocked_ldm):
    """k = 2: call 0 leaves parameters and moments alone and moves the shadow by LitEma's update at the warm-up decay of ITS batch
    (num_updates 1 -> 2/11 on unchanged weights is a no-op numerically only if shadow == weights: checked on the second window)."""
    ldm_train = pkg('ldm_train')
    *_, ft = _ldm_engine(use_ema=True, accumulate_grad_batches=2)
    ft.step(**_ldm_batch(0)); ft.step(**_ldm_batch(1))
    assert ft.num_updates == 2 and ft.step_count == 1 and not torch.equal(ft.ema, ft.flat_p[:ft.n_unet])
    p, m, v, s = ft.flat_p.clone(), ft.m.clone(), ft.v.clone(), ft.ema.clone()
    ft.step(**_ldm_batch(2))
    assert torch.equal(ft.flat_p, p) and torch.equal(ft.m, m) and torch.equal(ft.v, v) and ft.num_updates == 3 and ft.step_count == 1
    omd = np.float32(1) - np.float32(ldm_train.lit_ema_decay(0.9999, 3))
    assert float(omd) == float(np.float32(1) - np.float32(4) / np.float32(13))
    assert torch.equal(ft.ema, s - float(omd) * (s - p[:ft.n_unet]))


def test_flat_layout_and_exchange_ranges_are_pinned(mocked, mocked_ldm):
    """The flat layout of both engines at the tiny configs (names, shapes, offsets: tests/golden/flat_layout.json), n_unet, and the
    ranges of flat_g in the order they go to all_reduce -- DDPM: the buckets of the milestones up, mid, down, then 'rest'; LDM: its
    sorted list.  Every value was recorded from the engines as they were BEFORE the flat-buffer core moved into train_state
    (one hand-written offset walk per engine), never from the code under test: a state file or a two-rank run of either side of
    that move meets the same layout and the same collectives."""
    ts, want, cfg = pkg('train_state'), load_json('flat_layout.json'), gc.LDM_TINY_CFG
    ft = pkg('train').FinetuneEngine(pkg('unet').UNet2DModel(**gc.TINY_CFG), pkg('diffusion').DDPMScheduler())
    assert ts.param_layout(ft._state_named()) == want['ddpm'] and ft.flat_p.numel() == ft.ema.numel() == 2245763
    assert [(seg, lo, hi) for seg in ('up', 'mid', 'down', 'rest') for lo, hi in ft._buckets[seg]] == [
        ('up', 661600, 2063328), ('up', 2244832, 2245763), ('mid', 2063328, 2244832), ('down', 21632, 661600), ('rest', 0, 21632)]
    lf = pkg('ldm_train').LdmFinetuneEngine(pkg('ldm').UNetModel(**cfg), pkg('ldm_sweep').ClassEmbedder(cfg['context_dim'], 1001),
                                            use_ema=True)
    assert ts.param_layout(lf._state_named()) == want['ldm'] and lf.flat_p.numel() == 10956435
    assert lf.n_unet == lf.ema.numel() == 10940419
    assert [tuple(b) for b in lf._buckets] == [
        ('output_blocks', 4644640, 10940419), ('middle_block', 3159360, 4644640), ('input_blocks', 20736, 3159360),
        ('time_embed', 0, 20736), ('cond_stage_model', 10940419, 10956435)]
    # the views the engines hand out sit at those offsets of their buffers
    for eng, buf, named in ((ft, ft.flat_p, ft._state_named()), (lf, lf.flat_g, [(n, p.grad) for n, p in lf._state_named()])):
        for (name, shape, off), (n, t) in zip(ts.param_layout(named), named):
            assert n == name and tuple(t.shape) == tuple(shape) and t.data_ptr() == buf.data_ptr() + 4 * off
    offs = {n: off for n, _, off in want['ldm']}
    assert all(t.data_ptr() == lf.ema.data_ptr() + 4 * offs['model.diffusion_model.' + n] for n, t in lf.ema_state().items())


# ---- two ranks -------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_two_rank_state_is_identical_and_rank0_file_resumes_both(tmp_path):
    """world_size 2 (gloo, mocked kernels): after two data-parallel steps both ranks hold the same state; the file rank 0 wrote
    resumes BOTH ranks (new model, new engine) to the bits of the uninterrupted three steps."""
    out, port = str(tmp_path), str(_free_port())
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, '_dist_worker_train_state.py'), str(r), '2', port, out]) for r in range(2)]
    for p in procs:
        assert p.wait(timeout=600) == 0
    r0, r1 = (torch.load(os.path.join(out, 'ts_r%d.pt' % r)) for r in range(2))
    assert r0['state'].keys() == r1['state'].keys()
    for k, a in r0['state'].items():
        b = r1['state'][k]
        assert torch.equal(a, b) if torch.is_tensor(a) else a == b, k
    assert r0['state']['step_count'] == 2
    for r in (r0, r1):
        assert r['l_whole'] == r['l_resumed']
        for k, a in r['whole'].items():
            b = r['resumed'][k]
            assert torch.equal(a, b) if torch.is_tensor(a) else a == b, k
    assert torch.equal(r0['resumed']['p'], r1['resumed']['p'])
