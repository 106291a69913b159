"""Full-size CIFAR sampling against values the reference wrote (tests/golden/sampling_cifar*.npz, written by
tests/golden/make_golden_sampling.py): the model `bench.py --config ddim` times -- the ratio-0.3 pruned CIFAR UNet -- and the unpruned
one, through the forward paths a sampling loop can take and the scheduler steps around them.

On seeded weights the 100-step DDIM chain is chaotic (the reference's own fp32 run ends with almost every uint8 value different from
its fp64 run), so the bounds are per step, "teacher-forced": the reference's fp64 trajectory point x_k goes into the HIP path and one
forward / one scheduler step is compared with fp64.
  (a) eps:  max|eps_hip - eps64| <= max(4 e_ref32, 2e-5), e_ref32 = the reference's own fp32 eps error on that x_k;
  (b) step: dp_ddim_step / dp_ddpm_step on (x_k, eps64) within 2e-6 of the fp64 step; on (x_k, eps_hip) within twice the bound
      of (a); at the last step (t = 0) at most 0.5 % of the uint8 values differ from the fp64 image;
  (c) chain: the free-running pipeline from the same seed tracks fp64 over the first 10 steps within 10x the reference fp32 run's
      own gap (+1e-5); the rest of the 100 steps is reported, not asserted."""
import numpy as np
import pytest
import torch

import golden_common as gc
from conftest import isolated
from helpers import load_json, load_npz, make_model, pkg

pytestmark = pytest.mark.gpu
DEV = 'cuda'
SHAPE = (2, 3, 32, 32)
B_BENCH = 256                         # the batch bench.py --config ddim samples at
EPS_FACTOR, EPS_FLOOR = 4.0, 2e-5
STEP_FIXTURE_ABS = 2e-6
STEP_FACTOR = 2.0
U8_SHARE = 0.005
PAIR_GAP = 1e-6
CHAIN_FACTOR, CHAIN_FLOOR = 10.0, 1e-5
FIXTURE = {'full': 'sampling_cifar.npz', 'pruned': 'sampling_cifar_pruned.npz'}
# every supported layer on the F(2x2, 3x3) kernel (test_e2e_gpu.py, test_reference_fixtures_with_winograd_on_every_supported_layer)
WINO2D_FORCED = dict(WINO=True, WGRAD_WINO=True, WINO_MIN_TILES=0, WGRAD_WINO_MIN_WORK=0, WGRAD_WINO_MIN_FILL=0.0, WINO2D=True,
                     WINO2D_MIN_TILES=0, WINO2D_MIN_FILL=0.0, WGRAD_WINO2D=True, WGRAD_WINO2D_MIN_FILL=0.0)


def _model(which):
    """'full': the seeded CIFAR UNet; 'pruned': the same after config C1's sweep (B=4, 8 timesteps) and the ratio-0.3 Taylor prune,
    built as test_replay_at_the_benchmarked_sizes builds it (its masks are the reference's, test_cifar_c1_masks_bit_exact)."""
    model = make_model(gc.CIFAR_CFG, 0)
    if which == 'pruned':
        sweep, diffusion = pkg('sweep'), pkg('diffusion')
        clean = torch.from_numpy(gc.det_clean((4, 3, 32, 32), 1)).to(DEV)
        noise = torch.from_numpy(gc.det_noise((4, 3, 32, 32), 2)).to(DEV)
        sweep.taylor_sweep(model, diffusion.DDPMScheduler(), clean, noise, num_steps=8)
        sweep.prune_model(model, 0.3)
        for p in model.parameters():
            p.grad = None
        model.eval()
        assert {n: list(p.shape) for n, p in model.named_parameters()} == load_json('cifar_c1.json')['shapes_after']
    assert sum(p.numel() for p in model.parameters()) == int(load_npz(FIXTURE[which])['params'])
    return model


def _cases(which):
    """One entry per teacher-forced input: the stored DDIM steps of `which`, and on the full model the eta 0.5, quad-schedule and
    DDPM steps of sampling_cifar_edges.npz."""
    g = load_npz(FIXTURE[which])
    cases = [dict(name='step%02d' % k, kind='ddim', step=int(k), t=int(g['timesteps'][i]), x=g['x'][i], eps=g['eps'][i],
                  out=g['out'][i], e_ref32=float(g['e_ref32'][i])) for i, k in enumerate(g['steps'])]
    eta = None
    if which == 'full':
        e = load_npz('sampling_cifar_edges.npz')
        eta = float(e['eta'])
        for kind in ('eta', 'quad', 'ddpm'):
            for j in range(int(e['n_' + kind])):
                def f(key):
                    return e['%s:%d:%s' % (kind, j, key)]
                c = dict(name='%s%d_t%d' % (kind, j, int(f('t'))), kind=kind, t=int(f('t')), x=f('x'), eps=f('eps'), out=f('out'),
                         e_ref32=float(f('e_ref32')))
                if kind != 'quad':
                    c['noise'] = f('noise')
                if kind != 'ddpm':
                    c['step'] = int(f('step'))
                cases.append(c)
    return cases, eta


def _out_of_order(cases):
    """Call order for the captured forwards: alternately the smallest and the largest remaining timestep (99, 0, 98, 1, ...), so
    every replay changes t by hundreds -- a replayed launch list holding a stale timestep or embedding shows up."""
    by_t = sorted(range(len(cases)), key=lambda i: cases[i]['t'])
    order = []
    while by_t:
        order.append(by_t.pop(0))
        if by_t:
            order.append(by_t.pop())
    return order


def _counting(obj, name, box, monkeypatch):
    real = getattr(obj, name)
    monkeypatch.setattr(obj, name, lambda *a: (lambda r: (box.__setitem__(0, box[0] + bool(r)), r)[1])(real(*a)))


@torch.no_grad()
def _forward_paths(model, cases, monkeypatch):
    """{path: [eps of every case as [rows, 3, 32, 32] on the device]}; plus the B=256 duplicate-pair gaps and launch counts."""
    ops = pkg('ops')
    xs = [torch.from_numpy(c['x']).to(DEV) for c in cases]
    order = _out_of_order(cases)
    out, info = {}, {}

    def run(fwd, kind, inputs, take):
        assert type(fwd).__name__ == kind, type(fwd).__name__
        got = {}
        try:
            for i in order:
                got[i] = take(fwd(inputs(i), cases[i]['t']))          # the captured forward returns a tensor of its own pool
        finally:
            fwd.close()
        return [got[i] for i in range(len(cases))]

    out['captured_b2'] = run(model.sampling_forward(SHAPE, 100), '_CapturedForward', lambda i: xs[i], lambda y: y.clone())
    out['eager_b2'] = run(model.sampling_forward(SHAPE, 100, replay=False), '_EagerForward', lambda i: xs[i], lambda y: y.clone())
    # the benchmarked batch: the two fixture images at rows 0 / 128 and 127 / 255, seeded noise elsewhere
    fill = torch.from_numpy(gc.det_noise((B_BENCH,) + SHAPE[1:], 901)).to(DEV)

    def bench_rows(i):
        xb = fill.clone()
        xb[0] = xb[128] = xs[i][0]
        xb[127] = xb[255] = xs[i][1]
        return xb
    rows = run(model.sampling_forward((B_BENCH,) + SHAPE[1:], 100), '_CapturedForward', bench_rows,
               lambda y: y[[0, 128, 127, 255]].clone())
    out['captured_b256'] = [torch.stack([r[0], r[3]]) for r in rows]               # rows 0 and 255 against the fixture ...
    out['captured_b256_twin'] = [torch.stack([r[1], r[2]]) for r in rows]          # ... and their twins 128 and 127
    info['b256_pair_gap'] = [max(float((r[0] - r[1]).abs().max()), float((r[2] - r[3]).abs().max())) for r in rows]
    info['b256_pairs_bit_identical'] = [bool(torch.equal(r[0], r[1]) and torch.equal(r[2], r[3])) for r in rows]
    with monkeypatch.context() as mp:
        for k, v in WINO2D_FORCED.items():
            mp.setattr(ops, k, v)
        n2 = [0]
        _counting(ops, '_conv_wino2d', n2, mp)
        out['wino2d_forced_b2'] = run(model.sampling_forward(SHAPE, 100, replay=False), '_EagerForward', lambda i: xs[i],
                                      lambda y: y.clone())
        info['wino2d_launches'] = n2[0]
    with monkeypatch.context() as mp:
        mp.setattr(ops, 'WINO', False)                                 # test_e2e_gpu._direct_kernels
        mp.setattr(ops, 'WGRAD_WINO', False)
        nw = [0]
        _counting(ops, '_conv_wino', nw, mp)
        _counting(ops, '_conv_wino2d', nw, mp)
        out['direct_b2'] = run(model.sampling_forward(SHAPE, 100, replay=False), '_EagerForward', lambda i: xs[i],
                               lambda y: y.clone())
        info['direct_winograd_launches'] = nw[0]
    return out, info


def _step(case, eps, eta, generator=None):
    diffusion = pkg('diffusion')
    x = torch.from_numpy(case['x']).to(DEV)
    t = case['t']
    noise = torch.from_numpy(case['noise']).to(DEV) if 'noise' in case and generator is None else None
    if case['kind'] == 'ddpm':
        s = diffusion.DDPMScheduler(variance_type='fixed_small')
        s.set_timesteps(1000)
        return s.step(eps, t, x, generator=generator, variance_noise=noise).prev_sample
    s = diffusion.DDIMScheduler(skip_type='quad' if case['kind'] == 'quad' else 'uniform')
    s.set_timesteps(100)
    assert int(s.timesteps[case['step']]) == t, (case['name'], int(s.timesteps[case['step']]))
    if case['kind'] == 'eta':
        return s.step(eps, t, x, eta=eta, variance_noise=noise).prev_sample
    return s.step(eps, t, x, eta=0.0).prev_sample


def _u8(x):
    """pipeline_ddim.py:114-115 and numpy_to_pil: (x / 2 + 0.5).clamp(0, 1) * 255, rounded."""
    x = torch.as_tensor(x).double().cpu()
    return ((x / 2 + 0.5).clamp(0, 1) * 255).round().to(torch.uint8).numpy()


@pytest.mark.parametrize('which', ['full', 'pruned'])
@isolated(params=('which',))
def test_teacher_forced_sampling_full_size(which, report, monkeypatch):
    """(a) + (b) on the full-size model `which`: every stored x_k of the reference's fp64 100-step trajectory (t = 999 ... 0) through
    the captured forward (fed out of order through ONE capture), the eager forward, the captured forward at batch 256, the forward
    with every supported layer on F(2x2, 3x3) and the direct kernels only; then the scheduler step on the fixture's eps and on the
    HIP eps, including t = 0 (final_alpha_cumprod) and, on the full model, eta 0.5, the quad schedule and DDPM at t = 999, 500, 1, 0."""
    cases, eta = _cases(which)
    model = _model(which)
    eps_hip, info = _forward_paths(model, cases, monkeypatch)
    bad = []
    rep = dict(bound={}, e_ref32={}, eps_abs={}, eps_ratio={}, step_on_eps64_abs={}, step_on_hip_abs={}, **info)
    for c in cases:
        rep['bound'][c['name']] = bound = max(EPS_FACTOR * c['e_ref32'], EPS_FLOOR)
        rep['e_ref32'][c['name']] = c['e_ref32']
    for path, outs in eps_hip.items():
        rep['eps_abs'][path], rep['eps_ratio'][path] = {}, {}
        for c, y in zip(cases, outs):
            err = float((y.double().cpu() - torch.from_numpy(c['eps']).double()).abs().max())
            rep['eps_abs'][path][c['name']] = err
            rep['eps_ratio'][path][c['name']] = err / c['e_ref32']
            if not err <= rep['bound'][c['name']]:
                bad.append(('eps', path, c['name'], err, rep['bound'][c['name']]))
    for c, y in zip(cases, eps_hip['captured_b2']):
        ref = torch.from_numpy(c['out']).double()
        e_fix = float((_step(c, torch.from_numpy(c['eps']).to(DEV), eta).double().cpu() - ref).abs().max())
        out_hip = _step(c, y, eta)
        e_hip = float((out_hip.double().cpu() - ref).abs().max())
        rep['step_on_eps64_abs'][c['name']], rep['step_on_hip_abs'][c['name']] = e_fix, e_hip
        if not e_fix <= STEP_FIXTURE_ABS:
            bad.append(('step on eps64', c['name'], e_fix, STEP_FIXTURE_ABS))
        if not e_hip <= STEP_FACTOR * rep['bound'][c['name']]:
            bad.append(('step on eps_hip', c['name'], e_hip, STEP_FACTOR * rep['bound'][c['name']]))
        if c['kind'] == 'ddim' and c['t'] == 0:                     # the last step: the image the pipeline returns
            n_diff = int((_u8(out_hip) != _u8(c['out'])).sum())
            rep['last_step_u8_differing'] = n_diff
            rep['last_step_u8_total'] = int(c['out'].size)
            if not n_diff <= U8_SHARE * c['out'].size:
                bad.append(('uint8 at t=0', n_diff, U8_SHARE * c['out'].size))
        if c['kind'] == 'ddpm' and c['t'] == 0:                     # t = 0 adds no noise: nothing is drawn from the generator
            gen = torch.Generator().manual_seed(3)
            state = gen.get_state()
            drawn = _step(c, y, eta, generator=gen)
            rep['ddpm_t0_draws'] = int(not torch.equal(gen.get_state(), state))
            if rep['ddpm_t0_draws'] or not torch.equal(drawn, out_hip):
                bad.append(('ddpm t=0 drew noise', rep['ddpm_t0_draws']))
    report['sampling/teacher_forced/' + which] = rep
    assert len(cases) == (16 if which == 'full' else 8)
    assert info['wino2d_launches'] > 0 and info['direct_winograd_launches'] == 0, info
    assert all(g <= PAIR_GAP for g in info['b256_pair_gap']), info['b256_pair_gap']
    assert not bad, bad


@isolated()
def test_free_running_ddim_chain_full_size(report, monkeypatch):
    """(c) DDIMPipeline(batch_size=2, generator=torch.Generator().manual_seed(s), num_inference_steps=100) on the full model, with
    the captured forward (the automatic choice at 100 steps) and the eager one: x_T is the reference's draw bit for bit, the
    two runs are bit-identical, and over the first 10 steps the chain stays within 10x the reference fp32 run's own gap to fp64
    (+1e-5).  The 100-step endpoint is reported beside the reference's own fp32-vs-fp64 numbers, not asserted: on these weights
    the chain is chaotic."""
    diffusion, unet = pkg('diffusion'), pkg('unet')
    g = load_npz('sampling_cifar.npz')
    model = _model('full')
    runs, kinds = {}, {}
    real_sf = unet.UNet2DModel.sampling_forward
    for mode in (None, '0'):
        if mode is None:
            monkeypatch.delenv('DP_SAMPLE_REPLAY', raising=False)
        else:
            monkeypatch.setenv('DP_SAMPLE_REPLAY', mode)
        made = []
        monkeypatch.setattr(unet.UNet2DModel, 'sampling_forward',
                            lambda self, *a, **k: (lambda f: (made.append(type(f).__name__), f)[1])(real_sf(self, *a, **k)))
        pipe = diffusion.DDIMPipeline(model, diffusion.DDIMScheduler())
        states = []
        real_step = pipe.scheduler.step

        def step(eps, t, x, **kw):
            if not states:
                states.append(x.clone())                                  # x_T as the pipeline drew it
            r = real_step(eps, t, x, **kw)
            states.append(r.prev_sample.clone())
            return r
        pipe.scheduler.step = step
        pipe(batch_size=2, generator=torch.Generator().manual_seed(int(g['xT_seed'])), num_inference_steps=int(g['n_steps']),
             output_type='numpy')
        monkeypatch.setattr(unet.UNet2DModel, 'sampling_forward', real_sf)
        runs[mode], kinds[mode] = [s.double().cpu() for s in states], made
    assert kinds[None] == ['_CapturedForward'] and kinds['0'] == ['_EagerForward'], kinds
    cap, eager = runs[None], runs['0']
    assert len(cap) == int(g['n_steps']) + 1
    assert torch.equal(cap[0].float(), torch.from_numpy(g['x_T'])), 'x_T differs from the reference\'s randn_tensor draw'
    gap32 = g['chain_gap_ref32']
    gap_hip = {int(k): float((cap[int(k)] - torch.from_numpy(x).double()).abs().max()) for k, x in zip(g['chain_states'], g['chain_x'])}
    end64, end32 = torch.from_numpy(g['end_x_fp64']).double(), torch.from_numpy(g['end_x_fp32']).double()
    u_hip = _u8(cap[-1])
    rep = dict(chain_states=sorted(gap_hip), gap_hip=[gap_hip[k] for k in sorted(gap_hip)],
               gap_ref32=[float(gap32[k]) for k in sorted(gap_hip)],
               bound=[CHAIN_FACTOR * float(gap32[k]) + CHAIN_FLOOR for k in sorted(gap_hip)],
               gap_ref32_every_state=[float(v) for v in gap32],
               captured_vs_eager_max_abs=max(float((a - b).abs().max()) for a, b in zip(cap, eager)),
               end_abs_hip_vs_fp64=float((cap[-1] - end64).abs().max()), end_abs_hip_vs_ref32=float((cap[-1] - end32).abs().max()),
               end_abs_ref32_vs_fp64=float(g['end_abs_ref32']),
               u8_differing_hip_vs_fp64=int((u_hip != g['image_u8_fp64']).sum()),
               u8_differing_hip_vs_ref32=int((u_hip != g['image_u8_fp32']).sum()),
               u8_differing_ref32_vs_fp64=int((g['image_u8_fp32'] != g['image_u8_fp64']).sum()), u8_total=int(u_hip.size))
    report['sampling/free_running_chain/full'] = rep
    assert all(torch.equal(a, b) for a, b in zip(cap, eager)), rep['captured_vs_eager_max_abs']
    bad = [(k, h, b) for k, h, b in zip(rep['chain_states'], rep['gap_hip'], rep['bound']) if not h <= b]
    assert not bad, bad
