"""The stage study on the device (`-m gpu`): dp_fold_sum (csrc/stage.hip), the snapshots of a staged sweep
(sweep.taylor_sweep(stages=...), HipSweepStep.snapshot) and stage_study.run against the reference's own stage loop
(tests/golden/make_golden_stage_study.py).

  dp_fold_sum   bit-equal to the chained torch fp32 adds in the same order and to a copy followed by `axpby(src, 1, out, 1)` per
                further source; sources bit-unchanged; every size at which the launcher takes another path (n < 4, the n % 4 tail,
                more than one block, past the 4096-block cap of the 16-byte path, 8 388 613), k = 1 .. 4, every pointer aligned and
                `out` / one source at element offset 1; both zeros, denormals, infinities, a NaN; overlap and bad k refused.
  snapshots     every stage_grads[s] of a 12-step staged sweep equals BIT FOR BIT the flat gradient of a fresh s-step sweep in the
                same mode on a fresh model with the same weights; losses and final gradients equal those of the unstaged sweep; two
                staged sweeps give the same bits.  Modes: 2 and 3 timestep pipelines, 2 with the weight-gradient side streams forced
                on, one pipeline, half-batch pipelines, a captured and natively replayed timestep, micro-batches.
  the fixture   pruned indices and shapes of every stage equal the reference's; snapshot gradients within max(4 e_ref32, 2e-5) of the
                fp64 run (relative L2 on the stored samples, and on the stored norms; 2e-5 = the floor of
                tests/test_e2e_gpu.py::test_tiny_sweep_gradients_match_reference, e_ref32 = the reference's own fp32 error); each
                stage's 5-step chain within 10 x the reference fp32 chain's own gap + 1e-5 of fp64 (the sampler tests' rule);
                ssim_curve over the PNGs run() wrote equals run()'s values; the caller's model keeps its weights and holds the
                full sweep's gradients.  SSIM parity with pytorch_msssim stays unpinned (the package is in neither tree).

Launch-site tables of csrc/stage.hip (the discipline of tests/test_prune_global_gpu.py, for the file's own ST_LAUNCH macro):
  BRANCHES every kernel expression the file's launch sites can record; LAUNCH_SITES ST_LAUNCH( sites per file
  (tests/test_stage_study_cpu.py counts them); CASES entry -> the cases that reach it and assert the ring names.
Every measured value is printed beside its bound (pytest -s); profiles/stage_study_gpu_tests.txt holds them."""
import ctypes
import os

import numpy as np
import pytest
import torch

import golden_common as gc
from helpers import load_json, load_npz, pkg

pytestmark = pytest.mark.gpu
DEV = 'cuda'

LAUNCH_SITES = {'stage.hip': 8}
BRANCHES = ['(fold_sum_kernel<%d, %s>)' % (k, v) for k in (1, 2, 3, 4) for v in ('false', 'true')]
CASES = {}


def case(*entries):
    def deco(fn):
        for e in entries:
            assert e in BRANCHES, e
            CASES.setdefault(e, []).append(fn)
        return fn
    return deco


@pytest.fixture(scope='module')
def ops():
    o = pkg('ops')
    o.L.load()
    return o


def launched(ops, fn):
    """(fn(), the kernel expressions of the launches fn issued, oldest first)."""
    lib = ops.L.load()
    c0 = lib.dp_launch_count()
    r = fn()
    n = lib.dp_launch_count() - c0
    assert 0 < n <= 256, n
    arr = (ctypes.c_char_p * 256)()
    k = lib.dp_recent_launches(arr, 256)
    assert k >= n
    return r, [arr[i].decode() for i in range(k - n, k)]


def _line(report, key, **kw):
    report['stage_study/' + key] = kw
    print('stage_study/%s %s' % (key, ' '.join('%s=%.3e' % (k, v) if isinstance(v, float) else '%s=%s' % (k, v) for k, v in kw.items())))


def bits(t):
    return t.contiguous().view(torch.int32)


# ========================================================================================================================== dp_fold_sum
CAP = 4096 * 256 * 4                    # elements one launch of the 16-byte path covers without a second grid-stride trip
SIZES = [1, 3, 4, 5, 255, 256, 257, 1027, CAP + 1029, 8388613]
INF, NAN = float('inf'), float('nan')
# one row per leading element, one column per source: both zeros, denormals, infinities, an overflow, one NaN that is read and one
# that the adds make
SPECIALS = [(0.0, -0.0, 0.0, -0.0), (-0.0, -0.0, -0.0, -0.0), (1e-40, 1e-40, -2e-40, 1e-45), (INF, 1.0, INF, -3.0),
            (-INF, -INF, 2.0, 0.0), (NAN, 1.0, 2.0, 3.0), (1.0, INF, -INF, 5.0), (3e38, 3e38, -3e38, 1.0), (1e-38, -1e-38, 1e-45, -0.0)]


@pytest.fixture(scope='module')
def sources():
    """Four seeded buffers of the largest size + 1 with the special values in front (and again at the very end of every size's
    range -- the scalar tail -- through `fold_inputs`)."""
    gen = torch.Generator().manual_seed(23)
    return [torch.randn(SIZES[-1] + 1, generator=gen).to(DEV) for _ in range(4)]


def fold_inputs(sources, n, k, src_off):
    """k sources of n elements: views at element offset 0, the last one at `src_off`; specials at the head and at the tail."""
    srcs = []
    for j in range(k):
        off = src_off if j == k - 1 else 0
        base = sources[j][:n + 1].clone()
        v = base[off:off + n]
        col = torch.tensor([row[j] for row in SPECIALS], dtype=torch.float32, device=DEV)
        m = min(n, len(SPECIALS))
        v[:m] = col[:m]
        if n >= 2 * len(SPECIALS) + 4:
            v[n - len(SPECIALS):] = col.flip(0)
        assert v.data_ptr() % 16 == 4 * off
        srcs.append(v)
    return srcs


@case(*BRANCHES)
@pytest.mark.parametrize('n', SIZES)
def test_fold_sum_sizes_sources_layouts_and_values(n, ops, sources, report):
    checked = 0
    for k in (1, 2, 3, 4):
        for layout, out_off, src_off in (('aligned', 0, 0), ('out+1', 1, 0), ('src+1', 0, 1)):
            srcs = fold_inputs(sources, n, k, src_off)
            before = [s.clone() for s in srcs]
            out = torch.full((n + 1,), 7.0, device=DEV)[out_off:out_off + n]
            _, names = launched(ops, lambda: ops.fold_sum(out, srcs))
            vec = layout == 'aligned' and n >= 4
            assert names == ['(fold_sum_kernel<%d, %s>)' % (k, 'true' if vec else 'false')], (names, n, k, layout)
            want = srcs[0].clone()                                   # the chained torch fp32 adds, in the same order
            for s in srcs[1:]:
                want = want + s
            assert torch.equal(bits(out), bits(want)), (n, k, layout, 'torch adds')
            chain = torch.empty(n, device=DEV)                       # today's spelling: a copy, then axpby per further source
            chain.copy_(srcs[0])
            for s in srcs[1:]:
                ops.axpby(s.contiguous(), 1.0, chain, 1.0)
            assert torch.equal(bits(out), bits(chain)), (n, k, layout, 'copy + axpby')
            for s, b in zip(srcs, before):
                assert torch.equal(bits(s), bits(b)), (n, k, layout, 'a source was written')
            if n >= len(SPECIALS):
                head = out[:len(SPECIALS)].cpu()
                assert torch.isnan(head[5]) and (k < 3 or torch.isnan(head[6])) and (k < 2 or head[7] == INF)
            checked += 1
    _line(report, 'fold_sum/n=%d' % n, cases=checked, bit_equal_torch_adds=True, bit_equal_copy_axpby=True, sources_unchanged=True)


def test_fold_sum_refuses_overlap_and_bad_k(ops):
    DpHipError = pkg('_lib').DpHipError
    buf = torch.zeros(64, device=DEV)
    other = torch.ones(32, device=DEV)
    lib = ops.L.load()
    c0 = lib.dp_launch_count()
    for out, srcs in ((buf[:32], [buf[:32]]), (buf[:32], [other, buf[:32]]), (buf[8:40], [other, buf[:32]]),
                      (buf[:32], [other, other, other, buf[31:63]]), (buf[:32], []), (buf[:32], [other] * 5)):
        with pytest.raises(DpHipError) as e:
            ops.fold_sum(out, srcs)
        assert e.value.code == 1                                     # hipErrorInvalidValue
    assert lib.dp_launch_count() == c0 and not buf.any()
    ops.fold_sum(buf[:32], [other, buf[32:]])                        # adjacent, not overlapping
    assert torch.equal(buf[:32], other)
    empty = torch.empty(0, device=DEV)
    c0 = lib.dp_launch_count()
    ops.fold_sum(empty, [empty])                                     # n <= 0: a no-op
    assert lib.dp_launch_count() == c0


# ============================================================================================================ snapshots against fresh sweeps
def fixture_meta():
    return load_json('stage_study.json')


EXP = load_json('ddpm_original.json')                # the tiny 16 x 16 configuration of the ddpm_exp flavour (original-DDPM layout)
BATCH, CLEAN_SEED, NOISE_SEED = 4, 141, 142


def exp_model(seed=None):
    """The tiny ddpm_exp-flavour model with weights seeded by the original parameter names; (model, {original name: product name})."""
    ckpt, unet = pkg('checkpoint'), pkg('unet')
    c = EXP['cfg']
    cfg = ckpt.unet2d_config_from_ddpm_original(c['ch'], c['ch_mult'], c['num_res_blocks'], c['attn_resolutions'], c['image_size'])
    orig = {n: torch.from_numpy(gc.det_param(n, tuple(s), EXP['seed'] if seed is None else seed)) for n, s in EXP['shapes'].items()}
    model = unet.UNet2DModel(**cfg)
    model.load_state_dict(ckpt.convert_ddpm_original(orig))
    model.attention_scale_from_width = True              # an original-DDPM model, as train.load_teacher marks one
    return model.to(DEV).eval(), ckpt.ddpm_original_key_map(orig.keys())


def exp_inputs(clean_seed=CLEAN_SEED, noise_seed=NOISE_SEED):
    H = EXP['cfg']['image_size']
    return (torch.from_numpy(gc.det_clean((BATCH, 3, H, H), clean_seed)).to(DEV),
            torch.from_numpy(gc.det_noise((BATCH, 3, H, H), noise_seed)).to(DEV))


MODES = {
    'pipelines2': dict(timestep_pipelines=2),
    'pipelines3': dict(timestep_pipelines=3),
    'pipelines2_side_streams': dict(timestep_pipelines=2, overlap=True),
    'one_pipeline': dict(timestep_pipelines=1),
    'halves2': dict(halves=2),
    'replay': dict(timestep_pipelines=1, use_graph=True),
    'micro2': dict(timestep_pipelines=2, micro=2),
}
NUM_STEPS, STAGES = 12, (0, 1, 3, 4, 7, 12)


def sweep_in_mode(mode, num_steps, stages=None):
    """A sweep of `num_steps` timesteps in `mode` on a fresh model: (result, flat gradients, the step)."""
    sweep, diffusion = pkg('sweep'), pkg('diffusion')
    m = MODES[mode]
    model, _ = exp_model()
    clean, noise = exp_inputs()
    flat = sweep.flatten_grads(model)
    step = sweep.HipSweepStep(model, diffusion.DDPMScheduler(), clean, noise, clean.numel(), 'sum', clean.shape[0],
                              halves=m.get('halves', 1), timestep_pipelines=m.get('timestep_pipelines'))
    step.micro = m.get('micro')
    res = sweep.taylor_sweep(model, diffusion.DDPMScheduler(), clean, noise, num_steps=num_steps, loss_kind='sum', step_fn=step,
                             flat_grads=flat, use_graph=bool(m.get('use_graph')), stages=stages)
    torch.cuda.synchronize()
    return res, flat, step


@pytest.mark.parametrize('mode', list(MODES))
def test_snapshots_equal_fresh_sweeps_bit_for_bit(mode, monkeypatch, report):
    if MODES[mode].get('overlap'):
        monkeypatch.setenv('DP_OVERLAP', '1')                        # weight gradients on the engines' side streams at this size too
    staged, flat_s, step = sweep_in_mode(mode, NUM_STEPS, list(STAGES))
    assert sorted(staged['stage_grads']) == list(STAGES)
    # the mode is the one asked for
    want_tp = MODES[mode].get('timestep_pipelines', 1) if not (MODES[mode].get('micro') or MODES[mode].get('use_graph')) else 1
    if MODES[mode].get('halves') == 2:
        assert step._half is not None and not step._tp
    else:
        assert len(step._tp or []) == want_tp - 1 and step._tp_count == (NUM_STEPS if want_tp > 1 else 0)
    if MODES[mode].get('use_graph'):
        assert step._replay is not None, 'the captured timestep is replayed natively'
    if MODES[mode].get('overlap'):
        assert step.eng._side is not None and all(p.eng._side is not None for p in step._tp)
    if want_tp > 1:                                                  # stages 1, 3 and 7 leave the pipelines with unequal step counts
        assert [s % want_tp != 0 for s in (1, 3, 7)] == ([True, True, True] if want_tp == 2 else [True, False, True])
    plain, flat_p, _ = sweep_in_mode(mode, NUM_STEPS)
    assert 'stage_grads' not in plain
    assert staged['losses'] == plain['losses'] and len(plain['losses']) == NUM_STEPS
    assert torch.equal(bits(flat_s), bits(flat_p)), 'the staged sweep is not the sweep that was never interrupted'
    again, flat_a, _ = sweep_in_mode(mode, NUM_STEPS, list(STAGES))
    assert torch.equal(bits(flat_a), bits(flat_s)) and again['losses'] == staged['losses']
    nonzero = 0
    for s in STAGES:
        fresh, flat_f, _ = sweep_in_mode(mode, s)
        snap = staged['stage_grads'][s]
        assert snap.shape == flat_f.shape and snap.dtype == torch.float32
        assert torch.equal(bits(snap), bits(flat_f)), (mode, s, 'snapshot differs from the fresh %d-step sweep' % s)
        assert torch.equal(bits(again['stage_grads'][s]), bits(snap)), (mode, s, 'two staged sweeps differ')
        assert fresh['losses'] == staged['losses'][:s]
        nonzero += bool(snap.any())
    assert not staged['stage_grads'][0].any() and nonzero == len(STAGES) - 1
    assert torch.equal(bits(staged['stage_grads'][NUM_STEPS]), bits(flat_s))       # the last snapshot is the final gradient
    _line(report, 'snapshots/' + mode, stages=len(STAGES), bit_equal_fresh_sweeps=True, final_equal_unstaged=True, repeatable=True)


def test_staged_sweep_of_taylor_sweeps_own_step_and_its_refusals():
    """taylor_sweep builds the step itself (the mode it chooses for this shard) and snapshots it; thr, unsorted, repeated and
    out-of-range stages are refused before anything runs."""
    sweep, diffusion = pkg('sweep'), pkg('diffusion')
    clean, noise = exp_inputs()
    sch = diffusion.DDPMScheduler()
    model, _ = exp_model()
    res = sweep.taylor_sweep(model, sch, clean, noise, num_steps=4, loss_kind='sum', stages=[2, 4])
    flat = torch.cat([p.grad.reshape(-1) for p in model.parameters()])
    assert torch.equal(bits(res['stage_grads'][4]), bits(flat))
    model2, _ = exp_model()
    sweep.taylor_sweep(model2, sch, clean, noise, num_steps=2, loss_kind='sum')
    assert torch.equal(bits(res['stage_grads'][2]), bits(torch.cat([p.grad.reshape(-1) for p in model2.parameters()])))
    for bad in ([3, 1], [1, 1], [5], [-1, 2]):
        with pytest.raises(ValueError):
            sweep.taylor_sweep(model, sch, clean, noise, num_steps=4, loss_kind='sum', stages=bad)
    with pytest.raises(ValueError):
        sweep.taylor_sweep(model, sch, clean, noise, num_steps=4, loss_kind='sum', stages=[2], thr=0.05)


# ==================================================================================================== the reference fixture through run()
GRAD_FLOOR = 2e-5                       # the floor of tests/test_e2e_gpu.py::test_tiny_sweep_gradients_match_reference
CHAIN_FACTOR, CHAIN_FLOOR = 10.0, 1e-5  # the sampler tests' rule for a free-running chain


def group_key(root):
    """An attention block's q, k, v outputs and to_out inputs are ONE group in both trees (they meet in the attention product); the
    reference's tracer names it after `k`, the product's after `to_v`: the group is keyed by the block."""
    import re
    return re.sub(r'\.to_[qkv]$', '.to_qkv', root)


def expand(ranges):
    return [i for a, b in ranges for i in range(a, b)]


@pytest.fixture(scope='module')
def fixture_run(tmp_path_factory):
    """stage_study.run once on the fixture's model and inputs (HIP path), and one staged sweep on a second model with the same
    weights whose snapshots the gradient, shape and chain tests consume.  Shared, read-only."""
    S, sweep, diffusion = pkg('stage_study'), pkg('sweep'), pkg('diffusion')
    fx, arr, smp = fixture_meta(), load_npz('stage_study.npz'), load_npz('stage_study.samples.npz')
    model, kmap = exp_model(fx['model_seed'])
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    clean, noise = exp_inputs(fx['clean_seed'], fx['noise_seed'])
    x_T = torch.from_numpy(arr['x_T']).to(DEV)
    sampler_args = dict(timesteps=len(fx['chain_seq']), skip_type='uniform', eta=0.0)
    out_dir = str(tmp_path_factory.mktemp('stage_study'))
    res = S.run(model, diffusion.DDPMScheduler(), clean, noise, x_T, fx['stages'], pruning_ratio=fx['ratio'], loss_kind='sum',
                sampler_args=sampler_args, out_dir=out_dir, n_ssim=fx['n_chain'])
    model2, _ = exp_model(fx['model_seed'])
    staged = sweep.taylor_sweep(model2, diffusion.DDPMScheduler(), clean, noise, num_steps=fx['timesteps'], loss_kind='sum',
                                stages=[s for s in fx['stages'] if s > 0])
    torch.cuda.synchronize()
    return dict(fx=fx, arr=arr, smp=smp, res=res, model=model, model2=model2, kmap=kmap, before=before, out_dir=out_dir, x_T=x_T,
                staged=staged, sampler_args=sampler_args)


def test_study_masks_equal_the_references(fixture_run, report):
    fx, res, kmap = fixture_run['fx'], fixture_run['res'], fixture_run['kmap']
    assert res['stages'] == fx['stages'] and [p['stage'] for p in res['per_stage']] == fx['stages']
    base = res['per_stage'][0]
    assert base['pruned_idxs'] == {} and base['params'] == fx['per_stage']['0']['params_after'] and base['mse'] == 0.0
    assert abs(base['ssim'] - 1.0) < 1e-6
    e_loss = max(abs(a - b) / b for a, b in zip(res['losses'], fx['losses']))
    _line(report, 'fixture/losses', steps=len(res['losses']), loss_rel=e_loss, bound=2e-5)
    assert len(res['losses']) == 20 and e_loss < 2e-5            # tests/test_e2e_gpu.py's bound for this model's 'sum' losses
    for p in res['per_stage'][1:]:
        st = fx['per_stage'][str(p['stage'])]
        want = {group_key(kmap[root + '.weight'][:-len('.weight')]): expand(r) for root, _, r, _, _ in st['groups'] if r}
        mine = {group_key(root): idxs for root, idxs in p['pruned_idxs'].items() if idxs}
        margin = min(g[3] for g in st['groups'] if g[3] is not None)
        _line(report, 'fixture/masks/stage=%d' % p['stage'], groups=len(want), equal=mine == want, params=p['params'],
              ref_params=st['params_after'], smallest_gap=margin, ssim=p['ssim'], mse=p['mse'])
        assert len(mine) == sum(1 for i in p['pruned_idxs'].values() if i) and mine == want, p['stage']
        assert p['params'] == st['params_after'] and 0 < p['macs'] < base['macs']
        assert len(p['ssim_per_image']) == fx['n_chain'] and p['ssim'] < 1.0 and p['mse'] > 0.0


def test_snapshot_gradients_against_the_fp64_run(fixture_run, report):
    """Per tensor, in the reference's layout: relative L2 error on the stored samples and relative error of the L2 norm, each within
    max(4 e_ref32, 2e-5).  A tensor whose fp64 norm is below 1e-6 of the stage's largest (a gradient that is zero by symmetry, the
    k bias of an attention block: both runs hold rounding noise there) is held to 2e-5 of that largest norm instead."""
    ckpt = pkg('checkpoint')
    fx, arr, smp, staged, model2 = (fixture_run[k] for k in ('fx', 'arr', 'smp', 'staged', 'model2'))
    counts = arr['sample_count']
    offs = np.concatenate([[0], np.cumsum(counts)])
    names = [n for n, _ in model2.named_parameters()]
    shapes = [p.shape for _, p in model2.named_parameters()]
    for s in fx['stages'][1:]:
        flat = staged['stage_grads'][s].double().cpu()
        mine, off = {}, 0
        for n, sh in zip(names, shapes):
            mine[n] = flat[off:off + sh.numel()].view(sh)
            off += sh.numel()
        orig = ckpt.convert_to_ddpm_original(mine)
        norm64, norm_err32, sample_err32, s64 = arr['%d/norm64' % s], arr['%d/norm_err32' % s], arr['%d/sample_err32' % s], smp['%d/samples64' % s]
        top = float(norm64.max())
        worst = dict(sample=0.0, norm=0.0, small=0.0)
        for i, on in enumerate(fx['param_names']):
            g = orig[on].reshape(-1)
            idx = torch.from_numpy(arr['sample_idx'][offs[i]:offs[i + 1]].astype(np.int64))
            ref = torch.from_numpy(s64[offs[i]:offs[i + 1]])
            if norm64[i] <= 1e-6 * top:
                worst['small'] = max(worst['small'], float(g.norm()) / top / GRAD_FLOOR)
                assert float(g.norm()) <= GRAD_FLOOR * top, (s, on)
                continue
            e_s = float((g[idx] - ref).norm() / ref.norm()) if float(ref.norm()) > 0 else 0.0
            e_n = abs(float(g.norm()) - norm64[i]) / norm64[i]
            b_s, b_n = max(4 * sample_err32[i], GRAD_FLOOR), max(4 * norm_err32[i], GRAD_FLOOR)
            worst['sample'], worst['norm'] = max(worst['sample'], e_s / b_s), max(worst['norm'], e_n / b_n)
            assert e_s <= b_s and e_n <= b_n, (s, on, e_s, b_s, e_n, b_n)
        _line(report, 'fixture/grads/stage=%d' % s, tensors=len(fx['param_names']), worst_sample_err_over_bound=worst['sample'],
              worst_norm_err_over_bound=worst['norm'], worst_small_tensor_over_bound=worst['small'], floor=GRAD_FLOOR)


@pytest.fixture(scope='module')
def stage_models(fixture_run):
    """{stage: model}: prune_at_stage at every snapshot of the staged sweep (stage 0: the unpruned model itself)."""
    S = pkg('stage_study')
    fx, staged, model2 = (fixture_run[k] for k in ('fx', 'staged', 'model2'))
    unpruned = {n: tuple(p.shape) for n, p in model2.named_parameters()}
    out = {0: model2}
    for s in fx['stages'][1:]:
        out[s], _ = S.prune_at_stage(model2, staged['stage_grads'][s], fx['ratio'])
        assert out[s] is not model2 and {n: tuple(p.shape) for n, p in model2.named_parameters()} == unpruned       # never sliced
    return out


def test_pruned_shapes_of_every_stage_equal_the_references(fixture_run, stage_models):
    ckpt, fx = pkg('checkpoint'), fixture_run['fx']
    for s in fx['stages']:
        mine = ckpt.convert_to_ddpm_original({n: p.detach() for n, p in stage_models[s].named_parameters()})
        assert {n: list(t.shape) for n, t in mine.items()} == fx['per_stage'][str(s)]['shapes_after'], s


@pytest.mark.parametrize('stage', [0, 1, 5, 10, 15, 20])
def test_chain_of_every_stage_against_the_fp64_chain(stage, fixture_run, stage_models, report):
    """The 5-step chain of the stage's model from the stored x_T lies within 10 x the reference fp32 chain's own gap + 1e-5 of the
    fp64 chain (the sampler tests' rule).  The pruned stages hold it because a model of the original-DDPM layout scales its
    attention logits by the q width at run time (44 after the prune), as the reference's AttnBlock does (`int(c) ** -0.5`,
    ddpm_exp/models/diffusion.py): `UNet2DModel.attention_scale_from_width`, which prune_at_stage hands on.  With Diffusers' fixed
    scale (64 ** -0.5) the same chains lie 2.0 .. 2.6 from fp64; the last lines pin that the switch is what the pruned model runs
    with and that it changes nothing for the unpruned one."""
    E, ops = pkg('ddpm_exp_sampler'), pkg('ops')
    fx, arr, x_T = (fixture_run[k] for k in ('fx', 'arr', 'x_T'))
    st = fx['per_stage'][str(stage)]
    smp = E.Sampler(stage_models[stage], pkg('diffusion').DDPMScheduler().betas, tuple(x_T.shape[1:]), **fixture_run['sampler_args'])
    assert smp.seq == fx['chain_seq']
    with torch.no_grad():
        x = smp.sample_image(x_T)
        u8 = ops.image_to_u8(x, True).cpu().numpy()
    err = float(np.abs(x.double().cpu().numpy() - arr['%d/chain64' % stage]).max())
    bound = CHAIN_FACTOR * st['chain_gap'] + CHAIN_FLOOR
    diff = np.abs(u8.astype(np.int16) - arr['%d/bytes' % stage].astype(np.int16))
    _line(report, 'fixture/chain/stage=%d' % stage, err=err, bound=bound, ref_gap=st['chain_gap'], bytes_differing=int((diff > 0).sum()),
          bytes_max_diff=int(diff.max()))
    assert err <= bound, (stage, err, bound)
    # 127.5 x (bound + the reference's own gap) is far below one byte step: only a value at a rounding edge can move, by one
    assert 127.5 * (bound + st['chain_gap']) < 0.5 and int(diff.max()) <= 1
    m = stage_models[stage]
    assert m.attention_scale_from_width and m.engine().scale_from_q_width
    m.attention_scale_from_width = False                 # Diffusers' scale of the unpruned width
    try:
        with torch.no_grad():
            y = smp.sample_image(x_T)
    finally:
        m.attention_scale_from_width = True
    assert torch.equal(bits(y), bits(x)) == (stage == 0)


def test_ssim_curve_over_the_written_pngs_equals_the_studys_values(fixture_run, report):
    from PIL import Image
    S = pkg('stage_study')
    fx, res, out_dir = fixture_run['fx'], fixture_run['res'], fixture_run['out_dir']
    for s in fx['stages']:
        assert sorted(os.listdir(os.path.join(out_dir, str(s)))) == sorted('%d.png' % i for i in range(fx['n_chain']))
    img = np.asarray(Image.open(os.path.join(out_dir, '0', '0.png')))
    assert img.dtype == np.uint8 and img.shape == (16, 16, 3)
    curve = S.ssim_curve(out_dir, fx['stages'], base=0, n_samples=fx['n_chain'])
    _line(report, 'fixture/ssim_curve', curve=' '.join('%.6f' % v for v in curve), equal=curve == [p['ssim'] for p in res['per_stage']])
    assert curve == [p['ssim'] for p in res['per_stage']]


def test_the_callers_model_after_run(fixture_run):
    """Its weights are unchanged (bit for bit) and its gradients are those of the full sweep: the staged 20-step sweep's final
    gradient, which is also the last snapshot."""
    model, model2, staged, fx = (fixture_run[k] for k in ('model', 'model2', 'staged', 'fx'))
    for n, p in model.named_parameters():
        assert torch.equal(bits(p.detach()), bits(fixture_run['before'][n])), n
    flat = torch.cat([p.grad.reshape(-1) for p in model.parameters()])
    flat2 = torch.cat([p.grad.reshape(-1) for p in model2.parameters()])
    assert torch.equal(bits(flat), bits(flat2)) and torch.equal(bits(flat), bits(staged['stage_grads'][fx['timesteps']]))
    assert flat.any()
