"""Per-launch fp64 parity at the launch shapes of the benchmarked workloads.

The kernel tests (test_kernels_gpu.py) compare every kernel with fp64 at hand-picked shapes; the instantiation, tile, split count
and tail path of a launch are decided by its shape, so the launches the product actually makes are covered there only by luck,
and end to end a wrong tail tile or split-K slice of one layer moves the UNet output by ~1e-6 -- below every end-to-end
tolerance.  Here one step of each workload `bench.py` times runs with the `ops` entry points wrapped; every call is reduced to a
signature (shapes, strides, storage offsets, aliasing, optional operands, which packed weight operand, and the launch names the
call passed to `ops._run`), and every distinct signature is replayed with seeded random data through the same entry point --
same dispatch, same launch names (asserted) -- against an fp64 evaluation of the same operation on the kernels' edges
(tests/helpers.py: edge_images, edge_tiles).  A floor of instantiations per workload keeps a dispatch change from shrinking
the coverage without notice."""
import inspect
import math
import random

import pytest
import torch

import golden_common as gc
from conftest import isolated
from helpers import (edge_images, edge_tiles, make_model, pkg, ref_attention, ref_conv_dgrad, ref_conv_fwd, ref_conv_wgrad,
                     ref_groupnorm, relerr)

pytestmark = pytest.mark.gpu
DEV = 'cuda'

ENTRY = ('conv_forward', 'conv_dgrad', 'conv_dgrad_s2', 'conv_wgrad', 'linear_forward', 'linear_dgrad', 'linear_wgrad', 'bmm_tn',
         'bmm_nn', 'bmm_nt', 'attention_fwd', 'groupnorm_fwd', 'groupnorm_bwd', 'softmax_fwd', 'softmax_bwd')
WORKLOADS = ('cifar256', 'c4', 'ddim', 'bedroom256', 'ldm')

# Every contraction kernel of the round-6 rocprofv3 summary of each config (profiles/round6_bench_kernel_stats.csv, round6_c4_finetune_,
# round6_ddim_, round6_bedroom256_serial_ and round6_ldm_kernel_stats.csv) as ops._run / launch_name name it, plus 'ks' / 'sp': a
# split-K forward or input-gradient launch (ks > 1) and a split weight-gradient launch (sp > 1).  Left out: the split-K epilogues
# and reductions (conv_splitk_epilogue*, splitk_reduce*), which have no _run name; every split signature compares their output.
# 'attn_fwd_fused_kernel' is ops._run's name for dp_attention_fwd, whose launcher picks the schedule (attn_fwd_pipe_kernel<2>).
_CIFAR_SETUP = ('launched by the 2-timestep sweep of the unpruned model that builds the pruned one (bench.py _pruned_cifar), not '
                'by the timed step: the same counts appear in the c4 and ddim summaries')
FLOOR = {
    'cifar256': ('conv_few_out_kernel', 'conv_gemm_fast_kernel<128, 128, false, true>', 'conv_gemm_fast_kernel<128, 128, true, true>',
                 'conv_gemm_kernel<128, 128, false, false>', 'conv_gemm_kernel<128, 128, true, false>',
                 'conv_gemm_kernel<64, 64, false, false>', 'conv_gemm_kernel<64, 64, true, false>', 'conv_wino2d_kernel<4, 3, false>',
                 'conv_wino2d_kernel<8, 2, false>', 'nt_gemm_fast_kernel<4, false>', 'nt_gemm_fast_kernel<4, true>',
                 'nt_gemm_kernel<128, 128, false, false>', 'nt_gemm_kernel<64, 128, false, false>', 'nt_gemm_kernel<64, 64, false, false>',
                 'nt_gemm_kernel<64, 64, false, true>', 'wgrad_wino2d_kernel<3>', 'wgrad_wino2d_kernel<4>', 'wgrad_wino2d_kernel<5>',
                 'ks', 'sp'),
    'c4': ('conv_few_out_kernel', 'conv_gemm_fast_kernel<128, 128, false, true>', 'conv_gemm_fast_kernel<128, 128, true, true>',
           'conv_gemm_fast_kernel<96, 128, true, true>', 'conv_gemm_kernel<128, 128, false, false>', 'conv_gemm_kernel<128, 128, true, false>',
           'conv_gemm_kernel<64, 128, false, false>', 'conv_gemm_kernel<64, 128, true, false>', 'conv_gemm_kernel<64, 64, false, false>',
           'conv_gemm_kernel<64, 64, true, false>', 'conv_wino2d_kernel<4, 3, false>', 'conv_wino2d_kernel<8, 2, false>',
           'conv_wino2d_m32_kernel<4, 5, false>', 'conv_wino2d_tail_kernel<4, 3, false>', 'conv_wino2d_tail_kernel<8, 2, false>',
           'nt_gemm_fast_kernel<3, false>', 'nt_gemm_fast_kernel<3, true>', 'nt_gemm_kernel<128, 128, false, false>',
           'nt_gemm_kernel<64, 128, false, false>', 'nt_gemm_kernel<64, 64, false, false>', 'nt_gemm_kernel<64, 64, false, true>',
           'wgrad_wino2d_kernel<4>', 'wgrad_wino2d_tail_kernel<5>', 'ks', 'sp'),
    'ddim': ('attn_fwd_fused_kernel', 'conv_few_out_kernel', 'conv_gemm_fast_kernel<96, 128, true, true>',
             'conv_gemm_kernel<128, 128, false, false>', 'conv_gemm_kernel<64, 64, false, false>', 'conv_wino2d_kernel<4, 3, false>',
             'conv_wino2d_kernel<8, 2, false>', 'conv_wino2d_m32_kernel<4, 5, false>', 'nt_gemm_kernel<64, 64, false, false>', 'ks'),
    'bedroom256': ('conv_few_out_kernel', 'conv_gemm_fast_kernel<128, 128, false, true>', 'conv_gemm_fast_kernel<128, 128, true, true>',
                   'conv_gemm_kernel<128, 128, false, false>', 'conv_gemm_kernel<64, 64, false, false>', 'conv_gemm_kernel<64, 64, true, false>',
                   'conv_wino2d_kernel<4, 2, true>', 'conv_wino2d_kernel<4, 3, false>', 'conv_wino2d_kernel<8, 2, false>',
                   'nt_gemm_fast_kernel<4, false>', 'nt_gemm_fast_kernel<4, true>', 'nt_gemm_kernel<128, 128, false, false>',
                   'nt_gemm_kernel<64, 64, false, false>', 'nt_gemm_kernel<64, 64, false, true>', 'wgrad_wino2d_kernel<5>',
                   'wgrad_wino_kernel<2, 2>', 'ks', 'sp'),
    'ldm': ('conv_few_out_kernel', 'conv_gemm_fast_kernel<128, 128, false, true>', 'conv_gemm_fast_kernel<96, 128, true, false>',
            'conv_gemm_fast_kernel<96, 128, true, true>', 'conv_gemm_kernel<128, 128, false, false>', 'conv_gemm_kernel<64, 128, false, false>',
            'conv_gemm_kernel<64, 64, false, false>', 'conv_gemm_kernel<64, 64, true, false>', 'conv_wino2d_kernel<4, 3, false>',
            'conv_wino2d_kernel<8, 2, false>', 'nt_gemm_fast_kernel<3, false>', 'nt_gemm_fast_kernel<3, true>',
            'nt_gemm_fast_kernel<4, false>', 'nt_gemm_fast_kernel<4, true>', 'nt_gemm_kernel<128, 128, false, false>',
            'nt_gemm_kernel<64, 128, false, false>', 'nt_gemm_kernel<64, 64, false, false>', 'nt_gemm_kernel<64, 64, false, true>',
            'wgrad_wino2d_kernel<4>', 'wgrad_wino2d_kernel<5>', 'wgrad_wino_kernel<2, 2>', 'ks', 'sp'),
}
# Contraction kernels of a summary that the harvested step does not launch, each with its reason.
NOT_IN_STEP = {
    'c4': {k: _CIFAR_SETUP for k in ('nt_gemm_fast_kernel<4, false>', 'nt_gemm_fast_kernel<4, true>', 'wgrad_wino2d_kernel<5>')},
    'ddim': {k: _CIFAR_SETUP + ' (the sampling forward has no backward)' for k in (
        'conv_gemm_fast_kernel<128, 128, false, true>', 'conv_gemm_fast_kernel<128, 128, true, true>', 'conv_gemm_kernel<64, 64, true, false>',
        'nt_gemm_fast_kernel<4, false>', 'nt_gemm_fast_kernel<4, true>', 'nt_gemm_kernel<128, 128, false, false>',
        'nt_gemm_kernel<64, 64, false, true>', 'wgrad_wino2d_kernel<5>')},
}

TOL_FWD, TOL_WGRAD, TOL_GN, TOL_ATTN, TOL_SOFTMAX = 3e-6, 5e-6, 2e-5, 1e-5, 1e-5


LONG_CHAIN_TOL = 4e-6


def tol_fwd(entry, K):
    """TOL_FWD (the kernel tests' bound), with one measured exception: an input gradient of a Linear with fewer than 64 rows
    (linear_dgrad -> bmm_nn, no split-K below 64 output rows) reducing more than 4096 terms in one fp32 chain -- the bedroom
    model's time-embedding projections, 9984 terms, 3.1e-6."""
    return LONG_CHAIN_TOL if (entry == 'linear_dgrad' and K > 4096) else TOL_FWD


# ---------------------------------------------------------------------------------------------------------------------------
# signatures
# ---------------------------------------------------------------------------------------------------------------------------
def _few_out(p):
    """conv_few_out_ok (csrc/gemm.hip): dp_conv_gemm runs a <= 4-output-channel 3x3 'same' convolution on conv_few_out_kernel."""
    g = p.g
    return (p.M <= 4 and p.lda == 4 and not p.a_kc and p.ntaps == 9 and g.kw == 3 and g.stride == 1 and g.sden == 1 and g.ups == 0
            and g.pad_t == 1 and g.pad_l == 1 and g.Ho == g.Hs and g.Wo == g.Ws and g.Hs == g.Hv and g.Ws == g.Wv and not p.X2
            and not p.tadd and not p.res and not p.accumulate and p.ksplit <= 1 and p.batches <= 1 and p.NPIX % (g.Ho * g.Wo) == 0)


def launch_name(call, name):
    """ops._run's name, with the split count of the parameter block the launch closure holds (ks: K slices of a conv_gemm /
    Winograd forward or input gradient, sp: pixel slices of a weight gradient); dp_conv_gemm launches that its launcher sends to
    conv_few_out_kernel are named so."""
    for cell in call.__closure__ or ():
        p = cell.cell_contents
        fields = {f[0] for f in getattr(type(p), '_fields_', ())}
        if name.startswith('conv_gemm') and 'ksplit' in fields and _few_out(p):
            return 'conv_few_out_kernel'
        if 'ksplit' in fields and p.ksplit > 1:
            return '%s ks=%d' % (name, p.ksplit)
        if 'splits' in fields and 'ksplit' not in fields and p.splits > 1:
            return '%s sp=%d' % (name, p.splits)
    return name


def _extent(shape, stride):
    return 1 + sum((s - 1) * st for s, st in zip(shape, stride)) if all(shape) else 0


def describe(ops, entry, args):
    """(key, record) of one call: tensors by (storage group, shape, stride, storage offset) -- offsets shifted per storage group
    by a multiple of 64 floats so that identical launches on different buffers share a key while alignment and the readable
    floats in front of a view (ops.ACT_GUARD) are kept -- packed weight operands by kind and size, everything else by value."""
    groups, tensors = {}, []

    def tensor(t):
        assert t.dtype == torch.float32 and t.is_cuda, (entry, t.dtype)
        g = groups.setdefault(t.untyped_storage().data_ptr(), len(groups))
        tensors.append([g, tuple(t.shape), tuple(t.stride()), t.storage_offset()])
        return ('T', len(tensors) - 1)

    def enc(name, v):
        if isinstance(v, torch.Tensor):
            return ('P', v.numel()) if name in ('wp', 'wd') else tensor(v)
        if name in ('wino', 'wino43') and v is not None:
            if v[0] == '2d':
                return ('W2D', v[1].numel(), v[2])
            return ('W43' if name == 'wino43' else 'W1D', v[0].numel(), v[1])
        if name == 'packs':
            return ('S2',) + tuple((wd.numel(), ld) for wd, ld in v)
        if isinstance(v, ops.ConvSpec):
            return ('spec',) + tuple(getattr(v, s) for s in ops.ConvSpec.__slots__)
        if v is not None and type(v).__name__ == 'Dropout':
            return ('drop', v.thr24, v.scale, v.seed, v.site, v.step, v.n_off, bool(v.step_dev))
        assert v is None or isinstance(v, (bool, int, float, str, tuple)), (entry, name, type(v))
        return v

    a = {n: enc(n, v) for n, v in args.items()}
    for g in range(len(groups)):
        lo = min(t[3] for t in tensors if t[0] == g)
        shift = max(0, lo - 64) // 64 * 64
        for t in tensors:
            if t[0] == g:
                t[3] -= shift
    tensors = [tuple(t) for t in tensors]
    return (entry, tuple(sorted(a.items())), tuple(tensors)), dict(entry=entry, args=a, tensors=tensors)


class Harvest:
    """Wraps the ops entry points (and ops._run) for the duration of one workload step; records each outermost call's
    signature with the launch names it emitted.  Calls one entry point makes to another (linear_forward -> bmm_nt) belong to
    the outer call."""

    def __init__(self, ops, monkeypatch):
        self.ops, self.sigs, self.depth, self.names = ops, {}, 0, None
        self.eps, self.last_eps = {}, None
        real_run = ops._run

        def run(call, name, *a, **k):
            if self.names is not None:
                self.names.append(launch_name(call, name))
            return real_run(call, name, *a, **k)
        monkeypatch.setattr(ops, '_run', run)
        for e in ENTRY:
            monkeypatch.setattr(ops, e, self._wrap(e, getattr(ops, e)))

    def _wrap(self, entry, fn):
        sig = inspect.signature(fn)

        def w(*a, **k):
            if self.depth:
                return fn(*a, **k)
            b = sig.bind(*a, **k)
            b.apply_defaults()
            args = dict(b.arguments)
            if entry == 'groupnorm_bwd':          # the eps of the forward that made `stats` (the backward does not take it)
                args['_eps'] = self.eps.get(args['stats'].data_ptr(), self.last_eps)
            self.depth, self.names = 1, []
            try:
                r = fn(*a, **k)
            finally:
                self.depth, names, self.names = 0, self.names, None
            if entry == 'groupnorm_fwd':
                self.eps[r[1].data_ptr()] = self.last_eps = args['eps']
            key, rec = describe(self.ops, entry, args)
            key = key + (tuple(names),)
            if key not in self.sigs:
                self.sigs[key] = dict(rec, names=names, calls=0)
            self.sigs[key]['calls'] += 1
            return r
        return w


# ---------------------------------------------------------------------------------------------------------------------------
# the workloads, built as bench.py builds them (one step each; cifar256: one timestep on each of its two pipelines)
# ---------------------------------------------------------------------------------------------------------------------------
def _pruned_cifar():
    sweep, diffusion = pkg('sweep'), pkg('diffusion')
    m = make_model(gc.CIFAR_CFG, 0)
    c = torch.from_numpy(gc.det_clean((16, 3, 32, 32), 1)).to(DEV)
    n = torch.from_numpy(gc.det_noise((16, 3, 32, 32), 2)).to(DEV)
    sweep.taylor_sweep(m, diffusion.DDPMScheduler(), c, n, num_steps=2, reduce_grads=False)
    sweep.prune_model(m, 0.3)
    for p in m.parameters():
        p.grad = None
    assert sum(p.numel() for p in m.parameters()) == 19851157
    return m


def run_workload(name, ops, monkeypatch):
    """Set up `name` outside the harvest, then run one step of it inside; returns the Harvest."""
    sweep, diffusion = pkg('sweep'), pkg('diffusion')
    if name in ('cifar256', 'bedroom256'):
        cfg, hw, B = (gc.CIFAR_CFG, 32, 256) if name == 'cifar256' else (gc.BEDROOM_CFG, 256, 4)
        model = make_model(cfg, 0)
        clean = torch.from_numpy(gc.det_clean((B, 3, hw, hw), 100)).to(DEV)
        noise = torch.from_numpy(gc.det_noise((B, 3, hw, hw), 200)).to(DEV)
        sweep.flatten_grads(model)
        step = sweep.HipSweepStep(model, diffusion.DDPMScheduler(), clean, noise, clean.numel(), 'mse', B)
        h = Harvest(ops, monkeypatch)
        for k in range(step._tp_want):               # one timestep per pipeline (cifar256: two, each at the full batch)
            step(k)
        step.finish()
    elif name == 'c4':
        train = pkg('train')
        model = _pruned_cifar()
        B = 128
        ft = train.FinetuneEngine(model, diffusion.DDPMScheduler(), lr=2e-4, dropout=0.1, dropout_seed=1)    # (its first step is eager)
        clean = torch.from_numpy(gc.det_clean((B, 3, 32, 32), 300)).to(DEV)
        noise = torch.from_numpy(gc.det_noise((B, 3, 32, 32), 400)).to(DEV)
        ts = train.antithetic_timesteps(B, 1000, torch.Generator().manual_seed(0)).to(DEV)
        h = Harvest(ops, monkeypatch)
        ft.step(clean, noise, ts)
    elif name == 'ddim':
        model = _pruned_cifar()
        x = torch.from_numpy(gc.det_noise((256, 3, 32, 32), 500)).to(DEV)
        with torch.no_grad():
            h = Harvest(ops, monkeypatch)                               # (the forward is captured when it is made)
            fwd = model.sampling_forward(tuple(x.shape), 100)           # what a 100-step loop gets: the forward captured for replay
            fwd(x, 990)
            fwd.close()
    else:
        ldm, ldm_sweep = pkg('ldm'), pkg('ldm_sweep')
        m = ldm.UNetModel(**gc.LDM_CIN256_CFG)
        gc.det_init_(m, 1)
        model = m.to(DEV).eval()
        emb = ldm_sweep.ClassEmbedder(512, 1001)
        with torch.no_grad():
            emb.embedding.weight.copy_(torch.from_numpy(gc.det_param('embedding.weight', (1001, 512), 61)))
        emb = emb.to(DEV)
        with model.pin_weights():
            h = Harvest(ops, monkeypatch)
            ldm_sweep.ldm_importance_sweep(model, emb, num_steps=1, thr=0.1, n_samples=6, ddim_steps=20, latent_shape=(3, 64, 64),
                                           class_rng=random.Random(1), seed=1)
    torch.cuda.synchronize()
    monkeypatch.undo()
    return h


# ---------------------------------------------------------------------------------------------------------------------------
# replay
# ---------------------------------------------------------------------------------------------------------------------------
def _weight(g, *shape):
    fan = 1
    for s in shape[1:]:
        fan *= s
    return torch.randn(shape, generator=g, device=DEV) / math.sqrt(fan)


def _d(t):
    return None if t is None else t.double().cpu()


def replay(ops, rec, seed, monkeypatch):
    """Run one recorded signature on seeded data; returns (launch names, [(label, relerr, tol)])."""
    entry, enc = rec['entry'], rec['args']
    g = torch.Generator(device=DEV).manual_seed(seed)
    span = {}
    for grp, shape, stride, off in rec['tensors']:
        span[grp] = max(span.get(grp, 0), off + _extent(shape, stride))
    bufs = {grp: torch.randn(n + 64, generator=g, device=DEV) for grp, n in span.items()}

    def view(i, b=bufs):
        grp, shape, stride, off = rec['tensors'][i]
        return torch.as_strided(b[grp], shape, stride, off)

    live = {n: (view(v[1]) if isinstance(v, tuple) and v and v[0] == 'T' else v) for n, v in enc.items()}
    spec = None
    if 'spec' in enc:
        spec = ops.ConvSpec()
        for s, v in zip(ops.ConvSpec.__slots__, enc['spec'][1:]):
            setattr(spec, s, v)
        live['spec'] = spec
    if isinstance(enc.get('drop'), tuple):
        d = ops.L.Dropout()
        thr24, scale, seed_, site, step, n_off, step_dev = enc['drop'][1:]
        d.thr24, d.scale, d.seed, d.site, d.step, d.n_off, d.step_dev = thr24, scale, seed_, site, step, n_off, None
        if step_dev:                                   # the step read from a device scalar (replayed finetune steps)
            live['_step_dev'] = torch.tensor([step], dtype=torch.int32, device=DEV)
            d.step_dev = live['_step_dev'].data_ptr()
        live['drop'] = d
    # weights: a random logical weight packed by the per-layer packer of the recorded operand (same ld, same size)
    w = None
    if entry in ('conv_forward', 'conv_dgrad', 'conv_dgrad_s2'):
        if entry == 'conv_forward':
            Cout, Cin = live['Cout'], live['x'].shape[1] + (live['x2'].shape[1] if live['x2'] is not None else 0)
        else:
            Cout, Cin = live['dy'].shape[1], live['Cin']
        w = _weight(g, Cout, Cin, spec.kh, spec.kw).contiguous()
        mode = 0 if entry == 'conv_forward' else 1
        if entry == 'conv_dgrad_s2':
            packs = [ops.pack_weight_s2(w, ph, pw, spec.pad) for ph in (0, 1) for pw in (0, 1)]
            assert tuple((p.numel(), ld) for p, ld in packs) == enc['packs'][1:]
            live['packs'] = packs
        else:
            key = 'wp' if mode == 0 else 'wd'
            wp, ld = ops.pack_weight(w, mode)
            assert (wp.numel(), ld) == (enc[key][1], live['ld' if mode == 0 else 'ldd']), (entry, enc[key], ld)
            live[key] = wp
            for k in ('wino', 'wino43'):
                e = enc.get(k)
                if e is None:
                    continue
                if e[0] == 'W2D':
                    U, ld = ops.pack_weight_wino2d(w, mode)
                    live[k] = ('2d', U, ld)
                elif e[0] == 'W1D':
                    U, ld = ops.pack_weight_wino(w, mode)
                    live[k] = (U, ld)
                else:
                    U, ld = ops.pack_weight_wino43(w)
                    live[k] = (U, ld)
                assert (U.numel(), ld) == e[1:], (entry, k, e, U.numel(), ld)
    # inputs the operation needs to be meaningful
    if entry == 'softmax_bwd':
        live['p_'].copy_(torch.softmax(live['p_'] * 2.0, -1))
    if entry == 'groupnorm_bwd':
        x = live['x'] if live['x2'] is None else torch.cat([live['x'], live['x2']], 1)
        xg = x.double().reshape(x.shape[0] * live['G'], -1)
        var, mean = torch.var_mean(xg, -1, unbiased=False)
        live['stats'].copy_(torch.stack([mean, 1.0 / torch.sqrt(var + live['_eps'])], 1).float())
    pre_bufs = {grp: b.clone() for grp, b in bufs.items()}
    pre = {n: (view(v[1], pre_bufs) if isinstance(v, tuple) and v and v[0] == 'T' else None) for n, v in enc.items()}
    call = {n: v for n, v in live.items() if not n.startswith('_')}
    names = []
    real_run = ops._run
    monkeypatch.setattr(ops, '_run', lambda c, n, *a, **k: (names.append(launch_name(c, n)), real_run(c, n, *a, **k))[1])
    try:
        out = getattr(ops, entry)(**call)
    finally:
        monkeypatch.setattr(ops, '_run', real_run)
    torch.cuda.synchronize()
    return names, compare(ops, entry, live, pre, out, w)


def compare(ops, entry, a, pre, out, w):
    """fp64 evaluation of the replayed call on its edges; [(label, relerr, tol)]."""
    res = []
    if entry in ('conv_forward', 'conv_dgrad', 'conv_dgrad_s2'):
        spec, wd = a['spec'], w.double().cpu()
        imgs = edge_images(out.shape[0], out.shape[2] * out.shape[3])
        if entry == 'conv_forward':
            x = _d(pre['x'][imgs])
            if pre['x2'] is not None:
                x = torch.cat([x, _d(pre['x2'][imgs])], 1)
            ref = a['alpha'] * ref_conv_fwd(x, wd, spec)
            if pre['bias'] is not None:
                ref += _d(pre['bias'])[None, :, None, None]
            if pre['tadd'] is not None:
                ref += _d(pre['tadd'][imgs])[:, :, None, None]
            if pre['res'] is not None:
                ref += _d(pre['res'][imgs])
            ref *= a['post_scale']
            if a['relu']:
                ref = ref.clamp_min(0)
        elif entry == 'conv_dgrad':
            ref = a['alpha'] * ref_conv_dgrad(_d(pre['dy'][imgs]), wd, spec, a['in_hw'])
        else:
            ref = ref_conv_dgrad(_d(pre['dy'][imgs]), wd, spec, a['in_hw'])
            if pre['add'] is not None:
                ref += _d(pre['add'][imgs])
        if a.get('accumulate'):
            ref += _d(pre['out'][imgs])
        K = (w.shape[1] if entry == 'conv_forward' else w.shape[0]) * spec.kh * spec.kw
        res.append(('out', relerr(out[imgs], ref), tol_fwd(entry, K)))
    elif entry == 'conv_wgrad':
        spec, x1, x2, dy = a['spec'], pre['x'], pre['x2'], pre['dy']
        C1 = x1.shape[1]
        Cin = C1 + (x2.shape[1] if x2 is not None else 0)
        Cout = dy.shape[1]
        rows, cols = edge_tiles(Cout, 64), edge_tiles(Cin, 32)
        c1 = [c for c in cols if c < C1]
        xs = x1[:, c1]
        if x2 is not None and len(c1) < len(cols):
            xs = torch.cat([xs, x2[:, [c - C1 for c in cols if c >= C1]]], 1)
        ref = a['alpha'] * ref_conv_wgrad(dy[:, rows], xs, spec, spec.kh, spec.kw)
        got = out.view(Cout, Cin, spec.kh, spec.kw)[rows][:, cols]
        if a['accumulate']:
            ref += _d(pre['gw'].view(Cout, Cin, spec.kh, spec.kw)[rows][:, cols])
        res.append(('gw', relerr(got, ref), TOL_WGRAD))
    elif entry == 'linear_forward':
        ref = _d(pre['x']) @ _d(pre['w']).t()
        if pre['bias'] is not None:
            ref += _d(pre['bias'])
        res.append(('out', relerr(out, ref), tol_fwd(entry, pre['x'].shape[1])))
    elif entry == 'linear_dgrad':
        ref = _d(pre['dy']) @ _d(pre['w'])
        if a['accumulate']:
            ref += _d(pre['out'])
        res.append(('out', relerr(out, ref), tol_fwd(entry, pre['dy'].shape[1]) if pre['dy'].shape[0] < 64 else TOL_FWD))
    elif entry == 'linear_wgrad':
        ref = a['alpha'] * (_d(pre['dy']).t() @ _d(pre['x']))
        if a['accumulate']:
            ref += _d(pre['gw'])
        res.append(('gw', relerr(out, ref), TOL_WGRAD))
    elif entry in ('bmm_tn', 'bmm_nn', 'bmm_nt'):
        Z = out.shape[0]
        zs = sorted({0, Z // 2, Z - 1})
        A, B = _d(pre['a'][zs]), _d(pre['b'][zs])
        if entry == 'bmm_tn':
            ref = a['alpha'] * torch.bmm(A.transpose(1, 2), B)
        elif entry == 'bmm_nn':
            ref = a['alpha'] * torch.bmm(A, B)
        else:
            ref = a['alpha'] * torch.bmm(A, B.transpose(1, 2))
            if pre['col_bias'] is not None:
                ref += _d(pre['col_bias'])[None, None, :]
        if a.get('accumulate'):
            ref += _d(pre['out'][zs])
        res.append(('out', relerr(out[zs], ref), tol_fwd(entry, A.shape[1] if entry == 'bmm_tn' else A.shape[2])))
    elif entry == 'attention_fwd':
        imgs = edge_images(out.shape[0], out.shape[2] * out.shape[3])
        ref = ref_attention(_d(pre['q'][imgs]), _d(pre['k'][imgs]), _d(pre['v'][imgs]), a['heads'], a['scale'])
        res.append(('out', relerr(out[imgs], ref), TOL_ATTN))
    elif entry in ('softmax_fwd', 'softmax_bwd'):
        Z = out.shape[0]
        zs = sorted({0, Z // 2, Z - 1})
        if entry == 'softmax_fwd':
            ref = _d(pre['s'][zs]).softmax(-1)
        else:
            p, dp = _d(pre['p_'][zs]), _d(pre['dp_'][zs])
            ref = a['scale'] * p * (dp - (p * dp).sum(-1, keepdim=True))
        res.append(('out', relerr(out[zs], ref), TOL_SOFTMAX))
    elif entry in ('groupnorm_fwd', 'groupnorm_bwd'):
        x1, x2 = pre['x'], pre['x2']
        N, C1, H, W = x1.shape
        Cc = C1 + (x2.shape[1] if x2 is not None else 0)
        G = a['G']
        imgs = edge_images(N, H * W)
        x = _d(x1[imgs]) if x2 is None else torch.cat([_d(x1[imgs]), _d(x2[imgs])], 1)
        m = None
        if a['drop'] is not None:
            d0 = a['drop']
            dm = ops.L.Dropout()
            dm.thr24, dm.scale, dm.seed, dm.site, dm.step, dm.n_off, dm.step_dev = d0.thr24, d0.scale, d0.seed, d0.site, d0.step, 0, None
            m = _d(ops.dropout_mask(N * Cc * H * W, dm, DEV, d0.n_off * Cc * H * W).view(N, Cc, H, W)[imgs])
        eps = a['eps'] if entry == 'groupnorm_fwd' else a['_eps']
        if entry == 'groupnorm_fwd':
            y, stats = out
            ref = ref_groupnorm(x, _d(pre['gamma']), _d(pre['beta']), G, eps, a['silu'])
            if m is not None:
                ref = ref * m
            res.append(('out', relerr(y[imgs], ref), TOL_GN))
            xg = x.reshape(len(imgs), G, -1)
            ref_st = torch.stack([xg.mean(-1), 1.0 / torch.sqrt(xg.var(-1, unbiased=False) + eps)], -1)
            res.append(('stats', relerr(stats.view(N, G, 2)[imgs], ref_st), TOL_GN))
        else:
            xr = x.clone().requires_grad_(True)
            gm = _d(pre['gamma'])[None].repeat(len(imgs), 1).requires_grad_(True)
            bt = _d(pre['beta'])[None].repeat(len(imgs), 1).requires_grad_(True)
            z = ref_groupnorm(xr, gm, bt, G, eps, a['silu'])
            if m is not None:
                z = z * m
            z.backward(_d(pre['dz'][imgs]))
            dx = xr.grad
            for k in ('add1', 'add2'):
                if pre[k] is not None:
                    dx = dx + _d(pre[k][imgs])
            res.append(('dx', relerr(out[0][imgs], dx), TOL_GN))
            res.append(('pws', relerr(out[1][imgs], torch.stack([bt.grad, gm.grad], -1)), TOL_GN))
            if a['want_rows'] and out[2] is not None:
                res.append(('rows', relerr(out[2][imgs], dx.sum((2, 3))), TOL_GN))
    else:
        raise AssertionError(entry)
    return res


def _summary(rec):
    parts = []
    for n, v in sorted(rec['args'].items()):
        if isinstance(v, tuple) and v and v[0] == 'T':
            t = rec['tensors'][v[1]]
            parts.append('%s%s' % (n, list(t[1])))
        elif isinstance(v, tuple) and v and v[0] in ('W2D', 'W1D', 'W43', 'S2'):
            parts.append('%s=%s' % (n, v[0]))
        elif isinstance(v, tuple) and v and v[0] == 'spec':
            parts.append('k%dx%d s%d p%d,%d u%d%s' % (v[5], v[6], v[2], v[7], v[8], v[4], ' same' if v[10] else ''))
        elif v not in (None, False) and n not in ('ld', 'ldd', 'wp', 'wd'):
            parts.append('%s=%s' % (n, v if not (isinstance(v, tuple) and v and v[0] == 'drop') else 'drop'))
    return '%s(%s)' % (rec['entry'], ', '.join(parts))


@pytest.mark.parametrize('workload', WORKLOADS)
@isolated(timeout=900, params=('workload',))
def test_launch_parity_at_the_benchmarked_shapes(workload, report, monkeypatch):
    """Every distinct launch signature of one step of `workload` (bench.py's configs, built from the package APIs at the bench's
    sizes) replayed on seeded data against fp64 on the kernels' edges: forward / input gradient / accumulate within 3e-6 (one
    measured exception, tol_fwd), weight gradients 5e-6, GroupNorm 2e-5, attention and softmax 1e-5 (relative to the largest
    reference value); the replay emits the launch names of the harvested call; the harvest reaches every contraction kernel of the
    config's profile (FLOOR[workload]; NOT_IN_STEP: the ones one step does not launch, with the reason)."""
    import time
    ops = pkg('ops')
    t0 = time.time()
    h = run_workload(workload, ops, monkeypatch)
    t_harvest = time.time() - t0
    reached = {n for rec in h.sigs.values() for n in rec['names']}
    missing = [f for f in FLOOR[workload] if not any(n == f or n.startswith(f + ' ') or (f in ('ks', 'sp') and (' %s=' % f) in n)
                                                     for n in reached)]
    assert not set(FLOOR[workload]) & set(NOT_IN_STEP.get(workload, ()))
    table, bad = [], []
    for i, rec in enumerate(h.sigs.values()):
        names, errs = replay(ops, rec, 1000 + i, monkeypatch)
        row = dict(sig=_summary(rec), calls=rec['calls'], names=rec['names'], err={k: e for k, e, _ in errs},
                   tol={k: t for k, _, t in errs})
        if names != rec['names']:
            row['replay_names'] = names
            bad.append(row)
        elif any(not (e < tol) for _, e, tol in errs):
            bad.append(row)
        table.append(row)
    report['launch_parity/' + workload] = dict(signatures=len(table), harvest_s=t_harvest, replay_s=time.time() - t0 - t_harvest,
                                               instantiations=sorted(reached), floor=len(FLOOR[workload]), floor_missing=missing,
                                               not_in_step=NOT_IN_STEP.get(workload, {}), failures=len(bad), table=table)
    assert not missing, ('instantiations of the floor not reached', missing, sorted(reached))
    assert not bad, bad[:10]
