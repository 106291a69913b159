"""Reference-free restatements and case lists for the x0 / dynamic-thresholding kernels (csrc/threshold.hip) and the DDPM / DDIM
schedulers that use them.

`abs_quantile` and `step` are the fp32 stand-ins of dp_x0_abs_quantile and dp_x0_step: the kernel's operations in torch's eager fp32
ops, one rounding each, the scalars as 0-d fp32 tensors on the data's device (so that no division is rewritten into a multiplication
by a reciprocal), torch.sort for the order statistics and an exactly rounded fused multiply-add (`fma32`) for the one contraction the
kernel has, the lerp of torch.quantile.  They run on host and on device tensors.  `step64` restates a whole step in fp64."""
import os

import numpy as np
import torch

import golden_common as gc
from dpm_solver_ref import toy_model                 # noqa: F401  (the same closed-form model output as the solver chains)

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
U = 2.0 ** -24                                       # unit roundoff of fp32
EPSILON, SAMPLE, V = 0, 1, 2
PRED = {'epsilon': EPSILON, 'sample': SAMPLE, 'v_prediction': V}
NONE, CLIP, THRESHOLD = 0, 1, 2
DDIM, DDPM, CONVERT = 0, 1, 2
ROUTE_LDS, ROUTE_MULTI = 1, 2
COEF = ('sa', 'sb', 'range', 'c0', 'c1', 'cz')
HOST_COEF = ('ratio', 'max_value')


# ------------------------------------------------------------------------------------------------ exact fp32 fma
def fma32(a, b, c):
    """round_fp32(a * b + c) of fp32 arrays, rounded ONCE.  a * b is exact in fp64 (48 significant bits); the fp64 sum with c is
    rounded to odd -- TwoSum gives the sum's error, and an inexact sum whose last bit is even moves to its odd neighbour on the
    error's side -- so that the second rounding, to fp32 (29 bits fewer), sees on which side of every fp32 tie the exact value lies.
    Non-finite operands take the plain fp64 expression (inf - inf = NaN, as the hardware's)."""
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    with np.errstate(invalid='ignore', over='ignore'):
        p = a * b
        s = p + c
        bb = s - p
        err = (p - (s - bb)) + (c - bb)
        fin = np.isfinite(s) & np.isfinite(p) & np.isfinite(c)
        even = (s.view(np.int64) & 1) == 0
        move = fin & (err != 0) & even
        toward = np.where(err > 0, np.inf, -np.inf)
        s = np.where(move, np.nextafter(s, toward), s)
        return s.astype(np.float32)


def quantile_rank(ratio, n):
    """(lo, hi, w): r = fp32(ratio) * fp32(n - 1) rounded in fp32, lo = floor r, hi = ceil r, w = r - lo in fp32."""
    r = np.float32(ratio) * np.float32(n - 1)
    lo = np.floor(r)
    return int(lo), int(np.ceil(r)), np.float32(r - lo)


def lerp_quantile(v_lo, v_hi, w):
    """torch.quantile's lerp of fp32 arrays with ONE fma: w < 0.5: fma(w, v_hi - v_lo, v_lo), else fma(w - 1, v_hi - v_lo, v_hi)."""
    v_lo, v_hi, w = np.asarray(v_lo, np.float32), np.asarray(v_hi, np.float32), np.float32(w)
    with np.errstate(invalid='ignore'):
        d = (v_hi - v_lo).astype(np.float32)
    return fma32(w, d, v_lo) if w < np.float32(0.5) else fma32(np.float32(w - np.float32(1.0)), d, v_hi)


# ------------------------------------------------------------------------------------------------ the fp32 stand-ins
def _t(v, like):
    return torch.tensor(float(v), dtype=like.dtype, device=like.device)


def form(pred, x, m, sa, sb):
    """(x0, eps) of the three model types; sa, sb 0-d tensors."""
    if pred == EPSILON:
        return (x - sb * m) / sa, m
    if pred == SAMPLE:
        return m, (None if x is None else (x - sa * m) / sb)      # x None: the quantile, or CONVERT, of a sample model
    return sa * x - sb * m, sa * m + sb * x


def abs_quantile(x, m, pred, sa, sb, ratio, max_value):
    """stats[B, 4] = (v_lo, v_hi, quantile, s): torch.sort of |x0| per image (NaNs last), the two order statistics, the fma lerp
    (NaN for a row that holds one), s = torch.clamp(quantile, min=1, max=max_value)."""
    B = m.shape[0]
    x0 = form(pred, None if x is None else x.reshape(B, -1), m.reshape(B, -1), _t(sa, m), _t(sb, m))[0]
    n = x0.shape[1]
    lo, hi, w = quantile_rank(ratio, n)
    srt = torch.sort(x0.abs(), dim=1).values
    v_lo, v_hi, last = (srt[:, i].cpu().numpy() for i in (lo, hi, n - 1))
    q = lerp_quantile(v_lo, v_hi, w)
    q = np.where(np.isnan(last), np.float32(np.nan), q).astype(np.float32)
    s = torch.clamp(torch.from_numpy(q), min=1.0, max=float(max_value)).numpy()
    return torch.from_numpy(np.stack([v_lo, v_hi, q, s], axis=1).astype(np.float32)).to(m.device)


def step(x, m, mode, pred, treat, coef, stats=None, z=None, reclip=False):
    """-> (out, treated x0) as new tensors, dp_x0_step's operations in its order (CONVERT: out is the treated x0, the second None)."""
    B = m.shape[0]
    c = {k: _t(v, m) for k, v in coef.items() if k in COEF}
    x0, eps = form(pred, x, m, c['sa'], c['sb'])
    if treat == CLIP:
        x0 = torch.clamp(x0, -c['range'], c['range'])
    elif treat == THRESHOLD:
        if stats is None:
            stats = abs_quantile(x, m, pred, coef['sa'], coef['sb'], coef['ratio'], coef['max_value'])
        s = stats[:, 3].reshape((B,) + (1,) * (m.dim() - 1))
        x0 = torch.clamp(x0, -s, s) / s
    if mode == CONVERT:
        return x0.clone(), None
    if reclip:
        eps = (x - c['sa'] * x0) / c['sb']
    if mode == DDIM:
        out = c['c0'] * x0 + c['c1'] * eps
        if z is not None:
            out = out + c['cz'] * z
    else:
        out = c['c0'] * x0 + c['c1'] * x
        out = out + (c['cz'] * z if z is not None else 0.0)
    return out, x0.clone()


def step64(x, m, mode, pred, treat, coef, z=None, reclip=False):
    """The same step in fp64 from the fp32 inputs and scalars, the quantile by torch.quantile in fp64."""
    x64 = None if x is None else x.double()
    m64, z64 = m.double(), None if z is None else z.double()
    c = {k: torch.tensor(float(np.float32(v)), dtype=torch.float64, device=m.device) for k, v in coef.items() if k in COEF}
    x0, eps = form(pred, x64, m64, c['sa'], c['sb'])
    if treat == CLIP:
        x0 = torch.clamp(x0, -c['range'], c['range'])
    elif treat == THRESHOLD:
        B = m.shape[0]
        q = torch.quantile(x0.reshape(B, -1).abs(), float(np.float32(coef['ratio'])), dim=1)
        s = torch.clamp(q, min=1.0, max=float(coef['max_value'])).reshape((B,) + (1,) * (m.dim() - 1))
        x0 = torch.clamp(x0, -s, s) / s
    if mode == CONVERT:
        return x0, None
    if reclip:
        eps = (x64 - c['sa'] * x0) / c['sb']
    if mode == DDIM:
        out = c['c0'] * x0 + c['c1'] * eps
        if z is not None:
            out = out + c['cz'] * z64
    else:
        out = c['c0'] * x0 + c['c1'] * x64 + (c['cz'] * z64 if z is not None else 0.0)
    return out, x0


def same_bits(a, b):
    """Equal bit for bit, a NaN standing for any NaN."""
    a, b = (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v) for v in (a, b))
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    nan = np.isnan(a) & np.isnan(b)
    ai, bi = a.view(np.int32), b.view(np.int32)
    return bool(np.all(nan | (ai == bi)))


# ------------------------------------------------------------------------------------------------ the fixtures' case lists
STEP_SHAPE = (4, 3, 8, 8)
X_SEED0, M_SEED0, Z_SEED0 = 700, 800, 900
TARGETS = (0.6, 1.25, 2.5, 6.0)                      # the quantile of |x0| the four images are scaled to: below 1, between, at the maxima
PREDS = ('epsilon', 'sample', 'v_prediction')
# treatment name -> scheduler keywords
TREATS = {'none': dict(clip_sample=False), 'clip': dict(clip_sample=True),
          'thr1.0': dict(thresholding=True, sample_max_value=1.0), 'thr1.5': dict(thresholding=True, sample_max_value=1.5),
          'thr4.0': dict(thresholding=True, sample_max_value=4.0)}
WHERE = ('first', 'middle', 'last')
N_STEPS = 10                                         # set_timesteps of the single steps
DDIM_VARIANTS = [(eta, ucmo) for eta in (0.0, 0.5) for ucmo in (False, True)]


def ddpm_file():
    return 'threshold_ddpm_steps.npz'


def ddim_file(pred, eta):
    return 'threshold_ddim_steps_%s_eta%s.npz' % (pred, ('%g' % eta).replace('.', ''))


CHAINS_FILE, TOY_FILE = 'threshold_chains.npz', 'threshold_toy.npz'


def step_files():
    return [ddpm_file()] + [ddim_file(p, e) for p in PREDS for e in (0.0, 0.5)]


def group_index(sched, pred, where):
    return (('ddpm', 'ddim').index(sched) * 3 + PREDS.index(pred)) * 3 + WHERE.index(where)


def base_inputs(sched, pred, where):
    """The unscaled seeded (x, m, z) of one (scheduler, model type, timestep) group; the fixture stores the per-image scales."""
    g = group_index(sched, pred, where)
    return tuple(torch.from_numpy(gc.det_noise(STEP_SHAPE, s0 + g)) for s0 in (X_SEED0, M_SEED0, Z_SEED0))


def scaled_inputs(sched, pred, where, scale):
    """(x, m, z): x and m of image b times the fixture's fp32 scale[b] (one fp32 multiplication each), z as drawn."""
    x, m, z = base_inputs(sched, pred, where)
    sc = torch.from_numpy(np.asarray(scale, np.float32)).reshape(-1, 1, 1, 1)
    return x * sc, m * sc, z


def timestep_at(timesteps, where):
    ts = [int(t) for t in timesteps]
    return ts[{'first': 0, 'middle': len(ts) // 2, 'last': len(ts) - 1}[where]]


def ddpm_cases():
    return [(pred, treat, where) for pred in PREDS for treat in TREATS for where in WHERE]


def ddim_cases():
    return [(pred, treat, where, eta, ucmo) for pred in PREDS for treat in TREATS for where in WHERE for eta, ucmo in DDIM_VARIANTS]


def ddpm_key(case):
    return 'ddpm:%s:%s:%s' % case


def ddim_key(case):
    return 'ddim:%s:%s:%s:eta%g:%s' % (case[0], case[1], case[2], case[3], 'reclip' if case[4] else 'plain')


def scale_key(sched, pred, where):
    return 'scale:%s:%s:%s' % (sched, pred, where)


def sched_kwargs(pred, treat):
    return dict(TREATS[treat], prediction_type=pred)


# ---- chains: 10 steps, thresholding at sample_max_value = 2.0; (name, scheduler, scheduler keywords, step keywords)
CHAIN_B, CHAIN_SEED, MODEL_SEED, CHAIN_STEPS = 2, 91, 5, 10
_THR = dict(thresholding=True, sample_max_value=2.0)
CHAINS = [('ddim_eps', 'ddim', dict(_THR), dict(eta=0.0)),
          ('ddim_v', 'ddim', dict(_THR, prediction_type='v_prediction'), dict(eta=0.0, use_clipped_model_output=True)),
          ('ddpm_eps', 'ddpm', dict(_THR), dict()),
          ('ddpm_v', 'ddpm', dict(_THR, prediction_type='v_prediction'), dict())]
TOY_SHAPE = (2, 3, 8, 8)
CHAIN_FACTOR, CHAIN_FLOOR = 10.0, 1e-5               # a chain state: within 10 x the reference fp32 chain's own gap + 1e-5 of fp64


def load(name):
    g = np.load(os.path.join(GOLD, name))
    return {k: g[k] for k in g.files}


def single_step_bound(e_ref32, y64):
    """The bound of a fixture step: max(4 e_ref32, 4 * 2^-24 * max|y64|)."""
    return max(4.0 * float(e_ref32), 4.0 * U * float(np.abs(y64).max()))
