"""CPU stand-ins (tests/threshold_ref.py: fp32 torch, the kernels' order of operations, one rounding per operation, true divisions,
torch.sort for the order statistics, an exactly rounded fma for the quantile's lerp) for the three ops calls of csrc/threshold.hip:
ops.x0_abs_quantile, ops.x0_step, ops.dynamic_threshold.  They also run on device tensors.  ddim_step / ddpm_step only record that
the default path of the two schedulers still goes to them, with the arguments it always had."""
import torch

import threshold_ref as R

THRESHOLD_LDS_MAX = 16384
X0_STEP_MAX_BLOCKS = 4096
X0_PRED_EPSILON, X0_PRED_SAMPLE, X0_PRED_V = R.EPSILON, R.SAMPLE, R.V
X0_PRED = dict(R.PRED)
X0_TREAT_NONE, X0_TREAT_CLIP, X0_TREAT_THRESHOLD = R.NONE, R.CLIP, R.THRESHOLD
X0_MODE_DDIM, X0_MODE_DDPM, X0_MODE_CONVERT = R.DDIM, R.DDPM, R.CONVERT
X0_ROUTE_LDS, X0_ROUTE_MULTI = R.ROUTE_LDS, R.ROUTE_MULTI
X0_COEF, X0_HOST_COEF = R.COEF, R.HOST_COEF
calls = []                                       # ('x0_step', mode, pred, treat, reclip, z given) | ('ddim_step', kwargs) | ...


def x0_abs_quantile(x, m, pred, sa, sb, ratio, max_value, route=None):
    assert route in (None, X0_ROUTE_LDS, X0_ROUTE_MULTI) and m.dtype == torch.float32
    calls.append(('x0_abs_quantile', pred, route))
    return R.abs_quantile(x, m, pred, sa, sb, ratio, max_value)


def x0_step(x, m, mode, pred, treat, coef, stats=None, z=None, out=None, x0_out=None, reclip=False, route=None):
    assert m.dtype == torch.float32 and not set(coef) - set(X0_COEF) - set(X0_HOST_COEF)
    assert mode != X0_MODE_CONVERT or (z is None and x0_out is None)
    calls.append(('x0_step', mode, pred, treat, bool(reclip), z is not None))
    if treat == X0_TREAT_THRESHOLD and stats is None:
        stats = R.abs_quantile(x, m, pred, coef['sa'], coef['sb'], coef['ratio'], coef['max_value'])
    res, x0 = R.step(x, m, mode, pred, treat, coef, stats=stats, z=z, reclip=reclip)
    # every store after every read: out may be x
    if out is None:
        out = res
    else:
        out.copy_(res)
    if x0_out is not None:
        x0_out.copy_(x0)
    return out, x0_out, stats


def dynamic_threshold(sample, ratio=0.995, max_value=1.0, out=None):
    return x0_step(None, sample, X0_MODE_CONVERT, X0_PRED_SAMPLE, X0_TREAT_THRESHOLD, dict(sa=1.0, sb=0.0, ratio=ratio, max_value=max_value),
                   out=out)[0]


def ddim_step(x, eps, a_t, a_prev, std=0.0, vnoise=None, clip=True, out=None, clip_range=1.0):
    calls.append(('ddim_step', dict(a_t=a_t, a_prev=a_prev, std=std, vnoise=vnoise, clip=clip, out=out, clip_range=clip_range)))
    return x.clone()


def ddpm_step(x, eps, sqrt_a_t, sqrt_b_t, c_x0, c_xt, sigma=0.0, vnoise=None, clip=True, clip_range=1.0, out=None):
    calls.append(('ddpm_step', dict(sqrt_a_t=sqrt_a_t, sqrt_b_t=sqrt_b_t, c_x0=c_x0, c_xt=c_xt, sigma=sigma, vnoise=vnoise, clip=clip,
                                    clip_range=clip_range, out=out)))
    return x.clone()
