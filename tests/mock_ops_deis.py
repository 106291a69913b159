"""CPU stand-ins (fp32 torch, the kernels' order of operations, one rounding per operation, true divisions) for the ops calls of
diffusion.DEISMultistepScheduler and diffusion.DPMSolverSinglestepScheduler: ops.deis_step and ops.dpm_single_step (csrc/deis.hip
dp_deis_step, dp_dpm_single_step), and ops.x0_abs_quantile through tests/threshold_ref.py.  They also run on device tensors (the
GPU test compares the kernels with them there): every scalar is a 0-d fp32 tensor on the data's device, so that no operation is
rewritten into a multiplication by a reciprocal."""
import torch

import threshold_ref as TR

DEIS_COEF = ('sa', 'sb', 'kx', 'k0', 'at', 'as0', 'c1', 'c2', 'c3')
DPM_SINGLE_COEF = ('sa', 'sb', 'kx', 'k0', 'k1', 'k2', 'ir0', 'ir1', 'r0', 'r1', 'dr')
X0_PRED_EPSILON, X0_PRED_SAMPLE, X0_PRED_V = TR.EPSILON, TR.SAMPLE, TR.V
X0_PRED = dict(TR.PRED)
KEEP_DEIS, KEEP_X0, KEEP_EPS = 0, 1, 2
calls = []                # ('deis_step', order, pred, treated) | ('dpm_single_step', order, pred, data_pred, heun, treated) | ('x0_abs_quantile', pred)


def x0_abs_quantile(x, m, pred, sa, sb, ratio, max_value, route=None):
    assert m.dtype == torch.float32 and route is None
    calls.append(('x0_abs_quantile', pred))
    return TR.abs_quantile(x, m, pred, sa, sb, ratio, max_value)


def dpm_single_reads_x(order, pred, data_pred):
    return order == 1 or pred != (X0_PRED_SAMPLE if data_pred else X0_PRED_EPSILON)


def _scalars(coef, names, like):
    assert not set(coef) - set(names)
    return {k: torch.tensor(float(v), dtype=torch.float32, device=like.device) for k, v in coef.items()}


def convert(x, m, pred, keep, sa, sb, stats):
    """The value the history keeps (de_convert of csrc/deis.hip); sa, sb 0-d tensors; stats [B, 4] or None."""
    if keep == KEEP_EPS:
        assert stats is None
        if pred == X0_PRED_EPSILON:
            return m.clone()
        if pred == X0_PRED_SAMPLE:
            return (x - sa * m) / sb
        return sa * m + sb * x
    if pred == X0_PRED_EPSILON:
        x0 = (x - sb * m) / sa
    elif pred == X0_PRED_SAMPLE:
        x0 = m.clone()
    else:
        x0 = sa * x - sb * m
    if stats is not None:
        B = m.shape[0]
        s = stats[:, 3].reshape((B,) + (1,) * (m.dim() - 1))
        x0 = torch.clamp(x0, -s, s) / s
    if keep == KEEP_X0:
        return x0
    return (x - sa * x0) / sb


def _finish(nxt, m0, out, m0_out):
    if m0_out is None:
        m0_out = m0
    else:
        m0_out.copy_(m0)                         # after every read of the history: m0_out may be the oldest buffer the step read
    if out is None:
        return nxt, m0_out
    out.copy_(nxt)                               # after every read: out may be x or xs
    return out, m0_out


def _history(order, m, m1, m2):
    hist = [m1, m2][:order - 1]
    assert all(h is not None and h.dtype == torch.float32 and h.numel() == m.numel() for h in hist)
    return hist


def deis_step(x, m, coef, order=1, pred=X0_PRED_EPSILON, m1=None, m2=None, stats=None, out=None, m0_out=None):
    assert order in (1, 2, 3) and x.dtype == torch.float32 and m.dtype == torch.float32 and x.numel() == m.numel()
    _history(order, m, m1, m2)
    c = _scalars(coef, DEIS_COEF, m)
    calls.append(('deis_step', order, pred, stats is not None))
    m0 = convert(x, m, pred, KEEP_DEIS, c['sa'], c['sb'], stats)
    if order == 1:
        nxt = c['kx'] * x - c['k0'] * m0
    else:
        v = (x / c['as0'] + c['c1'] * m0) + c['c2'] * m1
        if order == 3:
            v = v + c['c3'] * m2
        nxt = c['at'] * v
    return _finish(nxt, m0, out, m0_out)


def dpm_single_step(x, m, coef, order=1, pred=X0_PRED_EPSILON, data_pred=True, heun=False, xs=None, m1=None, m2=None, stats=None,
                    out=None, m0_out=None):
    assert order in (1, 2, 3) and m.dtype == torch.float32
    assert stats is None or data_pred
    _history(order, m, m1, m2)
    if dpm_single_reads_x(order, pred, data_pred):
        assert x is not None and x.dtype == torch.float32 and x.numel() == m.numel()
    else:
        x = None                                 # not read: an error below if it were
    u = x if order == 1 else xs
    assert u is not None and u.dtype == torch.float32 and u.numel() == m.numel()
    c = _scalars(coef, DPM_SINGLE_COEF, m)
    calls.append(('dpm_single_step', order, pred, bool(data_pred), bool(heun), stats is not None))
    m0 = convert(x, m, pred, KEEP_X0 if data_pred else KEEP_EPS, c['sa'], c['sb'], stats)
    if order == 1:
        nxt = c['kx'] * u - c['k0'] * m0
    elif order == 2:
        D1 = c['ir0'] * (m0 - m1)
        nxt = (c['kx'] * u - c['k0'] * m1) - c['k1'] * D1
    else:
        D10 = c['ir1'] * (m1 - m2)
        D11 = c['ir0'] * (m0 - m2)
        nxt = c['kx'] * u - c['k0'] * m2
        if not heun:
            nxt = nxt - c['k1'] * D11
        else:
            D1 = (c['r0'] * D10 - c['r1'] * D11) / c['dr']
            D2 = (2.0 * (D11 - D10)) / c['dr']
            nxt = (nxt - c['k1'] * D1) - c['k2'] * D2
    return _finish(nxt, m0, out, m0_out)
