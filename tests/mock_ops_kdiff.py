"""CPU stand-in (fp32 torch, the kernels' order of operations, one rounding per operation, true divisions) for the ops calls of
LMSDiscreteScheduler, KDPM2DiscreteScheduler and KDPM2AncestralDiscreteScheduler of diffusion.py: ops.kdpm2_step (csrc/kdiff.hip
dp_kdpm2_step) and ops.lms_step (dp_lms_step); ops.sigma_scale and ops.sigma_add_noise are those of tests/mock_ops_sigma.py and
record into the same list.  It also runs on device tensors (the GPU test compares the kernels with it there): every scalar is a 0-d
fp32 tensor on the data's device, so that no operation is rewritten into a multiplication by a reciprocal."""
import torch

from mock_ops_sigma import SIGMA_EPSILON, SIGMA_V, SIGMA_SAMPLE, calls, sigma_add_noise, sigma_scale      # noqa: F401

KDPM2_COEF = ('sig', 'c_out', 'c_den', 'dt', 'sigma_up')
LMS_COEF = ('sig', 'c_out', 'c_den', 'c0', 'c1', 'c2', 'c3')
KDIFF_EPSILON, KDIFF_V, KDIFF_SAMPLE = range(3)
KDPM2_FIRST, KDPM2_SECOND, KDPM2_SECOND_NOISE = range(3)
KDPM2_INSTANCES = tuple((s, p) for s in range(3) for p in (KDIFF_EPSILON, KDIFF_V))
LMS_INSTANCES = tuple((o, p) for o in range(1, 5) for p in range(3))
# calls: ('kdpm2', shape, pred, False, coef) and ('lms', order, pred, False, coef) beside mock_ops_sigma's entries


def _scalar(coef, x):
    return lambda name: torch.tensor(float(coef[name]), dtype=torch.float32, device=x.device)


def _x0(x, e, pred, s):
    if pred == KDIFF_EPSILON:
        return x - s('sig') * e
    if pred == KDIFF_V:
        return e * s('c_out') + x / s('c_den')
    return e.clone()


def _store(value, out):
    if out is None:
        return value
    out.copy_(value.reshape(out.shape))
    return out


def kdpm2_step(x, e, coef, pred=KDIFF_EPSILON, saved=None, noise=None, out=None):
    assert pred in (KDIFF_EPSILON, KDIFF_V), pred
    assert noise is None or saved is not None
    assert x.dtype == torch.float32 and e.dtype == torch.float32 and e.numel() == x.numel()
    assert all(t is None or (t.dtype == torch.float32 and t.numel() == x.numel()) for t in (saved, noise))
    assert not set(coef) - set(KDPM2_COEF)
    s = _scalar(coef, x)
    calls.append(('kdpm2', 0 if saved is None else 1 if noise is None else 2, pred, False, dict(coef)))
    d = (x - _x0(x, e, pred, s)) / s('sig')
    r = (x if saved is None else saved) + d * s('dt')
    if noise is not None:
        r = r + noise * s('sigma_up')
    return _store(r, out)                                            # the write, after every read: out may be x or saved


def lms_step(x, e, coef, order, pred=KDIFF_EPSILON, history=(), out=None, d_out=None, x0_out=None):
    assert order in (1, 2, 3, 4) and pred in (KDIFF_EPSILON, KDIFF_V, KDIFF_SAMPLE), (order, pred)
    history = list(history)[:order - 1]
    assert len(history) == order - 1
    assert x.dtype == torch.float32 and e.dtype == torch.float32 and e.numel() == x.numel()
    assert all(t.dtype == torch.float32 and t.numel() == x.numel() for t in history)
    assert not set(coef) - set(LMS_COEF)
    s = _scalar(coef, x)
    calls.append(('lms', order, pred, False, dict(coef)))
    x0 = _x0(x, e, pred, s)
    d = (x - x0) / s('sig')
    acc = s('c0') * d
    for k, h in enumerate(history):
        acc = acc + s('c%d' % (k + 1)) * h
    nxt = x + acc
    d_out, x0_out = _store(d, d_out), _store(x0, x0_out)
    return _store(nxt, out), d_out, x0_out
