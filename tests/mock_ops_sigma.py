"""CPU stand-in (fp32 torch, the kernels' order of operations, one rounding per operation, true divisions) for the three ops calls of
the sigma-space schedulers of diffusion.py: ops.sigma_step (csrc/sigma.hip dp_sigma_step), ops.sigma_scale (dp_sigma_scale) and
ops.sigma_add_noise (dp_sigma_add_noise).  It also runs on device tensors (the GPU test compares the kernels with it there): every
scalar is a 0-d fp32 tensor on the data's device, so that no operation is rewritten into a multiplication by a reciprocal."""
import torch

SIGMA_COEF = ('s_noise', 'k', 'sig', 'c_out', 'c_den', 'dt', 'sigma_up')
SIGMA_EULER, SIGMA_ANCESTRAL, SIGMA_HEUN1, SIGMA_HEUN2 = range(4)
SIGMA_EPSILON, SIGMA_V, SIGMA_SAMPLE = range(3)
SIGMA_INSTANCES = tuple((m, p) for m in range(4) for p in range(3) if p != SIGMA_SAMPLE or m == SIGMA_EULER)
calls = []                                       # (op, mode, pred, churn, coef) of every call


def sigma_step(x, e, coef, mode, pred=SIGMA_EPSILON, noise=None, d1=None, saved=None, out=None, aux_out=None):
    assert (mode, pred) in SIGMA_INSTANCES, (mode, pred)
    assert x.dtype == torch.float32 and e.dtype == torch.float32 and e.numel() == x.numel()
    assert not set(coef) - set(SIGMA_COEF)
    if mode not in (SIGMA_EULER, SIGMA_ANCESTRAL):
        noise = None
    assert mode != SIGMA_ANCESTRAL or noise is not None
    assert mode != SIGMA_HEUN2 or (d1 is not None and saved is not None)
    assert all(t is None or (t.dtype == torch.float32 and t.numel() == x.numel()) for t in (noise, d1, saved))

    def s(name):
        return torch.tensor(float(coef[name]), dtype=torch.float32, device=x.device)
    calls.append(('step', mode, pred, mode == SIGMA_EULER and noise is not None, dict(coef)))
    xh = x
    if mode == SIGMA_EULER and noise is not None:
        xh = x + (noise * s('s_noise')) * s('k')
    if pred == SIGMA_EPSILON:
        x0 = xh - s('sig') * e
    elif pred == SIGMA_V:
        x0 = e * s('c_out') + xh / s('c_den')
    else:
        x0 = e.clone()
    d = (xh - x0) / s('sig')
    aux = d if mode == SIGMA_HEUN1 else x0
    if mode == SIGMA_HEUN2:
        d = (d1 + d) / torch.tensor(2.0, dtype=torch.float32, device=x.device)
        xh, aux = saved, None
    nxt = xh + d * s('dt')
    if mode == SIGMA_ANCESTRAL:
        nxt = nxt + noise * s('sigma_up')
    # the writes, after every read: out may be x (in HEUN2: saved)
    if aux is None:
        aux_out = None
    elif aux_out is None:
        aux_out = aux
    else:
        aux_out.copy_(aux.reshape(aux_out.shape))
    if out is None:
        return nxt, aux_out
    out.copy_(nxt.reshape(out.shape))
    return out, aux_out


def sigma_scale(x, c, out=None):
    assert x.dtype == torch.float32
    calls.append(('scale', None, None, False, dict(c=float(c))))
    y = x / torch.tensor(float(c), dtype=torch.float32, device=x.device)
    if out is None:
        return y
    out.copy_(y)
    return out


def sigma_add_noise(x0, noise, sigma, out=None):
    assert x0.dtype == torch.float32 and noise.dtype == torch.float32 and sigma.dtype == torch.float32
    assert sigma.numel() == x0.shape[0] and noise.numel() == x0.numel()
    calls.append(('add_noise', None, None, False, {}))
    B = x0.shape[0]
    y = (x0.reshape(B, -1) + noise.reshape(B, -1) * sigma.reshape(B, 1)).reshape(x0.shape)
    if out is None:
        return y
    out.copy_(y)
    return out
