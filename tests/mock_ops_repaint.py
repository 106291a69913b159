"""CPU stand-in (fp32 torch, the kernels' order of operations, one rounding per operation, a true division) for the two ops calls of
diffusion.RePaintScheduler: ops.repaint_step (csrc/repaint.hip dp_repaint_step) and ops.repaint_undo (dp_repaint_undo).  It also
runs on device tensors (the GPU test compares the kernels with it there): every scalar is a 0-d fp32 tensor on the data's device,
so that no operation is rewritten.  The mask is indexed exactly as the kernel indexes it, from the same three numbers."""
import math

import torch

REPAINT_COEF = ('sa', 'sb', 'sap', 's1', 'cd', 'sd')
REPAINT_UNDO_MAX = 8
calls = []                                       # ('step', clip, add_noise, full mask, x0 written, out is x) | ('undo', k, out is x)


def repaint_mask_geometry(shape, mask_shape):
    """(outer, stride, inner): element i of the data reads mask[(i // outer) * stride + i % inner]; None where the caller expands."""
    shape, mask_shape = tuple(shape), tuple(mask_shape)
    assert len(mask_shape) <= len(shape)
    ms = (1,) * (len(shape) - len(mask_shape)) + mask_shape
    assert all(m in (1, d) for m, d in zip(ms, shape)), (mask_shape, shape)
    n = math.prod(shape)
    if ms == shape or n == 0:
        return n, 0, n
    j = len(shape)
    while j > 1 and ms[j - 1] == shape[j - 1]:
        j -= 1
    if any(m != 1 for m in ms[1:j]):
        return None
    inner = math.prod(shape[j:])
    if ms[0] == shape[0] and shape[0] > 1:
        return n // shape[0], inner, inner
    return n, 0, inner


def mask_values(mask, geo, n):
    """The mask value of every data element, gathered by the kernel's index rule."""
    outer, stride, inner = geo
    i = torch.arange(n, device=mask.device)
    return mask.reshape(-1)[torch.div(i, outer, rounding_mode='floor') * stride + i % inner]


def repaint_step(x, e, noise, original, mask, coef, clip, add_noise, out=None, x0_out=None):
    n = x.numel()
    for t in (x, e, noise, original, mask):
        assert t.dtype == torch.float32 and t.is_contiguous() and t.device == x.device
    assert e.numel() == n and noise.numel() == n and original.numel() == n
    assert set(coef) == set(REPAINT_COEF), sorted(coef)
    geo = repaint_mask_geometry(x.shape, mask.shape)
    assert geo is not None, 'a mask of this shape is expanded by the caller'

    def s(v):
        return torch.tensor(float(v), dtype=torch.float32, device=x.device)
    c = {k: s(v) for k, v in coef.items()}
    calls.append(('step', bool(clip), bool(add_noise), geo[2] >= n, x0_out is not None, out is x))
    m = mask_values(mask, geo, n).reshape(x.shape)
    z, o = noise.reshape(x.shape), original.reshape(x.shape)
    ev = e.reshape(x.shape)
    x0 = (x - c['sb'] * ev) / c['sa']
    if clip:
        x0 = torch.clamp(x0, -1, 1)
    u = (c['sap'] * x0 + c['cd'] * ev) + (c['sd'] * z if add_noise else s(0.0))
    k = c['sap'] * o + c['s1'] * z
    nxt = m * k + (s(1.0) - m) * u
    # the writes, after every read: out may be x
    if x0_out is True:
        x0_out = x0
    elif x0_out is not None:
        x0_out.copy_(x0)
    if out is None:
        return nxt, x0_out
    out.copy_(nxt)
    return out, x0_out


def repaint_undo(x, noises, coefs, out=None):
    noises, coefs = list(noises), [(float(a), float(b)) for a, b in coefs]
    assert len(noises) == len(coefs) and len(noises) >= 1
    for t in [x] + noises:
        assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == x.numel() and t.device == x.device
    v = x
    for at in range(0, len(noises), REPAINT_UNDO_MAX):
        calls.append(('undo', len(noises[at:at + REPAINT_UNDO_MAX]), out is x))
    for z, (a, b) in zip(noises, coefs):
        a, b = (torch.tensor(q, dtype=torch.float32, device=x.device) for q in (a, b))
        v = a * v + b * z.reshape(x.shape)
    if out is None:
        return v
    out.copy_(v)
    return out
