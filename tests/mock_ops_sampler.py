"""CPU stand-ins (fp32 torch, the kernels' order of operations, one rounding per operation) for the two ops calls of
diff-pruning_amd/ddpm_exp_sampler.py: ops.denoise_step (csrc/sampler.hip dp_denoise_step) and ops.image_to_u8 (dp_image_to_u8)."""
import torch

DENOISE_GENERALIZED, DENOISE_DDPM = 0, 1
calls = []                                       # (mode, has_z, has_x0_out, in_place) of every denoise_step


def _s(v):
    return torch.tensor(float(v), dtype=torch.float32)


def denoise_step(x, eps, mode, coef, z=None, out=None, x0_out=None):
    assert x.dtype == torch.float32 and eps.dtype == torch.float32 and (z is None or z.dtype == torch.float32)
    c = [_s(v) for v in coef]
    assert len(c) == (5 if mode == DENOISE_GENERALIZED else 6)
    calls.append((mode, z is not None, x0_out is not None, out is x))
    if mode == DENOISE_GENERALIZED:
        s1, s2, s3, c1, c2 = c
        x0 = (x - eps * s1) / s2
        nxt = s3 * x0
        if z is not None:
            nxt = nxt + c1 * z
        nxt = nxt + c2 * eps
    else:
        r1, r2, k0, kx, d, sig = c
        x0 = torch.clamp(r1 * x - r2 * eps, -1, 1)
        nxt = (k0 * x0 + kx * x) / d
        if z is not None:
            nxt = nxt + sig * z
    if x0_out is not None:
        x0_out.copy_(x0)
    if out is None:
        return nxt
    out.copy_(nxt)
    return out


def image_to_u8(x, rescaled=True, out=None):
    v = (x + 1.0) / 2.0 if rescaled else x
    u8 = torch.clamp(v, 0.0, 1.0).mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    if out is None:
        return u8
    out.copy_(u8)
    return out
