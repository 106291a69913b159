"""CPU stand-in (fp32 torch, the kernel's order of operations, one rounding per operation, a true division) for the one ops call of
diffusion.DPMSolverMultistepScheduler: ops.dpm_solver_step (csrc/dpm_solver.hip dp_dpm_solver_step).  It also runs on device tensors
(the GPU test compares the kernel with it there): every scalar is a 0-d fp32 tensor on the data's device, so that no operation is
rewritten into a multiplication by a reciprocal."""
import torch

DPM_SOLVER_COEF = ('sigma_s', 'alpha_s', 'kx', 'k0', 'k1', 'k2', 'ir0', 'ir1', 'q', 'iq')
calls = []                                       # (order, data_pred, out is x, m0_out is m1 / m2) of every dpm_solver_step


def dpm_solver_step(x, e, coef, order=1, data_pred=True, m1=None, m2=None, out=None, m0_out=None):
    assert order in (1, 2, 3)
    assert x.dtype == torch.float32 and e.dtype == torch.float32 and e.numel() == x.numel()
    hist = [m1, m2][:order - 1]
    assert all(h is not None and h.dtype == torch.float32 and h.numel() == x.numel() for h in hist)
    assert not set(coef) - set(DPM_SOLVER_COEF)
    c = {k: torch.tensor(float(v), dtype=torch.float32, device=x.device) for k, v in coef.items()}
    calls.append((order, bool(data_pred), out is x, m0_out is not None and any(m0_out is h for h in hist)))
    if data_pred:
        m0 = (x - c['sigma_s'] * e) / c['alpha_s']
    else:
        m0 = e.clone()
    nxt = c['kx'] * x - c['k0'] * m0
    if order == 2:
        D1 = c['ir0'] * (m0 - m1)
        nxt = nxt - c['k1'] * D1
    elif order == 3:
        D10 = c['ir0'] * (m0 - m1)
        D11 = c['ir1'] * (m1 - m2)
        d = D10 - D11
        D1 = D10 + c['q'] * d
        D2 = c['iq'] * d
        nxt = (nxt - c['k1'] * D1) - c['k2'] * D2
    if m0_out is None:
        m0_out = m0
    else:
        m0_out.copy_(m0)                         # after every read of the history: m0_out may be m1 or m2
    if out is None:
        return nxt, m0_out
    out.copy_(nxt)
    return out, m0_out
