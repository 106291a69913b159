"""CPU stand-in (fp32 torch, the kernel's order of operations, one rounding per operation, true divisions) for the one ops call of
diffusion.UniPCMultistepScheduler: ops.unipc_step (csrc/unipc.hip dp_unipc_step).  It also runs on device tensors (the GPU test
compares the kernel with it there): every scalar is a 0-d fp32 tensor on the data's device, so that no operation is rewritten into
a multiplication by a reciprocal.  It takes the kernel's aliases: every output is formed before any of them is stored."""
import torch

UNIPC_COEF = ('sigma_s', 'alpha_s', 'c_cx', 'c_c0', 'c_cB', 'c_rk1', 'c_rk2', 'c_rho1', 'c_rho2', 'c_rho_last',
              'p_cx', 'p_c0', 'p_cB', 'p_rk1', 'p_rk2', 'p_rho1', 'p_rho2')
calls = []                                       # (pc, pp, predict_x0, out is x_pred, x_c is x_last, m_new is a history buffer)


def unipc_step(e, x_pred, coef, pc=0, pp=1, predict_x0=True, x_last=None, hist=(), m_new=None, x_c=None, out=None):
    assert pc in (0, 1, 2, 3) and pp in (1, 2, 3)
    assert e.dtype == torch.float32 and x_pred.dtype == torch.float32 and e.numel() == x_pred.numel()
    nh = max(pc, pp - 1)
    hist = list(hist)[:nh]
    assert len(hist) == nh and all(h is not None and h.dtype == torch.float32 and h.numel() == e.numel() for h in hist)
    assert pc == 0 or (x_last is not None and x_last.dtype == torch.float32)
    assert not set(coef) - set(UNIPC_COEF)
    c = {k: torch.tensor(float(v), dtype=torch.float32, device=e.device) for k, v in coef.items()}
    calls.append((pc, pp, bool(predict_x0), out is x_pred, pc > 0 and x_c is x_last, m_new is not None and any(m_new is h for h in hist)))
    m0, m1, m2 = (hist + [None] * 3)[:3]
    if predict_x0:
        mn = (x_pred - c['sigma_s'] * e) / c['alpha_s']
    else:
        mn = e.clone()
    xs, xc = x_pred, None
    if pc:
        base = c['c_cx'] * x_last - c['c_c0'] * m0
        inner = c['c_rho_last'] * (mn - m0)
        if pc == 2:
            inner = c['c_rho1'] * ((m1 - m0) / c['c_rk1']) + inner
        elif pc == 3:
            s = c['c_rho1'] * ((m1 - m0) / c['c_rk1']) + c['c_rho2'] * ((m2 - m0) / c['c_rk2'])
            inner = s + inner
        xs = xc = base - c['c_cB'] * inner
    nxt = c['p_cx'] * xs - c['p_c0'] * mn
    if pp == 2:
        nxt = nxt - c['p_cB'] * (c['p_rho1'] * ((m0 - mn) / c['p_rk1']))
    elif pp == 3:
        s = c['p_rho1'] * ((m0 - mn) / c['p_rk1']) + c['p_rho2'] * ((m1 - mn) / c['p_rk2'])
        nxt = nxt - c['p_cB'] * s
    # every store after every read: m_new may be a history buffer, x_c may be x_last, out may be x_pred
    if m_new is None:
        m_new = mn
    else:
        m_new.copy_(mn)
    if pc:
        if x_c is None:
            x_c = xc
        else:
            x_c.copy_(xc)
    else:
        x_c = None
    if out is None:
        out = nxt
    else:
        out.copy_(nxt)
    return out, x_c, m_new
