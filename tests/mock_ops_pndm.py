"""CPU stand-in (fp32 torch, the kernel's order of operations, one rounding per operation, true divisions) for the one ops call of
diffusion.PNDMScheduler: ops.pndm_step (csrc/pndm.hip dp_pndm_step).  It also runs on device tensors (the GPU test compares the
kernel with it there): every scalar, the small integers of the multistep formulas included, is a 0-d fp32 tensor on the data's
device, so that no operation is rewritten into a multiplication by a reciprocal."""
import torch

PNDM_COEF = ('sa', 'sb', 'sc', 'd', 'den', 'c6', 'c3', 'c24')
PNDM_PRK0, PNDM_PRK1, PNDM_PRK2, PNDM_PRK3, PNDM_PLMS1, PNDM_PLMS_AVG, PNDM_PLMS2, PNDM_PLMS3, PNDM_PLMS4 = range(9)
# mode -> (accumulator read, accumulator written, history entries read, hist_out written)
PNDM_MODES = {PNDM_PRK0: (False, True, 0, True), PNDM_PRK1: (True, True, 0, False), PNDM_PRK2: (True, True, 0, False),
              PNDM_PRK3: (True, False, 0, False), PNDM_PLMS1: (False, False, 0, True), PNDM_PLMS_AVG: (False, False, 1, False),
              PNDM_PLMS2: (False, False, 1, True), PNDM_PLMS3: (False, False, 2, True), PNDM_PLMS4: (False, False, 3, True)}
PNDM_FRACTIONS = dict(c6=1 / 6, c3=1 / 3, c24=1 / 24)
calls = []                                       # (mode, v_pred, out is x, hist_out is one of hist) of every pndm_step


def pndm_step(x, e, coef, mode, v_pred=False, acc=None, hist=(), out=None, hist_out=None):
    reads_acc, writes_acc, need, appends = PNDM_MODES[mode]
    assert x.dtype == torch.float32 and e.dtype == torch.float32 and e.numel() == x.numel()
    hist = list(hist)[:need]
    assert len(hist) == need and all(h is not None and h.dtype == torch.float32 and h.numel() == x.numel() for h in hist)
    assert not (reads_acc or writes_acc) or (acc is not None and acc.dtype == torch.float32 and acc.numel() == x.numel())
    assert not set(coef) - set(PNDM_COEF)

    def s(v):
        return torch.tensor(float(v), dtype=torch.float32, device=x.device)
    c = {k: s(v) for k, v in dict(PNDM_FRACTIONS, **coef).items()}
    calls.append((mode, bool(v_pred), out is x, appends and hist_out is not None and any(hist_out is h for h in hist)))
    m, new_acc = e, None
    if mode == PNDM_PRK0:
        new_acc = c['c6'] * e + s(0.0)
    elif mode in (PNDM_PRK1, PNDM_PRK2):
        new_acc = acc + c['c3'] * e
    elif mode == PNDM_PRK3:
        m = acc + c['c6'] * e
    elif mode == PNDM_PLMS_AVG:
        m = (e + hist[0]) / s(2)
    elif mode == PNDM_PLMS2:
        m = (s(3) * e - hist[0]) / s(2)
    elif mode == PNDM_PLMS3:
        m = ((s(23) * e - s(16) * hist[0]) + s(5) * hist[1]) / s(12)
    elif mode == PNDM_PLMS4:
        m = c['c24'] * (((s(55) * e - s(59) * hist[0]) + s(37) * hist[1]) - s(9) * hist[2])
    if v_pred:
        m = c['sa'] * m + c['sb'] * x
    nxt = c['sc'] * x - (c['d'] * m) / c['den']
    # the writes, after every read: out may be x, hist_out may be one of hist, acc is updated in place
    if new_acc is not None:
        acc.copy_(new_acc)
    if not appends:
        hist_out = None
    elif hist_out is None:
        hist_out = e.clone()
    else:
        hist_out.copy_(e)
    if out is None:
        return nxt, hist_out
    out.copy_(nxt)
    return out, hist_out
