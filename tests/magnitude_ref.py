"""The test suite's own fp64 restatement of the data-free magnitude criteria (ddpm_exp/torch_pruning/importance.py:18-126, 154-219),
written from the formulas, for tests/test_magnitude_family_{cpu,gpu}.py and tests/golden/make_golden_magnitude.py:
  member_rows   per member sum |w|^p (root: to the power 1 / p) per channel of its [R, C, T] view, in the member's index order;
  finish        the member reduction, the normaliser and LAMP in either scatter order;
  sample_positions  the channels of a group whose reference scores the fixture stores.
Everything is computed in float64 whatever the input's dtype."""
import numpy as np
import torch

REDUCTIONS = ['sum', 'mean', 'max', 'prod', 'first']
NORMALIZERS = [None, 'sum', 'standarization', 'mean', 'max', 'gaussian']
N_SAMPLES = 12


def sample_positions(n):
    """Up to N_SAMPLES channels spread over 0 .. n - 1, both ends included (all of them for a narrow group)."""
    return np.unique(np.round(np.linspace(0, n - 1, min(n, N_SAMPLES))).astype(np.int64))


def member_rows(members, p, root=False):
    """members: (w, R, C, T, dim, idxs) each -> float64 tensor [len(members), n0], n0 = the first list's length; a list of k * n0
    channels gives value j the sum over its entries j * k .. j * k + k - 1 (the `view` of importance.py:188-195)."""
    rows, n0 = [], len(members[0][5])
    for w, R, Cc, T, dim, idxs in members:
        w = w.detach().double().cpu().reshape(R, Cc, T)
        m = w.reshape(R, Cc * T) if dim == 0 else w.transpose(0, 1).reshape(Cc, R * T)
        v = m[torch.as_tensor(list(idxs), dtype=torch.long)].reshape(n0, -1).abs().pow(p).sum(1)
        rows.append(v.pow(1.0 / p) if root else v)
    return torch.stack(rows, dim=0)


def finish(rows, reduction, normalizer, lamp=None):
    """rows: float64 [members, n0]; lamp: None | 'vendored' | 'paper' -> float64 [n0]"""
    x = {'sum': lambda: rows.sum(0), 'mean': lambda: rows.sum(0) / rows.shape[0], 'max': lambda: rows.max(0)[0],
         'prod': lambda: rows.prod(0), 'first': lambda: rows[0]}[reduction]()
    n = x.numel()
    if normalizer == 'sum':
        x = x / x.sum()
    elif normalizer == 'standarization':
        x = (x - x.min()) / (x.max() - x.min() + 1e-8)
    elif normalizer == 'mean':
        x = x / (x.sum() / n)
    elif normalizer == 'max':
        x = x / x.max()
    elif normalizer == 'gaussian':
        mean = x.sum() / n
        var = ((x - mean) ** 2).sum() / (n - 1) if n > 1 else torch.tensor(float('nan'), dtype=torch.float64)
        x = (x - mean) / (var.sqrt() + 1e-8)
    else:
        assert normalizer is None
    if lamp is None:
        return x
    a = torch.argsort(x, descending=True, stable=True)            # ties: the lower channel first
    srt = x[a]
    q = srt / torch.cumsum(srt, 0)
    if lamp == 'vendored':                                        # importance.py:216-219: arange(n)[a] is a, so q is GATHERED at a
        return q[a]
    out = torch.empty_like(q)                                     # the paper: channel a[k] holds the k-th largest score's ratio
    out[a] = q
    return out
