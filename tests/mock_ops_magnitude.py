"""tests/mock_ops_prune_global.py plus torch stand-ins (fp32, on the host) of the two launchers of csrc/magnitude.hip:
  magnitude_rows    dp_magnitude_rows: per member sum |w|^p (root: to the power 1 / p) per channel, one row per member;
  magnitude_finish  dp_magnitude_finish: member reduction in member order, normaliser with IEEE divisions, LAMP (descending sort with
                    ties by ascending channel, torch.cumsum's sequential scan, vendored or paper scatter); a group wider than
                    MAGNITUDE_MAX_WIDTH is refused as the launcher refuses it.
`calls` (shared with mock_ops_prune_global) records every call, so a test can see which path the criterion took."""
import torch

import mock_ops_prune_global as base
from mock_ops_prune_global import *            # noqa: F401,F403

globals().update({k: v for k, v in vars(base).items() if not k.startswith('__')})

MAGNITUDE_MAX_WIDTH = 4096
MAGNITUDE_REDUCTIONS = {'sum': 0, 'mean': 1, 'max': 2, 'prod': 3, 'first': 4}
MAGNITUDE_NORMALIZERS = {None: 0, 'sum': 1, 'standarization': 2, 'mean': 3, 'max': 4, 'gaussian': 5}
MAGNITUDE_LAMP = {None: 0, 'vendored': 1, 'paper': 2}


def magnitude_rows(members, idx_dev, p, root, rows):
    calls.append(('magnitude_rows', len(members)))            # noqa: F405
    assert p > 0 and rows.dtype == torch.float32
    for m in members:
        R, Cc, T, dim, n0 = m['R'], m['C'], m['T'], m['dim'], m['n0']
        w = m['w']
        assert w.dtype == torch.float32 and w.is_contiguous() and w.numel() == R * Cc * T
        w = w.reshape(R, Cc, T)
        mat = w.reshape(R, Cc * T) if dim == 0 else w.transpose(0, 1).reshape(Cc, R * T)
        fold = m.get('fold', 1)
        if m['idx_off'] >= 0:
            ix = idx_dev[m['idx_off']:m['idx_off'] + n0 * fold]
            assert ix.numel() == n0 * fold and int(ix.min()) >= 0 and int(ix.max()) < mat.shape[0]
            mat = mat[ix].reshape(n0, -1)                       # fold > 1: `fold` consecutive channels of the list make one value
        else:
            assert n0 <= mat.shape[0] and fold == 1
            mat = mat[:n0]
        a = mat.abs()
        v = (a if p == 1 else a * a if p == 2 else a.pow(p)).sum(1)
        if root:
            v = v if p == 1 else v.sqrt() if p == 2 else v.pow(1.0 / p)
        assert 0 <= m['row_off'] and m['row_off'] + n0 <= rows.numel()
        rows[m['row_off']:m['row_off'] + n0] = v
    return rows


def magnitude_finish(groups, rows, reduction, normalizer, lamp, scores):
    calls.append(('magnitude_finish', len(groups), reduction, normalizer, lamp))            # noqa: F405
    red, norm, lamp = MAGNITUDE_REDUCTIONS[reduction], MAGNITUDE_NORMALIZERS[normalizer], MAGNITUDE_LAMP[lamp]
    if any(n0 > MAGNITUDE_MAX_WIDTH for _, n0, _ in groups):
        raise RuntimeError('dp_magnitude_finish failed with hipError 1')
    off = 0
    for row_off, n0, M in groups:
        r = rows[row_off:row_off + M * n0].view(M, n0)
        x = r[0].clone()
        for i in range(1, M if red != 4 else 1):
            x = torch.maximum(x, r[i]) if red == 2 else x * r[i] if red == 3 else x + r[i]
        if red == 1:
            x = x / float(M)
        if norm == 1:
            x = x / x.sum()
        elif norm == 2:
            x = (x - x.min()) / ((x.max() - x.min()) + 1e-8)
        elif norm == 3:
            x = x / (x.sum() / float(n0))
        elif norm == 4:
            x = x / x.max()
        elif norm == 5:
            mean = x.sum() / float(n0)
            dm = (x - mean).abs().max()                                  # squares of (x - mean) / dm: no overflow, as the kernel
            scale = dm if float(dm) > 0 else torch.tensor(1.0)
            var = (((x - mean) / scale) ** 2).sum() / torch.tensor(float(n0 - 1))
            x = (x - mean) / (scale * var.sqrt() + 1e-8)
        if lamp:
            a = torch.argsort(x, descending=True, stable=True)
            srt = x[a]
            q = srt / torch.cumsum(srt, 0)
            if lamp == 1:
                x = q[a]
            else:
                x = torch.empty_like(q)
                x[a] = q
        scores[off:off + n0] = x
        off += n0
    assert off == scores.numel()
    return scores
