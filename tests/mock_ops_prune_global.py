"""tests/mock_ops.py plus CPU stand-ins of the two launchers of csrc/prune_global.hip:
  score_groups     dp_score_groups through mock_ops.group_score, group by group (same member order);
  select_smallest  dp_select_smallest the way the kernel does it: the order-preserving integer image of the floats (-0.0 counted as
                   +0.0), the k-th smallest key by an integer selection, `score <= threshold` per group; a NaN is refused.
`calls` records every call of the two, so a test can see which path the pruner took."""
import numpy as np
import torch

import mock_ops
from mock_ops import *            # noqa: F401,F403

globals().update({k: v for k, v in vars(mock_ops).items() if not k.startswith('__')})

calls = []


def score_groups(groups, idx_dev, scratch, scores):
    calls.append(('score_groups', len(groups), sum(len(m) for m, _ in groups)))
    off = 0
    for members, n0 in groups:
        mock_ops.group_score(members, n0, idx_dev, scratch, scores[off:off + n0])
        off += n0
    assert off == scores.numel()
    return scores


def float_keys(x):
    """uint32 keys with key(a) < key(b) <=> a < b for non-NaN fp32; both zeros map to the key of +0.0."""
    x = np.ascontiguousarray(x, dtype=np.float32).copy()
    x[x == 0] = 0.0
    u = x.view(np.uint32)
    neg = (u >> 31).astype(bool)
    return np.where(neg, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def key_to_float(k):
    k = np.uint32(k)
    u = (k & np.uint32(0x7fffffff)) if (k >> 31) else ~k
    return float(np.array([u], dtype=np.uint32).view(np.float32)[0])


def select_smallest(scores, offsets, k):
    x = scores.detach().cpu().numpy().astype(np.float32)
    n, G = x.size, len(offsets) - 1
    calls.append(('select_smallest', n, G, int(k)))
    if not (G >= 1 and offsets[0] == 0 and offsets[-1] == n and 1 <= k <= n and all(a < b for a, b in zip(offsets, offsets[1:]))):
        raise ValueError('select_smallest: offsets must cover the %d scores and 1 <= k <= n (k = %d)' % (n, k))
    if np.isnan(x).any():
        raise RuntimeError('select_smallest: the scores contain NaN (no k-th smallest exists)')
    keys = float_keys(x)
    thres = key_to_float(np.partition(keys, k - 1)[k - 1])
    return thres, [np.nonzero(x[a:b] <= np.float32(thres))[0].astype(np.int64) for a, b in zip(offsets, offsets[1:])]
