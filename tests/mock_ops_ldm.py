"""tests/mock_ops.py plus CPU stand-ins (fp32 torch, the kernels' order of operations) for the ops of the LDM finetune step:
adamw_ema (csrc/optim.hip dp_adamw_ema), embedding_bwd (dp_embedding_bwd) and the host-side id check.  The context-gradient path
of LdmEngine.backward needs none: it is linear_dgrad / conv_dgrad with `out=` / `accumulate=`, which mock_ops already has."""
import importlib

import numpy as np
import torch

import mock_ops
from mock_ops import *            # noqa: F401,F403

globals().update({k: v for k, v in vars(mock_ops).items() if not k.startswith('__')})

_ops = importlib.import_module('diff-pruning_amd.ops')
check_class_ids = _ops.check_class_ids          # pure host code: the product's own
adamw_scalars = _ops.adamw_scalars
EMBEDDING_BWD_MAX_ROWS = _ops.EMBEDDING_BWD_MAX_ROWS


def adamw_ema(p_, g, m, v, ema, lr, b1, b2, eps, weight_decay, step, ema_decay=0.0, coef=None):
    s = {k: float(np.float32(x)) for k, x in adamw_scalars(lr, b1, b2, weight_decay, step).items()}
    if coef is not None:
        g = g * coef
    p_.mul_(s['p_scale'])
    m.add_((g - m) * s['one_minus_b1'])
    v.mul_(s['b2']).add_(s['one_minus_b2'] * g * g)
    denom = v.sqrt() / s['sqrt_bc2'] + float(np.float32(eps))
    p_.sub_(s['step_size'] * (m / denom))
    if ema is not None:
        ema.sub_(float(np.float32(1) - np.float32(ema_decay)) * (ema - p_))


def embedding_bwd(ids, dctx, dW):
    if dctx.shape[0] > EMBEDDING_BWD_MAX_ROWS:
        raise ValueError('embedding_bwd: at most %d rows per call' % EMBEDDING_BWD_MAX_ROWS)
    for b in range(dctx.shape[0]):                      # ascending b, like the kernel
        dW[int(ids[b])] += dctx[b]
    return dW
