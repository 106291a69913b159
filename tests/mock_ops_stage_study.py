"""tests/mock_ops.py plus CPU stand-ins of what the stage study adds or uses beyond the sweep and the pruner:
  fold_sum                    dp_fold_sum (csrc/stage.hip): out = ((s0 + s1) + s2) + s3 in fp32, in that order, no source written; an
                              `out` that overlaps a source and k outside 1 .. 4 are refused as the launcher refuses them;
  denoise_step, image_to_u8   the sampler's two kernels, from tests/mock_ops_sampler.py.
`calls` records every fold_sum as (number of sources, elements)."""
import torch

import mock_ops
import mock_ops_sampler
from mock_ops import *            # noqa: F401,F403

globals().update({k: v for k, v in vars(mock_ops).items() if not k.startswith('__')})

DENOISE_GENERALIZED, DENOISE_DDPM = mock_ops_sampler.DENOISE_GENERALIZED, mock_ops_sampler.DENOISE_DDPM
denoise_step, image_to_u8 = mock_ops_sampler.denoise_step, mock_ops_sampler.image_to_u8
FOLD_SUM_MAX_SRCS = 4
calls = []


def _overlap(a, b):
    a0, b0 = a.data_ptr(), b.data_ptr()
    return a0 < b0 + 4 * b.numel() and b0 < a0 + 4 * a.numel()


def fold_sum(out, srcs):
    srcs = list(srcs)
    n = out.numel()
    for t in [out] + srcs:
        assert t.dtype == torch.float32 and t.is_contiguous() and t.numel() == n
    if n <= 0:
        return out
    if not 1 <= len(srcs) <= FOLD_SUM_MAX_SRCS or any(_overlap(out, s) for s in srcs):
        raise ValueError('fold_sum: 1 .. 4 sources, none of which `out` overlaps')
    calls.append((len(srcs), n))
    acc = srcs[0].clone()
    for s in srcs[1:]:
        acc = acc + s
    out.copy_(acc)
    return out
