"""tests/mock_ops_ldm.py plus the CPU stand-in (fp32 torch, the kernel's order of operations) of ops.ema_update (csrc/ema.hip
dp_ema_update): LitEma's update alone, for the non-stepping calls of an accumulation window."""
import numpy as np

import mock_ops_ldm

# every name of the LDM mock, the underscore-prefixed helpers included (a star import would leave those out, and the package reaches
# some of them as `ops._name`)
globals().update({k: v for k, v in vars(mock_ops_ldm).items() if not k.startswith('__')})


def ema_update(shadow, p_, decay):
    shadow.sub_(float(np.float32(1) - np.float32(decay)) * (shadow - p_))
    return shadow
