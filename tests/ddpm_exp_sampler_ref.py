"""What the ddpm_exp sampler tests share: the fp64 restatement of one update of dp_denoise_step (from the SAME fp32 scalars the
kernel is handed), the rounding bound that goes with it, the smooth toy model of the CPU chains (tests/golden/
make_golden_ddpm_exp_sampler.py runs the reference's loops over it too) and the fixture readers.  No reference code: the
formulas are the two documented in include/dp_hip.h."""
import os

import numpy as np
import torch

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
U = 2.0 ** -24                                   # unit roundoff of fp32

STEPS_FILE = 'ddpm_exp_sampler_steps.npz'
SEQ_FILE = 'ddpm_exp_sampler_seq.npz'
TOY_FILE = 'ddpm_exp_sampler_toy.npz'
CHAIN_FILES = {'uniform': 'ddpm_exp_sampler_chain_uniform.npz', 'quad': 'ddpm_exp_sampler_chain_quad.npz'}
SEQ_CASES = [(1000, 100, 'uniform'), (1000, 100, 'quad'), (1000, 7, 'uniform'), (1000, 1000, 'uniform'), (1000, 10, 'quad')]
STEP_PAIRS = [(990, 980), (999, 998), (10, 0), (0, -1), (1, 1)]
ETAS = [0.0, 0.5, 1.0]
CLAMP_PAIR, CLAMP_SCALE = (500, 490), 0.3        # ddpm_steps with part of the x0 values at the clamp
CHAIN_KINDS = [('generalized', 0.0), ('generalized', 1.0), ('ddpm_noisy', 0.0)]
CHAIN_N, CHAIN_B = 10, 2
TOY_SHAPE = (2, 3, 8, 8)
STEP_SHAPE = (2, 3, 16, 16)


def load(name):
    return np.load(os.path.join(GOLD, name))


def step_case_names():
    names = ['gen:%d:%d:%g' % (i, j, eta) for (i, j) in STEP_PAIRS for eta in ETAS]
    names += ['ddpm:%d:%d' % (i, j) for (i, j) in STEP_PAIRS]
    return names + ['ddpm_clamp:%d:%d' % CLAMP_PAIR]


def chain_name(kind, eta):
    return 'gen_eta%g' % eta if kind == 'generalized' else 'ddpm_noisy'


def toy_model(x, t):
    """A smooth eps(x, t) with cross-pixel and cross-channel coupling, in x's dtype (the CPU chains run it in fp32 and fp64).  t:
    one value per image, as the reference's loops pass it."""
    s = (t.to(x.dtype) / 1000.0).view(-1, 1, 1, 1)
    mix = torch.roll(x, shifts=(1, 1), dims=(1, 3)) * 0.25 + torch.roll(x, shifts=1, dims=2) * 0.125
    return torch.tanh(0.5 * x + mix) * (0.75 + 0.25 * s) + 0.125 * torch.sin(3.0 * s + x.mean(dim=(1, 2, 3), keepdim=True))


def denoise64(mode, x, e, z, coef):
    """(next, x0, M, A) in fp64 from the fp32 scalars `coef` the kernel takes.  M: per element, the sum of the magnitudes of the terms
    that make up `next` (with A, the un-cancelled magnitude of x0, in x0's place), which every rounding of the kernel is relative to."""
    x, e = x.double(), e.double()
    c = [float(np.float32(v)) for v in coef]
    if mode == 0:
        s1, s2, s3, c1, c2 = c
        x0 = (x - e * s1) / s2
        a = (x.abs() + e.abs() * s1) / s2
        nxt = s3 * x0 + c2 * e
        m = s3 * a + abs(c2) * e.abs()
        if z is not None:
            nxt = s3 * x0 + c1 * z.double() + c2 * e
            m = m + abs(c1) * z.double().abs()
        return nxt, x0, m, a
    r1, r2, k0, kx, d, sig = c
    a = r1 * x.abs() + r2 * e.abs()
    x0 = (r1 * x - r2 * e).clamp(-1, 1)
    nxt = (k0 * x0 + kx * x) / d
    m = (abs(k0) * a + abs(kx) * x.abs()) / d               # a, not min(a, 1): an unclamped x0 carries the error of its two terms
    if z is not None:
        nxt = nxt + sig * z.double()
        m = m + abs(sig) * z.double().abs()
    return nxt, x0, m, a


def rounding_bound(m):
    """The kernel rounds at most 8 times on the way to an element of `next` (mode 0: product, difference, quotient, three products,
    two sums; mode 1 has as many), each rounding at most U times a partial result whose magnitude the term sum M bounds (the
    clamp of mode 1 only shrinks an error).  To first order the error is therefore below 8 U M; x0 alone takes 3 roundings."""
    return 8 * U * float(m.max())


def x0_bound(a):
    return 3 * U * float(a.max())


def single_step_bound(e_ref32, y64):
    """The issue's bound for a fixture step: max(4 e_ref32, 4 * 2^-24 * max|y64|)."""
    return max(4.0 * float(e_ref32), 4.0 * U * float(np.abs(y64).max()))
