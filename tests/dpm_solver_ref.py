"""What the DPMSolverMultistepScheduler tests and the fixture writer (tests/golden/make_golden_dpm_solver.py) share: the case lists,
the seeds the inputs are regenerated from, the smooth toy model of the CPU chains, the fp64 restatement of one kernel step and the
fixture readers.  No reference code: the formulas are the ones documented in include/dp_hip.h."""
import os

import numpy as np
import torch

import golden_common as gc

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
U = 2.0 ** -24                                   # unit roundoff of fp32

STEPS_FILE = 'dpm_solver_steps.npz'              # timestep tables + single steps
CHAINS_FILE = 'dpm_solver_chains.npz'            # free-running chains of the reference UNet2DModel (TINY_CFG)
TOY_FILE = 'dpm_solver_toy.npz'                  # the same chains over toy_model

# ---- timestep tables: (beta_schedule, lambda_min_clipped, use_karras_sigmas, n)
TABLE_NS = [5, 10, 14, 15, 20, 100, 1000]
CLIPPED = ('squaredcos_cap_v2', -5.1, False, 20)
TABLE_CASES = [('linear', None, karras, n) for karras in (False, True) for n in TABLE_NS] + [CLIPPED]


def table_name(case):
    sched, lam, karras, n = case
    return 'table:%s:%s:%d:%d' % (sched, 'inf' if lam is None else '%g' % lam, int(karras), n)


def table_kwargs(case):
    sched, lam, karras, n = case
    kw = dict(beta_schedule=sched, use_karras_sigmas=karras)
    if lam is not None:
        kw['lambda_min_clipped'] = lam
    return kw


# ---- single steps: a teacher-forced run of n steps per setting (step k is handed the seeded sample x_k and model output e_k,
# both regenerated from their seeds); the outputs of the listed steps are stored.  (algorithm, solver_type, solver_order, n, steps)
STEP_SHAPE = (2, 3, 8, 8)
X_SEED0, E_SEED0 = 300, 400
ALGOS = ('dpmsolver++', 'dpmsolver')
_AT_10 = {1: [0, 5, 9], 2: [0, 1, 5, 9], 3: [0, 2, 5, 8, 9]}       # first, warm-up, middle, lower_order_second, lower_order_final
STEP_RUNS = [(a, 'midpoint', 1, 10, _AT_10[1]) for a in ALGOS]
STEP_RUNS += [(a, s, so, 10, _AT_10[so]) for so in (2, 3) for a in ALGOS for s in ('midpoint', 'heun')]
STEP_RUNS += [(a, s, so, 20, [18, 19]) for so in (2, 3) for a, s in (('dpmsolver++', 'midpoint'), ('dpmsolver', 'heun'))]
# the order the reference's step takes at each of those steps (the fixture stores what it saw; the CPU test compares)
ORDERS_10 = {1: [1] * 10, 2: [1] + [2] * 8 + [1], 3: [1, 2] + [3] * 6 + [2, 1]}
ORDERS_20 = {2: [1] + [2] * 19, 3: [1, 2] + [3] * 18}


def run_name(run):
    a, s, so, n, _ = run
    return 'run:%s:%s:%d:%d' % (a, s, so, n)


def step_inputs(k):
    return (torch.from_numpy(gc.det_noise(STEP_SHAPE, X_SEED0 + k)), torch.from_numpy(gc.det_noise(STEP_SHAPE, E_SEED0 + k)))


def step_case_ids():
    return ['%s@%d' % (run_name(r), k) for r in STEP_RUNS for k in r[4]]


# ---- chains: (name, scheduler kwargs, n)
CHAIN_B = 2
CHAIN_SEED = 71                                  # torch.Generator().manual_seed: x_T = randn_tensor(shape, generator)
MODEL_SEED = 5
CHAINS = [
    ('pp_midpoint_o2', dict(algorithm_type='dpmsolver++', solver_type='midpoint', solver_order=2), 10),
    ('pp_heun_o3', dict(algorithm_type='dpmsolver++', solver_type='heun', solver_order=3), 14),
    ('dpm_midpoint_o2', dict(algorithm_type='dpmsolver', solver_type='midpoint', solver_order=2), 20),
    ('pp_o2_karras', dict(algorithm_type='dpmsolver++', solver_type='midpoint', solver_order=2, use_karras_sigmas=True), 10),
]
TOY_SHAPE = (2, 3, 8, 8)
CHAIN_FACTOR, CHAIN_FLOOR = 10.0, 1e-5           # a chain state: within 10 x the reference fp32 chain's own gap + 1e-5 of fp64


def load(name):
    g = np.load(os.path.join(GOLD, name))
    return {k: g[k] for k in g.files}


def toy_model(x, t):
    """A smooth eps(x, t) with cross-pixel and cross-channel coupling, in x's dtype (the CPU chains run it in fp32 and fp64).
    t: one timestep for the whole batch (int or 0-d tensor), as a scheduler loop passes it."""
    s = float(t) / 1000.0
    mix = torch.roll(x, shifts=(1, 1), dims=(1, 3)) * 0.25 + torch.roll(x, shifts=1, dims=2) * 0.125
    return torch.tanh(0.5 * x + mix) * (0.75 + 0.25 * s) + 0.125 * torch.sin(3.0 * s + x.mean(dim=(1, 2, 3), keepdim=True))


def single_step_bound(e_ref32, y64):
    """The bound of a fixture step: max(4 e_ref32, 4 * 2^-24 * max|y64|)."""
    return max(4.0 * float(e_ref32), 4.0 * U * float(np.abs(y64).max()))


def random_coefs(seed):
    """A full set of fp32 scalars of plausible size (every one read by some order / algorithm), seeded."""
    r = np.random.default_rng(seed)
    v = dict(sigma_s=r.uniform(0.2, 0.9), alpha_s=r.uniform(0.3, 0.95), kx=r.uniform(0.7, 1.0), k0=-r.uniform(0.05, 0.4),
             k1=r.uniform(-0.2, 0.2), k2=r.uniform(-0.05, 0.05), ir0=r.uniform(0.5, 2.0), ir1=r.uniform(0.5, 2.0),
             q=r.uniform(0.3, 0.7), iq=r.uniform(0.3, 1.0))
    return {k: float(np.float32(x)) for k, x in v.items()}
