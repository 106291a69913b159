"""What the PNDMScheduler tests and the fixture writer (tests/golden/make_golden_pndm.py) share: the case lists, the seeds the inputs
are regenerated from, the smooth toy model of the CPU chains, the mode a step of a run takes and the fixture readers.  No reference
code: the formulas are the ones documented in include/dp_hip.h."""
import os

import numpy as np
import torch

import golden_common as gc
from dpm_solver_ref import toy_model                                # noqa: F401  (the same closed-form eps(x, t))

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
U = 2.0 ** -24                                   # unit roundoff of fp32

STEPS_FILE = 'pndm_steps.npz'                    # timestep tables + single steps
CHAINS_FILE = 'pndm_chains.npz'                  # free-running chains of the reference UNet2DModel (TINY_CFG)
TOY_FILE = 'pndm_toy.npz'                        # the same chains over toy_model

MODES = ('PRK0', 'PRK1', 'PRK2', 'PRK3', 'PLMS1', 'PLMS_AVG', 'PLMS2', 'PLMS3', 'PLMS4')        # ops.PNDM_* in order

# ---- timestep tables: (skip_prk_steps, steps_offset, n).  Without skip_prk_steps the reference raises below n = 4: the fixture
# records that (an empty table and `raises` = 1)
TABLE_NS = [1, 2, 3, 4, 5, 6, 10, 50, 1000]
TABLE_CASES = [(skip, off, n) for skip in (False, True) for off in (0, 1) for n in TABLE_NS]


def table_name(case):
    skip, off, n = case
    return 'table:%d:%d:%d' % (int(skip), off, n)


def table_kwargs(case):
    skip, off, _ = case
    return dict(skip_prk_steps=skip, steps_offset=off)


# ---- single steps: a teacher-forced run per setting over the whole timestep list (call k is handed the seeded sample x_k and model
# output e_k, both regenerated from their seeds); the outputs of the listed calls are stored.  (name, scheduler kwargs)
STEP_SHAPE = (2, 3, 8, 8)
X_SEED0, E_SEED0 = 500, 600
SETTINGS = [
    ('default', dict()),
    ('skip', dict(skip_prk_steps=True)),
    ('alpha_one', dict(set_alpha_to_one=True)),
    ('v', dict(prediction_type='v_prediction')),
    ('v_skip', dict(prediction_type='v_prediction', skip_prk_steps=True)),       # the multistep warm-up modes under v-prediction
    ('scaled_linear_off1', dict(beta_schedule='scaled_linear', beta_start=0.00085, beta_end=0.012, steps_offset=1)),
]
STEP_NS = (5, 10)


def n_calls(kw, n):
    """len(timesteps): 12 Runge-Kutta calls + n - 3 multistep ones, or n + 1 with skip_prk_steps (n > 1)."""
    return n + 1 if kw.get('skip_prk_steps') else 12 + n - 3


def stored_calls(kw, n):
    """The calls of a run whose outputs the fixture stores: the first Runge-Kutta round, the last one, the first multistep call and
    the last call (a negative previous timestep); with skip_prk_steps the five warm-up calls and the last."""
    last = n_calls(kw, n) - 1
    return sorted({0, 1, 2, 3, 4, last}) if kw.get('skip_prk_steps') else sorted({0, 1, 2, 3, 8, 9, 10, 11, 12, last})


def mode_of_call(kw, k):
    """The mode (index into MODES) that call k of a run takes, from the reference's counter logic."""
    if kw.get('skip_prk_steps'):
        return 4 + min(k, 4)
    return k % 4 if k < 12 else 8


STEP_RUNS = [(name, kw, n, stored_calls(kw, n)) for name, kw in SETTINGS for n in STEP_NS]


def run_name(run):
    return 'run:%s:%d' % (run[0], run[2])


def step_inputs(k):
    return (torch.from_numpy(gc.det_noise(STEP_SHAPE, X_SEED0 + k)), torch.from_numpy(gc.det_noise(STEP_SHAPE, E_SEED0 + k)))


def step_case_ids():
    return ['%s@%d' % (run_name(r), k) for r in STEP_RUNS for k in r[3]]


def stored_coverage():
    """{(mode name, v_prediction)} over the stored calls."""
    return {(MODES[mode_of_call(kw, k)], kw.get('prediction_type') == 'v_prediction') for _, kw, _, at in STEP_RUNS for k in at}


# ---- chains: (name, scheduler kwargs, n)
CHAIN_B = 2
CHAIN_SEED = 73                                  # torch.Generator().manual_seed: x_T = randn_tensor(shape, generator)
MODEL_SEED = 5
CHAINS = [
    ('prk10', dict(), 10),
    ('plms10', dict(skip_prk_steps=True), 10),
    ('plms10_v', dict(skip_prk_steps=True, prediction_type='v_prediction'), 10),
    ('prk5', dict(), 5),
]
TOY_SHAPE = (2, 3, 8, 8)
CHAIN_FACTOR, CHAIN_FLOOR = 10.0, 1e-5           # a chain state: within 10 x the reference fp32 chain's own gap + 1e-5 of fp64


def load(name):
    g = np.load(os.path.join(GOLD, name))
    return {k: g[k] for k in g.files}


def single_step_bound(e_ref32, y64):
    """The bound of a fixture step: max(4 e_ref32, 4 * 2^-24 * max|y64|)."""
    return max(4.0 * float(e_ref32), 4.0 * U * float(np.abs(y64).max()))


def random_coefs(seed):
    """The five scalars of formula (9) and the v-conversion, of plausible size, seeded (the fractions keep their defaults)."""
    r = np.random.default_rng(seed)
    v = dict(sa=r.uniform(0.3, 0.95), sb=r.uniform(0.2, 0.9), sc=r.uniform(1.0, 1.3), d=r.uniform(0.01, 0.3), den=r.uniform(0.2, 1.2))
    return {k: float(np.float32(x)) for k, x in v.items()}
