"""What the tests of the sigma-space schedulers (EulerDiscreteScheduler, EulerAncestralDiscreteScheduler, HeunDiscreteScheduler) and
the fixture writer (tests/golden/make_golden_sigma.py) share: the case lists, the seeds the inputs are regenerated from, the toy model
of the CPU chains, the instantiation a call of a run takes and the fixture readers.  No reference code: the formulas are the ones
documented in include/dp_hip.h.  The bounds are those of tests/pndm_ref.py, imported, not retuned."""
import os

import numpy as np
import torch

import golden_common as gc
from pndm_ref import CHAIN_FACTOR, CHAIN_FLOOR, U, single_step_bound, toy_model      # noqa: F401

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

TABLES_FILE = 'sigma_tables.npz'                 # (a) timestep and sigma tables, init_noise_sigma
STEPS_FILE = 'sigma_steps.npz'                   # (b) single steps, (e) add_noise and scale_model_input cases
CHAINS_FILE = 'sigma_chains.npz'                 # (c) free-running chains of the reference UNet2DModel (TINY_CFG)
TOY_FILE = 'sigma_toy.npz'                       # (d) the same chains over toy_model

CLASSES = {'euler': 'EulerDiscreteScheduler', 'ancestral': 'EulerAncestralDiscreteScheduler', 'heun': 'HeunDiscreteScheduler'}
MODES = ('EULER', 'ANCESTRAL', 'HEUN1', 'HEUN2')                    # ops.SIGMA_* in order
PREDS = ('EPSILON', 'V', 'SAMPLE')
PRED_OF = {'epsilon': 0,'v_prediction': 1, 'sample': 2, 'original_sample': 2}
# every (mode, prediction type) the library instantiates: `sample` models on the Euler step only
INSTANCES = [(m, p) for m in range(4) for p in range(3) if p != 2 or m == 0]

# ---- (a) tables: (class, beta schedule, variant, n)
TABLE_NS = [1, 2, 3, 5, 7, 10, 50, 1000]
VARIANTS = {'euler': ('plain', 'log_linear', 'karras'), 'ancestral': ('plain',), 'heun': ('plain', 'karras')}
SCHEDULES = ('linear', 'scaled_linear', 'squaredcos_cap_v2')
TABLE_CASES = [(c, s, v, n) for c in CLASSES for s in SCHEDULES for v in VARIANTS[c] for n in TABLE_NS]


def table_name(case):
    return 'table:%s:%s:%s:%d' % case


def table_kwargs(case):
    c, sched, variant, _ = case
    kw = dict(beta_schedule=sched)
    if sched == 'scaled_linear':
        kw.update(beta_start=0.00085, beta_end=0.012)
    if variant == 'log_linear':
        kw['interpolation_type'] = 'log_linear'
    if variant == 'karras':
        kw['use_karras_sigmas'] = True
    return kw


def table_lengths(case):
    """(timesteps, sigmas) of a table: Heun doubles both, log_linear has one sigma more."""
    c, _, variant, n = case
    if c == 'heun':
        return max(2 * n - 1, 1), 2 * n
    return n, n + 1 + (variant == 'log_linear')


# ---- (b) single steps: a teacher-forced run per setting over the whole timestep list (call k is handed the seeded sample x_k and model
# output e_k, both regenerated from their seeds); the outputs of the listed calls are stored.  (name, class, scheduler kwargs, step kwargs)
STEP_SHAPE = (2, 3, 8, 8)
X_SEED0, E_SEED0, GEN_SEED = 700, 800, 91
X_SCALE = 5.0                                    # the sample lives at scale sigma
CHURN = dict(s_churn=3.0, s_tmin=0.05, s_tmax=100.0, s_noise=1.003)
SETTINGS = [
    ('euler', 'euler', dict(), dict()),
    ('euler_v', 'euler', dict(prediction_type='v_prediction'), dict()),
    ('euler_sample', 'euler', dict(prediction_type='sample'), dict()),
    ('euler_churn', 'euler', dict(), CHURN),
    ('euler_v_churn', 'euler', dict(prediction_type='v_prediction'), CHURN),
    ('euler_karras', 'euler', dict(use_karras_sigmas=True), dict()),
    ('ancestral', 'ancestral', dict(), dict()),
    ('ancestral_v', 'ancestral', dict(prediction_type='v_prediction', beta_schedule='scaled_linear', beta_start=0.00085, beta_end=0.012), dict()),
    ('heun', 'heun', dict(), dict()),
    ('heun_v', 'heun', dict(prediction_type='v_prediction'), dict()),
    ('heun_karras', 'heun', dict(use_karras_sigmas=True, beta_start=0.0001, beta_end=0.02), dict()),
]
STEP_NS = (10, 7)                                # integer timesteps (999 / 9 = 111) and fractional ones (999 / 6 = 166.5)


def n_calls(cls, n):
    return max(2 * n - 1, 1) if cls == 'heun' else n


def stored_calls(cls, n):
    """The calls whose outputs the fixture stores: the first two and the last; for Heun both states at either end."""
    last = n_calls(cls, n) - 1
    return sorted({0, 1, 2, last - 1, last}) if cls == 'heun' else sorted({0, 1, last})


def mode_of_call(cls, k):
    return {'euler': 0, 'ancestral': 1}.get(cls, 2 + k % 2)


STEP_RUNS = [(name, cls, kw, skw, n, stored_calls(cls, n)) for name, cls, kw, skw in SETTINGS for n in STEP_NS]


def run_name(run):
    return 'run:%s:%d' % (run[0], run[4])


def step_inputs(k):
    return (torch.from_numpy(gc.det_noise(STEP_SHAPE, X_SEED0 + k)) * X_SCALE, torch.from_numpy(gc.det_noise(STEP_SHAPE, E_SEED0 + k)))


def step_case_ids():
    return ['%s@%d' % (run_name(r), k) for r in STEP_RUNS for k in r[5]]


def stored_coverage():
    """{(mode, prediction type)} over the stored calls: which instantiations of dp_sigma_step they reach."""
    return {(mode_of_call(cls, k), PRED_OF[kw.get('prediction_type', 'epsilon')]) for _, cls, kw, _, _, at in STEP_RUNS for k in at}


COEF_NAMES = ('s_noise', 'k', 'sig', 'c_out', 'c_den', 'dt', 'sigma_up')     # the order of a stored `coefs` vector (unread ones 0)


# ---- (c), (d) chains: (name, class, scheduler kwargs, n, with a CPU generator)
CHAIN_B = 2
CHAIN_SEED = 73                                  # torch.Generator().manual_seed: x_T = randn_tensor(shape, generator)
NOISE_SEED = 74                                  # the ancestral chain's generator
MODEL_SEED = 5
CHAINS = [
    ('euler7', 'euler', dict(), 7, False),
    ('euler_karras10', 'euler', dict(use_karras_sigmas=True), 10, False),
    ('euler_v7', 'euler', dict(prediction_type='v_prediction'), 7, False),
    ('ancestral7', 'ancestral', dict(), 7, True),
    ('heun5', 'heun', dict(), 5, False),
]
TOY_SHAPE = (2, 3, 8, 8)

# ---- (e) add_noise: per-image table indices at n = 10; scale_model_input: table indices at n = 7
NOISE_CASES = [('euler', dict(), [0, 3]), ('euler', dict(use_karras_sigmas=True), [9, 9]), ('ancestral', dict(), [5, 1]), ('heun', dict(), [0, 18])]
SCALE_CASES = [('euler', dict(), 0), ('euler', dict(), 3), ('ancestral', dict(), 6), ('heun', dict(), 0), ('heun', dict(), 12)]


def load(name):
    g = np.load(os.path.join(GOLD, name))
    return {k: g[k] for k in g.files}


def random_coefs(seed):
    """The seven scalars of dp_sigma_step, of plausible size, seeded."""
    r = np.random.default_rng(seed)
    v = dict(s_noise=r.uniform(0.9, 1.1), k=r.uniform(0.5, 3.0), sig=r.uniform(0.5, 20.0), c_out=-r.uniform(0.3, 0.99), c_den=r.uniform(1.5, 300.0),
             dt=-r.uniform(0.1, 5.0), sigma_up=r.uniform(0.1, 3.0))
    return {k: float(np.float32(x)) for k, x in v.items()}
