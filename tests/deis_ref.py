"""What the DEISMultistepScheduler / DPMSolverSinglestepScheduler tests and the fixture writer (tests/golden/make_golden_deis.py)
share: the case lists, the seeds the inputs are regenerated from, the launch-site naming of csrc/deis.hip and the fixture readers.
No reference code: the formulas are the ones documented in include/dp_hip.h."""
import os

import numpy as np
import torch

import golden_common as gc
from dpm_solver_ref import U, toy_model, single_step_bound, load, CHAIN_FACTOR, CHAIN_FLOOR, CHAIN_B, CHAIN_SEED, MODEL_SEED, TOY_SHAPE  # noqa: F401

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

STEPS_FILES = {'deis': 'deis_steps.npz', 'single': 'dpm_single_steps.npz'}     # tables + single steps, per class
CHAINS_FILES = ('deis_chains_a.npz', 'deis_chains_b.npz')     # free-running chains of the reference UNet2DModel (TINY_CFG)
TOY_FILE = 'deis_toy.npz'                        # the same chains over toy_model

PREDS = ('epsilon', 'sample', 'v_prediction')
ALGOS = ('dpmsolver++', 'dpmsolver')
STYPES = ('midpoint', 'heun')
CLASSES = {'deis': 'DEISMultistepScheduler', 'single': 'DPMSolverSinglestepScheduler'}

# ---- timestep tables: (beta_schedule, lambda_min_clipped, n); lambda_min_clipped is singlestep's alone
TABLE_NS = [1, 2, 3, 5, 9, 10, 14, 15, 20]
SCHEDULES = ('linear', 'squaredcos_cap_v2')
CLIPPED = ('squaredcos_cap_v2', -5.1, 20)
TABLE_CASES = {'deis': [(s, None, n) for s in SCHEDULES for n in TABLE_NS],
               'single': [(s, None, n) for s in SCHEDULES for n in TABLE_NS] + [CLIPPED]}
# singlestep's `orders` and the order each step actually took: (solver_order, lower_order_final, n)
ORDER_CASES = [(so, lof, n) for so in (1, 2, 3) for lof in (True, False) for n in TABLE_NS]


def table_name(cls, case):
    sched, lam, n = case
    return 'table:%s:%s:%s:%d' % (cls, sched, 'inf' if lam is None else '%g' % lam, n)


def table_kwargs(case):
    sched, lam, _ = case
    kw = dict(beta_schedule=sched)
    if lam is not None:
        kw['lambda_min_clipped'] = lam
    return kw


def orders_name(case):
    return 'orders:%d:%d:%d' % (case[0], int(case[1]), case[2])


# ---- single steps: a teacher-forced run of n steps per setting (step k is handed the seeded sample x_k and model output e_k,
# regenerated from their seeds -- for a thresholded run times the per-image fp32 scales the fixture stores); the outputs of the
# listed steps are stored.  (class, scheduler kwargs, n, steps)
STEP_SHAPE = (3, 2, 8, 8)
X_SEED0, E_SEED0 = 1300, 1400
MAX_VALUE = 2.0                                  # sample_max_value of every thresholded run
TARGETS = (0.6, 1.5, 3.0)                        # the quantile of |x0| the three images are scaled to: below 1, inside (1, 2), above 2
_THR = dict(thresholding=True, sample_max_value=MAX_VALUE)


def _runs():
    runs = []
    for pred in PREDS:
        for thr in (False, True):                # orders 1 2 3 3 3 3 3 3 2 1: first, warm-up, middle, lower_order_second, lower_order_final
            runs.append(('deis', dict(solver_order=3, prediction_type=pred, **(_THR if thr else {})), 10, [0, 1, 5, 8, 9]))
    runs.append(('deis', dict(solver_order=2), 10, [0, 1, 9]))
    runs.append(('deis', dict(solver_order=1), 10, [0, 9]))
    runs.append(('deis', dict(solver_order=3), 20, [18, 19]))
    for algo in ALGOS:
        for stype in STYPES:
            for pred in PREDS:                   # orders 1 2 3 1 2 3 1 2 3: the last step is third order (order_list, not orders)
                runs.append(('single', dict(solver_order=3, algorithm_type=algo, solver_type=stype, prediction_type=pred), 9, [0, 1, 2, 8]))
    for stype in STYPES:
        for pred in PREDS:
            runs.append(('single', dict(solver_order=3, algorithm_type='dpmsolver++', solver_type=stype, prediction_type=pred, **_THR), 9,
                         [0, 1, 2]))
    runs.append(('single', dict(solver_order=2), 10, [1, 9]))
    runs.append(('single', dict(solver_order=2, algorithm_type='dpmsolver', **_THR), 10, [1]))        # thresholding ignored under dpmsolver
    return runs


STEP_RUNS = _runs()


def run_name(run):
    cls, kw, n, _ = run
    return 'run:%s:%s:%d' % (cls, ','.join('%s=%s' % (k, kw[k]) for k in sorted(kw)), n)


def run_thresholds(run):
    """Whether the run's steps are thresholded: singlestep ignores the option under dpmsolver."""
    cls, kw, _, _ = run
    return bool(kw.get('thresholding')) and (cls == 'deis' or kw.get('algorithm_type', 'dpmsolver++') == 'dpmsolver++')


def base_inputs(k):
    return (torch.from_numpy(gc.det_noise(STEP_SHAPE, X_SEED0 + k)), torch.from_numpy(gc.det_noise(STEP_SHAPE, E_SEED0 + k)))


def step_inputs(k, scale=None):
    """(x_k, e_k); `scale`: the fixture's fp32 per-image scales of step k (one fp32 multiplication each), None: as drawn."""
    x, e = base_inputs(k)
    if scale is None:
        return x, e
    sc = torch.from_numpy(np.asarray(scale, np.float32)).reshape(-1, 1, 1, 1)
    return x * sc, e * sc


def step_case_ids():
    return ['%s@%d' % (run_name(r), k) for r in STEP_RUNS for k in r[3]]


def load_steps():
    """The two step files as one table (their keys carry the class)."""
    out = {}
    for f in STEPS_FILES.values():
        out.update(load(f))
    return out


# ---- the launch sites of csrc/deis.hip and what reaches them
def deis_site(order):
    return '(deis_step_kernel<%d>)' % order


def single_site(order, heun):
    return '(dpm_single_step_kernel<%d, %s>)' % (order, 'true' if order == 3 and heun else 'false')


def run_site(run, order):
    cls, kw, _, _ = run
    return deis_site(order) if cls == 'deis' else single_site(order, kw.get('solver_type', 'midpoint') == 'heun')


# ---- chains: (name, class, scheduler kwargs, n, file index)
CHAINS = [
    ('deis_o2_10', 'deis', dict(solver_order=2), 10, 0),
    ('deis_o2_20', 'deis', dict(solver_order=2), 20, 0),
    ('deis_o3_10', 'deis', dict(solver_order=3), 10, 0),
    ('deis_o3_20', 'deis', dict(solver_order=3), 20, 0),
    ('single_pp_midpoint_o2_10', 'single', dict(solver_order=2, algorithm_type='dpmsolver++', solver_type='midpoint'), 10, 1),
    ('single_dpm_heun_o3_9', 'single', dict(solver_order=3, algorithm_type='dpmsolver', solver_type='heun'), 9, 1),
    ('deis_o2_thr_10', 'deis', dict(solver_order=2, **_THR), 10, 1),
    ('single_pp_o2_thr_10', 'single', dict(solver_order=2, **_THR), 10, 1),
]


def random_coefs(names, seed):
    """A full set of fp32 scalars of plausible size, seeded: sa^2 + sb^2 = 1, everything else of order one."""
    r = np.random.default_rng(seed)
    sa = r.uniform(0.3, 0.95)
    v = {k: r.uniform(0.3, 1.2) * r.choice([-1.0, 1.0]) for k in names}
    v.update(sa=sa, sb=float(np.sqrt(1 - sa * sa)))
    if 'dr' in v:
        v['dr'] = v['r0'] - v['r1']
    return {k: float(np.float32(x)) for k, x in v.items()}
