"""What the tests of LMSDiscreteScheduler, KDPM2DiscreteScheduler and KDPM2AncestralDiscreteScheduler and the fixture writer
(tests/golden/make_golden_kdiff.py) share: the case lists, the seeds the inputs are regenerated from, the instantiation a call of a
run takes and the fixture readers.  No reference code: the formulas are the ones documented in include/dp_hip.h.  The inputs, the
toy model and the bounds are those of tests/sigma_ref.py and tests/pndm_ref.py, imported, not retuned."""
import numpy as np

from sigma_ref import (CHAIN_B, CHAIN_FACTOR, CHAIN_FLOOR, CHAIN_SEED, GEN_SEED, GOLD, MODEL_SEED, NOISE_SEED, SCHEDULES,       # noqa: F401
                       STEP_SHAPE, TOY_SHAPE, U, X_SCALE, load, single_step_bound, step_inputs, toy_model)

TABLES_FILE = 'kdiff_tables.npz'                 # (a) timestep and sigma tables, init_noise_sigma, LMS coefficients
STEPS_FILES = {'lms': 'kdiff_steps_lms.npz',     # (b) single steps of LMS
               'kdpm2': 'kdiff_steps_kdpm2.npz'}  # ... of the two KDPM2 classes, (e) add_noise and scale_model_input cases
CHAINS_FILE = 'kdiff_chains.npz'                 # (c) free-running chains of the reference UNet2DModel (TINY_CFG)
TOY_FILE = 'kdiff_toy.npz'                       # (d) the same chains over toy_model

CLASSES = {'lms': 'LMSDiscreteScheduler', 'kdpm2': 'KDPM2DiscreteScheduler', 'kdpm2a': 'KDPM2AncestralDiscreteScheduler'}
ALL_CLASSES = ('DDPMScheduler', 'DDIMScheduler', 'DPMSolverMultistepScheduler', 'UniPCMultistepScheduler', 'PNDMScheduler',
               'RePaintScheduler', 'EulerDiscreteScheduler', 'EulerAncestralDiscreteScheduler', 'HeunDiscreteScheduler') + tuple(CLASSES.values())
PREDS = ('EPSILON', 'V', 'SAMPLE')               # ops.KDIFF_* in order
PRED_OF = {'epsilon': 0, 'v_prediction': 1, 'sample': 2}
SHAPES = ('FIRST', 'SECOND', 'SECOND_NOISE')     # ops.KDPM2_* in order: what a call of dp_kdpm2_step is handed
# every instantiation of the two launchers: ('kdpm2', shape, pred) and ('lms', order, pred)
KDPM2_INSTANCES = [(s, p) for s in range(3) for p in range(2)]
LMS_INSTANCES = [(o, p) for o in range(1, 5) for p in range(3)]
INSTANCES = [('kdpm2',) + i for i in KDPM2_INSTANCES] + [('lms',) + i for i in LMS_INSTANCES]
KDPM2_COEF = ('sig', 'c_out', 'c_den', 'dt', 'sigma_up')                     # the order of a stored `coefs` vector (unread ones 0)
LMS_COEF = ('sig', 'c_out', 'c_den', 'c0', 'c1', 'c2', 'c3')

# ---- (a) tables: (class, beta schedule, variant, n)
TABLE_NS = [1, 2, 3, 5, 7, 10, 50, 1000]
VARIANTS = {'lms': ('plain', 'karras'), 'kdpm2': ('plain',), 'kdpm2a': ('plain',)}
TABLE_CASES = [(c, s, v, n) for c in CLASSES for s in SCHEDULES for v in VARIANTS[c] for n in TABLE_NS]
EXTRA_TABLES = {'lms': (), 'kdpm2': ('sigmas_interpol',), 'kdpm2a': ('sigmas_interpol', 'sigmas_up', 'sigmas_down')}
LMS_COEF_NS = (2, 5, 10)                         # the multistep coefficients of every index and order 1 .. 4 (default config)


def table_name(case):
    return 'table:%s:%s:%s:%d' % case


def table_kwargs(case):
    _, sched, variant, _ = case
    kw = dict(beta_schedule=sched)
    if sched == 'scaled_linear':
        kw.update(beta_start=0.00085, beta_end=0.012)
    if variant == 'karras':
        kw['use_karras_sigmas'] = True
    return kw


def table_lengths(case):
    """(timesteps, sigmas) of a table: the KDPM2 classes double both."""
    c, _, _, n = case
    return (n, n + 1) if c == 'lms' else (2 * n - 1, 2 * n + 2)


def lms_coef_name(n, index, order):
    return 'lms_coef:%d:%d:%d' % (n, index, order)


# ---- (b) single steps: a teacher-forced run per setting over the whole timestep list (call k is handed the seeded sample x_k and model
# output e_k of sigma_ref.step_inputs); the outputs of the listed calls are stored.  (name, class, scheduler kwargs, step kwargs)
SCALED = dict(beta_schedule='scaled_linear', beta_start=0.00085, beta_end=0.012)
SETTINGS = [
    ('lms', 'lms', dict(), dict()),
    ('lms_v', 'lms', dict(prediction_type='v_prediction'), dict()),
    ('lms_sample', 'lms', dict(prediction_type='sample'), dict()),
    ('lms_karras', 'lms', dict(use_karras_sigmas=True), dict()),
    ('lms_order2', 'lms', dict(), dict(order=2)),
    ('lms_v_order3', 'lms', dict(prediction_type='v_prediction', **SCALED), dict(order=3)),
    ('lms_sample_order3', 'lms', dict(prediction_type='sample'), dict(order=3)),
    ('lms_order3', 'lms', dict(), dict(order=3)),
    ('kdpm2', 'kdpm2', dict(), dict()),
    ('kdpm2_v', 'kdpm2', dict(prediction_type='v_prediction'), dict()),
    ('kdpm2_scaled', 'kdpm2', dict(**SCALED), dict()),
    ('kdpm2a', 'kdpm2a', dict(), dict()),
    ('kdpm2a_v', 'kdpm2a', dict(prediction_type='v_prediction', **SCALED), dict()),
]
STEP_NS = (10, 7)                                # integer base timesteps (999 / 9 = 111) and fractional ones (999 / 6 = 166.5)


def n_calls(cls, n):
    return n if cls == 'lms' else 2 * n - 1


def stored_calls(cls, n):
    """The calls whose outputs the fixture stores: LMS 0, 1, 3, 4 and the last (orders 1, 2 and 4 and the full ring; order 3 comes
    from the `order=3` settings); the KDPM2 classes the first three and the last two (both states at either end)."""
    last = n_calls(cls, n) - 1
    return sorted({0, 1, 3, 4, last}) if cls == 'lms' else sorted({0, 1, 2, last - 1, last})


def instance_of_call(cls, kw, skw, k):
    """The instantiation that call k of a teacher-forced run launches."""
    pred = PRED_OF[kw.get('prediction_type', 'epsilon')]
    if cls == 'lms':
        return ('lms', min(k + 1, skw.get('order', 4)), pred)
    return ('kdpm2', 0 if k % 2 == 0 else (2 if cls == 'kdpm2a' else 1), pred)


def branch(inst):
    """The launch site's kernel expression, as the launch ring records it."""
    kind, a, p = inst
    return '(%s_step_kernel<%d, DP_KDIFF_%s>)' % (kind, a, PREDS[p])


STEP_RUNS = [(name, cls, kw, skw, n, stored_calls(cls, n)) for name, cls, kw, skw in SETTINGS for n in STEP_NS]


def run_name(run):
    return 'run:%s:%d' % (run[0], run[4])


def step_case_ids():
    return ['%s@%d' % (run_name(r), k) for r in STEP_RUNS for k in r[5]]


def stored_coverage():
    """The instantiations of dp_kdpm2_step and dp_lms_step that the stored calls reach."""
    return {instance_of_call(cls, kw, skw, k) for _, cls, kw, skw, _, at in STEP_RUNS for k in at}


# ---- (c), (d) chains: (name, class, scheduler kwargs, n, with a CPU generator)
CHAINS = [
    ('lms7', 'lms', dict(), 7, False),
    ('lms_karras10', 'lms', dict(use_karras_sigmas=True), 10, False),
    ('kdpm2_5', 'kdpm2', dict(), 5, False),
    ('kdpm2_v5', 'kdpm2', dict(prediction_type='v_prediction'), 5, False),
    ('kdpm2a_5', 'kdpm2a', dict(), 5, True),
]

# ---- (e) add_noise: per-image timestep-table indices at n = 10, the state the scheduler is in; scale_model_input: table index at
# n = 7 and the state.  A KDPM2 class in second-order state looks an equal pair of timesteps up at its first entry.
NOISE_CASES = [('lms', dict(), [0, 3], True), ('lms', dict(use_karras_sigmas=True), [9, 9], True), ('kdpm2', dict(), [0, 18], True),
               ('kdpm2', dict(), [2, 5], False), ('kdpm2a', dict(), [4, 1], True), ('kdpm2a', dict(), [3, 8], False)]
SCALE_CASES = [('lms', dict(), 0, True), ('lms', dict(), 3, True), ('kdpm2', dict(), 0, True), ('kdpm2', dict(), 12, True),
               ('kdpm2', dict(), 5, False), ('kdpm2a', dict(), 6, True), ('kdpm2a', dict(), 1, False), ('kdpm2a', dict(), 7, False)]


def steps_file(cls):
    return STEPS_FILES['lms' if cls == 'lms' else 'kdpm2']


def load_steps():
    return dict(load(STEPS_FILES['lms']), **load(STEPS_FILES['kdpm2']))


def random_coefs(seed):
    """The scalars of dp_kdpm2_step and dp_lms_step together, of plausible size, seeded."""
    r = np.random.default_rng(seed)
    v = dict(sig=r.uniform(0.5, 20.0), c_out=-r.uniform(0.3, 0.99), c_den=r.uniform(1.5, 300.0), dt=-r.uniform(0.1, 5.0), sigma_up=r.uniform(0.1, 3.0),
             c0=-r.uniform(0.5, 4.0), c1=r.uniform(0.5, 4.0), c2=-r.uniform(0.1, 2.0), c3=r.uniform(0.05, 1.0))
    return {k: float(np.float32(x)) for k, x in v.items()}


def kdpm2_coefs(c):
    return {k: c[k] for k in KDPM2_COEF}


def lms_coefs(c, order):
    return {k: c[k] for k in LMS_COEF[:3 + order]}
