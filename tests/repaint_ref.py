"""What the RePaintScheduler tests and the fixture writer (tests/golden/make_golden_repaint.py) share: the case lists, the seeds the
inputs are regenerated from, the smooth toy model of the CPU chains and the fixture readers.  No reference code: the formulas are
the ones documented in include/dp_hip.h."""
import os
from types import SimpleNamespace

import numpy as np
import torch

import golden_common as gc
from dpm_solver_ref import toy_model                                # noqa: F401  (the same closed-form eps(x, t))
from pndm_ref import CHAIN_FACTOR, CHAIN_FLOOR, MODEL_SEED, U, single_step_bound      # noqa: F401  (the same bounds, not retuned)

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')

TABLES_FILE = 'repaint_tables.npz'               # timestep tables
STEPS_FILE = 'repaint_steps.npz'                 # single steps, undo steps, preprocessor outputs
TOY_FILE = 'repaint_toy.npz'                     # free-running chains of the reference pipeline over toy_model
CHAIN_FILE = 'repaint_chain_%s.npz'              # ... over the reference UNet2DModel (TINY_CFG), one file per chain

# ---- timestep tables: (num_inference_steps, jump_length, jump_n_sample); 2000 is clamped to num_train_timesteps
TABLE_CASES = [(10, 3, 2), (8, 2, 3), (6, 1, 2), (4, 10, 10), (250, 10, 10), (1000, 10, 10), (2000, 10, 10), (1, 1, 1)]
TABLE_LENGTHS = {(10, 3, 2): 28, (8, 2, 3): 32, (6, 1, 2): 16, (4, 10, 10): 4, (250, 10, 10): 4570, (1000, 10, 10): 18820}


def table_name(case):
    return 'table:%d:%d:%d' % case


# ---- single steps at STEP_SHAPE: one call of `step` per case on seeded x, e, original image and 0 / 1 mask, the noise drawn from a
# seeded CPU generator (torch.Generator().manual_seed(NOISE_SEED0 + index)).  (name, scheduler kwargs, num_inference_steps, eta set
# after construction as the pipeline sets it, timestep, mask form)
STEP_SHAPE = (2, 3, 5, 7)
X_SEED0, E_SEED0, O_SEED0, M_SEED0, NOISE_SEED0 = 1500, 1600, 1700, 1800, 1900
MASK_FORMS = ('full', 'B1HW', '11HW', '1CHW', '1HW')
ETAS = (0.0, 0.5, 1.0)
STEP_T = (('last', 900), ('middle', 500), ('zero', 0))             # of the 10-step table: n = 100
STEP_CASES = [('eta%g:%s:%s:%s' % (eta, 'clip' if clip else 'noclip', tn, form), dict(clip_sample=clip), 10, eta, t, form)
              for eta in ETAS for clip in (True, False) for tn, t in STEP_T for form in MASK_FORMS]
# further schedules and strides, on the full mask
STEP_CASES += [('%s:%s' % (name, tn), kw, n, 0.5, t, 'full')
               for name, kw, n, tt in (('sigmoid', dict(beta_schedule='sigmoid'), 10, STEP_T),
                                       ('cosine', dict(beta_schedule='squaredcos_cap_v2'), 10, STEP_T),
                                       ('scaled_linear', dict(beta_schedule='scaled_linear', beta_start=0.00085, beta_end=0.012), 10, STEP_T),
                                       ('n4', dict(), 250, (('last', 996), ('middle', 500), ('zero', 0))),
                                       ('n1', dict(), 1000, (('last', 999), ('middle', 500), ('zero', 0))))
               for tn, t in tt]


def mask_shape(form, shape=STEP_SHAPE):
    B, C, H, W = shape
    return {'full': (B, C, H, W), 'B1HW': (B, 1, H, W), '11HW': (1, 1, H, W), '1CHW': (1, C, H, W), '1HW': (1, H, W)}[form]


def step_inputs(k, form, shape=STEP_SHAPE):
    """x, e, the original image and the 0 / 1 mask of case k, from their seeds."""
    x, e = (torch.from_numpy(gc.det_noise(shape, s + k)) for s in (X_SEED0, E_SEED0))
    o = torch.from_numpy(gc.det_noise(shape, O_SEED0 + k)).mul(0.5).clamp(-1, 1)
    m = torch.from_numpy((np.random.default_rng(M_SEED0 + k).integers(0, 2, mask_shape(form, shape)) > 0).astype(np.float32))
    return x, e, o, m


def noise_generator(k):
    return torch.Generator().manual_seed(NOISE_SEED0 + k)


def signed_zero_case():
    """x, e, o, m, z and scalars (cd = -1: not a scheduler's, chosen for the signs) at which sap * x0 + cd * e is -0 in element 0 and
    +0 in element 1 while m * k is -0: the output's sign is the sign of the unknown part after its `+ 0` (or `+ sd * z`)."""
    t = lambda *v: torch.tensor(v, dtype=torch.float32).reshape(1, 1, 1, 2)        # noqa: E731
    return t(-0.0, 0.0), t(0.0, 0.0), t(-1.0, -1.0), t(0.0, 0.0), t(0.0, 0.0), dict(sa=1.0, sb=1.0, sap=1.0, s1=0.0, cd=-1.0, sd=0.0)


# ---- undo steps: (num_inference_steps, timestep): n = 1000 // num_inference_steps re-noising steps from `timestep`
UNDO_CASES = [(1000, 500), (250, 496), (111, 450), (10, 300)]
UNDO_N = (1, 4, 9, 100)
UNDO_SEED0 = 2100


def undo_name(case):
    return 'undo:%d:%d' % case


def undo_input(k):
    return torch.from_numpy(gc.det_noise(STEP_SHAPE, UNDO_SEED0 + k))


# ---- chains of the pipeline: (name, (num_inference_steps, jump_length, jump_n_sample), eta)
CHAINS = [('j3x2_eta0', (10, 3, 2), 0.0), ('j3x2_eta1', (10, 3, 2), 1.0), ('j2x3_eta05', (8, 2, 3), 0.5)]
CHAIN_B = 2
CHAIN_SEED = 91                                  # torch.Generator().manual_seed: every draw of the pipeline call
IMAGE_SEED = 2300
TOY_SHAPE = (2, 3, 8, 8)


def chain_inputs(shape):
    """The image to inpaint (seeded, in [-1, 1]) and the half-plane mask, [1, H, W] as a PIL mask becomes: the left half is known."""
    B, C, H, W = shape
    image = torch.from_numpy(gc.det_noise(shape, IMAGE_SEED)).mul(0.5).clamp(-1, 1)
    mask = torch.zeros(1, H, W)
    mask[:, :, :W // 2] = 1.0
    return image, mask


def n_model_calls(ts):
    """The entries of a timestep list that lie below the one before them: a UNet call and a `step`; the others are `undo_step`s."""
    return sum(1 for prev, t in zip([ts[0] + 1] + list(ts[:-1]), ts) if t < prev)


class ToyUNet:
    """toy_model behind the call surface a pipeline uses (a foreign model object: no sampling_forward)."""
    dtype = torch.float32
    device = torch.device('cpu')

    def __call__(self, sample, t):
        return SimpleNamespace(sample=toy_model(sample, t))


# ---- preprocessors: one 37 x 45 RGB image and one 70 x 70 mask from seeded arrays
PRE_SEED = 2500


def pre_inputs():
    from PIL import Image
    r = np.random.default_rng(PRE_SEED)
    image = Image.fromarray(r.integers(0, 256, (45, 37, 3), dtype=np.uint8), 'RGB')            # size (37, 45)
    mask = Image.fromarray((r.integers(0, 256, (70, 70), dtype=np.uint8)), 'L')
    return image, mask


def load(name):
    g = np.load(os.path.join(GOLD, name))
    return {k: g[k] for k in g.files}
