"""What the UniPCMultistepScheduler tests and the fixture writer (tests/golden/make_golden_unipc.py) share: the case lists, the seeds
the inputs are regenerated from, the order / corrector decisions of a run restated in plain Python, the smooth toy model of the CPU
chains and the fixture readers.  No reference code: the formulas are the ones documented in include/dp_hip.h."""
import os

import numpy as np
import torch

import golden_common as gc
from dpm_solver_ref import toy_model                 # noqa: F401  (the same closed-form eps(x, t) as the DPM-Solver chains)

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
U = 2.0 ** -24                                   # unit roundoff of fp32

STEPS_FILE = 'unipc_steps.npz'                   # timestep tables + single steps
CHAINS_FILE = 'unipc_chains.npz'                 # free-running chains of the reference UNet2DModel (TINY_CFG)
TOY_FILE = 'unipc_toy.npz'                       # the same chains over toy_model

# ---- timestep tables: (beta_schedule, n); n == 1000 removes duplicates
TABLE_CASES = [('linear', n) for n in (1, 2, 5, 7, 10, 20, 100, 999, 1000)] + [('squaredcos_cap_v2', 10)]
SCHEDULES = ('linear', 'scaled_linear', 'squaredcos_cap_v2')       # the alpha_t / sigma_t / lambda_t tables stored (default betas)


def table_name(case):
    return 'table:%s:%d' % case


# ---- single steps: a teacher-forced run of n steps per setting (step k is handed the seeded sample x_k and model output e_k,
# both regenerated from their seeds); the state entering and leaving the listed steps is stored.
# (solver_type, predict_x0, solver_order, lower_order_final, disable_corrector, beta_schedule, n, steps)
STEP_SHAPE = (2, 3, 6, 6)
X_SEED0, E_SEED0 = 500, 600
_BOTH = [(st, x0) for st in ('bh1', 'bh2') for x0 in (True, False)]
_TWO = [('bh2', True), ('bh1', False)]
STEP_RUNS = [(st, x0, 3, True, (), 'linear', 8, (0, 1, 2, 4, 6, 7)) for st, x0 in _BOTH]     # (0,1) (1,2) (2,3) (3,3) (3,2) (2,1)
STEP_RUNS += [(st, x0, 2, True, (), 'linear', 6, (2, 5)) for st, x0 in _TWO]                 # (2,2) (2,1)
STEP_RUNS += [('bh2', True, 1, True, (), 'linear', 5, (0, 3)), ('bh1', False, 1, True, (), 'linear', 5, (3,))]    # (0,1) (1,1)
STEP_RUNS += [(st, x0, 3, False, (), 'linear', 6, (5,)) for st, x0 in _TWO]                  # (3,3) at the last step
STEP_RUNS += [(st, x0, 3, True, (0, 2, 3), 'linear', 8, (1, 2, 3)) for st, x0 in _TWO]       # (0,2) (2,3) (0,3)
# squaredcos_cap_v2 away from t = 999, where alpha_t is almost 0 and x0 = (x - sigma e) / alpha blows up for reasons of the schedule:
# with the corrector off for the first steps, last_sample restarts from the seeded sample of step 3 and the history from t <= 874
STEP_RUNS += [('bh2', True, 3, True, (0, 1, 2), 'squaredcos_cap_v2', 8, (5, 6))]             # (3,3) (3,2)
STEP_RUNS += [(st, x0, 3, True, (), 'linear', 2, (1,)) for st, x0 in _TWO]                   # (1,1) of a two-step run


def run_kwargs(run):
    st, x0, so, lof, dc, sched, _, _ = run
    return dict(solver_type=st, predict_x0=x0, solver_order=so, lower_order_final=lof, disable_corrector=list(dc), beta_schedule=sched)


def run_name(run):
    st, x0, so, lof, dc, sched, n, _ = run
    return 'run:%s:%s:%d:%s:%s:%s:%d' % (st, 'x0' if x0 else 'eps', so, 'lof' if lof else 'nolof', '-'.join(map(str, dc)) or 'none', sched, n)


def step_inputs(k):
    return (torch.from_numpy(gc.det_noise(STEP_SHAPE, X_SEED0 + k)), torch.from_numpy(gc.det_noise(STEP_SHAPE, E_SEED0 + k)))


def step_case_ids():
    return ['%s@%d' % (run_name(r), k) for r in STEP_RUNS for k in r[7]]


def decisions(solver_order, n, lower_order_final=True, disable_corrector=()):
    """[(pc, pp)] of an n-step run from a fresh set_timesteps (n distinct timesteps): the corrector's order (0: absent) and the
    predictor's, as scheduling_unipc_multistep.py:554-583 decides them."""
    out, lower, this_order, have_last = [], 0, None, False
    for i in range(n):
        pc = this_order if (i > 0 and i - 1 not in disable_corrector and have_last) else 0
        cap = min(solver_order, n - i) if lower_order_final else solver_order
        this_order = min(cap, lower + 1)
        have_last = True
        lower = min(lower + 1, solver_order)
        out.append((pc, this_order))
    return out


def reachable_pairs():
    """Every (pc, pp) a run of `step` from set_timesteps can produce, by enumeration of the decisions above."""
    seen = set()
    for so in (1, 2, 3):
        for n in range(1, 12):
            for lof in (True, False):
                for dc in ((), (0,), (1,), (0, 1), (0, 2, 3), tuple(range(12))):
                    seen.update(decisions(so, n, lof, dc))
    return seen


# ---- chains: (name, scheduler kwargs, n).  `low`: only orders <= 2 occur, so the toy chain is held to the reference's fp32 bits.
CHAIN_B = 2
CHAIN_SEED = 73                                  # torch.Generator().manual_seed: x_T = randn_tensor(shape, generator)
MODEL_SEED = 5
CHAINS = [
    ('bh2_x0_o2', dict(solver_type='bh2', predict_x0=True, solver_order=2), 8),
    ('bh1_x0_o3', dict(solver_type='bh1', predict_x0=True, solver_order=3), 10),
    ('bh2_eps_o3_nolof', dict(solver_type='bh2', predict_x0=False, solver_order=3, lower_order_final=False), 7),
    ('bh1_eps_o2_dc0', dict(solver_type='bh1', predict_x0=False, solver_order=2, disable_corrector=[0]), 6),
]
CHAIN_LOW = {name: kw['solver_order'] <= 2 for name, kw, _ in CHAINS}
TOY_SHAPE = (2, 3, 8, 8)
CHAIN_FACTOR, CHAIN_FLOOR = 10.0, 1e-5           # a chain state: within 10 x the reference fp32 chain's own gap + 1e-5 of fp64


def load(name):
    g = np.load(os.path.join(GOLD, name))
    return {k: g[k] for k in g.files}


def single_step_bound(e_ref32, y64):
    """The bound of a fixture step: max(4 e_ref32, 4 * 2^-24 * max|y64|)."""
    return max(4.0 * float(e_ref32), 4.0 * U * float(np.abs(y64).max()))


def place(s, g, key, device=None):
    """Put scheduler `s` (after set_timesteps) into the recorded state entering fixture step `key`; returns (sample, model_output, t)."""
    so = s.config.solver_order

    def dev(a):
        return torch.from_numpy(np.ascontiguousarray(a)).to(device) if device else torch.from_numpy(np.ascontiguousarray(a))
    have = int(g[key + ':in_n_hist'])
    hist = [dev(g[key + ':in_hist'][j]) for j in range(have)]
    s.model_outputs = [None] * (so - have) + hist
    s.timestep_list = [None if v < 0 else int(v) for v in g[key + ':in_timestep_list']]
    s.last_sample = dev(g[key + ':in_last_sample']) if int(g[key + ':in_has_last']) else None
    s.lower_order_nums = int(g[key + ':in_lower_order_nums'])
    s.this_order = int(g[key + ':in_this_order']) or None
    k = int(key.rsplit('@', 1)[1])
    x, e = step_inputs(k)
    return (x.to(device), e.to(device), int(g[key + ':t'])) if device else (x, e, int(g[key + ':t']))


MICRO = os.path.join(GOLD, 'ldm_pipeline_micro')


def _micro_cfg(rel):
    import json
    with open(os.path.join(MICRO, rel)) as f:
        return {k: v for k, v in json.load(f).items() if not k.startswith('_')}


def micro_scheduler_kwargs(**kw):
    """The beta schedule of the micro LDM pipeline directory's scheduler config, with the solver's own options added."""
    sc = _micro_cfg('scheduler/scheduler_config.json')
    return dict(kw, beta_schedule=sc['beta_schedule'], beta_start=sc['beta_start'], beta_end=sc['beta_end'])


def micro_pipe(scheduler, device=None):
    """The LDMPipeline of tests/golden/ldm_pipeline_micro (its configs; the weights are deterministic by name, as
    tests/test_vq_gpu.py builds them) around `scheduler`."""
    import vq_ref
    from helpers import pkg
    diffusion, vq, unet, syn = pkg('diffusion'), pkg('vq'), pkg('unet'), pkg('synthetic')
    vqm = vq.VQModel(**_micro_cfg('vqvae/config.json'))
    vqm.load_state_dict({k: v.float() for k, v in vq_ref.params(dict(vqm.config), 3).items()})
    u = unet.UNet2DModel(**_micro_cfg('unet/config.json'))
    syn.det_init_(u, 81)
    pipe = diffusion.LDMPipeline(vqvae=vqm.eval(), unet=u, scheduler=scheduler)
    return pipe.to(device) if device else pipe


def random_coefs(seed):
    """A full set of fp32 scalars of plausible size (every one read by some instantiation), seeded."""
    r = np.random.default_rng(seed)
    v = dict(sigma_s=r.uniform(0.2, 0.9), alpha_s=r.uniform(0.3, 0.95), c_cx=r.uniform(0.7, 1.0), c_c0=-r.uniform(0.05, 0.4),
             c_cB=-r.uniform(0.05, 0.4), c_rk1=-r.uniform(0.5, 2.0), c_rk2=-r.uniform(1.5, 3.0), c_rho1=r.uniform(-0.3, 0.3),
             c_rho2=r.uniform(-0.1, 0.1), c_rho_last=r.uniform(0.3, 0.6), p_cx=r.uniform(0.7, 1.0), p_c0=-r.uniform(0.05, 0.4),
             p_cB=-r.uniform(0.05, 0.4), p_rk1=-r.uniform(0.5, 2.0), p_rk2=-r.uniform(1.5, 3.0), p_rho1=r.uniform(0.3, 0.7),
             p_rho2=r.uniform(-0.2, 0.2))
    return {k: float(np.float32(x)) for k, x in v.items()}
