"""The inputs of the dense-activation tests (tests/test_dense_act_cpu.py, tests/test_dense_act_gpu.py): every case is a
pure function of its shape and a committed seed, built as float32 values held in float64 tensors (the kernels see
exactly the numbers the restatement does).

Seeds.  A ReLU pre-activation within fp32 rounding of zero has no agreed derivative (and an fp32 kernel may put it on
the other side of zero than the float64 restatement).  The seeds below were searched on the CPU with tests/act_ref.py
alone -- first seed >= 0 at which every dense pre-activation of the case's float64 restatement, under "relu", has
|pre| >= act_ref.PRE_MARGIN -- and test_dense_act_cpu.py re-asserts that property for every case; the kernels' results
were never consulted.  Larger cases have more pre-activations, so their inputs (the 33-row rollout:
two layers' parameters) are scaled up -- a wider pre-activation distribution puts fewer of them inside the margin; the
scale is part of the case."""
from collections import OrderedDict, namedtuple

import numpy as np
import torch

from oracle import fixtures as fx

E = 1024
Width = namedtuple("Width", "id D Hd S A")
DEFAULT = Width("default", 200, 200, 30, 6)
WIDEST_PAD = Width("widest-pad", 196, 196, 30, 3)   # tests/test_widths_gpu.py: the most padding columns the engines take


def f64(rs, *shape, scale=1.0):
    return torch.from_numpy((rs.standard_normal(shape) * scale).astype(np.float32)).double()


def params64(w, mod, seed=7):
    p = fx.make_params(w.A, seed, belief=w.D, state=w.S, hidden=w.Hd)[mod]
    return OrderedDict((k, torch.tensor(v, dtype=torch.float64, requires_grad=True)) for k, v in p.items())


# ----------------------------------------------------------------------------- MLP heads
MlpCase = namedtuple("MlpCase", "mod layers rows")
MLP_CASES = [MlpCase(m, L, r) for m, L in (("value_model", 4), ("actor_model", 5)) for r in (1, 17, 100)]
MLP_SEEDS = {("value_model", 1): 0, ("value_model", 17): 5, ("value_model", 100): 1,
             ("actor_model", 1): 0, ("actor_model", 17): 18, ("actor_model", 100): 81}
MLP_SCALE = {1: 1.0, 17: 4.0, 100: 16.0}   # by rows: 1.0-1.4 * 10^4 pre-activations at 17 rows, 6-8 * 10^4 at 100


def mlp_inputs(c, seed=None):
    rs = np.random.RandomState(1000 + (MLP_SEEDS[(c.mod, c.rows)] if seed is None else seed))
    p = params64(DEFAULT, c.mod)
    x = f64(rs, c.rows, DEFAULT.D + DEFAULT.S, scale=MLP_SCALE[c.rows]).requires_grad_(True)
    out_dim = p[f"fc{c.layers}.weight"].shape[0]
    return p, x, f64(rs, c.rows, out_dim)


# ----------------------------------------------------------------------------- observe scan
ObsCase = namedtuple("ObsCase", "width T B")
OBS_CASES = [ObsCase(DEFAULT, 3, 1), ObsCase(DEFAULT, 3, 5), ObsCase(DEFAULT, 3, 17), ObsCase(WIDEST_PAD, 3, 5)]
OBS_SEEDS = {("default", 1): 1, ("default", 5): 66, ("default", 17): 7762, ("widest-pad", 5): 2}
EMB_SCALE = 4.0   # the posterior hidden layer sees 1024 embedding columns: its pre-activations widen with them


def obs_inputs(c, seed=None):
    """-> (params, dict of inputs, list of 7 upstream gradients)."""
    w, T, B = c.width, c.T, c.B
    rs = np.random.RandomState(2000 + (OBS_SEEDS[(w.id, B)] if seed is None else seed))
    p = params64(w, "transition_model")
    x = dict(
        actions=f64(rs, T, B, w.A),
        nonterms=torch.from_numpy((rs.uniform(size=(T, B, 1)) > 0.2).astype(np.float64)),
        embeds=torch.relu(f64(rs, T, B, E, scale=EMB_SCALE)).requires_grad_(True),
        eps_prior=f64(rs, T, B, w.S), eps_post=f64(rs, T, B, w.S),
        b0=f64(rs, B, w.D, scale=0.3), s0=f64(rs, B, w.S),
    )
    shapes = [(T, B, w.D)] + [(T, B, w.S)] * 6
    ups = [f64(rs, *s, scale=0.1) for s in shapes]
    return p, x, ups


# ----------------------------------------------------------------------------- rollout
ImgCase = namedtuple("ImgCase", "Hm N")
# horizon H = 3: Hm = H - 1 steps.  N = 1 and 33 (one row; two 16-row tiles and a ragged third, one 32-row tile and a ragged
# second); N = 19 is the several-row case at the fixtures' OWN parameters (gain 1: the trained regime's gate statistics)
IMG_CASES = [ImgCase(2, 1), ImgCase(2, 33), ImgCase(2, 19)]
IMG_SEEDS = {1: 0, 33: 4, 19: 2112}
# 33 rows x 2 steps x 400 relu columns of standard deviation ~0.2: no seed in 32000 keeps all of them off zero.  The case
# therefore multiplies the parameters of the RSSM's two relu layers (fc_embed_state_action, fc_embed_belief_prior: weight
# and bias, i.e. their pre-activations) by a power of two -- exact in float32, so both sides still see the same numbers
IMG_GAIN = {1: 1.0, 33: 8.0, 19: 1.0}


def img_inputs(c, seed=None):
    w = DEFAULT
    rs = np.random.RandomState(3000 + (IMG_SEEDS[c.N] if seed is None else seed))
    rp = params64(w, "transition_model")
    ap = params64(w, "actor_model")
    for k in list(rp):
        if k.startswith(("fc_embed_state_action.", "fc_embed_belief_prior.")):
            rp[k] = (rp[k].detach() * IMG_GAIN[c.N]).requires_grad_(True)
    x = dict(b0=f64(rs, c.N, w.D, scale=0.3).requires_grad_(True),
             s0=f64(rs, c.N, w.S).requires_grad_(True),
             eps_act=f64(rs, c.Hm, c.N, w.A), eps_prior=f64(rs, c.Hm, c.N, w.S))
    ups = [f64(rs, c.Hm, c.N, n, scale=0.1) for n in (w.D, w.S, w.S, w.S)]
    return rp, ap, x, ups
