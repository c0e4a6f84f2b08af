"""Plain-torch restatement of the state-vector modules (reference models/encoder.py:6-18 SymbolicEncoder,
models/decoder.py:6-25 SymbolicObservationModel) and of the observation-loss line for pixel_obs=False
(dreamer.py:262-267 with .sum(2)), written the way tests/act_ref.py is: the activation is a parameter ("elu" / "relu"), run
it on float64 leaves under autograd, and every ReLU pre-activation is recorded in `pre` so that a test can assert
min |pre| >= PRE_MARGIN before it compares.  tests/test_symbolic_cpu.py ties it to the reference's own modules and loss.

make_symbolic_params / make_obs are the seeded parameters and observation vectors shared by the golden generator (which
loads them into the reference's modules) and the GPU tests (which load them into repo_amd's): no weights are committed."""
import math
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

from tests.act_ref import PRE_MARGIN, _dense, min_abs_pre  # noqa: F401  (re-exported for the tests)

SYM_SEED = 29   # the goldens' symbolic encoder / decoder parameters (fx.make_params' modules use 7)
OBS_SEED = 31   # ... and their observation vectors (added to the update's batch seed)


def symbolic_shapes(obs, D, S, E):
    """{module: OrderedDict(name -> shape)} in state_dict order."""
    enc = [(E, obs), (E, E), (E, E)]
    dec = [(E, D + S), (E, E), (obs, E)]
    out = OrderedDict()
    for mod, shapes in (("encoder", enc), ("obs_model", dec)):
        d = OrderedDict()
        for i, shp in enumerate(shapes, 1):
            d[f"fc{i}.weight"] = shp
            d[f"fc{i}.bias"] = shp[:1]
        out[mod] = d
    return out


def make_symbolic_params(obs, D=200, S=30, E=1024, seed=SYM_SEED):
    """{"encoder": ..., "obs_model": ...}: OrderedDict(name -> float32 ndarray); uniform(-k, k) with k = fan_in ** -0.5, a
    bias under the bound of its weight: the recipe of oracle/fixtures.py:make_params."""
    rs = np.random.RandomState(seed)
    out = OrderedDict()
    for mod, shapes in symbolic_shapes(obs, D, S, E).items():
        d, k = OrderedDict(), 1.0
        for name, shp in shapes.items():
            if len(shp) > 1:
                k = 1.0 / np.sqrt(float(shp[1]))
            d[name] = rs.uniform(-k, k, size=shp).astype(np.float32)
        out[mod] = d
    return out


def make_obs(L, B, obs, seed):
    """State vectors (L, B, obs) float32, standard normal."""
    return np.random.RandomState(seed + OBS_SEED).standard_normal((L, B, obs)).astype(np.float32)


def chain(p, x, act, pre=None):
    """fc1 -> act -> fc2 -> act -> fc3: both modules (the decoder on cat([belief, state], 1))."""
    h = _dense(act, x, p["fc1.weight"], p["fc1.bias"], pre)
    h = _dense(act, h, p["fc2.weight"], p["fc2.bias"], pre)
    return F.linear(h, p["fc3.weight"], p["fc3.bias"])


def encoder(p, observation, act, pre=None):
    return chain(p, observation, act, pre)


def decoder(p, belief, state, act, pre=None):
    return chain(p, torch.cat([belief, state], dim=1), act, pre)


def nll_sum(recon, target):
    """sum over every element of 0.5 (recon - target)^2: what repo_linear_unit_nll's sums[0] holds."""
    return (0.5 * (recon - target) ** 2).sum()


def obs_loss(recon, target):
    """-Normal(recon, 1).log_prob(target).sum(2).mean((0, 1)) on (T, B, obs) tensors (dreamer.py:262-267)."""
    return (0.5 * (recon - target) ** 2 + 0.5 * math.log(2 * math.pi)).sum(2).mean((0, 1))
