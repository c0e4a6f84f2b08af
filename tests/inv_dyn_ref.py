"""Plain-torch restatement of the inverse-dynamics auxiliary (reference models/utils.py:84-109 and the loss lines of
dreamer.py:221-233), written the way tests/act_ref.py is: the dense activation is a parameter ("elu" / "relu"), run it on
float64 leaves under autograd, and every ReLU pre-activation is recorded in `pre` so that a test can assert
min |pre| >= PRE_MARGIN before it compares.  tests/test_inv_dyn_cpu.py ties it to the reference's own module and loss.

make_inv_params is the seeded parameter set of the module, shared by the golden generator (which loads it into the
reference's InverseDynamicsModel) and the GPU tests (which load it into repo_amd's): no weights are committed."""
import math
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

from tests.act_ref import PRE_MARGIN, _dense, min_abs_pre  # noqa: F401  (re-exported for the tests)

INV_SEED = 23   # the goldens' inverse-dynamics parameters (fx.make_params' modules use 7)


def make_inv_params(D, S, A, hidden, seed=INV_SEED):
    """OrderedDict(name -> float32 ndarray) in state_dict order (fc1..fc4, weight then bias); uniform(-k, k) with
    k = fan_in ** -0.5, a bias under the bound of its weight: the recipe of oracle/fixtures.py:make_params."""
    rs = np.random.RandomState(seed)
    shapes = [(hidden, 2 * D + S), (hidden, hidden), (hidden, hidden), (2 * A, hidden)]
    out = OrderedDict()
    for i, shp in enumerate(shapes, 1):
        k = 1.0 / np.sqrt(float(shp[1]))
        out[f"fc{i}.weight"] = rs.uniform(-k, k, size=shp).astype(np.float32)
        out[f"fc{i}.bias"] = rs.uniform(-k, k, size=shp[:1]).astype(np.float32)
    return out


def pack(beliefs, states):
    """(T, B, D), (T, B, S) -> ((T-1)*B, 2D+S): row t*B + b = [beliefs[t,b] | states[t,b] | beliefs[t+1,b]]."""
    return torch.cat((beliefs[:-1], states[:-1], beliefs[1:]), dim=2).flatten(0, 1)


def model(p, x, act, pre=None, min_std=0.1):
    """-> (mean, std, raw): fc1..fc3 with `act`, raw = fc4, mean = raw[:, :A], std = softplus(raw[:, A:]) + min_std."""
    h = x
    for i in (1, 2, 3):
        h = _dense(act, h, p[f"fc{i}.weight"], p[f"fc{i}.bias"], pre)
    raw = F.linear(h, p["fc4.weight"], p["fc4.bias"])
    A = raw.shape[1] // 2
    return raw[:, :A], F.softplus(raw[:, A:]) + min_std, raw


def nll_rows(mean, std, target):
    """Per-row -Independent(Normal(mean, std), 1).log_prob(target)."""
    z = (target - mean) / std
    return (0.5 * z * z + std.log() + 0.5 * math.log(2 * math.pi)).sum(1)


def masked_nll(raw, target, mask, min_std=0.1):
    """-> (sum of the per-row NLL over the rows with mask == 1, their count) from the head's raw output (N, 2A)."""
    A = raw.shape[1] // 2
    sel = mask.flatten() == 1
    rows = nll_rows(raw[:, :A], F.softplus(raw[:, A:]) + min_std, target)
    return (rows * sel).sum(), int(sel.sum())


def loss(p, beliefs, states, actions, nonterms, act, pre=None, min_std=0.1):
    """dreamer.py:221-233 on (T, B, .) latents and (T+1, B, .) actions / nonterms: the mean NLL over the selected rows
    (NaN when none is selected, like the reference)."""
    x = pack(beliefs.detach(), states.detach())
    _, _, raw = model(p, x, act, pre, min_std)
    total, count = masked_nll(raw, actions[1:-1].flatten(0, 1), nonterms[1:-1].flatten(), min_std)
    return total / count if count else total * float("nan")
