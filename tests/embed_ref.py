"""Seeded parameters at any embedding_size, shared by the golden generator (tests/golden/gen_golden_embed.py, which loads
them into the reference's modules) and the tests: no weights are committed.

make_params is oracle/fixtures.py's make_params with `embed` a free argument: the shapes are fx.param_shapes(..., embed=E)
with the reference's optional encoder layer `fc` = Linear(1024, E) (models/encoder.py:30-32) inserted behind conv4.bias --
in front of film.* on the conditioned encoder -- when the frames are 64 x 64 and E != 1024, and the values are drawn by the
same rule: one RandomState in (module, state_dict) order, uniform(-k, k) with k = fan_in ** -0.5, a bias with the bound of
the weight registered before it.  At E = 1024 it equals fx.make_params bit for bit."""
from collections import OrderedDict

import numpy as np

from oracle import fixtures as fx


def param_shapes(A, E, image=64, tia=False, cond=0, belief=200, state=30, hidden=200):
    shapes = fx.param_shapes(A, belief=belief, state=state, hidden=hidden, embed=E, image=image, tia=tia, cond=cond)
    if image == 64 and E != 1024:
        enc = OrderedDict()
        for name, shp in shapes["encoder"].items():
            enc[name] = shp
            if name == "conv4.bias":
                enc["fc.weight"] = (E, 1024)
                enc["fc.bias"] = (E,)
        shapes["encoder"] = enc
    return shapes


def make_params(A, E, seed=7, image=64, tia=False, cond=0, belief=200, state=30, hidden=200):
    """{module: OrderedDict(name -> float32 ndarray)}, the rule of oracle/fixtures.py:make_params."""
    rs = np.random.RandomState(seed)
    out = OrderedDict()
    for mod, shapes in param_shapes(A, E, image=image, tia=tia, cond=cond, belief=belief, state=state, hidden=hidden).items():
        d = OrderedDict()
        k = 1.0
        for name, shp in shapes.items():
            if len(shp) > 1:
                k = 1.0 / np.sqrt(float(np.prod(shp[1:])))
            d[name] = rs.uniform(-k, k, size=shp).astype(np.float32)
        out[mod] = d
    return out


class FixturesAt:
    """oracle.fixtures with embedding_size = E: default_config and make_params at that width, everything else forwarded.
    The golden generator puts it in the place of the `fx` its run_* functions read; the GPU tests build their agents'
    configuration and parameters from it."""

    def __init__(self, E):
        self.E = E

    def __getattr__(self, name):
        return getattr(fx, name)

    def default_config(self, **over):
        over.setdefault("embedding_size", self.E)
        return fx.default_config(**over)

    def make_params(self, action_size, seed=7, image=64, **kw):
        return make_params(action_size, self.E, seed=seed, image=image, **kw)
