"""tests/inv_dyn_ref.py against the REFERENCE's own InverseDynamicsModel (models/utils.py:84-109) under the reference's own
Dreamer.train_inv_dynamics (dreamer.py:220-239, called on a stand-in agent), in float64 on the CPU: the loss and every parameter gradient at 1e-10, for elu and relu, with a mask
that selects some rows and drops others.  (make_inv_params is checked against the module's state_dict on the way.)"""
import os
import sys
import types

import numpy as np
import pytest
import torch

from tests import inv_dyn_ref as ir

REF = "/root/reference"
pytestmark = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "algorithms")),
                                reason="needs the reference checkout (build container only)")


@pytest.fixture(scope="module")
def ref():
    """(the reference's InverseDynamicsModel, its Dreamer class)."""
    for name in ("wandb", "wandb.data_types"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.path.insert(0, REF)
    try:
        from algorithms.repo import Dreamer
        from algorithms.repo.models.utils import InverseDynamicsModel
    finally:
        sys.path.remove(REF)
    return InverseDynamicsModel, Dreamer


class _NoOptimizer:
    def zero_grad(self):
        pass

    def step(self):
        pass


class _Recorder:
    def __init__(self):
        self.kv = {}

    def record(self, k, v, exclude=None):
        self.kv[k] = v


def _reference_step(Dreamer, model, beliefs, states, actions, nonterms):
    """The reference's OWN Dreamer.train_inv_dynamics, run unbound on a stand-in agent: the module, an optimiser that
    does nothing (the gradients stay in the module's parameters, unclipped: grad_clip_norm = inf) and a logger that
    records.  -> the logged loss."""
    stub = types.SimpleNamespace(inv_dynamics=model, inv_dynamics_optimizer=_NoOptimizer(), logger=_Recorder(),
                                 c=types.SimpleNamespace(grad_clip_norm=float("inf")))
    Dreamer.train_inv_dynamics(stub, beliefs, states, actions, nonterms)
    return stub.logger.kv["train/inv_dyn_loss"]


@pytest.mark.parametrize("act", ["elu", "relu"])
@pytest.mark.parametrize("T,B,D,S,A,hidden", [(7, 4, 200, 30, 6, 100), (4, 5, 7, 5, 3, 33)])
def test_restatement_matches_the_reference_module_and_loss(ref, act, T, B, D, S, A, hidden):
    RefModel, Dreamer = ref
    rs = np.random.RandomState(100 + T)
    params = ir.make_inv_params(D, S, A, hidden, seed=5)
    model = RefModel(D, S, A, hidden, act).double()
    sd = model.state_dict()
    assert list(sd.keys()) == list(params.keys())
    assert [tuple(v.shape) for v in sd.values()] == [v.shape for v in params.values()]
    model.load_state_dict({k: torch.from_numpy(v).double() for k, v in params.items()})
    t = lambda *s: torch.from_numpy(rs.standard_normal(s))  # noqa: E731  (float64)
    beliefs, states, actions = t(T, B, D) * 0.5, t(T, B, S), torch.from_numpy(rs.uniform(-1, 1, (T + 1, B, A)))
    nonterms = torch.from_numpy((rs.uniform(size=(T + 1, B, 1)) > 0.3).astype(np.float64))
    selected = int(nonterms[1:-1].sum())
    assert 0 < selected < (T - 1) * B
    want = _reference_step(Dreamer, model, beliefs, states, actions, nonterms)
    p = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in params.items()}
    pre = []
    got = ir.loss(p, beliefs, states, actions, nonterms, act, pre)
    got.backward()
    assert (len(pre) == 3) == (act == "relu")
    assert abs(float(got.detach()) - want) <= 1e-10 * abs(want)
    for (k, v), w in zip(p.items(), model.parameters()):
        err = float((v.grad - w.grad).abs().max()) / (float(w.grad.abs().max()) + 1e-30)
        assert err <= 1e-10, (k, err)


def test_restatement_of_an_empty_selection_is_nan_like_the_reference():
    p = {k: torch.from_numpy(v).double() for k, v in ir.make_inv_params(8, 3, 2, 16).items()}
    z = torch.zeros
    out = ir.loss(p, z(3, 2, 8).double(), z(3, 2, 3).double(), z(4, 2, 2).double(), z(4, 2, 1).double(), "elu")
    assert torch.isnan(out)
