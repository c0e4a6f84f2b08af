"""tests/calib_ref.py against the REFERENCE's own VDBDiscriminator.train and MLP (common/models/gans.py:56-156,
mlps.py:11-32) in float64 on the CPU: the logged losses, every parameter gradient (the gradient penalty's second-order part
included) and beta after the step at 1e-10, in both modes; the state-dict keys of repo_amd's modules; and CalibrationBuffer
/ load_source_data against the reference's under the same np.random seed and files."""
import os
import sys
import types

import numpy as np
import pytest
import torch

from tests import calib_ref as cr

REF = "/root/reference"
pytestmark = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "algorithms")),
                                reason="needs the reference checkout (build container only)")


@pytest.fixture(scope="module")
def ref():
    for name in ("wandb", "wandb.data_types"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.path.insert(0, REF)
    try:
        from common.models.gans import VDBDiscriminator
        from common.models.mlps import MLP
    finally:
        sys.path.remove(REF)
    return VDBDiscriminator, MLP


class _Feeder:
    """torch.randn_like stand-in: serves the queued tensors in order."""

    def __init__(self, *tensors):
        self.queue = list(tensors)

    def __call__(self, like, **kw):
        t = self.queue.pop(0)
        assert t.shape == like.shape
        return t


@pytest.mark.parametrize("support", [False, True])
@pytest.mark.parametrize("Nr,Nf,E,Hf,Z", [(6, 6, 32, 16, 4), (3, 7, 10, 9, 5)])
def test_restatement_matches_the_reference_discriminator_step(ref, monkeypatch, support, Nr, Nf, E, Hf, Z):
    RefDisc, _ = ref
    params = cr.make_disc_params(E, Hf, Z, seed=5)
    model = RefDisc(E, [Hf] * 4, Z, lr=1e-4).double()
    sd = model.state_dict()
    assert list(sd.keys()) == list(params.keys())
    assert [tuple(v.shape) for v in sd.values()] == [v.shape for v in params.values()]
    model.load_state_dict({k: torch.from_numpy(v).double() for k, v in params.items()})
    rs = np.random.RandomState(Nr)
    t = lambda *s: torch.from_numpy(rs.standard_normal(s))  # noqa: E731  (float64)
    x_real, x_fake, eps_r, eps_f = t(Nr, E), t(Nf, E), t(Nr, Z), t(Nf, Z)
    tau = torch.exp(0.3 * t(Nr, 1)) if support else None
    monkeypatch.setattr(torch, "randn_like", _Feeder(eps_r, eps_f))
    info = model.train(x_real.clone(), x_fake.clone(), tau)
    monkeypatch.undo()
    p = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in params.items()}
    pre = []
    out = cr.disc_losses(p, x_real, x_fake, eps_r, eps_f, 0.1, tau=None if tau is None else tau[:, 0], pre=pre)
    assert len(pre) == 10   # four LeakyReLU inputs and lat, per set
    (out["real"] + out["fake"] + out["kl_loss"] + out["gp"]).backward()
    for k, name in (("real", "real_loss"), ("fake", "fake_loss"), ("kl", "kl"), ("gp", "gp")):
        assert abs(float(out[k]) - info[name]) <= 1e-10 * abs(info[name]), (k, float(out[k]), info[name])
    assert abs(cr.beta_step(0.1, out["kl"]) - info["beta"]) <= 1e-12
    for (k, v), w in zip(p.items(), model.parameters()):
        err = float((v.grad - w.grad).abs().max()) / (float(w.grad.abs().max()) + 1e-30)
        assert err <= 1e-10, (k, err)
    # the Adam step the reference took is the first-step formula of the restatement
    for (k, v), w in zip(p.items(), model.parameters()):
        want = cr.adam_first_step(torch.from_numpy(params[k]).double(), v.grad, 1e-4)
        assert float((want - w.detach()).abs().max()) <= 1e-12, k


def test_restatement_matches_the_reference_mlp_and_the_support_losses(ref):
    _, RefMLP = ref
    E, Hf, N = 12, 7, 5
    params = cr.make_tau_params(E, Hf, seed=3)
    model = RefMLP(E, [Hf] * 4, 1).double()
    assert list(model.state_dict().keys()) == list(params.keys())
    model.load_state_dict({k: torch.from_numpy(v).double() for k, v in params.items()})
    rs = np.random.RandomState(1)
    x, d_src = torch.from_numpy(rs.standard_normal((N, E))), torch.from_numpy(rs.standard_normal((N, 1)))
    u = torch.tensor(0.7, dtype=torch.float64, requires_grad=True)
    # the reference's lines (repo_adapt.py:465-476) on its own module
    tau = model(x).exp()
    want_tau = (tau * d_src).mean() + u.detach() * (tau - 1).mean()
    want_u = -u * (tau - 1).mean().detach()
    want_tau.backward()
    p = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in params.items()}
    pre = []
    got_tau_val = cr.mlp(p, x, "relu", pre).exp()
    assert len(pre) == 4
    u2 = torch.tensor(0.7, dtype=torch.float64, requires_grad=True)
    got_tau, got_u = cr.tau_losses(got_tau_val[:, 0], d_src[:, 0], u2)
    got_tau.backward()
    assert abs(float(got_tau) - float(want_tau)) <= 1e-12 and abs(float(got_u) - float(want_u)) <= 1e-12
    for (k, v), w in zip(p.items(), model.parameters()):
        assert float((v.grad - w.grad).abs().max()) <= 1e-12 * (1 + float(w.grad.abs().max())), k
    a, b = torch.from_numpy(rs.standard_normal((4, 3, 6))), torch.from_numpy(rs.standard_normal((4, 3, 6)))
    want = -torch.distributions.Normal(a, 1).log_prob(b).mean()
    assert abs(float(cr.calib_loss(a, b)) - float(want)) <= 1e-12


# ----------------------------------------------------------------------------- host side
@pytest.fixture(scope="module")
def ref_adapt():
    for name in ("wandb", "wandb.data_types"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.path.insert(0, REF)
    try:
        from algorithms.repo import repo_adapt
    finally:
        sys.path.remove(REF)
    return repo_adapt


def test_calibration_buffer_samples_what_the_reference_samples(ref_adapt):
    from repo_amd.common.buffers import CalibrationBuffer

    rs = np.random.RandomState(4)
    ours = CalibrationBuffer(40, (6, 8, 8), (3,), obs_type=np.uint8)
    theirs = ref_adapt.CalibrationBuffer(40, (6, 8, 8), (3,), obs_type=np.uint8)
    for i in range(57):   # wraps
        tr = (rs.randint(0, 256, (6, 8, 8)).astype(np.uint8), rs.uniform(-1, 1, 3).astype(np.float32), float(rs.randn()),
              float(i % 9 == 8))
        ours.push(*tr)
        theirs.push(*tr)
    np.random.seed(12)
    got = ours.sample(5, 7)
    np.random.seed(12)
    want = theirs.sample(5, 7)
    assert len(got) == len(want) == 5
    for a, b in zip(got, want):
        assert a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a, b)
    assert got[0].shape == (7, 5, 3, 8, 8) and got[1].shape == (7, 5, 3, 8, 8)


def test_load_source_data_adopts_what_the_reference_loads(ref_adapt, tmp_path):
    from repo_amd.algorithms.repo.repo_adapt import CalibratedRePo
    from repo_amd.common.buffers import SequenceReplayBuffer

    rs = np.random.RandomState(6)
    for name, n_push in (("buffer_a.npz", 13), ("buffer_b.npz", 31)):   # one ring not full, one wrapped
        ring = SequenceReplayBuffer(20, (3, 4, 4), (2,), obs_type=np.uint8)
        for i in range(n_push):
            ring.push(rs.randint(0, 256, (3, 4, 4)).astype(np.uint8), rs.uniform(-1, 1, 2).astype(np.float32),
                      float(rs.randn()), float(i % 7 == 6))
        ring.save(str(tmp_path / name))
    cfg = types.SimpleNamespace(source_dir=str(tmp_path), offline_truncate_size=17)
    ours = types.SimpleNamespace(c=cfg, src_buffer=SequenceReplayBuffer(5, (3, 4, 4), (2,), obs_type=np.uint8))
    theirs = types.SimpleNamespace(c=cfg, src_buffer=types.SimpleNamespace())
    CalibratedRePo.load_source_data(ours)
    ref_adapt.CalibratedRePo.load_source_data(theirs)
    for k in ("observations", "actions", "rewards", "dones"):
        assert np.array_equal(getattr(ours.src_buffer, k), getattr(theirs.src_buffer, k)), k
    assert (ours.src_buffer.capacity, ours.src_buffer.pos, ours.src_buffer.full) == (30, 0, True)
    assert (theirs.src_buffer.capacity, theirs.src_buffer.pos, theirs.src_buffer.full) == (30, 0, True)


def test_state_dict_keys_equal_the_references(ref):
    RefDisc, RefMLP = ref
    from repo_amd.common.models.mlps import MLP

    ours, theirs = MLP(12, [7] * 4, 1), RefMLP(12, [7] * 4, 1)
    assert [(k, tuple(v.shape)) for k, v in ours.state_dict().items()] == \
           [(k, tuple(v.shape)) for k, v in theirs.state_dict().items()]
    # the same construction order and initialisation: a seed gives the same parameters
    torch.manual_seed(3)
    a = MLP(12, [7] * 4, 1, act="LeakyReLU")
    torch.manual_seed(3)
    b = RefMLP(12, [7] * 4, 1, act="LeakyReLU")
    for (k, v), w in zip(a.state_dict().items(), b.state_dict().values()):
        assert torch.equal(v, w), k
    want = list(RefDisc(12, [7] * 4, 3).state_dict().keys())
    assert want == list(cr.make_disc_params(12, 7, 3).keys())   # (repo_amd's module is built on a device: test_calib_gpu)
