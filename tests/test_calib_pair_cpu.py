"""tests/calib_pair_ref.py against the REFERENCE's own CalibratedRePo.pair_calibration (algorithms/repo/repo_adapt.py:245-398,
the inv_dynamics branch), run unbound on a stand-in agent in float64 on the CPU: the reference's TransitionModel,
InverseDynamicsModel, VDBDiscriminator and MLP at small widths, two lookup tables in place of the conv encoders (so that the
gradient of the encoder loss with respect to the embeddings can be read), stand-in rings and an encoder optimiser that does
nothing.  The logged losses and the gradient with respect to the two target embeddings at 1e-10, in both alignment modes;
what the reference leaves frozen; and the order of its noise draws."""
import os
import sys
import types

import numpy as np
import pytest
import torch

from tests import calib_pair_ref as cp
from tests import calib_ref as cr
from tests import inv_dyn_ref as ir

REF = "/root/reference"
pytestmark = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "algorithms")),
                                reason="needs the reference checkout (build container only)")

L, B, A, D, S, HD, E, HI, HF, Z = 6, 3, 3, 12, 5, 10, 16, 14, 9, 4


@pytest.fixture(scope="module")
def ref():
    for name in ("wandb", "wandb.data_types"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.path.insert(0, REF)
    try:
        from algorithms.repo import repo_adapt
        from algorithms.repo.models.rssm import TransitionModel
        from algorithms.repo.models.utils import InverseDynamicsModel
        from common.models.gans import VDBDiscriminator
        from common.models.mlps import MLP
    finally:
        sys.path.remove(REF)
    return types.SimpleNamespace(adapt=repo_adapt, Rssm=TransitionModel, Inv=InverseDynamicsModel, Disc=VDBDiscriminator,
                                 MLP=MLP)


class _Table(torch.nn.Module):
    """Stands in for an encoder: call k returns the k-th (L B, E) table, whatever the frames."""

    def __init__(self, *tables):
        super().__init__()
        self.tables = torch.nn.ParameterList([torch.nn.Parameter(t.clone()) for t in tables])
        self.calls = 0

    def forward(self, obs):
        self.calls += 1
        return self.tables[self.calls - 1] + 0.0


class _Ring:
    def __init__(self, *batch):
        self.batch = batch

    def sample(self, batch_size, seq_len):
        return self.batch


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


class _Feeder:
    """torch.randn_like stand-in: serves the queued tensors in order and notes the shapes asked for."""

    def __init__(self, tensors):
        self.queue, self.shapes = list(tensors), []

    def __call__(self, like, **kw):
        t = self.queue.pop(0)
        assert t.shape == like.shape, (t.shape, like.shape)
        self.shapes.append(tuple(t.shape))
        return t


def _rssm_params(rs):
    shapes = [("fc_embed_state_action", (D, S + A)), ("rnn.weight_ih", (3 * D, D)), ("rnn.weight_hh", (3 * D, D)),
              ("rnn.bias_ih", (3 * D,)), ("rnn.bias_hh", (3 * D,)), ("fc_embed_belief_prior", (HD, D)),
              ("fc_state_prior", (2 * S, HD)), ("fc_embed_belief_posterior", (HD, D + E)), ("fc_state_posterior", (2 * S, HD))]
    out = {}
    for name, shp in shapes:
        if name.startswith("rnn."):
            out[name] = torch.from_numpy(rs.uniform(-0.3, 0.3, shp))
        else:
            out[name + ".weight"] = torch.from_numpy(rs.uniform(-0.3, 0.3, shp))
            out[name + ".bias"] = torch.from_numpy(rs.uniform(-0.3, 0.3, shp[:1]))
    return out


@pytest.mark.parametrize("support", [False, True])
def test_restatement_matches_the_reference_pair_calibration(ref, monkeypatch, support):
    rs = np.random.RandomState(17 + support)
    t = lambda *s: torch.from_numpy(rs.standard_normal(s))  # noqa: E731  (float64)
    T, N = L - 1, L * B
    aln_src, aln_tgt, cal_src, cal_tgt = (t(N, E).abs() for _ in range(4))
    acts = [rs.uniform(-1, 1, (L, B, A)) for _ in range(2)]
    dones = [(rs.uniform(size=(L, B, 1)) < 0.3).astype(np.float64) for _ in range(2)]
    for d in dones:
        assert 0 < cp.selected(1 - d)[0] < cp.selected(1 - d)[1]
    eps_prior, eps_post = t(T, 3 * B, S), t(T, 3 * B, S)
    eps_disc = [t(N, Z) for _ in range(4 if support else 3)]

    rssm_p = _rssm_params(rs)
    rssm = ref.Rssm(D, S, A, HD, E, "elu").double()
    assert set(rssm.state_dict().keys()) == set(rssm_p.keys())
    rssm.load_state_dict(rssm_p)
    inv_p = {k: torch.from_numpy(v).double() for k, v in ir.make_inv_params(D, S, A, HI, seed=5).items()}
    inv = ref.Inv(D, S, A, HI, "elu").double()
    inv.load_state_dict(inv_p)
    disc = ref.Disc(E, [HF] * 4, Z, lr=1e-4).double()
    disc.load_state_dict({k: torch.from_numpy(v).double() for k, v in cr.make_disc_params(E, HF, Z, seed=5).items()})
    log_tau = ref.MLP(E, [HF] * 4, 1).double()
    log_tau.load_state_dict({k: torch.from_numpy(v).double() for k, v in cr.make_tau_params(E, HF, seed=3).items()})
    u = torch.tensor(1e-2, dtype=torch.float64, requires_grad=True)
    frames = np.zeros((L, B, 1, 1, 1), dtype=np.uint8)
    coefs = (0.7, 1.3, 0.9)
    cfg = types.SimpleNamespace(batch_size=B, chunk_size=L, belief_size=D, state_size=S, disag_model=False,
                                inv_dynamics=True, alignment_mode="support" if support else "js", aln_coef=coefs[0],
                                dyn_coef=coefs[1], calib_coef=coefs[2])
    src_enc, enc = _Table(aln_src, cal_src), _Table(aln_tgt, cal_tgt)
    stub = types.SimpleNamespace(
        c=cfg, device=torch.device("cpu"), logger=_Recorder(), src_encoder=src_enc, encoder=enc, transition_model=rssm,
        inv_dynamics=inv, disc=disc, log_tau=log_tau, u=u, encoder_optimizer=_NoOptimizer(), tau_optimizer=_NoOptimizer(),
        u_optimizer=_NoOptimizer(), src_buffer=_Ring(frames, None, None, None),
        buffer=_Ring(frames, acts[0], None, dones[0]), calib_buffer=_Ring(frames, frames, acts[1], None, dones[1]))
    queue = [e for s in range(T) for e in (eps_prior[s], eps_post[s])] + eps_disc
    feeder = _Feeder(queue)
    monkeypatch.setattr(torch, "randn_like", feeder)
    torch.set_default_dtype(torch.float64)   # the reference builds its initial belief and state at the default dtype
    try:
        ref.adapt.CalibratedRePo.pair_calibration(stub)
    finally:
        torch.set_default_dtype(torch.float32)
        monkeypatch.undo()
    # the draws: prior then posterior per step over all 3 B columns, then the discriminator's
    assert not feeder.queue
    assert feeder.shapes == [(3 * B, S)] * (2 * T) + [(N, Z)] * len(eps_disc)
    kv = stub.logger.kv
    assert "train/dyn_loss" in kv and ("train/tau_loss" in kv) == support
    # frozen: the transition model gets no gradient at all; the inverse-dynamics model collects one nobody applies
    assert all(p.grad is None for p in rssm.parameters())
    assert all(p.grad is not None for p in inv.parameters())

    disc_after = {k: v.detach().clone() for k, v in disc.state_dict().items()}
    leaves = [x.clone().view(L, B, E).requires_grad_(True) for x in (cal_tgt, aln_tgt)]
    fl = lambda a: torch.from_numpy(a)  # noqa: E731
    out = cp.encoder_loss(rssm_p, inv_p, "elu", disc_after, support, cal_src.view(L, B, E), leaves[0], leaves[1],
                          fl(acts[1]), fl(1 - dones[1]), fl(acts[0]), fl(1 - dones[0]), eps_prior, eps_post, eps_disc[2],
                          coefs)
    for k, name in (("aln", "aln_loss"), ("dyn", "dyn_loss"), ("calib", "calib_loss"), ("encoder", "encoder_loss")):
        assert abs(float(out[k].detach()) - kv[f"train/{name}"]) <= 1e-10 * abs(kv[f"train/{name}"]), (k, out[k], kv)
    g_ct, g_at = torch.autograd.grad(out["encoder"], leaves)
    for name, got, want in (("cal_tgt", g_ct, enc.tables[1].grad), ("aln_tgt", g_at, enc.tables[0].grad)):
        err = float((got.reshape(N, E) - want).abs().max()) / float(want.abs().max())
        assert err <= 1e-10, (name, err)
    assert float(g_ct[0].abs().max()) == 0.0 and float(g_ct[1:].abs().max()) > 0.0   # frame 0 never enters the scan
    assert float(g_at[0].abs().max()) > 0.0                                           # but it does enter the alignment
    # (cal_src: the reference leaves a gradient in its source encoder too, which no optimiser holds -- nothing to build)


def test_restatement_of_an_empty_selection_is_nan_like_the_reference():
    rs = np.random.RandomState(2)
    t = lambda *s: torch.from_numpy(rs.standard_normal(s))  # noqa: E731
    rssm_p = _rssm_params(rs)
    inv_p = {k: torch.from_numpy(v).double() for k, v in ir.make_inv_params(D, S, A, HI, seed=5).items()}
    e = [t(L, B, E) for _ in range(3)]
    a = [torch.from_numpy(rs.uniform(-1, 1, (L, B, A))) for _ in range(2)]
    ones, none = torch.ones(L, B, 1, dtype=torch.float64), torch.ones(L, B, 1, dtype=torch.float64)
    none[1:-1] = 0
    dyn, calib = cp.latent_losses(rssm_p, inv_p, "elu", *e, a[0], none, a[1], ones, t(L - 1, 3 * B, S), t(L - 1, 3 * B, S))
    assert torch.isfinite(dyn) and torch.isnan(calib)
