"""tests/symbolic_ref.py against the REFERENCE's own SymbolicEncoder (models/encoder.py:6-18), SymbolicObservationModel
(models/decoder.py:6-25) and the obs-loss line of dreamer.py:262-267 (pixel_obs=False: .sum(2)), in float64 on the CPU:
outputs, the loss and every parameter gradient at 1e-10, for elu and relu.  And repo_amd's two modules against the
reference's: state-dict names, shapes and order, and the same default initialisation under a seed."""
import os
import sys
import types

import numpy as np
import pytest
import torch
from torch.distributions import Normal

from tests import symbolic_ref as sr

REF = "/root/reference"
needs_ref = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "algorithms")),
                               reason="needs the reference checkout (build container only)")


@pytest.fixture(scope="module")
def ref():
    """(the reference's Encoder factory, its ObservationModel factory)."""
    for name in ("wandb", "wandb.data_types"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.path.insert(0, REF)
    try:
        from algorithms.repo.models.decoder import ObservationModel
        from algorithms.repo.models.encoder import Encoder
    finally:
        sys.path.remove(REF)
    return Encoder, ObservationModel


def _load(module, params):
    sd = module.state_dict()
    assert list(sd.keys()) == list(params.keys())
    assert [tuple(v.shape) for v in sd.values()] == [v.shape for v in params.values()]
    module.load_state_dict({k: torch.from_numpy(v).double() for k, v in params.items()})


@needs_ref
@pytest.mark.parametrize("act", ["elu", "relu"])
@pytest.mark.parametrize("T,B,obs,D,S,E", [(7, 4, 17, 200, 30, 64), (3, 5, 24, 7, 5, 33)])
def test_restatement_matches_the_reference_modules_and_loss(ref, act, T, B, obs, D, S, E):
    Encoder, ObservationModel = ref
    rs = np.random.RandomState(50 + T)
    params = sr.make_symbolic_params(obs, D, S, E, seed=5)
    enc = Encoder(True, obs, E, act).double()
    dec = ObservationModel(True, obs, D, S, E, act).double()
    _load(enc, params["encoder"])
    _load(dec, params["obs_model"])
    t = lambda *s: torch.from_numpy(rs.standard_normal(s))  # noqa: E731  (float64)
    x, beliefs, states = t(T, B, obs), t(T, B, D) * 0.5, t(T, B, S)
    # the reference: encoder over flattened rows, then dreamer.py:262-267 on the decoder's output
    want_emb = enc(x.flatten(0, 1))
    want_recon = dec(beliefs.flatten(0, 1), states.flatten(0, 1)).view(T, B, obs)
    want_loss = -Normal(want_recon, 1).log_prob(x).sum(2).mean((0, 1))
    (want_loss + want_emb.pow(2).sum()).backward()
    pe = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in params["encoder"].items()}
    pd = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in params["obs_model"].items()}
    pre = []
    got_emb = sr.encoder(pe, x.flatten(0, 1), act, pre)
    got_recon = sr.decoder(pd, beliefs.flatten(0, 1), states.flatten(0, 1), act, pre).view(T, B, obs)
    got_loss = sr.obs_loss(got_recon, x)
    (got_loss + got_emb.pow(2).sum()).backward()
    assert (len(pre) == 4) == (act == "relu")
    assert float((got_emb - want_emb).detach().abs().max()) <= 1e-10 * float(want_emb.detach().abs().max())
    assert float((got_recon - want_recon).detach().abs().max()) <= 1e-10 * float(want_recon.detach().abs().max())
    assert abs(float(got_loss.detach()) - float(want_loss.detach())) <= 1e-10 * abs(float(want_loss.detach()))
    # ... and the sum the kernel reports is that loss without its constant
    n = T * B
    assert abs(float(sr.nll_sum(got_recon, x)) / n + 0.5 * np.log(2 * np.pi) * obs - float(want_loss)) <= 1e-10 * abs(float(want_loss))
    for p, m in ((pe, enc), (pd, dec)):
        for (k, v), w in zip(p.items(), m.parameters()):
            err = float((v.grad - w.grad).abs().max()) / (float(w.grad.abs().max()) + 1e-30)
            assert err <= 1e-10, (k, err)


@needs_ref
@pytest.mark.parametrize("act", ["relu", "elu"])
def test_modules_have_the_reference_state_dict_and_default_init(ref, act):
    from repo_amd.algorithms.repo.models.decoder import ObservationModel as OurObs
    from repo_amd.algorithms.repo.models.decoder import SymbolicObservationModel
    from repo_amd.algorithms.repo.models.encoder import Encoder as OurEnc
    from repo_amd.algorithms.repo.models.encoder import SymbolicEncoder

    Encoder, ObservationModel = ref
    obs, D, S, E = 17, 200, 30, 128
    torch.manual_seed(3)
    theirs = (Encoder(True, obs, E, act), ObservationModel(True, obs, D, S, E, act))
    torch.manual_seed(3)
    ours = (OurEnc(True, obs, E, act), OurObs(True, obs, D, S, E, act))
    assert isinstance(ours[0], SymbolicEncoder) and isinstance(ours[1], SymbolicObservationModel)
    for a, b in zip(ours, theirs):
        sa, sb = a.state_dict(), b.state_dict()
        assert list(sa.keys()) == list(sb.keys())
        for k in sa:
            assert sa[k].shape == sb[k].shape and torch.equal(sa[k], sb[k]), k
        assert [id(t) for t in a.plist()] == [id(t) for t in a.parameters()]   # plist() is the state_dict order


def test_modules_expose_act_and_refuse_what_is_not_built():
    from repo_amd import ops
    from repo_amd.algorithms.repo.models.decoder import ObservationModel
    from repo_amd.algorithms.repo.models.encoder import Encoder

    assert Encoder(True, 17, 64, "relu").act == ops.ACT_RELU and Encoder(True, 17, 64, "elu").act == ops.ACT_ELU
    assert ObservationModel(True, 17, 20, 3, 64, "elu").act == ops.ACT_ELU
    assert Encoder(True, 1, 8).observation_size == 1 and Encoder(True, 1024, 8).observation_size == 1024
    for bad in (0, 1025):
        with pytest.raises(NotImplementedError, match="observation_size"):
            Encoder(True, bad, 64)
        with pytest.raises(NotImplementedError, match="observation_size"):
            ObservationModel(True, bad, 20, 3, 64)
    with pytest.raises(NotImplementedError):
        Encoder(True, 17, 64, "tanh")
    with pytest.raises(NotImplementedError):
        ObservationModel(True, 17, 20, 3, 64, "tanh")
    # the pixel classes keep their refusals
    with pytest.raises(NotImplementedError):
        Encoder(False, (3, 64, 64), 1024, "elu")
    with pytest.raises(NotImplementedError):
        ObservationModel(False, (3, 64, 64), 200, 30, 1024, "elu")


def test_seeded_recipe_is_stable():
    p = sr.make_symbolic_params(17)
    assert list(p) == ["encoder", "obs_model"]
    assert [v.shape for v in p["encoder"].values()] == [(1024, 17), (1024,), (1024, 1024), (1024,), (1024, 1024), (1024,)]
    assert [v.shape for v in p["obs_model"].values()] == [(1024, 230), (1024,), (1024, 1024), (1024,), (17, 1024), (17,)]
    q = sr.make_symbolic_params(17)
    assert all(np.array_equal(p[m][k], q[m][k]) for m in p for k in p[m])
    assert sr.make_obs(8, 4, 17, 11).shape == (8, 4, 17) and sr.make_obs(8, 4, 17, 11).dtype == np.float32
