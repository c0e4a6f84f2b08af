"""embedding_size != 1024 on the CPU: repo_amd's pixel modules against the REFERENCE's own (state_dict names, order and
shapes, and equal tensors after construction under one torch.manual_seed), tests/embed_ref.py's parameter recipe, and the
oracle's encoder_fwd / decoder_fwd against the reference's modules in float64 at 1e-10.  At 1024 the encoder keeps its
eight tensors and an Identity `fc`."""
import os
import sys
import types

import numpy as np
import pytest
import torch

from oracle import fixtures as fx
from oracle import repo_oracle as orc
from tests import embed_ref as er

REF = "/root/reference"
needs_ref = pytest.mark.skipif(not os.path.isdir(os.path.join(REF, "algorithms")),
                               reason="needs the reference checkout (build container only)")
WIDTHS = [64, 250, 1536]
D, S, C, A = 200, 30, 3, 6


@pytest.fixture(scope="module")
def ref():
    for name in ("wandb", "wandb.data_types"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.path.insert(0, REF)
    try:
        from algorithms.repo.models import decoder, encoder
    finally:
        sys.path.remove(REF)
    return encoder, decoder


def _pairs(ref, E):
    """(name, constructor of ours, constructor of the reference's)."""
    from repo_amd.algorithms.repo.models import conditional as ocond
    from repo_amd.algorithms.repo.models import decoder as odec
    from repo_amd.algorithms.repo.models import encoder as oenc

    renc, rdec = ref
    shape = (3, 64, 64)
    return [
        ("Encoder", lambda: oenc.Encoder(False, shape, E), lambda: renc.Encoder(False, shape, E)),
        ("ObservationModel", lambda: odec.ObservationModel(False, shape, D, S, E), lambda: rdec.ObservationModel(False, shape, D, S, E)),
        ("TIAObservationModel", lambda: odec.TIAObservationModel(D, S, E), lambda: rdec.TIAObservationModel(D, S, E)),
        ("ConditionalEncoder", lambda: ocond.ConditionalEncoder(False, shape, E, C), lambda: renc.ConditionalEncoder(False, shape, E, C)),
        ("ConditionalObservationModel", lambda: ocond.ConditionalObservationModel(False, shape, D, S, E, C),
         lambda: rdec.ConditionalObservationModel(False, shape, D, S, E, C)),
    ]


@needs_ref
@pytest.mark.parametrize("E", WIDTHS)
def test_modules_have_the_reference_state_dict_and_default_init(ref, E):
    for name, ours, theirs in _pairs(ref, E):
        torch.manual_seed(3)
        a = ours().state_dict()
        torch.manual_seed(3)
        b = theirs().state_dict()
        assert list(a.keys()) == list(b.keys()), name
        for k in a:
            assert a[k].shape == b[k].shape, (name, k)
            assert torch.equal(a[k], b[k]), (name, k)


@needs_ref
@pytest.mark.parametrize("E", WIDTHS)
def test_helper_shapes_are_the_reference_modules(ref, E):
    renc, rdec = ref
    shape = (3, 64, 64)
    plain, tia, cond = er.param_shapes(A, E), er.param_shapes(A, E, tia=True), er.param_shapes(A, E, cond=C)
    for shapes, mod in ((plain["encoder"], renc.Encoder(False, shape, E)),
                        (plain["obs_model"], rdec.ObservationModel(False, shape, D, S, E)),
                        (tia["obs_model"], rdec.TIAObservationModel(D, S, E)),
                        (cond["encoder"], renc.ConditionalEncoder(False, shape, E, C)),
                        (cond["obs_model"], rdec.ConditionalObservationModel(False, shape, D, S, E, C))):
        sd = mod.state_dict()
        assert list(sd.keys()) == list(shapes.keys())
        assert [tuple(v.shape) for v in sd.values()] == [tuple(s) for s in shapes.values()]
    assert plain["transition_model"]["fc_embed_belief_posterior.weight"] == (200, D + E)


@pytest.mark.parametrize("kw", [dict(), dict(tia=True), dict(cond=3), dict(image=128), dict(belief=64, state=9, hidden=48)])
def test_helper_at_1024_is_fixtures_make_params(kw):
    a, b = er.make_params(A, 1024, seed=7, **kw), fx.make_params(A, seed=7, **kw)
    assert list(a.keys()) == list(b.keys())
    for mod in a:
        assert list(a[mod].keys()) == list(b[mod].keys()), mod
        for k in a[mod]:
            assert a[mod][k].dtype == b[mod][k].dtype and np.array_equal(a[mod][k], b[mod][k]), (mod, k)


def test_helper_inserts_fc_behind_conv4_and_in_front_of_film():
    enc = list(er.param_shapes(A, 250, cond=3)["encoder"].keys())
    assert enc[6:] == ["conv4.weight", "conv4.bias", "fc.weight", "fc.bias", "film.weight", "film.bias"]
    assert er.param_shapes(A, 250)["encoder"]["fc.weight"] == (250, 1024)
    assert er.param_shapes(A, 250, image=128)["encoder"]["fc.weight"] == (250, 9216)   # fx's own fc: nothing inserted
    assert len(er.param_shapes(A, 250, image=128)["encoder"]) == 10
    fa = er.FixturesAt(250)
    assert fa.default_config(algo="repo").embedding_size == 250 and fa.MODULES is fx.MODULES
    assert np.array_equal(fa.make_params(A, seed=9)["encoder"]["fc.bias"], er.make_params(A, 250, seed=9)["encoder"]["fc.bias"])


@needs_ref
@pytest.mark.parametrize("E", WIDTHS)
def test_oracle_encoder_and_decoder_equal_the_reference_modules(ref, E):
    renc, rdec = ref
    params = er.make_params(A, E)
    rs = np.random.RandomState(5)
    enc = renc.Encoder(False, (3, 64, 64), E).double()
    dec = rdec.ObservationModel(False, (3, 64, 64), D, S, E).double()
    pe = {k: torch.from_numpy(v).double() for k, v in params["encoder"].items()}
    pd = {k: torch.from_numpy(v).double() for k, v in params["obs_model"].items()}
    enc.load_state_dict(pe)
    dec.load_state_dict(pd)
    obs = torch.from_numpy(rs.uniform(-1, 1, size=(5, 3, 64, 64)))
    belief, state = torch.from_numpy(rs.standard_normal((5, D))), torch.from_numpy(rs.standard_normal((5, S)))
    with torch.no_grad():
        want_e, got_e = enc(obs), orc.encoder_fwd(pe, obs)
        want_d, got_d = dec(belief, state), orc.decoder_fwd(pd, belief, state)
    assert got_e.shape == (5, E) and got_d.shape == (5, 3, 64, 64)
    assert (got_e - want_e).abs().max().item() <= 1e-10
    assert (got_d - want_d).abs().max().item() <= 1e-10


def test_encoder_at_1024_keeps_eight_tensors_and_an_identity_fc():
    from repo_amd.algorithms.repo.models.encoder import VisualEncoder

    enc = VisualEncoder(1024)
    assert isinstance(enc.fc, torch.nn.Identity) and len(enc.plist()) == 8
    assert list(enc.state_dict().keys()) == list(fx.param_shapes(A)["encoder"].keys())
    enc = VisualEncoder(250)
    assert len(enc.plist()) == 10 and enc.plist()[8] is enc.fc.weight and enc.plist()[9] is enc.fc.bias
    assert tuple(enc.fc.weight.shape) == (250, 1024)
    wide = VisualEncoder(250, image_size=128)
    assert len(wide.plist()) == 10 and tuple(wide.fc.weight.shape) == (250, 9216)


def test_conditional_plist_keeps_film_last():
    from repo_amd.algorithms.repo.models.conditional import ConditionalVisualEncoder

    enc = ConditionalVisualEncoder(250, 3)
    p = enc.plist()
    assert len(p) == 12 and p[8] is enc.fc.weight and p[-2] is enc.film.weight and p[-1] is enc.film.bias
    assert len(ConditionalVisualEncoder(1024, 3).plist()) == 10


def test_compose_rule_counts_multiplications(monkeypatch):
    """Compose when rows >= 512 and E (F + 3200) > F 3200: at F = 230 from E = 215 up; at E = 1024 for every F < 1506."""
    from repo_amd import functional as Fn

    monkeypatch.delenv("REPO_DEC_COMPOSE", raising=False)

    def p(E, F_):
        return [torch.empty(E, F_)]

    assert not Fn._dec_compose(512, p(214, 230)) and Fn._dec_compose(512, p(215, 230))
    assert not Fn._dec_compose(512, p(64, 230)) and Fn._dec_compose(512, p(250, 230)) and Fn._dec_compose(512, p(1536, 231))
    assert not Fn._dec_compose(511, p(1024, 230))
    for F_ in (1, 230, 231, 264, 1054, 1505):
        assert Fn._dec_compose(512, p(1024, F_)) and Fn._dec_compose(2450, p(1024, F_))
    monkeypatch.setenv("REPO_DEC_COMPOSE", "0")
    assert not Fn._dec_compose(2450, p(1024, 230))


@pytest.mark.parametrize("bad", [0, -3, 250.5, True])
def test_embedding_size_must_be_a_positive_integer(bad):
    from repo_amd.algorithms.repo.models.conditional import ConditionalVisualEncoder, ConditionalVisualObservationModel
    from repo_amd.algorithms.repo.models.decoder import TIAObservationModel, VisualObservationModel
    from repo_amd.algorithms.repo.models.encoder import VisualEncoder

    for build in (lambda: VisualEncoder(bad), lambda: VisualEncoder(bad, image_size=128), lambda: VisualObservationModel(D, S, bad),
                  lambda: TIAObservationModel(D, S, bad), lambda: ConditionalVisualEncoder(bad, C),
                  lambda: ConditionalVisualObservationModel(D, S, bad, C)):
        with pytest.raises(ValueError, match="embedding_size must be a positive integer"):
            build()
    assert VisualEncoder(1).fc.out_features == 1 and VisualEncoder(251.0).embedding_size == 251
