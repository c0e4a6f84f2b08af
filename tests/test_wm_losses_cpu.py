"""tests/wm_losses_ref.py tied down on the CPU: the mode-2 KL's hand gradients against autograd, mode 2 at
unit scales against mode 1, the oracle classes against their parents with the keys off, the distance the keys move the
quantities the GPU comparisons check, and every configuration error that needs no device."""
import types

import numpy as np
import pytest
import torch

from oracle import fixtures as fx
from tests import symbolic_ref as sr
from tests import twohot_ref as th
from tests import wm_losses_ref as wl

L, B, H, A, OBS = 10, 5, 6, 6, 17     # the GPU suite's whole-update shape


def _bits(t):
    return t.detach().contiguous().view(torch.int64 if t.dtype == torch.float64 else torch.int32)


def _kl_inputs(rows, S, seed, dtype=torch.float64):
    rs = np.random.RandomState(seed)
    pm, qm = (torch.from_numpy(rs.standard_normal((rows, S))).to(dtype) for _ in range(2))
    ps, qs = (torch.from_numpy(rs.uniform(0.3, 2.0, (rows, S))).to(dtype) for _ in range(2))
    return pm, ps, qm, qs


@pytest.mark.parametrize("dyn,rep", [(0.5, 0.1), (1.0, 1.0), (0.0, 2.5), (3.0, 0.0)])
@pytest.mark.parametrize("rows,S", [(1, 1), (5, 30), (41, 64)])
def test_mode2_gradients_match_autograd(rows, S, dyn, rep):
    pm, ps, qm, qs = _kl_inputs(rows, S, 100 * rows + S)
    klrow = wl._kl_terms(pm, ps, qm, qs)[0]
    free = wl.free_between(klrow)     # about half the rows clipped
    scale = 1.0 / rows
    leaves = [t.clone().requires_grad_(True) for t in (pm, ps, qm, qs)]
    (wl.kl_mode2_loss(*leaves, dyn, rep, free).sum() * scale).backward()
    total, *grads = wl.kl_mode2(pm, ps, qm, qs, dyn, rep, free, scale)
    clipped = int((klrow <= free).sum())
    assert rows == 1 or 0 < clipped < rows
    for name, got, leaf in zip(("dpm", "dps", "dqm", "dqs"), grads, leaves):
        err = float((got - leaf.grad).abs().max() / max(float(leaf.grad.abs().max()), 1e-300))
        assert err < 1e-12, (name, err)
    want = torch.maximum(klrow, torch.full_like(klrow, free)).sum()
    assert abs(float(total - want)) <= 1e-12 * abs(float(want))


def test_mode2_tie_rule_matches_autograd():
    """A row whose KL equals free_nats exactly: half the gradient on each side, as torch.maximum gives."""
    pm, ps, qm, qs = _kl_inputs(3, 8, 5)
    klrow = wl._kl_terms(pm, ps, qm, qs)[0]
    free = float(klrow[1])
    leaves = [t.clone().requires_grad_(True) for t in (pm, ps, qm, qs)]
    wl.kl_mode2_loss(*leaves, 0.5, 0.1, free).sum().backward()
    _, *grads = wl.kl_mode2(pm, ps, qm, qs, 0.5, 0.1, free, 1.0)
    for got, leaf in zip(grads, leaves):
        assert float((got - leaf.grad).abs().max()) <= 1e-12 * float(leaf.grad.abs().max())
        assert float(got[1].abs().max()) > 0.0


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_mode2_at_unit_scales_is_mode1_in_bits(dtype):
    pm, ps, qm, qs = _kl_inputs(57, 30, 9, dtype)
    free = float(wl._kl_terms(pm, ps, qm, qs)[0].median())
    one = wl.kl_mode1(pm, ps, qm, qs, free, 1.0 / 57)
    two = wl.kl_mode2(pm, ps, qm, qs, 1.0, 1.0, free, 1.0 / 57)
    for a, b in zip(one, two):
        assert torch.equal(_bits(a), _bits(b))


def test_reward_loss_matches_autograd_of_its_definition():
    rs = np.random.RandomState(3)
    z = torch.from_numpy(rs.standard_normal((12, 31))).requires_grad_(True)
    r = torch.from_numpy(rs.standard_normal(12) * 30.0)
    mask = torch.tensor([1.0, 0.0] * 6, dtype=torch.float64)
    loss, sums = wl.reward_loss(z, r, mask, -5.0, 5.0)
    t, _, _ = th.target(r, 31, -5.0, 5.0)
    want = (mask * -(t * torch.log_softmax(z, 1)).sum(1)).mean()
    assert abs(float((loss - want).detach())) <= 1e-12 * abs(float(want.detach())) and float(sums[1]) == 6.0
    loss.backward()
    assert not z.grad[1::2].any() and z.grad[0::2].any()      # masked rows take no gradient
    v = wl.decode_reward(z.detach(), -5.0, 5.0)
    assert torch.equal(v, th.symexp((torch.softmax(z.detach(), 1) * th.bins(31, -5.0, 5.0)).sum(1)))
    assert not wl.decode_reward(torch.zeros(4, 255, dtype=torch.float64), -20.0, 20.0).abs().max() > 1e-15


# ----------------------------------------------------------------------------- the oracle classes
def _host_batch(seed, symbolic, scaled=False):
    obs, act, rew, done = fx.make_batch(L, B, A, seed=seed)
    if symbolic:
        obs = wl.scaled_obs(L, B, OBS, seed) if scaled else sr.make_obs(L, B, OBS, seed)
    return obs, act, rew, done


def _cfg(algo, **over):
    return fx.default_config(algo=algo, batch_size=B, chunk_size=L, horizon=H, **over)


@pytest.mark.parametrize("algo", ["repo", "dreamer"])
def test_oracle_with_the_keys_off_is_its_parent_in_bits(algo):
    cfg = _cfg(algo, reward_dist="normal", obs_symlog=False)
    host, nz = _host_batch(60, False), fx.make_noise(L, B, H, A, seed=160)
    child = wl.OracleWm(cfg, A, params=fx.make_params(A, 7))
    parent = th.OracleTwoHot(cfg, A, params=fx.make_params(A, 7))
    assert not child.wm["rd_on"] and not child.wm["symlog_on"] and not child.wm["kl_on"]
    for u in range(2):
        sc, sp = child.update(*host, nz)[2], parent.update(*host, nz)[2]
        assert sc == sp, (u, sc, sp)
        for a, b in zip(child.last["model_grads"], parent.last["model_grads"]):
            assert torch.equal(_bits(a), _bits(b)), u
    for a, b in zip(child.model_params + child.actor_params, parent.model_params + parent.actor_params):
        assert torch.equal(_bits(a), _bits(b))


def _flat(grads):
    return torch.cat([g.reshape(-1) for g in grads if g is not None])


def _moved(keyed, plain, keys):
    """Relative distance of the logged scalars in `keys` and of the flat model gradient between two oracles' last update."""
    (ks, kg), (ps, pg) = keyed, plain
    out = {k: wl.rel_gap(ks[k], ps[k]) for k in keys}
    out["model gradient"] = float((kg - pg).norm() / pg.norm())
    return out


def _one_update(cls, cfg, params, host, nz, **kw):
    o = cls(cfg, A, params=params, **kw)
    sc = o.update(*host, nz)[2]
    return sc, _flat(o.last["model_grads"])


def test_each_key_moves_what_the_gpu_comparisons_check():
    """For the GPU suite's inputs: the keyed oracle's reward loss / observation loss / model gradient lie more than 1e-2
    (relative) from the unkeyed one's -- the GPU bounds are 1e-3, so a build that ignores a key cannot pass them."""
    nz = fx.make_noise(L, B, H, A, seed=160)
    # reward_dist: the unkeyed oracle is the fixtures' scalar head (the two model gradients have different lengths: the
    # loss is what is compared)
    host = _host_batch(60, False)
    for algo in ("repo", "dreamer"):
        cfg = _cfg(algo, reward_dist="twohot", reward_bins=31, reward_bin_low=-5.0, reward_bin_high=5.0)
        keyed = _one_update(wl.OracleWm, cfg, wl.wm_params(A, cfg, reward_K=31), host, nz)
        plain = _one_update(wl.OracleWm, _cfg(algo), fx.make_params(A, 7), host, nz)
        gap = wl.rel_gap(keyed[0]["train/reward_loss"], plain[0]["train/reward_loss"])
        assert gap > 1e-2, (algo, gap)
    # the KL scales, at a free_nats that clips some rows and not others (wl.KL_FREE_NATS): the logged losses do not
    # move, the gradient does
    over = dict(free_nats=wl.KL_FREE_NATS)
    keyed_o = wl.OracleWm(_cfg("dreamer", kl_dyn_scale=0.5, kl_rep_scale=0.1, **over), A, params=fx.make_params(A, 7))
    plain_o = wl.OracleWm(_cfg("dreamer", **over), A, params=fx.make_params(A, 7))
    ks, ps = keyed_o.update(*host, nz)[2], plain_o.update(*host, nz)[2]
    _, _, pm, pstd, _, qm, qstd = keyed_o.last["observe"]
    klrow = wl._kl_terms(pm, pstd, qm, qstd)[0].reshape(-1)
    clipped = float((klrow <= wl.KL_FREE_NATS).float().mean())
    assert 0.1 < clipped < 0.9, clipped
    assert ks["train/kl_loss"] == ps["train/kl_loss"]
    # on pixels the decoder's gradient is ~1000 times the KL's, so the FLAT model gradient moves by 1.3e-3 only; the prior
    # head's tensors take their gradient from the KL alone and move by 1 - dyn: the per-tensor comparison (5e-3) sees the key
    names = [f"{m}.{k}" for m in fx.MODEL_MODULES for k in keyed_o.p[m]]
    per = {n: float((a - b).norm() / b.norm()) for n, a, b in
           zip(names, keyed_o.last["model_grads"], plain_o.last["model_grads"]) if a is not None}
    prior = {n: v for n, v in per.items() if "prior" in n}
    assert len(prior) == 4 and min(prior.values()) > 0.4, per
    host = _host_batch(60, True, scaled=True)
    for algo in ("repo", "dreamer"):
        over = dict(pixel_obs=False, cnn_activation_function="elu")
        cfg = _cfg(algo, obs_symlog=True, **over)
        params = wl.wm_params(A, cfg, obs=OBS)
        moved = _moved(_one_update(wl.OracleWm, cfg, params, host, nz),
                       _one_update(wl.OracleWm, _cfg(algo, **over), params, host, nz), ["train/obs_loss"])
        assert min(moved.values()) > 1e-2, (algo, moved)


# ----------------------------------------------------------------------------- the config readers
def _ns(**kw):
    return types.SimpleNamespace(pixel_obs=kw.pop("pixel_obs", True), **kw)


def test_reward_dist_config():
    from repo_amd.algorithms.repo.models.decoder import reward_dist_config

    assert reward_dist_config(_ns()) == ("normal", 255, -20.0, 20.0)
    assert reward_dist_config(_ns(reward_dist="twohot", reward_bins=31, reward_bin_low=-5, reward_bin_high=5.0)) == (
        "twohot", 31, -5.0, 5.0)
    for over in ({"reward_dist": "categorical"}, {"reward_bins": 1}, {"reward_bins": 1025}, {"reward_bins": 31.5},
                 {"reward_bins": True}, {"reward_bin_low": 5.0, "reward_bin_high": -5.0}, {"reward_bin_high": float("inf")},
                 {"reward_bin_low": float("nan")}, {"reward_bin_low": "0"}):
        for name in ("normal", "twohot"):      # validated whichever head is asked for
            with pytest.raises(ValueError, match="reward_"):
                reward_dist_config(_ns(**dict({"reward_dist": name}, **over)))


def test_obs_symlog_config():
    from repo_amd.algorithms.repo.dreamer import obs_symlog_config

    assert obs_symlog_config(_ns()) is False and obs_symlog_config(_ns(obs_symlog=False)) is False
    assert obs_symlog_config(_ns(obs_symlog=True, pixel_obs=False)) is True
    with pytest.raises(ValueError, match="obs_symlog"):
        obs_symlog_config(_ns(obs_symlog=True, pixel_obs=True))
    for bad in (1, 0, "yes", None, 1.0):
        with pytest.raises(ValueError, match="obs_symlog"):
            obs_symlog_config(_ns(obs_symlog=bad, pixel_obs=False))


def test_kl_scales_config():
    from repo_amd.algorithms.repo.dreamer import kl_scales_config

    assert kl_scales_config(_ns()) == (False, 1.0, 1.0)
    assert kl_scales_config(_ns(kl_dyn_scale=0.7)) == (True, 0.7, 0.1)
    assert kl_scales_config(_ns(kl_rep_scale=0)) == (True, 0.5, 0.0)
    assert kl_scales_config(_ns(kl_dyn_scale=1, kl_rep_scale=1.0)) == (True, 1.0, 1.0)
    for key in ("kl_dyn_scale", "kl_rep_scale"):
        for bad in (-0.1, float("nan"), float("inf"), "0.5", None, True):
            with pytest.raises(ValueError, match=key):
                kl_scales_config(_ns(**{key: bad}))


def test_sibling_families_carry_the_refusal_flags():
    """The NotImplementedError itself needs a device (the constructors refuse to run without one); what raises it is the
    flag, which every sibling family sets and Dreamer / RePo do not -- except RePo's for the KL scales."""
    from repo_amd.algorithms.repo import TIA, CalibratedRePo, Dreamer, FinetunedRePo, MultitaskDreamer, MultitaskRePo, RePo

    for fam in (TIA, CalibratedRePo, FinetunedRePo, MultitaskDreamer, MultitaskRePo):
        assert not fam._BUILDS_REWARD_DIST and not fam._BUILDS_OBS_SYMLOG and not fam._BUILDS_KL_SCALES, fam
    assert Dreamer._BUILDS_REWARD_DIST and Dreamer._BUILDS_OBS_SYMLOG and Dreamer._BUILDS_KL_SCALES
    assert RePo._BUILDS_REWARD_DIST and RePo._BUILDS_OBS_SYMLOG and not RePo._BUILDS_KL_SCALES


def test_reward_model_wide_head_draws_nothing_from_the_stream():
    from repo_amd.algorithms.repo.models.decoder import RewardModel

    torch.manual_seed(5)
    plain = RewardModel(200, 30, 200, "elu")
    after_plain = torch.rand(3)
    torch.manual_seed(5)
    wide = RewardModel(200, 30, 200, "elu", bins=31)
    after_wide = torch.rand(3)
    assert torch.equal(after_plain, after_wide)
    assert tuple(wide.fc4.weight.shape) == (31, 200) and not wide.fc4.weight.any() and not wide.fc4.bias.any()
    for a, b in zip(plain.plist()[:6], wide.plist()[:6]):
        assert torch.equal(a, b)
