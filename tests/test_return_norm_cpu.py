"""tests/return_norm_ref.py against tests/actor_grad_ref.py's OracleActorGrad and autograd (no GPU), the rank formulas, the
config parsing of repo_amd.algorithms.repo.dreamer.return_norm_config, and the refusals of the five other families: the
restatement is what tests/test_return_norm_gpu.py holds the kernels and the agents to, so each of its pieces is tied here
to something that is not this feature's code.  (The checkpoint round trip needs a constructed agent, and an agent needs a
device: it is in the GPU file.)"""
import math
import types

import numpy as np
import pytest
import torch

from oracle import fixtures as fx
from tests import actor_grad_ref as ag
from tests import return_norm_ref as rn
from tests.test_slow_value_cpu import _relmax, float64_default, to_float64, update64


# ----------------------------------------------------------------------------- 1. ranks, order statistics, the EMA
def test_rank_formulas():
    """k_lo = floor(low (n - 1)), k_hi = ceil(high (n - 1)), written out by hand at n = 1, 2, 20, 21."""
    want = {(1, 0.05, 0.95): (0, 0), (2, 0.05, 0.95): (0, 1), (20, 0.05, 0.95): (0, 19), (21, 0.05, 0.95): (1, 19),
            (1, 0.0, 1.0): (0, 0), (2, 0.0, 1.0): (0, 1), (20, 0.0, 1.0): (0, 19), (21, 0.0, 1.0): (0, 20),
            (21, 0.25, 0.5): (5, 10), (20, 0.25, 0.5): (4, 10), (101, 0.05, 0.95): (5, 95)}
    from repo_amd import ops

    for (n, low, high), k in want.items():
        assert rn.ranks(n, low, high) == k, (n, low, high)
        assert ops.return_ranks(n, low, high) == k, (n, low, high)
        assert 0 <= k[0] <= k[1] <= n - 1
    for n in range(1, 300):   # every valid pair of percentiles gives valid ranks
        for low, high in ((0.0, 1.0), (0.05, 0.95), (0.0, 1e-9), (1.0 - 1e-9, 1.0), (0.49, 0.51)):
            k_lo, k_hi = rn.ranks(n, low, high)
            assert 0 <= k_lo <= k_hi <= n - 1, (n, low, high)


def test_order_stats_are_elements_of_the_array():
    rs = np.random.RandomState(0)
    x = torch.from_numpy(rs.standard_normal(21).astype(np.float32))
    lo, hi = rn.order_stats(x, 1, 19)
    s = sorted(x.tolist())
    assert float(lo) == s[1] and float(hi) == s[19]
    x[3] = float("nan")   # NaNs sort last
    lo, hi = rn.order_stats(x, 0, 20)
    assert float(lo) == min(v for v in x.tolist() if v == v) and math.isnan(float(hi))
    lo, hi = rn.order_stats(x.reshape(3, 7), 0, 19)
    assert float(hi) == max(v for v in x.tolist() if v == v)


def test_ema_scale_and_its_guard():
    st, scale, inv = rn.ema_scale((0.0, 0.0), 1.0, 21.0, 0.75, 1.0)
    assert st == (0.25, 5.25) and scale == 5.0 and inv == 0.2
    st2, scale2, inv2 = rn.ema_scale(st, 1.0, 21.0, 0.75, 1.0)
    assert st2 == (0.4375, 9.1875) and scale2 == 8.75
    assert rn.ema_scale((0.0, 0.0), 0.0, 2.0, 0.75, 1.0)[1:] == (1.0, 1.0)     # the limit: small returns are not scaled up
    for bad in ((float("nan"), 1.0), (0.0, float("nan")), (float("-inf"), 1.0), (0.0, float("inf"))):
        assert rn.ema_scale(st, bad[0], bad[1], 0.75, 1.0) == (st, 5.0, 0.2)
    assert rn.ema_scale(st, 1.0, 21.0, 0.75, 1.0, skip=True) == (st, 5.0, 0.2)
    assert rn.ema_scale((0.0, 0.0), 3.0, 9.0, 0.0, 1.0)[0] == (3.0, 9.0)       # decay 0: the batch statistics themselves


def test_regimes_follow_the_constants():
    assert rn.SEL_PER_TRIP % rn.SEL_THREADS == 0 and rn.SEL_PER_TRIP > rn.SEL_THREADS
    assert [rn.regime(n) for n in (1, rn.SEL_THREADS - 1, rn.SEL_THREADS, rn.SEL_PER_TRIP, rn.SEL_PER_TRIP + 1)] == \
        ["partial-wave", "partial-wave", "one-trip", "one-trip", "stride"]


# ----------------------------------------------------------------------------- 2. the class against OracleActorGrad and autograd
CASES = [("repo", "dynamics", None), ("dreamer", "reinforce", None), ("repo", "both", 0.1), ("dreamer", "both", 0.6)]


def _flat(gs):
    return torch.cat([g.reshape(-1) for g in gs])


@pytest.mark.parametrize("algo,name,mix", CASES)
def test_oracle_multiplies_the_returns_term_and_nothing_else(algo, name, mix):
    """float64.  The actor loss is  inv * L_ret + L_ent  with L_ret = -(m mean(w R) + (1 - m) mean(w logp sg(R - b))) and
    L_ent the two entropy terms; differentiation is linear, so with g_ret the gradient OracleActorGrad forms at zero entropy
    coefficients and g_full the one at the configured ones, the normalised gradient must be inv g_ret + (g_full - g_ret),
    with inv = 1 / max(limit, spread of the two order statistics) held constant -- torch differentiates the oracle's loss,
    and the right-hand side is assembled from a class that knows nothing of this feature.  Two updates: the second starts
    from a non-zero state; the two plain agents are re-created at the normalised agent's point (parameters, dual variable,
    Adam moments) before each."""
    L, B, H, A = 6, 3, 4, 3
    over = {"actor_grad": name}
    if mix is not None:
        over["actor_grad_mix"] = mix
    on = dict(over, return_norm=True, return_norm_decay=0.5, return_norm_limit=1e-3)
    cfg = fx.default_config(algo=algo, batch_size=B, chunk_size=L, horizon=H, **on)
    cfg_full = fx.default_config(algo=algo, batch_size=B, chunk_size=L, horizon=H, **over)
    cfg_ret = fx.default_config(algo=algo, batch_size=B, chunk_size=L, horizon=H, action_ent_coef=0.0, latent_ent_coef=0.0,
                                **over)
    with float64_default():
        agent = to_float64(rn.OracleReturnNorm(cfg, A))
        assert agent.rn_on and (agent.rn_decay, agent.rn_low, agent.rn_high, agent.rn_limit) == (0.5, 0.05, 0.95, 1e-3)
        state = (0.0, 0.0)
        for u in range(2):
            batch, noise = fx.make_batch(L, B, A, seed=5 + u), fx.make_noise(L, B, H, A, seed=50 + u)
            full, ret = to_float64(ag.OracleActorGrad(cfg_full, A)), to_float64(ag.OracleActorGrad(cfg_ret, A))
            for other in (full, ret):   # the same point: parameters, dual variable, Adam moments and step counts
                for m in agent.p:
                    for k, q in agent.p[m].items():
                        other.p[m][k].data.copy_(q.data)
                opts = ["model_opt", "actor_opt", "value_opt"]
                if other.is_repo:
                    other.log_beta.data.copy_(agent.log_beta.data)
                    opts.append("beta_opt")
                for name in opts:
                    src, dst = getattr(agent, name), getattr(other, name)
                    dst.t = src.t
                    dst.m, dst.v = [t.clone() for t in src.m], [t.clone() for t in src.v]
            s_full, s_ret = update64(full, batch, noise), update64(ret, batch, noise)
            got = update64(agent, batch, noise)
            # the statistics: plain elements of the returns every class agrees on
            R = full.last["returns"]
            assert _relmax(agent.last["returns"], R) <= 1e-12
            n = R.numel()
            k_lo, k_hi = rn.ranks(n, 0.05, 0.95)
            srt = sorted(R.reshape(-1).tolist())
            state = (0.5 * state[0] + 0.5 * srt[k_lo], 0.5 * state[1] + 0.5 * srt[k_hi])
            scale = max(1e-3, state[1] - state[0])
            assert scale > 1e-3, "the case is to exercise the spread, not the limit"
            inv = 1.0 / scale
            assert abs(agent.last["return_norm"][2] - inv) <= 1e-12 * inv
            assert abs(got["train/return_scale"] - scale) <= 1e-12 * scale
            assert abs(got["train/return_lo"] - state[0]) <= 1e-12 and abs(got["train/return_hi"] - state[1]) <= 1e-12
            # the gradient and the loss
            g_full, g_ret = _flat(full.last["actor_grads"]), _flat(ret.last["actor_grads"])
            want = inv * g_ret + (g_full - g_ret)
            assert _relmax(_flat(agent.last["actor_grads"]), want) <= 1e-10, u
            assert abs(inv - 1.0) > 0.05 and _relmax(want, g_full) > 1e-3, "the multiplier shows in the gradient"
            l_ret = s_ret["train/actor_loss"]
            want_loss = inv * l_ret + (s_full["train/actor_loss"] - l_ret)
            assert abs(got["train/actor_loss"] - want_loss) <= 1e-10 * abs(want_loss)
            # untouched: the critic's gradients and loss, the entropies, the world model's half
            for g, w in zip(agent.last["value_grads"], full.last["value_grads"]):
                assert _relmax(g, w) <= 1e-10
            for g, w in zip(agent.last["model_grads"], full.last["model_grads"]):
                assert (g is None) == (w is None) and (w is None or _relmax(g, w) <= 1e-10)
            for k in ("train/value_loss", "train/action_entropy", "train/latent_entropy"):
                assert abs(got[k] - s_full[k]) <= 1e-10 * abs(s_full[k]), k


def test_key_off_is_the_actor_grad_oracle():
    L, B, H, A = 6, 3, 4, 3
    cfg = fx.default_config(algo="repo", batch_size=B, chunk_size=L, horizon=H, actor_grad="both")
    with float64_default():
        off, plain = to_float64(rn.OracleReturnNorm(cfg, A)), to_float64(ag.OracleActorGrad(cfg, A))
        assert not off.rn_on
        batch, noise = fx.make_batch(L, B, A, seed=5), fx.make_noise(L, B, H, A, seed=50)
        got, want = update64(off, batch, noise), update64(plain, batch, noise)
        assert got == want and off.rn_state == (0.0, 0.0)
        assert torch.equal(_flat(off.last["actor_grads"]), _flat(plain.last["actor_grads"]))


def test_limit_makes_small_returns_inert():
    """limit = 1 and returns whose spread stays below 1: inv is exactly 1.0, the update is OracleActorGrad's."""
    L, B, H, A = 6, 3, 4, 3
    cfg = fx.default_config(algo="dreamer", batch_size=B, chunk_size=L, horizon=H, return_norm=True)
    with float64_default():
        on, plain = to_float64(rn.OracleReturnNorm(cfg, A)), to_float64(ag.OracleActorGrad(cfg, A))
        batch, noise = fx.make_batch(L, B, A, seed=5), fx.make_noise(L, B, H, A, seed=50)
        got, want = update64(on, batch, noise), update64(plain, batch, noise)
        lo_b, hi_b = on.last["return_norm"][0]
        assert hi_b - lo_b < 1.0 and on.last["return_norm"][1:] == (1.0, 1.0)
        assert all(got[k] == w for k, w in want.items())
        assert torch.equal(_flat(on.last["actor_grads"]), _flat(plain.last["actor_grads"]))
        assert got["train/return_scale"] == 1.0 and got["train/return_hi"] == (1.0 - 0.99) * hi_b


# ----------------------------------------------------------------------------- 3. config parsing and refusals
def test_config_parsing():
    from repo_amd.algorithms.repo.dreamer import return_norm_config

    cfg = types.SimpleNamespace
    assert return_norm_config(cfg()) == (False, 0.99, 0.05, 0.95, 1.0)
    assert return_norm_config(cfg(return_norm=True)) == (True, 0.99, 0.05, 0.95, 1.0)
    assert rn.config(cfg()) == return_norm_config(cfg())[1:]
    got = return_norm_config(cfg(return_norm=True, return_norm_decay=0, return_norm_low=0.0, return_norm_high=1,
                                 return_norm_limit=1e-3))
    assert got == (True, 0.0, 0.0, 1.0, 1e-3)
    bad = [{"return_norm_decay": 1.0}, {"return_norm_decay": -0.1}, {"return_norm_decay": float("nan")},
           {"return_norm_decay": "0.9"}, {"return_norm_decay": True},
           {"return_norm_low": -0.01}, {"return_norm_high": 1.01}, {"return_norm_low": 0.5, "return_norm_high": 0.5},
           {"return_norm_low": 0.6, "return_norm_high": 0.4}, {"return_norm_low": float("nan")},
           {"return_norm_high": None},
           {"return_norm_limit": 0.0}, {"return_norm_limit": -1.0}, {"return_norm_limit": float("nan")},
           {"return_norm_limit": float("inf")}, {"return_norm": 1}, {"return_norm": "yes"}]
    for over in bad:
        with pytest.raises(ValueError, match="return_norm"):
            return_norm_config(cfg(return_norm=True, **over) if "return_norm" not in over else cfg(**over))


@pytest.mark.parametrize("family", ["FinetunedRePo", "CalibratedRePo", "TIA", "MultitaskDreamer", "MultitaskRePo"])
def test_other_families_refuse_before_touching_a_device(family):
    """build_models is the first thing a constructor does with its config, and the refusal is raised ahead of every module:
    called on a bare instance, it needs no device."""
    from repo_amd.algorithms import repo as algos

    cls = getattr(algos, family)
    assert cls._BUILDS_RETURN_NORM is False and algos.Dreamer._BUILDS_RETURN_NORM and algos.RePo._BUILDS_RETURN_NORM
    cfg = fx.default_config(algo="repo", batch_size=4, chunk_size=8, horizon=5, return_norm=True)
    env = types.SimpleNamespace(observation_space=types.SimpleNamespace(shape=(3, 64, 64)),
                                action_space=types.SimpleNamespace(shape=(6,)), num_tasks=3)
    with pytest.raises(NotImplementedError, match="return_norm"):
        cls.build_models(object.__new__(cls), cfg, env)
    cfg_bad = fx.default_config(algo="repo", batch_size=4, chunk_size=8, horizon=5, return_norm_decay=1.5)
    with pytest.raises(ValueError, match="return_norm_decay"):   # a bad value raises whether the key is on or not
        cls.build_models(object.__new__(cls), cfg_bad, env)
