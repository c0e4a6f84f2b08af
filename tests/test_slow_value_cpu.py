"""tests/slow_value_ref.py against closed forms and against oracle.repo_oracle.OracleAgent (no GPU): the restatement is what
tests/test_slow_value_gpu.py holds the kernel, FlatAdam's schedule and the agents to, so each of its pieces is tied here
to something that is not this feature's code."""
import contextlib

import numpy as np
import pytest
import torch

from oracle import fixtures as fx
from oracle import repo_oracle as ro
from tests import act_ref as ar
from tests import slow_value_ref as sv


# ----------------------------------------------------------------------------- slow_mix, mixes
@pytest.mark.parametrize("fraction", [1.0, 0.5, 2.0 ** -7, 0.3])
def test_slow_mix_is_the_convex_combination(fraction):
    rs = np.random.RandomState(3)
    t, p = torch.from_numpy(rs.standard_normal(1000)), torch.from_numpy(rs.standard_normal(1000))
    got = sv.slow_mix(t, p, fraction)
    assert got.dtype == torch.float64
    want = (1.0 - fraction) * t + fraction * p
    assert float((got - want).abs().max()) <= 1e-12
    if fraction == 1.0:
        assert torch.equal(got, p) and got.data_ptr() != p.data_ptr()
    t32 = sv.slow_mix(t.float(), p.float(), fraction)
    assert t32.dtype == torch.float32


def test_mixes_against_a_written_out_table():
    table = {1: [1, 2, 3, 4, 5, 6, 7], 2: [2, 4, 6], 100: [100, 200, 300]}
    for every, ks in table.items():
        top = 7 if every < 100 else 301
        assert [k for k in range(0, top + 1) if sv.mixes(k, every)] == ks, every
    assert not sv.mixes(0, 1) and not sv.mixes(99, 100) and not sv.mixes(101, 100)


# ----------------------------------------------------------------------------- the oracle in float64
@contextlib.contextmanager
def float64_default():
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        yield
    finally:
        torch.set_default_dtype(old)


def to_float64(agent):
    """Every parameter, the target and the optimisers' moments of an oracle agent as float64 (in place)."""
    for mod in agent.p.values():
        for q in mod.values():
            q.data = q.data.double()
    if hasattr(agent, "slow"):
        for k in agent.slow:
            agent.slow[k] = agent.slow[k].double()
    opts = [agent.model_opt, agent.actor_opt, agent.value_opt]
    if agent.is_repo:
        agent.log_beta.data = agent.log_beta.data.double()
        opts.append(agent.beta_opt)
    for opt in opts:
        opt.m = [torch.zeros_like(q) for q in opt.params]
        opt.v = [torch.zeros_like(q) for q in opt.params]
    return agent


def update64(agent, batch, noise):
    obs, act, rew, done = batch
    t = {k: torch.from_numpy(v).double() for k, v in noise.items()}
    o = torch.from_numpy(fx.preprocess_u8(obs)).double()
    a, r, nt = torch.from_numpy(act).double(), torch.from_numpy(rew).double(), 1 - torch.from_numpy(done).double()
    beliefs, post, scal = agent.train_dynamics(o, a, r, nt, t["obs_prior"], t["obs_post"])
    scal.update(agent.train_actor_critic(beliefs.flatten(0, 1), post.flatten(0, 1), t["img_act"], t["img_prior"],
                                         t["entropy"]))
    return scal


def _relmax(a, b):
    return float((a - b).abs().max()) / (float(b.abs().max()) + 1e-300)


@pytest.mark.parametrize("algo", ["repo", "dreamer"])
def test_equal_target_is_the_plain_oracle(algo):
    """Target == online head, every = 1, fraction = 1: the target is the online head before every update, so the two heads
    compute the same numbers and the class is OracleAgent -- scalars and all three gradient lists, over two updates."""
    L, B, H, A = 6, 3, 4, 3
    cfg = fx.default_config(algo=algo, batch_size=B, chunk_size=L, horizon=H)
    with float64_default():
        plain = to_float64(ro.OracleAgent(cfg, A))
        slow = to_float64(sv.OracleSlowValue(cfg, A, every=1, fraction=1.0))
        for u in range(2):
            batch, noise = fx.make_batch(L, B, A, seed=5 + u), fx.make_noise(L, B, H, A, seed=50 + u)
            want, got = update64(plain, batch, noise), update64(slow, batch, noise)
            assert got.keys() == want.keys()
            for k, w in want.items():
                assert abs(got[k] - w) <= 1e-10 * abs(w), (u, k, got[k], w)
            for name in ("model_grads", "actor_grads", "value_grads"):
                assert len(slow.last[name]) == len(plain.last[name])
                for g, w in zip(slow.last[name], plain.last[name]):
                    assert (g is None) == (w is None)
                    if w is not None:
                        assert g.dtype == torch.float64 and _relmax(g, w) <= 1e-10, (u, name, tuple(w.shape))
            for k, q in slow.p["value_model"].items():   # fraction 1 after every step: a copy of the stepped head
                assert torch.equal(slow.slow[k], q.detach())


def test_distinct_target_chains_and_schedule():
    """Target from another seed, every = 2, fraction = 0.5, three updates: the value head's weight gradients are those of
    the online chain alone, nothing reaches the transition model or the target, and the target follows the schedule."""
    L, B, H, A = 6, 3, 4, 3
    every, fraction = 2, 0.5
    cfg = fx.default_config(algo="repo", batch_size=B, chunk_size=L, horizon=H)
    with float64_default():
        agent = to_float64(sv.OracleSlowValue(cfg, A, slow_params=sv.make_slow_params(), every=every, fraction=fraction))
        assert not any(torch.equal(agent.slow[k], q.detach()) for k, q in agent.p["value_model"].items())
        want_t = {k: v.clone() for k, v in agent.slow.items()}
        for u in range(3):
            before = {k: q.detach().clone() for k, q in agent.p["value_model"].items()}
            batch, noise = fx.make_batch(L, B, A, seed=5 + u), fx.make_noise(L, B, H, A, seed=50 + u)
            update64(agent, batch, noise)
            # the online chain on its own: the pre-step head on the detached rows against the detached returns
            ib, istate = agent.last["imagine"][:2]
            Hm, N = ib.shape[:2]
            nv = (Hm - 1) * N
            x = torch.cat([ib, istate], 2).reshape(Hm * N, -1)[:nv]
            leaves = {k: v.clone().requires_grad_(True) for k, v in before.items()}
            v = ar.mlp_head(leaves, x, 4, "elu").squeeze(1)
            loss = (0.5 * (v - agent.last["returns"].reshape(-1)) ** 2 + 0.5 * sv.LOG_2PI).mean()
            grads = torch.autograd.grad(loss, list(leaves.values()))
            for g, w in zip(agent.last["value_grads"], grads):
                assert _relmax(g, w) <= 1e-12
            # the returns are the TARGET's: its values and bootstrap row, not the online head's
            assert torch.isfinite(agent.last["returns"]).all()
            assert not torch.allclose(agent.last["v_slow"].reshape(-1)[:nv], agent.last["v_online"], rtol=1e-3, atol=0)
            assert all(q.grad is None for q in agent.p["transition_model"].values())
            assert all(q.grad is None and not q.requires_grad for q in agent.slow.values())
            k_step = agent.value_opt.t
            assert k_step == u + 1
            if sv.mixes(k_step, every):
                want_t = {k: sv.slow_mix(want_t[k], agent.p["value_model"][k].detach(), fraction) for k in want_t}
            assert (k_step == 2) == sv.mixes(k_step, every)
            for k in want_t:
                assert torch.equal(agent.slow[k], want_t[k]), (u, k)


# ----------------------------------------------------------------------------- the GPU oracle test is sharp
@pytest.mark.parametrize("algo", ["repo", "dreamer"])
def test_gpu_case_tells_the_target_from_the_online_head(algo):
    """The first update of tests/test_slow_value_gpu.py's oracle case (same shapes, seeds and target): the distinct-target
    oracle's actor and value losses each differ from the plain oracle's by more than 1e-2 relative, ten times the GPU
    test's scalar bound -- an agent that read the online head would fail there."""
    g = sv.GPU_CASE
    L, B, H, A = g["L"], g["B"], g["H"], g["A"]
    cfg = fx.default_config(algo=algo, batch_size=B, chunk_size=L, horizon=H)
    obs, act, rew, done = fx.make_batch(L, B, A, seed=g["batch_seed"])
    noise = fx.make_noise(L, B, H, A, seed=g["noise_seed"])
    plain = ro.OracleAgent(cfg, A, params=fx.make_params(A, 7)).update(obs, act, rew, done, noise)[2]
    slow = sv.OracleSlowValue(cfg, A, params=fx.make_params(A, 7), slow_params=sv.make_slow_params(),
                              every=g["every"], fraction=g["fraction"]).update(obs, act, rew, done, noise)[2]
    for k in ("train/actor_loss", "train/value_loss"):
        rel = abs(slow[k] - plain[k]) / abs(plain[k])
        assert rel > 1e-2, (algo, k, slow[k], plain[k], rel)
    for k in ("train/model_loss", "train/action_entropy", "train/latent_entropy"):   # what the target does not touch
        assert abs(slow[k] - plain[k]) <= 1e-6 * abs(plain[k]), (k, slow[k], plain[k])
