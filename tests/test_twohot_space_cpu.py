"""tests/twohot_space_ref.py against autograd, tests/twohot_ref.py and tests/wm_losses_ref.py's classes (no GPU), the config
parsing of repo_amd.algorithms.repo.dreamer.twohot_space_config, and the refusals of the five other families: the
restatement is what tests/test_twohot_space_gpu.py holds the kernels and the agents to, so each of its pieces is tied here to
something that is not this feature's code."""
import math
import types

import numpy as np
import pytest
import torch

from oracle import fixtures as fx
from tests import twohot_ref as th
from tests import twohot_space_ref as ts
from tests import wm_losses_ref as wl
from tests.test_slow_value_cpu import _relmax

F64 = torch.float64
SHAPES = [(2, -1.0, 1.0), (3, -2.0, 2.0), (31, -5.0, 5.0), (255, -20.0, 20.0), (64, -3.0, 12.0)]


def _logits(rows, K, seed, scale=3.0):
    return torch.from_numpy(np.random.RandomState(seed).standard_normal((rows, K)) * scale).to(F64)


# ----------------------------------------------------------------------------- 1. hand formulas against autograd
@pytest.mark.parametrize("K,low,high", SHAPES)
def test_symexp_decode_is_the_expectation_and_its_reverse_the_derivative(K, low, high):
    z = _logits(7, K, K).requires_grad_(True)
    g = torch.from_numpy(np.random.RandomState(1).standard_normal(7)).to(F64)
    B = ts.symexp(th.bins(K, low, high))            # tests/twohot_ref.py's bins, not this file's
    want_v = (torch.softmax(z, 1) * B).sum(1)
    (want_v * g).sum().backward()
    v, m, p = ts.decode(z.detach(), low, high, "symexp")
    assert _relmax(v, want_v.detach()) <= 1e-12 and torch.equal(v, m)
    got = ts.decode_bwd(z.detach(), low, high, g, space="symexp")
    assert _relmax(got, z.grad) <= 1e-12
    assert _relmax(ts.decode_bwd(z.detach(), low, high, g, gmul=0.25, space="symexp"), 0.25 * z.grad) <= 1e-12
    assert float(z.grad.abs().max()) > 0


@pytest.mark.parametrize("K", [2, 3, 255, 256])
def test_symexp_bins_mirror_in_bits_and_equal_logits_decode_to_zero(K):
    for dtype in (torch.float32, F64):
        B = ts.symexp_bins(K, -20.0, 20.0, dtype)
        assert torch.equal(B.flip(0), -B)
        z = torch.full((3, K), 0.7, dtype=dtype)
        v, _, _ = ts.decode(z, -20.0, 20.0, "symexp")
        assert torch.equal(v, torch.zeros(3, dtype=dtype))


@pytest.mark.parametrize("space", ts.SPACES)
@pytest.mark.parametrize("K,low,high", SHAPES)
def test_paired_ce_gradient_is_autograds(K, low, high, space):
    rs = np.random.RandomState(K)
    rows, reg, scale = 9, 0.7, 0.37
    z = _logits(rows, K, K + 1).requires_grad_(True)
    Ra = torch.from_numpy(rs.standard_normal(rows) * 50.0).to(F64)
    Rb = torch.from_numpy(rs.standard_normal(rows) * 5.0).to(F64)
    # a target exactly on a bin, in either space: the whole weight sits on that bin
    Bk = ts.symexp(th.bins(K, low, high))
    Ra[0] = Bk[K // 2]
    Rb[1] = Bk[min(1, K - 1)]
    w = torch.from_numpy(rs.uniform(0.1, 1.0, rows)).to(F64)
    lp = torch.log_softmax(z, 1)
    ta, _, _ = ts.target(Ra, K, low, high, space)
    tb, _, _ = ts.target(Rb, K, low, high, space)
    assert abs(float(ta[0, K // 2]) - 1.0) <= 1e-12 and abs(float(tb[1, min(1, K - 1)]) - 1.0) <= 1e-12
    assert float((ta.sum(1) - 1.0).abs().max()) <= 1e-15 and float(ta.min()) >= 0.0 and int((ta != 0).sum(1).max()) <= 2
    ce_a, ce_b = -(ta * lp).sum(1), -(tb * lp).sum(1)
    (scale * (w * (ce_a + reg * ce_b)).sum()).backward()
    out = ts.nll(z.detach(), Ra, w, low, high, scale, space, target_b=Rb, reg=reg)
    assert _relmax(out["dz"], z.grad) <= 1e-12
    assert _relmax(out["ce"], ce_a.detach()) <= 1e-12 and _relmax(out["ce_b"], ce_b.detach()) <= 1e-12
    want = torch.stack([(w * ce_a.detach()).sum(), w.sum(), (w * ce_b.detach()).sum()])
    assert _relmax(out["sums"], want) <= 1e-12
    # the plain-torch loss the oracle differentiates is the same function
    loss, reg_mean = ts.paired_loss(z.detach(), Ra, Rb, w, low, high, reg, space)
    assert abs(float(loss) - float((w * (ce_a + reg * ce_b)).mean().detach())) <= 1e-12 * abs(float(loss))
    assert abs(float(reg_mean) - float(want[2] / want[1])) <= 1e-12 * abs(float(reg_mean))
    # reg = 0 leaves the unpaired gradient
    one = ts.nll(z.detach(), Ra, w, low, high, scale, space)
    zero = ts.nll(z.detach(), Ra, w, low, high, scale, space, target_b=Rb, reg=0.0)
    assert torch.equal(one["dz"], zero["dz"]) and torch.equal(one["sums"][:2], zero["sums"][:2])
    assert float(one["sums"][2]) == 0.0


def test_symexp_target_specials():
    K, low, high = 31, -5.0, 5.0
    B = ts.symexp_bins(K, low, high)
    R = torch.tensor([float("inf"), float("-inf"), 1e30, -1e30, 0.0, -0.0, float("nan"), 5e-324], dtype=F64)
    t, pos, k0 = ts.target(R, K, low, high, "symexp")
    assert float(t[0, K - 1]) == 1.0 and float(t[2, K - 1]) == 1.0 and float(t[1, 0]) == 1.0 and float(t[3, 0]) == 1.0
    assert float(t[4, 15]) == 1.0 and torch.equal(t[4], t[5]) and abs(float(t[7, 15]) - 1.0) <= 1e-300
    assert torch.isfinite(t[:6]).all() and torch.isnan(t[6]).all() and int(k0.max()) <= K - 2
    # the mean of the two-hot weights over the B_k is the clamped target itself: the encoding is the inverse of the decode
    y = torch.from_numpy(np.random.RandomState(3).uniform(float(B[0]), float(B[-1]), 300)).to(F64)
    t, _, _ = ts.target(y, K, low, high, "symexp")
    assert float(((t * B).sum(1) - y).abs().max()) <= 1e-12 * float(B[-1])
    for k in range(K):   # on every bin, and one float64 step to either side of it
        tk, _, _ = ts.target(torch.stack([torch.nextafter(B[k], -B[-1] * 2), B[k], torch.nextafter(B[k], B[-1] * 2)]),
                             K, low, high, "symexp")
        assert float((tk[:, k] - 1.0).abs().max()) <= 1e-12


# ----------------------------------------------------------------------------- 2. keys off: tests/twohot_ref.py in bits
@pytest.mark.parametrize("dtype", [torch.float32, F64])
def test_symlog_space_is_twohot_ref_in_bits(dtype):
    K, low, high, rows = 31, -5.0, 5.0, 11
    rs = np.random.RandomState(5)
    z = _logits(rows, K, 5).to(dtype)
    R = torch.from_numpy(rs.standard_normal(rows) * 50.0).to(dtype)
    w = torch.from_numpy(rs.uniform(0.1, 1.0, rows)).to(dtype)
    g = torch.from_numpy(rs.standard_normal(rows)).to(dtype)
    for a, b in zip(ts.decode(z, low, high), th.decode(z, low, high)):
        assert torch.equal(a, b)
    assert torch.equal(ts.decode_bwd(z, low, high, g, 0.25), th.decode_bwd(z, low, high, g, 0.25))
    for a, b in zip(ts.target(R, K, low, high), th.target(R, K, low, high)):
        assert torch.equal(a, b)
    a, b = ts.nll(z, R, w, low, high, 0.37), th.nll(z, R, w, low, high, 0.37)
    assert torch.equal(a["dz"], b["dz"]) and torch.equal(a["ce"], b["ce"]) and torch.equal(a["sums"][:2], b["sums"])
    assert float(a["sums"][2]) == 0.0


# ----------------------------------------------------------------------------- 3. the classes
BASE = dict(algo="repo", batch_size=5, chunk_size=10, horizon=6, value_dist="twohot", value_bins=31, value_bin_low=-5.0,
            value_bin_high=5.0)
LBHA = (10, 5, 6, 6)


def _update(cls, over, **kw):
    L, B, H, A = LBHA
    cfg = fx.default_config(**dict(BASE, **over))
    K = cfg.value_bins
    rK = cfg.reward_bins if getattr(cfg, "reward_dist", "normal") == "twohot" else None
    oracle = cls(cfg, A, params=wl.wm_params(A, cfg, reward_K=rK, value_K=K), **kw)
    host, nz = fx.make_batch(L, B, A, seed=60), fx.make_noise(L, B, H, A, seed=160)
    return oracle, oracle.update(*host, nz)[2]


@pytest.fixture(scope="module")
def unkeyed():
    return _update(wl.OracleWm, {})[1]


def test_keys_off_is_the_parent_class_in_bits(unkeyed):
    oracle, got = _update(ts.OracleSpace, dict(value_slow_reg=0.0, value_bin_space="symlog", reward_bin_space="symlog"))
    assert not oracle.sp_on and oracle.slow_copy() is None
    assert got == unkeyed


@pytest.mark.parametrize("over", [dict(value_slow_reg=1.0, slow_value_update=1, slow_value_fraction=0.02),
                                  dict(value_slow_reg=1.0, slow_value_target=True, slow_value_update=1,
                                       slow_value_fraction=0.02),
                                  dict(value_bin_space="symexp")])
def test_gpu_case_sees_each_value_key(unkeyed, over):
    """The GPU suite's whole-update case: with the key on train/value_loss lies more than 1e-2 from the unkeyed oracle's, ten
    times that test's bound -- an agent that ignored the key could not pass it."""
    slow = th.make_twohot_value_params(31, seed=th.TWOHOT_SLOW_SEED)
    oracle, got = _update(ts.OracleSpace, over, slow_params=slow if "value_slow_reg" in over else None)
    assert oracle.sp_on and all(np.isfinite(v) for v in got.values())
    assert abs(got["train/value_loss"] - unkeyed["train/value_loss"]) > 1e-2, (got, unkeyed)
    if "value_slow_reg" in over:
        assert got["train/value_reg"] > 1e-2 and oracle.slow_copy() is not None
        assert (getattr(oracle, "slow", None) is not None) == bool(over.get("slow_value_target", False))


def test_gpu_case_sees_the_reward_key():
    rew = dict(reward_dist="twohot", reward_bins=31, reward_bin_low=-5.0, reward_bin_high=5.0)
    _, off = _update(wl.OracleWm, rew)
    _, on = _update(ts.OracleSpace, dict(rew, reward_bin_space="symexp"))
    # (the fixtures' rewards are small, where symexp is close to linear: the encoding moves train/reward_loss by 4e-3 only;
    # the decoded imagined rewards, spread over bins up to symexp(5), move the actor's returns by far more)
    assert on["train/reward_loss"] != off["train/reward_loss"]
    assert abs(on["train/actor_loss"] - off["train/actor_loss"]) > 1e-2, (on, off)


# ----------------------------------------------------------------------------- 4. config parsing and refusals
def test_config_parsing():
    from repo_amd.algorithms.repo.dreamer import twohot_space_config

    cfg = types.SimpleNamespace
    two = dict(value_dist="twohot", reward_dist="twohot")
    assert twohot_space_config(cfg()) == (0.0, "symlog", "symlog") == ts.config(cfg())
    assert twohot_space_config(cfg(value_slow_reg=0, value_bin_space="symlog", reward_bin_space="symlog")) == \
        (0.0, "symlog", "symlog")
    got = twohot_space_config(cfg(value_slow_reg=np.float32(0.5), value_bin_space="symexp", **two))
    assert got == (0.5, "symexp", "symlog") == ts.config(cfg(value_slow_reg=0.5, value_bin_space="symexp", **two))
    assert twohot_space_config(cfg(reward_bin_space="symexp", reward_dist="twohot")) == (0.0, "symlog", "symexp")
    assert twohot_space_config(cfg(value_slow_reg=2, **two))[0] == 2.0
    bad = [("value_slow_reg", dict(value_slow_reg=-1.0)), ("value_slow_reg", dict(value_slow_reg=float("nan"))),
           ("value_slow_reg", dict(value_slow_reg=float("inf"))), ("value_slow_reg", dict(value_slow_reg=True)),
           ("value_slow_reg", dict(value_slow_reg="1")), ("value_slow_reg", dict(value_slow_reg=None)),
           ("value_bin_space", dict(value_bin_space="linear")), ("value_bin_space", dict(value_bin_space=None)),
           ("value_bin_space", dict(value_bin_space=1)), ("reward_bin_space", dict(reward_bin_space="SYMEXP")),
           ("reward_bin_space", dict(reward_bin_space=True))]
    for key, over in bad:
        for dist in ({}, two):      # a bad value raises whichever head is asked for
            with pytest.raises(ValueError, match=key):
                twohot_space_config(cfg(**dict(dist, **over)))
    # the keys need their two-hot head: the message names both keys
    with pytest.raises(ValueError, match="value_slow_reg.*value_dist"):
        twohot_space_config(cfg(value_slow_reg=1.0))
    with pytest.raises(ValueError, match="value_slow_reg.*value_dist"):
        twohot_space_config(cfg(value_slow_reg=1.0, value_dist="normal", reward_dist="twohot"))
    with pytest.raises(ValueError, match="value_bin_space.*value_dist"):
        twohot_space_config(cfg(value_bin_space="symexp", reward_dist="twohot"))
    with pytest.raises(ValueError, match="reward_bin_space.*reward_dist"):
        twohot_space_config(cfg(reward_bin_space="symexp", value_dist="twohot"))
    for over in (dict(value_slow_reg=1.0), dict(value_bin_space="symexp"), dict(reward_bin_space="symexp")):
        with pytest.raises(ValueError):
            ts.config(cfg(**over))
    assert math.isclose(ts.config(cfg(value_slow_reg=1.0, **two))[0], 1.0)


@pytest.mark.parametrize("key,over", [("value_slow_reg", dict(value_slow_reg=1.0)),
                                      ("value_bin_space", dict(value_bin_space="symexp")),
                                      ("reward_bin_space", dict(reward_bin_space="symexp"))])
@pytest.mark.parametrize("family", ["FinetunedRePo", "CalibratedRePo", "TIA", "MultitaskDreamer", "MultitaskRePo"])
def test_other_families_refuse_before_touching_a_device(family, key, over):
    """build_models is the first thing a constructor does with its config, and the refusal is raised ahead of every module:
    called on a bare instance, it needs no device."""
    from repo_amd.algorithms import repo as algos

    cls = getattr(algos, family)
    for flag in ("_BUILDS_VALUE_SLOW_REG", "_BUILDS_BIN_SPACE"):
        assert getattr(cls, flag) is False and getattr(algos.Dreamer, flag) and getattr(algos.RePo, flag)
    cfg = fx.default_config(algo="repo", batch_size=4, chunk_size=8, horizon=5, **over)
    env = types.SimpleNamespace(observation_space=types.SimpleNamespace(shape=(3, 64, 64)),
                                action_space=types.SimpleNamespace(shape=(6,)), num_tasks=3)
    with pytest.raises(NotImplementedError, match=key):
        cls.build_models(object.__new__(cls), cfg, env)
    bad = {"value_slow_reg": -1.0} if key == "value_slow_reg" else {key: "linear"}
    with pytest.raises(ValueError, match=key):   # a bad value raises in every family
        cls.build_models(object.__new__(cls), fx.default_config(algo="repo", batch_size=4, chunk_size=8, horizon=5, **bad),
                         env)
