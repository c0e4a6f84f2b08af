"""config.slow_value_target restated on the CPU (not a test): the slow (target) critic of Hafner et al. 2021 in the shapes
of this project.  The reference has no counterpart, so DESIGN.md 6l is the specification and this file is its executable
form:

 * `slow_mix`           t + fraction * (p - t), elementwise, in the dtype it is given; fraction == 1 gives p itself;
 * `mixes`              whether the value optimiser's 1-based step k is a mixing step;
 * `OracleSlowValue`    OracleAgent with a `slow` parameter dict: train_actor_critic builds the lambda-returns from the
                        target, sends the actor's gradient through the target's chain and the critic's loss through the
                        online head, then steps and mixes on the schedule;
 * `OracleSlowValuePcont`  the same override on tests/pcont_ref.py's OraclePcont (the combined configuration).

The override runs the heads and the rollout through tests/act_ref.py, so cfg.dense_activation_function = "relu" is
restated too -- in train_actor_critic only: train_dynamics is the base class's (ELU, pixel frames).
tests/test_slow_value_cpu.py ties the class to OracleAgent; tests/test_slow_value_gpu.py holds the kernel, FlatAdam's
schedule and whole updates of the HIP agents to this file."""
from collections import OrderedDict

import numpy as np
import torch

from oracle import fixtures as fx
from oracle import repo_oracle as ro
from tests import act_ref as ar
from tests import pcont_ref as pr

LOG_2PI = ro.LOG_2PI
HEAD_KEYS = pr.HEAD_KEYS
# the distinct target of the tests: fx.make_params draws the online head from seed 7.  tests/test_slow_value_cpu.py
# checks that with this seed the first update of tests/test_slow_value_gpu.py's oracle case (shapes and seeds below) moves
# train/actor_loss and train/value_loss by more than 1e-2 relative against the plain oracle -- ten times that test's bound
SLOW_SEED = 41
GPU_CASE = dict(L=10, B=5, H=6, A=6, every=2, fraction=0.5, updates=3, batch_seed=60, noise_seed=160)


def make_slow_params(belief=200, state=30, hidden=200, seed=SLOW_SEED):
    """A value head's state dict by the fixtures.make_params recipe (tests/pcont_ref.py, make_pcont_params)."""
    rs = np.random.RandomState(seed)
    shapes = fx.param_shapes(1, belief=belief, state=state, hidden=hidden)["value_model"]
    out, k = OrderedDict(), 1.0
    for name, shp in shapes.items():
        if len(shp) > 1:
            k = 1.0 / np.sqrt(float(np.prod(shp[1:])))
        out[name] = rs.uniform(-k, k, size=shp).astype(np.float32)
    return out


def slow_mix(t, p, fraction):
    """The target after a mixing step: d = p - t, t + fraction * d; fraction == 1 is p itself (a copy, not t + (p - t))."""
    if fraction == 1:
        return p.clone()
    return t + fraction * (p - t)


def mixes(k, every):
    """Does the value optimiser's step with the 1-based count k mix?  (k = 0 is the construction's bit copy.)"""
    return k >= 1 and k % every == 0


class _SlowValue:
    """The override, on whichever oracle class stands behind it in the MRO."""

    def _init_slow(self, cfg, slow_params, every, fraction):
        self.every = int(getattr(cfg, "slow_value_update", 100) if every is None else every)
        self.fraction = float(getattr(cfg, "slow_value_fraction", 1.0) if fraction is None else fraction)
        assert self.every >= 1 and 0.0 < self.fraction <= 1.0
        self.act = getattr(cfg, "dense_activation_function", "elu")
        if slow_params is None:   # the construction's bit copy of the online head
            slow_params = {k: v.detach().numpy() for k, v in self.p["value_model"].items()}
        assert list(slow_params.keys()) == list(self.p["value_model"].keys())
        # never a leaf that requires a gradient: no optimiser holds it, .grad stays None
        self.slow = OrderedDict((k, torch.tensor(np.asarray(v), dtype=torch.float32)) for k, v in slow_params.items())

    def train_actor_critic(self, beliefs, post_states, eps_act, eps_prior, eps_ent, apply=True):
        c, p, act = self.c, self.p, self.act
        pcont = "pcont_model" in p
        frozen = self.model_params + self.value_params
        for q in frozen:
            q.requires_grad_(False)
        try:
            ib, istate, im, isd, _ = ar.imagine(p["transition_model"], p["actor_model"], beliefs, post_states, c.horizon,
                                                eps_act, eps_prior, act, "elu")
            Hm, N = ib.shape[:2]
            nv = (Hm - 1) * N
            x = torch.cat([ib, istate], 2).reshape(Hm * N, -1)
            r_pred = ar.mlp_head(p["reward_model"], x, 4, act).reshape(Hm, N)
            # 1. the target on all Hm * N rows; 3. the returns' values AND bootstrap row are the target's
            v_slow = ar.mlp_head(self.slow, x, 4, act).reshape(Hm, N)
            if pcont and self.const_p is None:
                pc = torch.sigmoid(ar.mlp_head(p["pcont_model"], x, 4, act)).reshape(Hm, N)
            elif pcont:
                pc = float(self.const_p) * torch.ones_like(r_pred)
            else:
                pc = c.gamma * torch.ones_like(r_pred)
        finally:
            for q in frozen:
                q.requires_grad_(True)
        a_mean, a_std, _ = ar.actor_fwd(p["actor_model"], x[:, : ib.shape[2]], x[:, ib.shape[2]:], "elu")
        action_entropy = ro.tanh_normal_entropy(a_mean, a_std, eps_ent).mean()
        latent_entropy = (0.5 + 0.5 * LOG_2PI + isd.log()).sum(-1).mean()
        if pcont:
            returns, w = pr.weighted_returns(r_pred[:-1], v_slow[:-1], pc[:-1], v_slow[-1], c.gae_lambda)
            w = torch.ones_like(w) if self.unit_weights else w.detach()
            ret_mean = (w * returns).mean()
        else:
            returns, w = ro.lambda_return(r_pred[:-1], v_slow[:-1], pc[:-1], v_slow[-1], c.gae_lambda), None
            ret_mean = returns.mean()
        # 4. the actor objective: its gradient reaches the imagined states through the TARGET head's chain
        actor_loss = -ret_mean - c.action_ent_coef * action_entropy - c.latent_ent_coef * latent_entropy
        self.actor_opt.zero_grad()
        for q in self.model_params + self.value_params:
            q.grad = None
        actor_loss.backward()
        self.last["actor_grads"] = [q.grad.detach().clone() for q in self.actor_params]
        self.last["actor_total_norm"] = float(ro.clip_grad_norm(self.actor_params, c.grad_clip_norm))
        if apply:
            self.actor_opt.step()
        # 2. + 5. the ONLINE head on the rows its loss reads, detached inputs, against the detached returns
        v = ar.mlp_head(p["value_model"], x[:nv].detach(), 4, act).squeeze(1)
        nll = 0.5 * (v - returns.detach().reshape(-1)) ** 2 + 0.5 * LOG_2PI
        value_loss = (w.reshape(-1) * nll).mean() if pcont else nll.mean()
        self.value_opt.zero_grad()
        value_loss.backward()
        self.last["value_grads"] = [q.grad.detach().clone() for q in self.value_params]
        self.last["value_total_norm"] = float(ro.clip_grad_norm(self.value_params, c.grad_clip_norm))
        # 6. the value step, and on a mixing step the target's move towards the parameters just written
        if apply:
            self.value_opt.step()
            if mixes(self.value_opt.t, self.every):
                with torch.no_grad():
                    for k, q in p["value_model"].items():
                        self.slow[k] = slow_mix(self.slow[k], q.detach(), self.fraction)
        self.last["imagine"] = [t.detach() for t in (ib, istate, im, isd)]
        self.last["returns"], self.last["v_slow"], self.last["v_online"] = returns.detach(), v_slow.detach(), v.detach()
        return {"train/actor_loss": float(actor_loss.detach()), "train/value_loss": float(value_loss.detach()),
                "train/action_entropy": float(action_entropy.detach()),
                "train/latent_entropy": float(latent_entropy.detach())}


class OracleSlowValue(_SlowValue, ro.OracleAgent):
    """OracleAgent with cfg.slow_value_target.  slow_params: the target's state dict (None: a copy of the online head);
    every / fraction: the schedule (None: cfg's keys, defaults 100 and 1.0)."""

    def __init__(self, cfg, action_size, params=None, slow_params=None, every=None, fraction=None, seed=7):
        super().__init__(cfg, action_size, params=params, seed=seed)
        assert cfg.algo in ("repo", "dreamer")
        self._init_slow(cfg, slow_params, every, fraction)


class OracleSlowValuePcont(_SlowValue, pr.OraclePcont):
    """The same on OraclePcont: sigmoid(pcont head) in place of gamma, its stop-gradiented cumulative product on both losses."""

    def __init__(self, cfg, action_size, params=None, pcont_params=None, slow_params=None, every=None, fraction=None,
                 seed=7, const_p=None, unit_weights=False):
        super().__init__(cfg, action_size, params=params, pcont_params=pcont_params, seed=seed, const_p=const_p,
                         unit_weights=unit_weights)
        self._init_slow(cfg, slow_params, every, fraction)
