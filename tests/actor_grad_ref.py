"""config.actor_grad restated on the CPU (not a test): the score-function (REINFORCE) estimator of the actor's gradient of
Hafner et al. 2021, alone or mixed with the gradient through the imagined dynamics, in the shapes of this project.  The
reference has no counterpart, so DESIGN.md 6m is the specification and this file is its executable form:

 * `effective_mix`      (actor_grad, actor_grad_mix) -> m, the weight of the dynamics term;
 * `score_logprob`      log tanh-Normal(tanh(u)) with u = sg(mean + std eps), without the atanh(tanh(u)) round trip, summed
                        over the action dimension, in the dtype it is given (float64 in the tests);
 * `reinforce_grads`    the hand formulas of repo_tanh_normal_reinforce (include/repo_hip.h): dmean, dstd and the two sums;
 * `reinforce_blocks`   that entry point's grid;
 * `OracleActorGrad`    OracleAgent with train_actor_critic per 6m's objective;
 * `OracleActorGradSlowPcont`  the same objective on tests/slow_value_ref.py's OracleSlowValuePcont: baseline and values
                        from the slow head, 6k's weights.

tests/test_actor_grad_cpu.py ties the first three to oracle.repo_oracle and autograd, and the class to OracleAgent;
tests/test_actor_grad_gpu.py holds the kernel and whole updates of the HIP agents to this file."""
import math

import torch

from oracle import repo_oracle as ro
from tests import act_ref as ar
from tests import pcont_ref as pr
from tests import reduce_ref as rr
from tests import slow_value_ref as sv

LOG_2PI = ro.LOG_2PI
NAMES = ("dynamics", "reinforce", "both")


def effective_mix(cfg):
    name = getattr(cfg, "actor_grad", "dynamics")
    assert name in NAMES, name
    return {"dynamics": 1.0, "reinforce": 0.0, "both": float(getattr(cfg, "actor_grad_mix", 0.1))}[name]


def softplus(x):
    """max(x, 0) + log1p(exp(-|x|)): no threshold, finite for every finite x."""
    return x.clamp(min=0) + torch.log1p(torch.exp(-x.abs()))


def score_logprob(mean, std, eps):
    """sum_a [ -0.5 ((u - mean)/std)^2 - log std - 0.5 log 2pi - 2 (log 2 - u - softplus(-2u)) ], u = sg(mean + std eps).
    Holding u constant, autograd gives d/dmean = eps/std and d/dstd = (eps^2 - 1)/std; the log-det term carries none."""
    u = (mean + std * eps).detach()
    z = (u - mean) / std
    return (-0.5 * z * z - std.log() - 0.5 * LOG_2PI - 2.0 * (math.log(2.0) - u - softplus(-2.0 * u))).sum(-1)


def reinforce_grads(mean, std, eps, returns, baseline, weights=None, gscale=1.0):
    """-> (dmean, dstd (rows, A), [sum w adv logp, sum logp], the per-element terms of both sums): the hand formulas."""
    w = torch.ones_like(returns) if weights is None else weights
    wa = (w * (returns - baseline))[:, None]
    u = mean + std * eps
    lp = -0.5 * eps * eps - std.log() - 0.5 * LOG_2PI - 2.0 * (math.log(2.0) - u - softplus(-2.0 * u))
    dmean = gscale * wa * eps / std
    dstd = gscale * wa * (eps * eps - 1.0) / std
    return dmean, dstd, torch.stack([(wa * lp).sum(), lp.sum()]), (wa * lp, lp)


def reinforce_blocks(rows, A):             # repo_tanh_normal_reinforce: one thread per element
    return rr.red_blocks(rows * A, 256)


class _ActorGrad:
    """The override, on whichever oracle class stands behind it in the MRO.  `slow` (tests/slow_value_ref.py) and a
    "pcont_model" entry are used when the class behind has them.  freeze = False leaves the world model and the critic
    attached during the actor's backward and records what reaches them in last["other_grads"] (the CPU tests)."""
    freeze = True

    def _init_actor_grad(self, cfg, mix):
        self.mix = effective_mix(cfg) if mix is None else float(mix)
        assert 0.0 <= self.mix <= 1.0
        if not hasattr(self, "act"):
            self.act = getattr(cfg, "dense_activation_function", "elu")

    def train_actor_critic(self, beliefs, post_states, eps_act, eps_prior, eps_ent, apply=True):
        c, p, act, m = self.c, self.p, self.act, self.mix
        pcont = "pcont_model" in p
        slow = getattr(self, "slow", None)
        vhead = slow if slow is not None else p["value_model"]
        frozen = (self.model_params + self.value_params) if self.freeze else []
        for q in frozen:
            q.requires_grad_(False)
        try:
            ib, istate, im, isd, _ = ar.imagine(p["transition_model"], p["actor_model"], beliefs, post_states, c.horizon,
                                                eps_act, eps_prior, act, "elu")
            Hm, N = ib.shape[:2]
            L_, D = Hm - 1, ib.shape[2]
            nv = L_ * N
            x = torch.cat([ib, istate], 2).reshape(Hm * N, -1)
            r_pred = ar.mlp_head(p["reward_model"], x, 4, act).reshape(Hm, N)
            v_ret = ar.mlp_head(vhead, x, 4, act).reshape(Hm, N)
            if pcont and self.const_p is None:
                pc = torch.sigmoid(ar.mlp_head(p["pcont_model"], x, 4, act)).reshape(Hm, N)
            elif pcont:
                pc = float(self.const_p) * torch.ones_like(r_pred)
            else:
                pc = c.gamma * torch.ones_like(r_pred)
            # the states the actor SAW at steps 0..L'-1: the start states, then imag[0..L'-2]; the baseline is the returns'
            # head on them (slot 0 is the one forward the returns do not already hold)
            x_seen = torch.cat([torch.cat([beliefs, post_states], 1), x[: (L_ - 1) * N]], 0).detach()
            v0 = ar.mlp_head(vhead, x_seen[:N], 4, act).reshape(1, N)
            baseline = torch.cat([v0, v_ret[: L_ - 1]], 0).detach()
        finally:
            for q in frozen:
                q.requires_grad_(True)
        a_mean, a_std, _ = ar.actor_fwd(p["actor_model"], x[:, :D], x[:, D:], "elu")
        action_entropy = ro.tanh_normal_entropy(a_mean, a_std, eps_ent).mean()
        latent_entropy = (0.5 + 0.5 * LOG_2PI + isd.log()).sum(-1).mean()
        if pcont:
            returns, w = pr.weighted_returns(r_pred[:-1], v_ret[:-1], pc[:-1], v_ret[-1], c.gae_lambda)
            w = torch.ones_like(w) if self.unit_weights else w.detach()
        else:
            returns, w = ro.lambda_return(r_pred[:-1], v_ret[:-1], pc[:-1], v_ret[-1], c.gae_lambda), None
        # the score-function term: the actor head on the (detached) states it saw, the rollout's own action noise
        s_mean, s_std, _ = ar.actor_fwd(p["actor_model"], x_seen[:, :D], x_seen[:, D:], "elu")
        logp = score_logprob(s_mean, s_std, eps_act[:L_].reshape(nv, -1)).reshape(L_, N)
        adv = (returns - baseline).detach()
        objective = m * returns + (1.0 - m) * logp * adv
        ret_mean = (w * objective).mean() if pcont else objective.mean()
        actor_loss = -ret_mean - c.action_ent_coef * action_entropy - c.latent_ent_coef * latent_entropy
        self.actor_opt.zero_grad()
        others = self.model_params + self.value_params
        for q in others:
            q.grad = None
        actor_loss.backward()
        self.last["actor_grads"] = [q.grad.detach().clone() for q in self.actor_params]
        self.last["other_grads"] = [None if q.grad is None else q.grad.detach().clone() for q in others]
        self.last["actor_total_norm"] = float(ro.clip_grad_norm(self.actor_params, c.grad_clip_norm))
        if apply:
            self.actor_opt.step()
        # the critic: unchanged -- the online head on the detached rows against the same detached returns
        v = ar.mlp_head(p["value_model"], x[:nv].detach(), 4, act).squeeze(1)
        nll = 0.5 * (v - returns.detach().reshape(-1)) ** 2 + 0.5 * LOG_2PI
        value_loss = (w.reshape(-1) * nll).mean() if pcont else nll.mean()
        self.value_opt.zero_grad()
        value_loss.backward()
        self.last["value_grads"] = [q.grad.detach().clone() for q in self.value_params]
        self.last["value_total_norm"] = float(ro.clip_grad_norm(self.value_params, c.grad_clip_norm))
        if apply:
            self.value_opt.step()
            if slow is not None and sv.mixes(self.value_opt.t, self.every):
                with torch.no_grad():
                    for k, q in p["value_model"].items():
                        self.slow[k] = sv.slow_mix(self.slow[k], q.detach(), self.fraction)
        self.last["imagine"] = [t.detach() for t in (ib, istate, im, isd)]
        self.last["returns"], self.last["baseline"], self.last["logp"] = returns.detach(), baseline, logp.detach()
        self.last["weights"] = w
        self.last["score_inputs"] = (x_seen, s_mean.detach(), s_std.detach())
        out = {"train/actor_loss": float(actor_loss.detach()), "train/value_loss": float(value_loss.detach()),
               "train/action_entropy": float(action_entropy.detach()),
               "train/latent_entropy": float(latent_entropy.detach())}
        if m < 1.0:
            out["train/actor_logprob"] = float(logp.detach().mean())
        return out


class OracleActorGrad(_ActorGrad, ro.OracleAgent):
    """OracleAgent with cfg.actor_grad / cfg.actor_grad_mix (mix: overrides the effective m)."""

    def __init__(self, cfg, action_size, params=None, seed=7, mix=None):
        super().__init__(cfg, action_size, params=params, seed=seed)
        assert cfg.algo in ("repo", "dreamer")
        self._init_actor_grad(cfg, mix)


class OracleActorGradSlowPcont(_ActorGrad, sv.OracleSlowValuePcont):
    """The same objective with sigmoid(pcont head) in place of gamma, its stop-gradiented cumulative product as the weights,
    and the slow head for the returns' values AND the baseline."""

    def __init__(self, cfg, action_size, params=None, pcont_params=None, slow_params=None, every=None, fraction=None,
                 seed=7, const_p=None, unit_weights=False, mix=None):
        super().__init__(cfg, action_size, params=params, pcont_params=pcont_params, slow_params=slow_params, every=every,
                         fraction=fraction, seed=seed, const_p=const_p, unit_weights=unit_weights)
        self._init_actor_grad(cfg, mix)
