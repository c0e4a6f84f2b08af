"""config.return_norm restated on the CPU (not a test): DreamerV3's return normalisation (Hafner et al. 2023) in the shapes
of this project.  The reference has no counterpart, so DESIGN.md 6n is the specification and this file is its executable
form:

 * `ranks`            (n, low, high) -> the 0-based ranks k_lo = floor(low (n - 1)), k_hi = ceil(high (n - 1));
 * `order_stats`      the k_lo-th and k_hi-th smallest element by torch.sort: no interpolation;
 * `ema_scale`        the guard, the running average, scale = max(limit, hi - lo) and its inverse, in float64;
 * `SEL_THREADS`, `SEL_PER_TRIP`, `regime`   repo_return_scale's one workgroup (csrc/select.hip: kSelThreads, kSelThreads *
                      kSelUnroll) and the regime of its walk at a size -- the GPU suite checks the two constants against
                      repo_return_scale_geometry() and derives its sizes from them;
 * `OracleReturnNorm` tests/actor_grad_ref.py's OracleActorGrad with the returns term of the actor objective times sg(inv);
 * `OracleReturnNormSlowPcont`   the same on OracleActorGradSlowPcont (pcont and the slow value target on).

tests/test_return_norm_cpu.py ties the class to OracleActorGrad and autograd; tests/test_return_norm_gpu.py holds the
kernels and whole updates of the HIP agents to this file."""
import math

import torch

from oracle import repo_oracle as ro
from tests import act_ref as ar
from tests import actor_grad_ref as ag
from tests import pcont_ref as pr
from tests import slow_value_ref as sv

LOG_2PI = ro.LOG_2PI
SEL_THREADS = 1024            # kSelThreads: the one workgroup of repo_return_scale
SEL_PER_TRIP = 4 * 1024       # kSelThreads * kSelUnroll: elements per trip of its walk over x


def regime(n):
    """How repo_return_scale's walk covers n elements: "partial-wave" (fewer than one element per thread), "one-trip"
    (at most SEL_PER_TRIP, some threads hold several), "stride" (the walk loops)."""
    return "partial-wave" if n < SEL_THREADS else "one-trip" if n <= SEL_PER_TRIP else "stride"


def ranks(n, low, high):
    return int(math.floor(low * (n - 1))), int(math.ceil(high * (n - 1)))


def order_stats(x, k_lo, k_hi):
    """The k_lo-th and k_hi-th smallest element of x (0-based), NaNs last (torch.sort's order)."""
    s = torch.sort(x.reshape(-1)).values
    return s[k_lo], s[k_hi]


def ema_scale(state, lo_b, hi_b, d, limit, skip=False):
    """state = (lo, hi) -> (new state, scale, inv) in float64.  A non-finite statistic or `skip` leaves the state as it is;
    the scale comes from the state that stands afterwards."""
    lo, hi = float(state[0]), float(state[1])
    lo_b, hi_b, d = float(lo_b), float(hi_b), float(d)
    if math.isfinite(lo_b) and math.isfinite(hi_b) and not skip:
        lo = d * lo + (1.0 - d) * lo_b
        hi = d * hi + (1.0 - d) * hi_b
    scale = max(float(limit), hi - lo)
    return (lo, hi), scale, 1.0 / scale


def config(cfg):
    """(decay, low, high, limit) with the defaults of DESIGN.md 6n."""
    return (float(getattr(cfg, "return_norm_decay", 0.99)), float(getattr(cfg, "return_norm_low", 0.05)),
            float(getattr(cfg, "return_norm_high", 0.95)), float(getattr(cfg, "return_norm_limit", 1.0)))


class _ReturnNorm:
    """tests/actor_grad_ref.py's _ActorGrad.train_actor_critic, line for line, with the running state and the returns term
    of the actor objective multiplied by the (constant) inverse scale.  Everything else -- the value loss, both entropy
    terms, the returns the critic regresses on -- is as there."""

    def _init_return_norm(self, cfg):
        self.rn_on = bool(getattr(cfg, "return_norm", False))
        self.rn_decay, self.rn_low, self.rn_high, self.rn_limit = config(cfg)
        self.rn_state = (0.0, 0.0)

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
        # -- the normalisation: unweighted order statistics of the returns, the running range, a constant multiplier
        inv, scale, batch = 1.0, None, None
        if self.rn_on:
            k_lo, k_hi = ranks(nv, self.rn_low, self.rn_high)
            batch = tuple(float(v) for v in order_stats(returns.detach(), k_lo, k_hi))
            self.rn_state, scale, inv = ema_scale(self.rn_state, batch[0], batch[1], self.rn_decay, self.rn_limit)
        s_mean, s_std, _ = ar.actor_fwd(p["actor_model"], x_seen[:, :D], x_seen[:, D:], "elu")
        logp = ag.score_logprob(s_mean, s_std, eps_act[:L_].reshape(nv, -1)).reshape(L_, N)
        adv = (returns - baseline).detach()
        objective = m * returns + (1.0 - m) * logp * adv
        ret_mean = (w * objective).mean() if pcont else objective.mean()
        actor_loss = -ret_mean * inv - c.action_ent_coef * action_entropy - c.latent_ent_coef * latent_entropy
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
        self.last["return_norm"] = (batch, scale, inv)
        self.last["ret_mean"] = float(ret_mean.detach())
        out = {"train/actor_loss": float(actor_loss.detach()), "train/value_loss": float(value_loss.detach()),
               "train/action_entropy": float(action_entropy.detach()),
               "train/latent_entropy": float(latent_entropy.detach())}
        if m < 1.0:
            out["train/actor_logprob"] = float(logp.detach().mean())
        if self.rn_on:
            out["train/return_scale"] = scale
            out["train/return_lo"], out["train/return_hi"] = self.rn_state
        return out


class OracleReturnNorm(_ReturnNorm, ag.OracleActorGrad):
    """OracleActorGrad with cfg.return_norm and its four keys."""

    def __init__(self, cfg, action_size, params=None, seed=7, mix=None):
        super().__init__(cfg, action_size, params=params, seed=seed, mix=mix)
        self._init_return_norm(cfg)


class OracleReturnNormSlowPcont(_ReturnNorm, ag.OracleActorGradSlowPcont):
    """The same with pcont's weights on the objective (the statistics stay unweighted) and the slow head behind the returns."""

    def __init__(self, cfg, action_size, **kw):
        super().__init__(cfg, action_size, **kw)
        self._init_return_norm(cfg)
