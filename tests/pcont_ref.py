"""config.pcont restated on the CPU (not a test): the continuation predictor of Hafner et al. 2020 in the shapes of this
project.  The reference has no counterpart, so DESIGN.md 6k is the specification and this file is its executable form:

 * `bernoulli_nll`      BCE-with-logits against a soft target, elementwise, in the dtype it is given (float64 in the tests);
 * `weighted_returns`   oracle.repo_oracle.lambda_return plus the cumulative-product weights w_0 = 1, w_t = w_{t-1} d_{t-1};
 * `returns_backward`   the hand-written gradient recursion of repo_lambda_return_disc (include/repo_hip.h), which
                        tests/test_pcont_cpu.py holds to autograd;
 * `OraclePcont`        OracleAgent with the head: its loss in train_dynamics, p in place of gamma and the weights in
                        train_actor_critic.

tests/test_pcont_cpu.py ties the first three to torch's own functions; tests/test_pcont_gpu.py holds the kernels and whole
updates of the HIP agents to all four."""
from collections import OrderedDict

import numpy as np
import torch

from oracle import fixtures as fx
from oracle import repo_oracle as ro

LOG_2PI = ro.LOG_2PI
HEAD_KEYS = [f"fc{i}.{w}" for i in (1, 2, 3, 4) for w in ("weight", "bias")]


def make_pcont_params(belief=200, state=30, hidden=200, seed=23):
    """The head's state dict by the fixtures.make_params recipe: uniform(-k, k), k = fan_in ** -0.5, one RandomState drawn in
    state_dict order, a bias with the bound of the weight before it.  The reward head's shapes."""
    rs = np.random.RandomState(seed)
    shapes = fx.param_shapes(1, belief=belief, state=state, hidden=hidden)["reward_model"]
    out, k = OrderedDict(), 1.0
    for name, shp in shapes.items():
        if len(shp) > 1:
            k = 1.0 / np.sqrt(float(np.prod(shp[1:])))
        out[name] = rs.uniform(-k, k, size=shp).astype(np.float32)
    return out


def bernoulli_nll(logit, target):
    """max(l, 0) - l y + log1p(exp(-|l|)), elementwise: -[y log sigmoid(l) + (1 - y) log(1 - sigmoid(l))] for any y in [0, 1]."""
    return logit.clamp(min=0) - logit * target + torch.log1p(torch.exp(-logit.abs()))


def weighted_returns(rewards, values, discounts, bootstrap, lambda_):
    """-> (returns, weights), both (L', N): the reference's recursion with a discount per element, and
    weights[t] = prod_{s < t} discounts[s] (weights[0] = 1), NOT detached here."""
    returns = ro.lambda_return(rewards, values, discounts, bootstrap, lambda_)
    weights = torch.cumprod(torch.cat([torch.ones_like(discounts[:1]), discounts[:-1]], 0), 0)
    return returns, weights


def returns_backward(rewards, values, p, lambda_, gret, from_logit=False):
    """The gradient of gret * sum_t w_t R_t with w held constant, by the recursion of include/repo_hip.h.
    rewards, values, p: (Hm, N); rows 0..Hm-2 of rewards and p are used.  from_logit: p is sigmoid(logit) and the third
    output is the gradient with respect to that logit.  -> (drewards, dvalues, ddisc), each (Hm, N)."""
    Hm = rewards.shape[0]
    L = Hm - 1
    R, w = weighted_returns(rewards[:-1], values[:-1], p[:-1], values[-1], lambda_)
    dr, dv, dd = torch.zeros_like(rewards), torch.zeros_like(values), torch.zeros_like(p)
    G = torch.zeros_like(rewards[0])
    for t in range(L):
        G = gret * w[t] + (p[t - 1] * lambda_ * G if t > 0 else 0.0)
        dr[t] = G
        dv[t + 1] = dv[t + 1] + p[t] * (1 - lambda_) * G
        if t == L - 1:
            dv[L] = dv[L] + p[t] * lambda_ * G
        r_next = R[t + 1] if t < L - 1 else values[L]
        dp = G * ((1 - lambda_) * values[t + 1] + lambda_ * r_next)
        dd[t] = dp * p[t] * (1 - p[t]) if from_logit else dp
    return dr, dv, dd


class OraclePcont(ro.OracleAgent):
    """OracleAgent with cfg.pcont: `pcont_model` joins model_params behind the reward head (one Adam, one clip).
    const_p: use this constant in place of sigmoid(head) in train_actor_critic; unit_weights: w = 1.  With
    cfg.pcont_scale = 0, const_p = cfg.gamma and unit_weights the class computes what OracleAgent computes."""

    def __init__(self, cfg, action_size, params=None, pcont_params=None, seed=7, const_p=None, unit_weights=False):
        super().__init__(cfg, action_size, params=params, seed=seed)
        assert cfg.algo in ("repo", "dreamer")
        if pcont_params is None:
            pcont_params = make_pcont_params(cfg.belief_size, cfg.state_size, cfg.hidden_size)
        self.p["pcont_model"] = OrderedDict(
            (k, torch.tensor(np.asarray(v), dtype=torch.float32).requires_grad_(True)) for k, v in pcont_params.items())
        self.model_params = self.model_params + list(self.p["pcont_model"].values())
        self.model_opt = ro.Adam(self.model_params, cfg.model_lr)
        self.pcont_scale = float(getattr(cfg, "pcont_scale", 10.0))
        self.const_p, self.unit_weights = const_p, unit_weights

    def train_dynamics(self, obs, actions, rewards, nonterms, eps_prior, eps_post, apply=True):
        c, p = self.c, self.p
        L, B = obs.shape[:2]
        T = L - 1
        embeds = ro.encoder_fwd(p["encoder"], obs.reshape(L * B, *obs.shape[2:])).reshape(L, B, -1)
        b0, s0 = torch.zeros(B, c.belief_size), torch.zeros(B, c.state_size)
        beliefs, prior_s, pm, ps, post_s, qm, qs = ro.observe(
            p["transition_model"], b0, s0, actions[:-1], embeds[1:], nonterms[:-1], eps_prior, eps_post)
        fb, fs = beliefs.reshape(T * B, -1), post_s.reshape(T * B, -1)
        recon = ro.decoder_fwd(p["obs_model"], fb.detach(), fs.detach()) if self.is_repo else ro.decoder_fwd(p["obs_model"], fb, fs)
        recon = recon.reshape(T, B, *obs.shape[2:])
        obs_loss = (0.5 * (recon - obs[1:]) ** 2 + 0.5 * LOG_2PI).sum((2, 3, 4)).mean((0, 1))
        mask = nonterms[:-1].squeeze(-1)
        r_pred = ro.scalar_head(p["reward_model"], fb, fs).reshape(T, B)
        reward_loss = ((0.5 * (r_pred - rewards[:-1].squeeze(-1)) ** 2 + 0.5 * LOG_2PI) * mask).mean((0, 1))
        # the continuation head on the attached latents: soft target gamma * nonterm, mean over all T*B rows, no mask
        logit = ro.scalar_head(p["pcont_model"], fb, fs).reshape(T, B)
        pcont_loss = self.pcont_scale * bernoulli_nll(logit, c.gamma * mask).mean((0, 1))
        out = {}
        if self.is_repo:
            kl_prior = ro.normal_kl(qm.detach(), qs.detach(), pm, ps).sum(2).mean((0, 1))
            kl_post = ro.normal_kl(qm, qs, pm.detach(), ps.detach()).sum(2).mean((0, 1))
            alpha = c.prior_train_steps / (1 + c.prior_train_steps)
            kl_div = alpha * kl_prior + (1 - alpha) * kl_post
            kl_viol = kl_div - c.target_kl
            kl_loss = self.log_beta.exp().detach() * kl_viol
            out["train/kl_div"] = kl_div
        else:
            kl = ro.normal_kl(qm, qs, pm, ps).sum(2)
            kl_loss = torch.max(kl, torch.full((1,), float(c.free_nats))).mean((0, 1))
        model_loss = obs_loss + reward_loss + kl_loss + pcont_loss
        self.model_opt.zero_grad()
        model_loss.backward()
        self.last["model_grads"] = [None if q.grad is None else q.grad.detach().clone() for q in self.model_params]
        self.last["model_total_norm"] = float(ro.clip_grad_norm(self.model_params, c.grad_clip_norm))
        if apply:
            self.model_opt.step()
        out.update({"train/obs_loss": obs_loss, "train/reward_loss": reward_loss, "train/kl_loss": kl_loss,
                    "train/pcont_loss": pcont_loss, "train/model_loss": model_loss})
        if self.is_repo:
            beta_loss = -self.log_beta * kl_viol.detach()
            self.beta_opt.zero_grad()
            beta_loss.backward()
            if apply:
                self.beta_opt.step()
            out["train/beta"] = self.log_beta.exp()
            out["train/beta_loss"] = beta_loss
        self.last["observe"] = [x.detach() for x in (beliefs, prior_s, pm, ps, post_s, qm, qs)]
        return beliefs.detach(), post_s.detach(), {k: float(v.detach()) for k, v in out.items()}

    def train_actor_critic(self, beliefs, post_states, eps_act, eps_prior, eps_ent, apply=True):
        c, p = self.c, self.p
        frozen = self.model_params + self.value_params     # pcont_model included
        for q in frozen:
            q.requires_grad_(False)
        try:
            ib, istate, im, isd = ro.imagine(p["transition_model"], p["actor_model"], beliefs, post_states, c.horizon,
                                             eps_act, eps_prior)
            Hm, N = ib.shape[:2]
            fb, fs = ib.reshape(Hm * N, -1), istate.reshape(Hm * N, -1)
            r_pred = ro.scalar_head(p["reward_model"], fb, fs).reshape(Hm, N)
            v_pred = ro.scalar_head(p["value_model"], fb, fs).reshape(Hm, N)
            if self.const_p is None:
                pc = torch.sigmoid(ro.scalar_head(p["pcont_model"], fb, fs)).reshape(Hm, N)
            else:
                pc = float(self.const_p) * torch.ones_like(r_pred)
        finally:
            for q in frozen:
                q.requires_grad_(True)
        a_mean, a_std = ro.actor_fwd(p["actor_model"], fb, fs)
        action_entropy = ro.tanh_normal_entropy(a_mean, a_std, eps_ent).mean()
        latent_entropy = (0.5 + 0.5 * LOG_2PI + isd.log()).sum(-1).mean()
        # p is NOT multiplied by gamma again; the weights are stop-gradiented, p inside the returns is not
        returns, w = weighted_returns(r_pred[:-1], v_pred[:-1], pc[:-1], v_pred[-1], c.gae_lambda)
        w = torch.ones_like(w) if self.unit_weights else w.detach()
        actor_loss = -(w * returns).mean() - c.action_ent_coef * action_entropy - c.latent_ent_coef * latent_entropy
        self.actor_opt.zero_grad()
        for q in self.model_params + self.value_params:
            q.grad = None
        actor_loss.backward()
        self.last["actor_grads"] = [q.grad.detach().clone() for q in self.actor_params]
        self.last["actor_total_norm"] = float(ro.clip_grad_norm(self.actor_params, c.grad_clip_norm))
        if apply:
            self.actor_opt.step()
        vb, vs = ib[:-1].detach().reshape((Hm - 1) * N, -1), istate[:-1].detach().reshape((Hm - 1) * N, -1)
        v = ro.scalar_head(p["value_model"], vb, vs)
        value_loss = (w.reshape(-1) * (0.5 * (v - returns.detach().reshape(-1)) ** 2 + 0.5 * LOG_2PI)).mean()
        self.value_opt.zero_grad()
        value_loss.backward()
        self.last["value_grads"] = [q.grad.detach().clone() for q in self.value_params]
        self.last["value_total_norm"] = float(ro.clip_grad_norm(self.value_params, c.grad_clip_norm))
        if apply:
            self.value_opt.step()
        self.last["imagine"] = [x.detach() for x in (ib, istate, im, isd)]
        self.last["returns"], self.last["weights"] = returns.detach(), w
        return {"train/actor_loss": float(actor_loss.detach()), "train/value_loss": float(value_loss.detach()),
                "train/action_entropy": float(action_entropy.detach()),
                "train/latent_entropy": float(latent_entropy.detach())}
