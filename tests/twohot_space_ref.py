"""config.value_slow_reg, config.value_bin_space and config.reward_bin_space restated on the CPU (not a test): the slow
critic as a regulariser and the symexp-spaced bins of the revised DreamerV3 (Hafner et al. 2023) in the shapes of this
project.  The reference has no counterpart, so DESIGN.md 6r is the specification and this file is its executable form:

 * `symexp_bins`                    B_k = symexp(b_k) with b_k counted from the middle, so B_{K-1-k} = -B_k for low = -high;
 * `decode`, `decode_bwd`           space "symlog": tests/twohot_ref.py's, untouched.  "symexp": v = sum p B summed in
                                    mirrored pairs, and dz = g p (B - v);
 * `target`                         "symexp": the two-hot weights of clamp(R, B_0, B_{K-1}) between the B_k;
 * `nll`                            the cross-entropy against one target or against two (target_b weighed by reg) with ONE
                                    log-softmax, sums [sum w CE_a, sum w, sum w CE_b], dz = scale w ((p - t_a) + reg (p - t_b));
   all in the dtype of their inputs: the GPU tests pass float64 copies of the float32 operands, and float32 ones to measure
   what float32 arithmetic alone costs;
 * `OracleSpace`, `OracleSpaceSlowPcont`   tests/wm_losses_ref.py's classes with the three keys.

tests/test_twohot_space_cpu.py ties the formulas to autograd and the classes to their parents;
tests/test_twohot_space_gpu.py holds the kernels and whole updates of the HIP agents to this file."""
import contextlib
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

from oracle import repo_oracle as ro
from tests import act_ref as ar
from tests import actor_grad_ref as ag
from tests import pcont_ref as pr
from tests import return_norm_ref as rn
from tests import slow_value_ref as sv
from tests import twohot_ref as th
from tests import wm_losses_ref as wl

LOG_2PI = ro.LOG_2PI
SPACES = ("symlog", "symexp")
symlog, symexp = th.symlog, th.symexp


def symexp_bins(K, low, high, dtype=torch.float64):
    """B_k = symexp(b_k) in `dtype`, b_k = mid + (2k - (K - 1)) (high - low) / (2 (K - 1)) as csrc/twohot.hip counts them: for
    low == -high the mirrored bins are each other's negatives in bits, and the middle bin of an odd K is exactly 0."""
    low, high = float(np.float32(low)), float(np.float32(high))     # the kernels take the bounds as float32
    k = torch.arange(K, dtype=torch.float64)
    b = 0.5 * (low + high) + (2.0 * k - (K - 1)) * ((high - low) / (2.0 * (K - 1)))
    return symexp(b.to(dtype))


def _pair_sum(terms):
    """sum over k of terms[:, k], mirrored pairs first: (terms[K-1-j] + terms[j]) for j < K // 2, the middle bin of an odd K
    alone, then across the pairs."""
    K = terms.shape[1]
    h = K // 2
    pairs = terms[:, K - h:].flip(1) + terms[:, :h]
    out = pairs.sum(1)
    return out + terms[:, h] if K % 2 else out


def decode(z, low, high, space="symlog"):
    """z (rows, K) -> (v, m, p); in "symexp" space m is v."""
    if space == "symlog":
        return th.decode(z, low, high)
    B = symexp_bins(z.shape[1], low, high, z.dtype)
    p = torch.softmax(z, 1)
    v = _pair_sum(p * B)
    return v, v, p


def decode_bwd(z, low, high, g, gmul=1.0, space="symlog"):
    if space == "symlog":
        return th.decode_bwd(z, low, high, g, gmul)
    v, _, p = decode(z, low, high, space)
    B = symexp_bins(z.shape[1], low, high, z.dtype)
    return (g * gmul)[:, None] * p * (B[None, :] - v[:, None])


def target(R, K, low, high, space="symlog"):
    """-> (t (rows, K), pos, k0); "symexp": pos = k0 + t_{k0+1}.  A NaN target gives a NaN row (k0 reported as 0)."""
    if space == "symlog":
        return th.target(R, K, low, high)
    B = symexp_bins(K, low, high, R.dtype)
    bad = torch.isnan(R)
    y = torch.clamp(torch.where(bad, torch.zeros_like(R), R), B[0], B[-1])
    # the bin below y; a y exactly on a bin may take either neighbour: both give the same one-hot row
    k0 = (torch.searchsorted(B, y.contiguous(), right=True) - 1).clamp(0, K - 2)
    f = ((y - B[k0]) / (B[k0 + 1] - B[k0])).clamp(0.0, 1.0)
    t = torch.zeros(R.shape[0], K, dtype=R.dtype)
    t.scatter_(1, k0[:, None], (1.0 - f)[:, None])
    t.scatter_(1, (k0 + 1)[:, None], f[:, None])
    t[bad] = float("nan")
    pos = k0.to(R.dtype) + f
    pos[bad] = float("nan")
    k0 = torch.where(bad, torch.zeros_like(k0), k0)
    return t, pos, k0


def _ce(logp, t, k0):
    """-sum t logp over the two hot columns only (a zero weight of a -inf log-probability must not make a NaN)."""
    hot = torch.stack([logp.gather(1, k0[:, None])[:, 0], logp.gather(1, (k0 + 1)[:, None])[:, 0]], 1)
    tw = torch.stack([t.gather(1, k0[:, None])[:, 0], t.gather(1, (k0 + 1)[:, None])[:, 0]], 1)
    return -(tw * hot).sum(1), hot


def nll(z, R, w, low, high, scale, space="symlog", target_b=None, reg=0.0):
    """-> dict(ce, ce_b, sums (3,), dz (rows, K), pos, pos_b, k0, hot, hot_b).  Without target_b in "symlog" space the first
    two sums and dz are tests/twohot_ref.py's nll, bit for bit."""
    K = z.shape[1]
    if space == "symlog" and target_b is None:
        out = th.nll(z, R, w, low, high, scale)
        out["sums"] = torch.cat([out["sums"], torch.zeros(1, dtype=z.dtype)])
        out["ce_b"] = torch.zeros_like(out["ce"])
        return out
    ww = torch.ones_like(R) if w is None else w
    logp = torch.log_softmax(z, 1)      # once, for both targets
    p = torch.softmax(z, 1)
    t, pos, k0 = target(R, K, low, high, space)
    ce, hot = _ce(logp, t, k0)
    out = dict(ce=ce, pos=pos, k0=k0, hot=hot, logp=logp)
    if target_b is None:
        out["ce_b"] = torch.zeros_like(ce)
        out["dz"] = scale * ww[:, None] * (p - t)
    else:
        tb, pos_b, k0b = target(target_b, K, low, high, space)
        out["ce_b"], out["hot_b"] = _ce(logp, tb, k0b)
        out["pos_b"], out["k0_b"] = pos_b, k0b
        out["dz"] = scale * ww[:, None] * ((p - t) + reg * (p - tb))
    out["sums"] = torch.stack([(ww * ce).sum(), ww.sum(), (ww * out["ce_b"]).sum()])
    return out


def paired_loss(z, R, v_slow, w, low, high, reg, space="symlog"):
    """The critic's loss of DESIGN.md 6r as plain torch, for autograd: mean over rows of w (CE(z; twohot(R)) + reg
    CE(z; twohot(v_slow))) -> (loss, sum w CE_b / sum w)."""
    K = z.shape[1]
    logp = F.log_softmax(z, 1)
    ta, _, _ = target(R, K, low, high, space)
    tb, _, _ = target(v_slow, K, low, high, space)
    ce_a, ce_b = -(ta * logp).sum(1), -(tb * logp).sum(1)
    ww = torch.ones_like(R) if w is None else w
    return (ww * (ce_a + reg * ce_b)).mean(), (ww * ce_b).sum() / ww.sum()


# ----------------------------------------------------------------------------- the oracle classes
def config(cfg):
    """-> (reg, value space, reward space) with the defaults of DESIGN.md 6r, and its ValueErrors."""
    reg = getattr(cfg, "value_slow_reg", 0.0)
    if isinstance(reg, bool) or not isinstance(reg, (int, float)) or not np.isfinite(reg) or reg < 0:
        raise ValueError(f"value_slow_reg={reg!r}: expected a finite float >= 0")
    vs, rs = getattr(cfg, "value_bin_space", "symlog"), getattr(cfg, "reward_bin_space", "symlog")
    for key, s in (("value_bin_space", vs), ("reward_bin_space", rs)):
        if s not in SPACES:
            raise ValueError(f'{key}={s!r}: expected "symlog" or "symexp"')
    if reg > 0 and getattr(cfg, "value_dist", "normal") != "twohot":
        raise ValueError('value_slow_reg needs value_dist="twohot"')
    if vs == "symexp" and getattr(cfg, "value_dist", "normal") != "twohot":
        raise ValueError('value_bin_space="symexp" needs value_dist="twohot"')
    if rs == "symexp" and getattr(cfg, "reward_dist", "normal") != "twohot":
        raise ValueError('reward_bin_space="symexp" needs reward_dist="twohot"')
    return float(reg), vs, rs


class _Space:
    """The three keys on whichever of tests/wm_losses_ref.py's classes stands behind it.  With the keys off every method
    hands over to that class.  The reward head's space reaches the parents' train_dynamics and imagination by standing in for
    tests/wm_losses_ref.py's `reward_loss` and `decode_reward` while they run; the critic's space and its regulariser are
    tests/twohot_ref.py's train_actor_critic restated line for line with `decode`, `target` and the second cross-entropy."""

    def _init_space(self, cfg, slow_params=None):
        self.sp_reg, self.sp_value, self.sp_reward = config(cfg)
        self.sp_on = self.sp_reg > 0.0 or self.sp_value != "symlog" or self.sp_reward != "symlog"
        self.reg_slow = None
        want_target = bool(getattr(cfg, "slow_value_target", False))
        if getattr(self, "slow", None) is None and (want_target or self.sp_reg > 0.0):
            # a slow copy on a class that has none: the returns read it only under slow_value_target
            if slow_params is None:
                slow_params = {k: v.detach().numpy() for k, v in self.p["value_model"].items()}
            copy = OrderedDict((k, torch.tensor(np.asarray(v), dtype=torch.float32)) for k, v in slow_params.items())
            self.every = int(getattr(cfg, "slow_value_update", 100))
            self.fraction = float(getattr(cfg, "slow_value_fraction", 1.0))
            if want_target:
                self.slow = copy
            else:
                self.reg_slow = copy

    def slow_copy(self):
        slow = getattr(self, "slow", None)
        return slow if slow is not None else self.reg_slow

    def set_slow_copy(self, sd):
        copy = self.slow_copy()
        for k in copy:
            copy[k] = sd[k].detach().cpu().clone()

    @contextlib.contextmanager
    def _reward_space(self):
        orig_loss, orig_dec, space = wl.reward_loss, wl.decode_reward, self.sp_reward

        def reward_loss(z, r, mask, low, high):
            out = nll(z, r, mask, low, high, 1.0, space)
            return (mask * out["ce"]).mean(), out["sums"][:2]

        def decode_reward(z, low, high):
            return decode(z, low, high, space)[0]

        wl.reward_loss, wl.decode_reward = reward_loss, decode_reward
        try:
            yield
        finally:
            wl.reward_loss, wl.decode_reward = orig_loss, orig_dec

    def train_dynamics(self, *a, **kw):
        if self.sp_reward == "symlog":
            return super().train_dynamics(*a, **kw)
        with self._reward_space():
            return super().train_dynamics(*a, **kw)

    def _value(self, head, x, act):
        return decode(ar.mlp_head(head, x, 4, act), self.th_low, self.th_high, self.sp_value)[0]

    def train_actor_critic(self, beliefs, post_states, eps_act, eps_prior, eps_ent, apply=True):
        if not self.sp_on:
            return super().train_actor_critic(beliefs, post_states, eps_act, eps_prior, eps_ent, apply=apply)
        with self._reward_space():
            if self.sp_reg == 0.0 and self.sp_value == "symlog":   # the reward head's space alone: the parents' critic
                return super().train_actor_critic(beliefs, post_states, eps_act, eps_prior, eps_ent, apply=apply)
            if self.wm["rd_on"]:
                with self._decoded_reward():
                    return self._space_actor_critic(beliefs, post_states, eps_act, eps_prior, eps_ent, apply)
            return self._space_actor_critic(beliefs, post_states, eps_act, eps_prior, eps_ent, apply)

    def _space_actor_critic(self, beliefs, post_states, eps_act, eps_prior, eps_ent, apply):
        assert self.th_on, "the three keys act on two-hot heads"
        c, p, act, m = self.c, self.p, self.act, self.mix
        pcont = "pcont_model" in p
        slow = getattr(self, "slow", None)
        copy = self.slow_copy()
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
            v_ret = self._value(vhead, x, act).reshape(Hm, N)
            if pcont and self.const_p is None:
                pc = torch.sigmoid(ar.mlp_head(p["pcont_model"], x, 4, act)).reshape(Hm, N)
            elif pcont:
                pc = float(self.const_p) * torch.ones_like(r_pred)
            else:
                pc = c.gamma * torch.ones_like(r_pred)
            x_seen = torch.cat([torch.cat([beliefs, post_states], 1), x[: (L_ - 1) * N]], 0).detach()
            v0 = self._value(vhead, x_seen[:N], act).reshape(1, N)
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
        inv, scale, batch = 1.0, None, None
        if self.rn_on:
            k_lo, k_hi = rn.ranks(nv, self.rn_low, self.rn_high)
            batch = tuple(float(v) for v in rn.order_stats(returns.detach(), k_lo, k_hi))
            self.rn_state, scale, inv = rn.ema_scale(self.rn_state, batch[0], batch[1], self.rn_decay, self.rn_limit)
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
        # the critic: the online head's logits on the detached rows against the two-hot target of the detached returns and,
        # with value_slow_reg, against the two-hot target of the slow copy's DECODED value on the same rows, held constant
        z = ar.mlp_head(p["value_model"], x[:nv].detach(), 4, act)
        lp = F.log_softmax(z, 1)
        t, _, _ = target(returns.detach().reshape(-1), self.th_K, self.th_low, self.th_high, self.sp_value)
        ce = -(t * lp).sum(1)
        total, reg_mean = ce, None
        if self.sp_reg > 0.0:
            with torch.no_grad():
                v_slow = v_ret.detach().reshape(-1)[:nv] if slow is not None else self._value(copy, x[:nv].detach(), act)
            tb, _, _ = target(v_slow, self.th_K, self.th_low, self.th_high, self.sp_value)
            ce_b = -(tb * lp).sum(1)
            total = ce + self.sp_reg * ce_b
            ww = w.reshape(-1) if pcont else torch.ones_like(ce_b)
            reg_mean = float(((ww * ce_b).sum() / ww.sum()).detach())
            self.last["v_slow"] = v_slow.detach()
        value_loss = (w.reshape(-1) * total).mean() if pcont else total.mean()
        self.value_opt.zero_grad()
        value_loss.backward()
        self.last["value_grads"] = [q.grad.detach().clone() for q in self.value_params]
        self.last["value_total_norm"] = float(ro.clip_grad_norm(self.value_params, c.grad_clip_norm))
        if apply:
            self.value_opt.step()
            if copy is not None and sv.mixes(self.value_opt.t, self.every):
                with torch.no_grad():
                    for k, q in p["value_model"].items():
                        copy[k] = sv.slow_mix(copy[k], q.detach(), self.fraction)
        self.last["imagine"] = [t_.detach() for t_ in (ib, istate, im, isd)]
        self.last["returns"], self.last["baseline"], self.last["logp"] = returns.detach(), baseline, logp.detach()
        self.last["weights"] = w
        self.last["values"] = v_ret.detach()
        self.last["return_norm"] = (batch, scale, inv)
        self.last["ret_mean"] = float(ret_mean.detach())
        out = {"train/actor_loss": float(actor_loss.detach()), "train/value_loss": float(value_loss.detach()),
               "train/action_entropy": float(action_entropy.detach()),
               "train/latent_entropy": float(latent_entropy.detach())}
        if reg_mean is not None:
            out["train/value_reg"] = reg_mean
        if m < 1.0:
            out["train/actor_logprob"] = float(logp.detach().mean())
        if self.rn_on:
            out["train/return_scale"] = scale
            out["train/return_lo"], out["train/return_hi"] = self.rn_state
        return out


class OracleSpace(_Space, wl.OracleWm):
    """OracleWm with the three keys; slow_params: the slow copy's state dict (None: a copy of the online head), held when
    cfg.slow_value_target or cfg.value_slow_reg > 0 asks for one."""

    def __init__(self, cfg, action_size, params=None, seed=7, mix=None, slow_params=None):
        super().__init__(cfg, action_size, params=params, seed=seed, mix=mix)
        self._init_space(cfg, slow_params)


class OracleSpaceSlowPcont(_Space, wl.OracleWmSlowPcont):
    """The same on pcont's head and weights, with the slow value head behind the returns, the baseline and the regulariser."""

    def __init__(self, cfg, action_size, **kw):
        super().__init__(cfg, action_size, **kw)
        self._init_space(cfg)
