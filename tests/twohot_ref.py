"""config.value_dist = "twohot" restated on the CPU (not a test): DreamerV3's two-hot symlog critic (Hafner et al. 2023) in
the shapes of this project.  The reference has no counterpart, so DESIGN.md 6o is the specification and this file is its
executable form:

 * `symlog`, `symexp`, `bins`       the transform pair and b_k = low + k delta, delta = (high - low) / (K - 1);
 * `decode`                         p = softmax(z), m = sum p b, v = symexp(m);
 * `decode_bwd`                     dz_k = g (|v| + 1) p_k (b_k - m), the hand formula of dv / dz;
 * `target`                         the two-hot weights of clamp(symlog(R), low, high), with pos and k0;
 * `nll`                            CE = -sum t log_softmax(z), its weighted sums and dz = scale w (p - t);
   all in the dtype of their inputs: the GPU tests pass float64 copies of the float32 operands;
 * `ROWS_PER_BLOCK`, `LAST_BLOCK_MAX_GRID`, `MAX_BLOCKS`, `regime`   csrc/twohot.hip's launch shape (the GPU suite checks
                                    the constants against repo_twohot_geometry() and derives its row counts from them);
 * `make_twohot_value_params`       a value head with K outputs and a NON-zero last layer, by the fixtures' recipe;
 * `OracleTwoHot`, `OracleTwoHotSlowPcont`   tests/return_norm_ref.py's classes with the two-hot head decoded wherever a
                                    value is read and the cross-entropy as the critic's loss.

tests/test_twohot_cpu.py ties the formulas to autograd and the classes to OracleReturnNorm; tests/test_twohot_gpu.py holds
the kernels and whole updates of the HIP agents to this file."""
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

from oracle import fixtures as fx
from oracle import repo_oracle as ro
from tests import act_ref as ar
from tests import actor_grad_ref as ag
from tests import pcont_ref as pr
from tests import return_norm_ref as rn
from tests import slow_value_ref as sv

LOG_2PI = ro.LOG_2PI
ROWS_PER_BLOCK = 4            # kThRowsPerBlock: one wave per row, four waves per block
LAST_BLOCK_MAX_GRID = 64      # kLastBlockMaxGrid: grids up to this finish their own sum
MAX_BLOCKS = 1024             # kRedBlocks: above it the rows are walked in a grid-stride loop
TWOHOT_SEED, TWOHOT_SLOW_SEED = 53, 59


def blocks(rows):
    return min(-(-rows // ROWS_PER_BLOCK), MAX_BLOCKS)


def regime(rows):
    """How the repo_twohot_* launches cover `rows`: "partial-block" (one block, some of its waves without a row),
    "self-finish" (whole blocks, at most LAST_BLOCK_MAX_GRID of them: the launch's last block sums the partials),
    "follow-up" (more blocks, one row per wave: a second launch sums), "stride" (past the block cap: waves loop over rows)."""
    if rows < ROWS_PER_BLOCK:
        return "partial-block"
    if -(-rows // ROWS_PER_BLOCK) <= LAST_BLOCK_MAX_GRID:
        return "self-finish"
    return "follow-up" if rows <= MAX_BLOCKS * ROWS_PER_BLOCK else "stride"


def regime_sizes():
    """Row counts on both sides of every boundary of `regime`, and one ragged size past the cap."""
    r, g, b = ROWS_PER_BLOCK, LAST_BLOCK_MAX_GRID, MAX_BLOCKS
    return [1, 3, 4, 5, r * (g - 1), r * g, r * g + 1, r * (g + 1), r * (b - 1), r * b, r * b + 1, r * (b + 1), 2 * r * b + 7]


def symlog(x):
    return torch.sign(x) * torch.log1p(x.abs())


def symexp(y):
    return torch.sign(y) * torch.expm1(y.abs())


def bins(K, low, high, dtype=torch.float64):
    low, high = float(np.float32(low)), float(np.float32(high))     # the kernels take the bounds as float32
    return (low + torch.arange(K, dtype=torch.float64) * ((high - low) / (K - 1))).to(dtype)


def decode(z, low, high):
    """z (rows, K) -> (v, m, p)."""
    b = bins(z.shape[1], low, high, z.dtype)
    p = torch.softmax(z, 1)
    m = (p * b).sum(1)
    return symexp(m), m, p


def decode_bwd(z, low, high, g, gmul=1.0):
    v, m, p = decode(z, low, high)
    b = bins(z.shape[1], low, high, z.dtype)
    return (g * gmul * (v.abs() + 1.0))[:, None] * p * (b[None, :] - m[:, None])


def target(R, K, low, high):
    """-> (t (rows, K), pos, k0).  A NaN return gives a NaN row (k0 reported as 0)."""
    lo, hi = float(np.float32(low)), float(np.float32(high))
    delta = (hi - lo) / (K - 1)
    y = torch.clamp(symlog(R), lo, hi)
    pos = (y - lo) / delta
    bad = torch.isnan(pos)
    safe = torch.where(bad, torch.zeros_like(pos), pos).clamp(0.0, float(K - 1))
    k0 = torch.clamp(torch.floor(safe), max=float(K - 2)).long()
    f = safe - k0.to(pos.dtype)
    t = torch.zeros(R.shape[0], K, dtype=R.dtype)
    t.scatter_(1, k0[:, None], (1.0 - f)[:, None])
    t.scatter_(1, (k0 + 1)[:, None], f[:, None])
    t[bad] = float("nan")
    return t, pos, k0


def nll(z, R, w, low, high, scale):
    """-> dict(ce (rows,), sums (2,), dz (rows, K), pos, k0, logp)."""
    K = z.shape[1]
    t, pos, k0 = target(R, K, low, high)
    logp = torch.log_softmax(z, 1)
    # (a zero weight of a -inf log-probability must not make a NaN: only the two hot columns enter)
    hot = torch.stack([logp.gather(1, k0[:, None])[:, 0], logp.gather(1, (k0 + 1)[:, None])[:, 0]], 1)
    th = torch.stack([t.gather(1, k0[:, None])[:, 0], t.gather(1, (k0 + 1)[:, None])[:, 0]], 1)
    ce = -(th * hot).sum(1)
    ww = torch.ones_like(R) if w is None else w
    dz = scale * ww[:, None] * (torch.softmax(z, 1) - t)
    return dict(ce=ce, sums=torch.stack([(ww * ce).sum(), ww.sum()]), dz=dz, pos=pos, k0=k0, logp=logp, hot=hot)


def make_twohot_value_params(K, belief=200, state=30, hidden=200, seed=TWOHOT_SEED):
    """A value head's state dict by the fixtures.make_params recipe with a (K, hidden) last layer, that layer scaled up so
    that the softmax is far from uniform: the tests then do not run at the agent's degenerate zero initialisation."""
    rs = np.random.RandomState(seed)
    shapes = OrderedDict(fx.param_shapes(1, belief=belief, state=state, hidden=hidden)["value_model"])
    shapes["fc4.weight"], shapes["fc4.bias"] = (K, hidden), (K,)
    out, k = OrderedDict(), 1.0
    for name, shp in shapes.items():
        if len(shp) > 1:
            k = 1.0 / np.sqrt(float(np.prod(shp[1:])))
        gain = 8.0 if name.startswith("fc4") else 1.0
        out[name] = (gain * rs.uniform(-k, k, size=shp)).astype(np.float32)
    return out


def twohot_params(A, K, seed=7, value_seed=TWOHOT_SEED):
    """fixtures.make_params with the value head replaced by a K-wide one."""
    params = fx.make_params(A, seed)
    params["value_model"] = make_twohot_value_params(K, seed=value_seed)
    return params


def config(cfg):
    """(on, K, low, high) with the defaults of DESIGN.md 6o."""
    return (getattr(cfg, "value_dist", "normal") == "twohot", int(getattr(cfg, "value_bins", 255)),
            float(getattr(cfg, "value_bin_low", -20.0)), float(getattr(cfg, "value_bin_high", 20.0)))


class _TwoHot:
    """tests/return_norm_ref.py's _ReturnNorm.train_actor_critic, line for line, with every value read through `decode` and
    the critic's loss the two-hot cross-entropy.  value_dist "normal": the class behind it, untouched."""

    def _init_twohot(self, cfg):
        self.th_on, self.th_K, self.th_low, self.th_high = config(cfg)

    def _value(self, head, x, act):
        return decode(ar.mlp_head(head, x, 4, act), self.th_low, self.th_high)[0]

    def train_actor_critic(self, beliefs, post_states, eps_act, eps_prior, eps_ent, apply=True):
        if not self.th_on:
            return super().train_actor_critic(beliefs, post_states, eps_act, eps_prior, eps_ent, apply=apply)
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
        # the critic: the online head's logits on the detached rows against the two-hot target of the detached returns
        z = ar.mlp_head(p["value_model"], x[:nv].detach(), 4, act)
        t, _, _ = target(returns.detach().reshape(-1), self.th_K, self.th_low, self.th_high)
        ce = -(t * F.log_softmax(z, 1)).sum(1)
        value_loss = (w.reshape(-1) * ce).mean() if pcont else ce.mean()
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
        self.last["imagine"] = [t_.detach() for t_ in (ib, istate, im, isd)]
        self.last["returns"], self.last["baseline"], self.last["logp"] = returns.detach(), baseline, logp.detach()
        self.last["weights"] = w
        self.last["values"] = v_ret.detach()
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


class OracleTwoHot(_TwoHot, rn.OracleReturnNorm):
    """OracleReturnNorm with cfg.value_dist and its three keys; `params` carries the K-wide value head (twohot_params)."""

    def __init__(self, cfg, action_size, params=None, seed=7, mix=None):
        super().__init__(cfg, action_size, params=params, seed=seed, mix=mix)
        self._init_twohot(cfg)


class OracleTwoHotSlowPcont(_TwoHot, rn.OracleReturnNormSlowPcont):
    """The same on pcont's weights with the slow head (K-wide too) behind the returns and the baseline."""

    def __init__(self, cfg, action_size, **kw):
        super().__init__(cfg, action_size, **kw)
        self._init_twohot(cfg)
