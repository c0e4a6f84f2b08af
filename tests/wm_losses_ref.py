"""config.reward_dist = "twohot", config.obs_symlog and config.kl_dyn_scale / kl_rep_scale restated on the CPU (not a test):
DreamerV3's world-model losses (Hafner et al. 2023) in the shapes of this project.  The reference has no counterpart, so
DESIGN.md 6q is the specification and this file is its executable form:

 * `symlog`                         tests/twohot_ref.py's, sign(x) log1p(|x|): the observation transform;
 * `reward_loss`, `decode_reward`   the two-hot cross-entropy of the reward head's logits with the nonterminal mask as its
                                    weights (the mean over ALL rows), and the imagined reward symexp(sum p b);
 * `kl_mode2_loss`                  dyn max(KL(sg q || p), free) + rep max(KL(q || sg p), free) per row, plain torch, so
                                    autograd gives its gradients;
 * `kl_mode1`, `kl_mode2`           csrc/loss.hip's kl_kernel restated expression for expression (sum, four gradients);
 * `symlog_blocks`, `symlog_sizes`  repo_symlog's launch shape from its geometry;
 * `make_twohot_reward_params`      a reward head with K outputs and a NON-zero last layer, by the fixtures' recipe;
 * `OracleWm`, `OracleWmSlowPcont`  tests/twohot_ref.py's classes with the three keys placed into train_dynamics (pixel or
                                    state-vector, tests/symbolic_ref.py's chains) and the decoded reward into the imagination.

tests/test_wm_losses_cpu.py ties the formulas to autograd and the classes to their parents; tests/test_wm_losses_gpu.py
holds the kernels and whole updates of the HIP agents to this file."""
import contextlib
from collections import OrderedDict

import numpy as np
import torch

from oracle import fixtures as fx
from oracle import repo_oracle as ro
from tests import act_ref as ar
from tests import pcont_ref as pr
from tests import symbolic_ref as sr
from tests import twohot_ref as th

LOG_2PI = ro.LOG_2PI
REWARD_SEED = 61
KL_ROWS_PER_BLOCK, LAST_BLOCK_MAX_GRID, MAX_BLOCKS = 40, 64, 1024   # repo_kl_balance's launch (tests/reduce_ref.py)
# free_nats of the whole-update cases with the KL scales.  The per-row KL of the fixtures' model on the tests' batches lies in
# 0.16 .. 0.32 before the first model step and in 0.10 .. 0.27 after it (this oracle, on the CPU): at 0.18 the threshold
# clips 13 % of the rows in the first update and 76 % in the second, and no row lies within 2e-4 of it.  At the fixtures'
# 3 nats every row is clipped and the KL has no gradient at all.
KL_FREE_NATS = 0.18
symlog = th.symlog


# ----------------------------------------------------------------------------- the reward head
def reward_loss(z, r, mask, low, high):
    """z (rows, K) logits, r and mask (rows,) -> (loss = mean over all rows of mask * CE, sums [sum mask CE, sum mask])."""
    out = th.nll(z, r, mask, low, high, 1.0)
    return (mask * out["ce"]).mean(), out["sums"]


def decode_reward(z, low, high):
    return th.decode(z, low, high)[0]


def make_twohot_reward_params(K, belief=200, state=30, hidden=200, seed=REWARD_SEED):
    """tests/twohot_ref.py's make_twohot_value_params under the reward head's seed: a (K, hidden) last layer scaled up so
    that the softmax is far from uniform and every gradient through the head is non-trivial."""
    return th.make_twohot_value_params(K, belief=belief, state=state, hidden=hidden, seed=seed)


# ----------------------------------------------------------------------------- the KL
def kl_mode2_loss(pm, ps, qm, qs, dyn, rep, free_nats):
    """Per row: dyn max(KL(sg q || p), free) + rep max(KL(q || sg p), free); torch.max is torch.maximum (half the gradient
    to each side at a tie)."""
    free = torch.full((1,), float(free_nats), dtype=pm.dtype)
    kl_dyn = ro.normal_kl(qm.detach(), qs.detach(), pm, ps).sum(-1)
    kl_rep = ro.normal_kl(qm, qs, pm.detach(), ps.detach()).sum(-1)
    return dyn * torch.max(kl_dyn, free) + rep * torch.max(kl_rep, free)


def _kl_terms(pm, ps, qm, qs):
    ratio = qs / ps
    vr = ratio * ratio
    dm = (qm - pm) / ps
    kl = 0.5 * (vr + dm * dm - 1.0 - torch.log(vr))
    isp2 = 1.0 / (ps * ps)
    gqm = (qm - pm) * isp2
    gpm = -gqm
    gqs = -1.0 / qs + qs * isp2
    gps = 1.0 / ps - (qs * qs + (qm - pm) * (qm - pm)) * isp2 / ps
    return kl.sum(-1), gpm, gps, gqm, gqs


def _tie_weight(klrow, free_nats, s):
    s = torch.as_tensor(s, dtype=klrow.dtype)
    return torch.where(klrow > free_nats, s, torch.where(klrow == free_nats, 0.5 * s, torch.zeros_like(s)))[..., None]


def kl_mode1(pm, ps, qm, qs, free_nats, scale):
    """kl_kernel mode 1 -> (sum_rows max(KL, free), dpm, dps, dqm, dqs) in the dtype of the inputs."""
    klrow, gpm, gps, gqm, gqs = _kl_terms(pm, ps, qm, qs)
    w = _tie_weight(klrow, free_nats, scale)
    total = torch.where(klrow > free_nats, klrow, torch.full_like(klrow, free_nats)).sum()
    return total, gpm * w, gps * w, gqm * w, gqs * w


def kl_mode2(pm, ps, qm, qs, dyn, rep, free_nats, scale):
    """kl_kernel mode 2: mode 1's sum; the prior side at sp = dyn * scale, the posterior side at sq = rep * scale, each ONE
    product in the dtype of the inputs."""
    klrow, gpm, gps, gqm, gqs = _kl_terms(pm, ps, qm, qs)
    one = torch.ones((), dtype=pm.dtype)
    wp, wq = _tie_weight(klrow, free_nats, (one * dyn) * scale), _tie_weight(klrow, free_nats, (one * rep) * scale)
    total = torch.where(klrow > free_nats, klrow, torch.full_like(klrow, free_nats)).sum()
    return total, gpm * wp, gps * wp, gqm * wq, gqs * wq


def free_between(klrow):
    """A free_nats (a float32 value) in the widest gap between consecutive sorted row KLs of the central fifth: about half
    the rows are clipped and no row sits where a float32 evaluation could land on the other side of the threshold."""
    srt = klrow.detach().double().reshape(-1).sort().values
    n = srt.numel()
    if n == 1:
        return float(np.float32(0.5 * float(srt[0])))
    lo = min(int(0.4 * n), n - 2)
    hi = max(int(0.6 * n), lo + 1)
    i = lo + int(torch.argmax(srt[lo + 1 : hi + 1] - srt[lo:hi]))
    return float(np.float32(0.5 * (float(srt[i]) + float(srt[i + 1]))))


def kl_sizes():
    """Row counts around every boundary of repo_kl_balance's launch: one launch up to 64 blocks of 40 rows, two above, a
    grid-stride loop past 1024 blocks."""
    r, g, b = KL_ROWS_PER_BLOCK, LAST_BLOCK_MAX_GRID, MAX_BLOCKS
    return [1, 3, 4, 5, r * g, r * g + 1, r * b + 41]


# ----------------------------------------------------------------------------- repo_symlog's launch
def symlog_blocks(n, threads, vec, cap, aligned=True):
    items = n // vec if (aligned and n >= vec) else n
    return min(-(-items // threads), cap)


def symlog_sizes(threads, vec, cap):
    """The issue's fixed sizes, both sides of every boundary of the vector form's launch (the first whole vector, one full
    block, the block cap) and of the dword form's (one full block, the cap), and one ragged size past the cap."""
    per_block, full = threads * vec, threads * vec * cap
    sizes = [1, 3, 4, 5, 255, 256, 257, vec - 1, vec, vec + 1, per_block - 1, per_block, per_block + 1, full - 1, full,
             full + 1, threads * cap, threads * cap + 1, full + 3 * per_block + 7]
    return sorted(set(sizes))


# ----------------------------------------------------------------------------- the oracle classes
def config(cfg):
    """-> dict of the three keys with the defaults of DESIGN.md 6q."""
    kl_on = hasattr(cfg, "kl_dyn_scale") or hasattr(cfg, "kl_rep_scale")
    return dict(rd_on=getattr(cfg, "reward_dist", "normal") == "twohot", rd_K=int(getattr(cfg, "reward_bins", 255)),
                rd_low=float(getattr(cfg, "reward_bin_low", -20.0)), rd_high=float(getattr(cfg, "reward_bin_high", 20.0)),
                symlog_on=bool(getattr(cfg, "obs_symlog", False)), kl_on=kl_on,
                kl_dyn=float(getattr(cfg, "kl_dyn_scale", 0.5)) if kl_on else 1.0,
                kl_rep=float(getattr(cfg, "kl_rep_scale", 0.1)) if kl_on else 1.0)


class _WmLosses:
    """train_dynamics of oracle/repo_oracle.py's OracleAgent (tests/pcont_ref.py's when the class behind has a pcont head),
    line for line, with the three keys; pixel_obs=False runs tests/symbolic_ref.py's chains on (L, B, obs) vectors.  With
    the keys off it computes what the class behind it computes, bit for bit (tests/test_wm_losses_cpu.py).  The imagined
    reward is placed into the parents' train_actor_critic -- which all read `ar.mlp_head(p["reward_model"], ...)` -- by
    standing in for that one call while they run."""

    def _init_wm(self, cfg):
        self.wm = config(cfg)
        self.symbolic = not cfg.pixel_obs
        self.cnn_act = getattr(cfg, "cnn_activation_function", "relu")
        if not hasattr(self, "act"):
            self.act = getattr(cfg, "dense_activation_function", "elu")
        assert self.act == "elu", "train_dynamics here restates the ELU world model"

    def train_dynamics(self, obs, actions, rewards, nonterms, eps_prior, eps_post, apply=True):
        c, p, wm = self.c, self.p, self.wm
        pcont = "pcont_model" in p
        L, B = obs.shape[:2]
        T = L - 1
        if wm["symlog_on"]:
            assert self.symbolic
            obs = symlog(obs)
        if self.symbolic:
            embeds = sr.encoder(p["encoder"], obs.reshape(L * B, -1), self.cnn_act).reshape(L, B, -1)
        else:
            embeds = ro.encoder_fwd(p["encoder"], obs.reshape(L * B, *obs.shape[2:])).reshape(L, B, -1)
        b0, s0 = torch.zeros(B, c.belief_size), torch.zeros(B, c.state_size)
        beliefs, prior_s, pm, ps, post_s, qm, qs = ro.observe(
            p["transition_model"], b0, s0, actions[:-1], embeds[1:], nonterms[:-1], eps_prior, eps_post)
        fb, fs = beliefs.reshape(T * B, -1), post_s.reshape(T * B, -1)
        db, ds = (fb.detach(), fs.detach()) if self.is_repo else (fb, fs)
        if self.symbolic:
            recon = sr.decoder(p["obs_model"], db, ds, self.cnn_act).reshape(T, B, -1)
            obs_loss = sr.obs_loss(recon, obs[1:])
        else:
            recon = ro.decoder_fwd(p["obs_model"], db, ds).reshape(T, B, *obs.shape[2:])
            obs_loss = (0.5 * (recon - obs[1:]) ** 2 + 0.5 * LOG_2PI).sum((2, 3, 4)).mean((0, 1))
        mask = nonterms[:-1].squeeze(-1)
        r_tgt = rewards[:-1].squeeze(-1)
        if wm["rd_on"]:
            z = ro.mlp_head(p["reward_model"], fb, fs, 4)
            reward_loss_, _ = reward_loss(z, r_tgt.reshape(-1), mask.reshape(-1), wm["rd_low"], wm["rd_high"])
        else:
            r_pred = ro.scalar_head(p["reward_model"], fb, fs).reshape(T, B)
            reward_loss_ = ((0.5 * (r_pred - r_tgt) ** 2 + 0.5 * LOG_2PI) * mask).mean((0, 1))
        if pcont:
            logit = ro.scalar_head(p["pcont_model"], fb, fs).reshape(T, B)
            pcont_loss = self.pcont_scale * pr.bernoulli_nll(logit, c.gamma * mask).mean((0, 1))
        out = {}
        if self.is_repo:
            assert not wm["kl_on"], "RePo refuses the KL scales"
            kl_prior = ro.normal_kl(qm.detach(), qs.detach(), pm, ps).sum(2).mean((0, 1))
            kl_post = ro.normal_kl(qm, qs, pm.detach(), ps.detach()).sum(2).mean((0, 1))
            alpha = c.prior_train_steps / (1 + c.prior_train_steps)
            kl_div = alpha * kl_prior + (1 - alpha) * kl_post
            kl_viol = kl_div - c.target_kl
            kl_loss = self.log_beta.exp().detach() * kl_viol
            kl_term = kl_loss
            out["train/kl_div"] = kl_div
        else:
            kl = ro.normal_kl(qm, qs, pm, ps).sum(2)
            kl_loss = torch.max(kl, torch.full((1,), float(c.free_nats))).mean((0, 1))
            kl_term = kl_loss
            if wm["kl_on"]:   # the logged kl_loss stays mode 1's; the loss weighs the two sides apart
                kl_term = kl_mode2_loss(pm, ps, qm, qs, wm["kl_dyn"], wm["kl_rep"], c.free_nats).mean((0, 1))
        model_loss = obs_loss + reward_loss_ + kl_term
        if pcont:
            model_loss = model_loss + pcont_loss
        self.model_opt.zero_grad()
        model_loss.backward()
        self.last["model_grads"] = [None if q.grad is None else q.grad.detach().clone() for q in self.model_params]
        self.last["model_total_norm"] = float(ro.clip_grad_norm(self.model_params, c.grad_clip_norm))
        if apply:
            self.model_opt.step()
        out.update({"train/obs_loss": obs_loss, "train/reward_loss": reward_loss_, "train/kl_loss": kl_loss})
        if pcont:
            out["train/pcont_loss"] = pcont_loss
        out["train/model_loss"] = model_loss
        if self.is_repo:
            beta_loss = -self.log_beta * kl_viol.detach()
            self.beta_opt.zero_grad()
            beta_loss.backward()
            if apply:
                self.beta_opt.step()
            out["train/beta"] = self.log_beta.exp()
            out["train/beta_loss"] = beta_loss
        self.last["embeds"] = embeds.detach()
        self.last["observe"] = [x.detach() for x in (beliefs, prior_s, pm, ps, post_s, qm, qs)]
        return beliefs.detach(), post_s.detach(), {k: float(v.detach()) for k, v in out.items()}

    @contextlib.contextmanager
    def _decoded_reward(self):
        """While the block runs, ar.mlp_head on THIS oracle's reward head returns the decoded reward as a (rows, 1) column
        (what the scalar head returns); every other head passes through."""
        orig, wm, head = ar.mlp_head, self.wm, self.p["reward_model"]

        def mlp_head(p, x, n_layers, act, pre=None):
            out = orig(p, x, n_layers, act, pre)
            return decode_reward(out, wm["rd_low"], wm["rd_high"])[:, None] if p is head else out

        ar.mlp_head = mlp_head
        try:
            yield
        finally:
            ar.mlp_head = orig

    def train_actor_critic(self, beliefs, post_states, eps_act, eps_prior, eps_ent, apply=True):
        if not self.wm["rd_on"]:
            return super().train_actor_critic(beliefs, post_states, eps_act, eps_prior, eps_ent, apply=apply)
        with self._decoded_reward():
            return super().train_actor_critic(beliefs, post_states, eps_act, eps_prior, eps_ent, apply=apply)

    def update(self, obs, actions, rewards, dones, noise):
        """OracleAgent.update; state vectors arrive as float32 (L, B, obs) and are not preprocessed."""
        if not self.symbolic:
            return super().update(obs, actions, rewards, dones, noise)
        t = {k: torch.as_tensor(v) for k, v in noise.items()}
        beliefs, post, scal = self.train_dynamics(torch.as_tensor(obs), torch.as_tensor(actions), torch.as_tensor(rewards),
                                                  1 - torch.as_tensor(dones), t["obs_prior"], t["obs_post"])
        scal.update(self.train_actor_critic(beliefs.flatten(0, 1), post.flatten(0, 1), t["img_act"], t["img_prior"],
                                            t["entropy"]))
        return beliefs, post, scal


class OracleWm(_WmLosses, th.OracleTwoHot):
    """OracleTwoHot with the three keys; `params` carries the K-wide reward head (wm_params) and, for pixel_obs=False, the
    symbolic encoder / decoder."""

    def __init__(self, cfg, action_size, params=None, seed=7, mix=None):
        super().__init__(cfg, action_size, params=params, seed=seed, mix=mix)
        self._init_wm(cfg)


class OracleWmSlowPcont(_WmLosses, th.OracleTwoHotSlowPcont):
    """The same on pcont's head and weights, with the slow value head behind the returns and the baseline."""

    def __init__(self, cfg, action_size, **kw):
        super().__init__(cfg, action_size, **kw)
        self._init_wm(cfg)


def wm_params(A, cfg, reward_K=None, value_K=None, obs=None, seed=7):
    """fixtures.make_params with the reward head replaced by a K-wide one (reward_K), the value head likewise (value_K), and
    the encoder / decoder by tests/symbolic_ref.py's for state vectors of `obs` floats."""
    params = fx.make_params(A, seed)
    if reward_K is not None:
        params["reward_model"] = make_twohot_reward_params(reward_K)
    if value_K is not None:
        params["value_model"] = th.make_twohot_value_params(value_K)
    if obs is not None:
        params.update(sr.make_symbolic_params(obs, cfg.belief_size, cfg.state_size, cfg.embedding_size))
    return OrderedDict(params)


def scaled_obs(L, B, obs, seed):
    """tests/symbolic_ref.py's state vectors with the issue's scaling: every 7th value times 1e3, every 11th times 1e-4,
    every 13th times 1e6 (flat index)."""
    x = sr.make_obs(L, B, obs, seed).reshape(-1)
    x[::7] *= 1e3
    x[::11] *= 1e-4
    x[::13] *= 1e6
    return x.reshape(L, B, obs)


def symlog_inputs(n, seed):
    """repo_symlog's test inputs: N(0, 1) under the same scaling."""
    x = np.random.RandomState(seed).standard_normal(n).astype(np.float32)
    x[::7] *= 1e3
    x[::11] *= 1e-4
    x[::13] *= 1e6
    return x


def rel_gap(a, b):
    return abs(a - b) / max(abs(b), 1e-30)

