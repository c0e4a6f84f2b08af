"""bottle, the inverse-dynamics model + the flat-buffer Adam that replaces torch.optim.Adam / clip_grad_norm_.

bottle: /root/reference/algorithms/repo/models/utils.py:9-16.
InverseDynamicsModel: /root/reference/algorithms/repo/models/utils.py:84-109.
FlatAdam: the reference builds Adam(list_of_params, lr) (dreamer.py:96,106,114; repo.py:23) and
calls zero_grad / clip_grad_norm_ / step (repo.py:87-90).  Here all parameters of a group live
in ONE contiguous device buffer (each nn.Parameter is a view into it, as is its .grad), so the
global-norm clip and the Adam update are two streaming kernels over the flat buffers, and a
data-parallel all-reduce is one collective.  state_dict()/load_state_dict() keep
torch.optim.Adam's layout so reference checkpoints round-trip.
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from .... import ops


def bottle(f, xs):
    """Apply f to (time*batch, ...) views of (time, batch, ...) tensors and fold back."""
    horizon, batch_size = xs[0].shape[:2]
    ys = f(*(x.reshape(horizon * batch_size, *x.shape[2:]) for x in xs))
    if isinstance(ys, tuple):
        return tuple(y.reshape(horizon, batch_size, *y.shape[1:]) for y in ys)
    return ys.reshape(horizon, batch_size, *ys.shape[1:])


class InverseDynamicsModel(nn.Module):
    """(2 belief + state) -> hidden^3 -> 2 action MLP on cat([belief, state, next_belief]): the action that led from
    one latent to the next, as a Normal (mean, softplus + min_std_dev).  activation_function "elu" or "relu" (the
    reference's default argument), `self.act` its REPO_ACT_* id.  Trained by Dreamer.train_inv_dynamics."""

    def __init__(self, belief_size, state_size, action_size, hidden_size, activation_function="relu", min_std_dev=0.1):
        super().__init__()
        self.act = ops.dense_act_id(activation_function, type(self).__name__)
        self.min_std_dev = min_std_dev
        self.fc1 = nn.Linear(belief_size + state_size + belief_size, hidden_size)
        self.fc2 = nn.Linear(hidden_size, hidden_size)
        self.fc3 = nn.Linear(hidden_size, hidden_size)
        self.fc4 = nn.Linear(hidden_size, 2 * action_size)

    def plist(self):
        return [t for m in (self.fc1, self.fc2, self.fc3, self.fc4) for t in (m.weight, m.bias)]

    @torch.no_grad()
    def forward(self, belief, state, next_belief):
        x = torch.cat((belief, state, next_belief), dim=1).float().contiguous()
        raw, _ = ops.mlp_fwd([t.detach() for t in self.plist()], x, act=self.act)
        mean, std_dev = torch.chunk(raw, chunks=2, dim=1)
        return mean, F.softplus(std_dev) + self.min_std_dev


def adam_param_group(lr, betas, eps, n_params):
    """The `param_groups[0]` entry torch.optim.Adam of THIS torch build would write for these
    hyper-parameters: key set and key order come from a throw-away torch.optim.Adam instance, so a
    checkpoint written here has the layout the reference's `Adam.state_dict()` has on the same install
    (tests/golden/checkpoint_manifest.json pins it for the build container's torch)."""
    probe = torch.optim.Adam([torch.nn.Parameter(torch.zeros(1))], lr=float(lr), betas=tuple(betas), eps=float(eps))
    group = dict(probe.state_dict()["param_groups"][0])
    group["params"] = list(range(n_params))
    return group


GRAD_CLIPS = ("norm", "agc")
OPTIMIZERS = ("adam", "laprop")


def _positive(config, key, default):
    v = getattr(config, key, default)
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not math.isfinite(v) or not v > 0:
        raise ValueError(f"{key}={v!r}: expected a finite number > 0")
    return float(v)


def optim_config(config):
    """config.grad_clip / config.optimizer and their keys -> the keyword arguments of FlatAdam that carry
    them.  grad_clip: "norm" (the default: the global-norm clip at grad_clip_norm) or "agc" (per tensor, a gradient at
    most agc_clip (0.3) times max(agc_pmin (1e-3), its tensor's norm); grad_clip_norm is then not applied).  optimizer:
    "adam" (the default) or "laprop"; optimizer_eps, where present, replaces the rule's eps (1e-8 / 1e-20).  An unknown
    name or an out-of-range number: ValueError naming the key."""
    clip = getattr(config, "grad_clip", "norm")
    if clip not in GRAD_CLIPS:
        raise ValueError(f'grad_clip={clip!r}: expected "norm" or "agc"')
    rule = getattr(config, "optimizer", "adam")
    if rule not in OPTIMIZERS:
        raise ValueError(f'optimizer={rule!r}: expected "adam" or "laprop"')
    kw = {"rule": rule, "grad_clip": clip, "agc_clip": _positive(config, "agc_clip", 0.3),
          "agc_pmin": _positive(config, "agc_pmin", 1e-3)}
    kw["eps"] = _positive(config, "optimizer_eps", LAPROP_EPS if rule == "laprop" else 1e-8)
    return kw


LAPROP_EPS = 1e-20


class FlatAdam:
    """Adam (or LaProp: rule="laprop") over a flat parameter buffer with fused global-norm clipping (or per-tensor adaptive
    clipping: grad_clip="agc"), DESIGN.md 6p.  With the defaults every launch is the one it was before the two keys."""

    @staticmethod
    def padded_numel(params):
        """Length of the flat buffer FlatAdam lays these parameters out in (16-byte aligned sub-views)."""
        return sum((p.numel() + 3) // 4 * 4 for p in params)

    def __init__(self, params, lr, betas=(0.9, 0.999), eps=None, grad=None, rule="adam", grad_clip="norm", agc_clip=0.3,
                 agc_pmin=1e-3):
        """eps: None = the rule's default (1e-8, LaProp 1e-20).  grad: optional caller-owned storage for the flat gradient (padded_numel floats) -- the agents
        lay the actor's and the critic's gradients out in ONE buffer so that a data-parallel job exchanges
        them with one collective."""
        self.params = list(params)
        assert self.params, "FlatAdam needs at least one parameter"
        assert rule in OPTIMIZERS and grad_clip in GRAD_CLIPS, (rule, grad_clip)
        if eps is None:
            eps = LAPROP_EPS if rule == "laprop" else 1e-8
        self.lr, self.betas, self.eps = float(lr), tuple(betas), float(eps)
        self.rule, self.grad_clip, self.agc_clip, self.agc_pmin = rule, grad_clip, float(agc_clip), float(agc_pmin)
        self.step_count = 0
        dev = self.params[0].device
        sizes = [p.numel() for p in self.params]
        # 16-byte aligned offsets so every view can be read with 128-bit loads
        self.offsets, off = [], 0
        for n in sizes:
            self.offsets.append(off)
            off += (n + 3) // 4 * 4
        self.numel = off
        self.flat = torch.zeros(off, dtype=torch.float32, device=dev)
        if grad is None:
            grad = torch.zeros(off, dtype=torch.float32, device=dev)
        assert grad.shape == (off,) and grad.dtype == torch.float32 and grad.is_contiguous(), (grad.shape, off)
        self.grad = grad
        self.exp_avg = torch.zeros(off, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(off, dtype=torch.float32, device=dev)
        self.sqnorm = torch.zeros(1, dtype=torch.float32, device=dev)
        self.agc = None
        if grad_clip == "agc":
            # the tables, uploaded once; the pre-clip global squared norm lands in self.sqnorm, the clipped-tensor count
            # behind it in self.agc_count
            self.agc = ops.AgcTables(self.offsets, sizes, off, dev)
            self.sqnorm, self.agc_count = self.agc.stats[:1], self.agc.stats[1:]
        self.skip = None   # the current update's status word (ops.take_scan_status): non-zero = the step is skipped
        self.target = None   # (flat, every, fraction) of a tracked slow copy: track_target
        self.gviews = []
        with torch.no_grad():
            for p, o, n in zip(self.params, self.offsets, sizes):
                self.flat[o : o + n].copy_(p.detach().reshape(-1))
                p.data = self.flat[o : o + n].view(p.shape)
                gv = self.grad[o : o + n].view(p.shape)
                p.grad = gv
                self.gviews.append(gv)

    @classmethod
    def view(cls, parent, n_params, lr):
        """A second optimiser over the FIRST n_params parameters of `parent` (same storage for values and gradients,
        its own moments and step count): the reference's `Adam(self.encoder.parameters())` beside the model optimiser
        (repo_adapt.py:29) -- two torch optimisers over shared parameters."""
        self = cls.__new__(cls)
        self.params = parent.params[:n_params]
        self.lr, self.betas, self.eps = float(lr), parent.betas, (parent.eps if parent.rule == "adam" else 1e-8)
        self.rule, self.grad_clip, self.agc = "adam", "norm", None   # a view stays Adam with the global clip
        self.step_count = 0
        self.offsets = parent.offsets[:n_params]
        self.numel = parent.offsets[n_params] if n_params < len(parent.params) else parent.numel
        self.flat, self.grad = parent.flat[: self.numel], parent.grad[: self.numel]
        self.exp_avg = torch.zeros_like(self.flat)
        self.exp_avg_sq = torch.zeros_like(self.flat)
        self.sqnorm = torch.zeros(1, dtype=torch.float32, device=self.flat.device)
        self.skip = None
        self.target = None
        self.gviews = parent.gviews[:n_params]
        return self

    # -- reference-style surface -----------------------------------------------------
    def zero_grad(self, set_to_none=False):
        self.grad.zero_()

    def track_target(self, flat, every, fraction):
        """A slow copy of the parameters (config.slow_value_target): `flat` has this optimiser's layout.  After
        the step with the 1-based count k, if k % every == 0, flat += fraction * (self.flat - flat) (fraction == 1: a bit
        copy), in the step's own launch (ops.clip_adam_target) and under its skip word; every other step is the plain one
        and leaves `flat` alone.  step_count advances on a skipped step too, so a mixing step that a fault skipped is lost
        until the next period.  The phase is step_count's: a checkpoint restores it with the optimiser's state."""
        every, fraction = int(every), float(fraction)
        assert flat.shape == self.flat.shape and flat.dtype == torch.float32 and flat.is_contiguous(), flat.shape
        assert flat.device == self.flat.device and flat.data_ptr() != self.flat.data_ptr()
        assert every >= 1 and 0.0 < fraction <= 1.0, (every, fraction)
        self.target = (flat, every, fraction)

    def _step(self, sqnorm, max_norm):
        target = self.target
        if self.rule != "adam" or self.agc is not None:
            mix = target is not None and self.step_count % target[1] == 0
            mode = ops.CLIP_TABLE if self.agc is not None else ops.CLIP_GLOBAL if sqnorm is not None else ops.CLIP_NONE
            ops.optim_step(self.flat, self.grad, self.exp_avg, self.exp_avg_sq, self.lr, self.step_count, self.rule, mode,
                           sqnorm, max_norm, self.agc, None, self.betas, self.eps, self.skip,
                           target[0] if mix else None, target[2] if mix else 1.0)
        elif target is not None and self.step_count % target[1] == 0:
            ops.clip_adam_target(self.flat, self.grad, self.exp_avg, self.exp_avg_sq, sqnorm, max_norm, self.lr,
                                 self.step_count, target[0], target[2], self.betas, self.eps, skip=self.skip)
        else:
            ops.clip_adam(self.flat, self.grad, self.exp_avg, self.exp_avg_sq, sqnorm, max_norm, self.lr,
                          self.step_count, self.betas, self.eps, skip=self.skip)

    def clip_and_step(self, max_norm):
        """clip_grad_norm_(params, max_norm) + step() (repo.py:89-90).  The squared global
        norm stays on the device in self.sqnorm (read it after the update's single sync)."""
        self.step_count += 1
        if self.agc is not None:   # per tensor: max_norm is not applied
            ops.agc_coef(self.agc, self.flat, self.grad, self.agc_clip, self.agc_pmin)
        else:
            ops.grad_sqnorm(self.grad, out=self.sqnorm)
        self._step(self.sqnorm, max_norm)

    def step(self):
        """The unclipped step (the GAN discriminator's): no clipping of either kind."""
        assert self.agc is None, "step() is the unclipped step; an AGC optimiser steps through clip_and_step"
        self.step_count += 1
        self._step(None, 0.0)

    # -- torch.optim.Adam-compatible checkpoint layout -------------------------------------
    def state_dict(self):
        state = {}
        if self.step_count > 0:
            for i, (p, o) in enumerate(zip(self.params, self.offsets)):
                n = p.numel()
                state[i] = {
                    "step": torch.tensor(float(self.step_count)),
                    "exp_avg": self.exp_avg[o : o + n].view(p.shape).clone(),
                    "exp_avg_sq": self.exp_avg_sq[o : o + n].view(p.shape).clone(),
                }
        group = adam_param_group(self.lr, self.betas, self.eps, len(self.params))
        if self.rule != "adam":   # the moments keep Adam's slots; one entry names the rule (Adam's layout is unchanged)
            group["optimizer"] = self.rule
        return {"state": state, "param_groups": [group]}

    def check_rule(self, sd, what="the checkpoint's optimiser state"):
        """ValueError naming `optimizer` if the state dict `sd` was written under the other update rule (the other rule's
        first moment is another quantity).  Copies nothing: an agent calls it for every optimiser entry before it loads
        anything (Dreamer.load_param_dict)."""
        rule = sd["param_groups"][0].get("optimizer", "adam")
        if rule != self.rule:
            raise ValueError(f"optimizer={self.rule!r}: {what} was written under optimizer={rule!r}; the first moments "
                             "of the two rules are not interchangeable")

    def load_state_dict(self, sd):
        self.check_rule(sd)   # ahead of any copy
        g = sd["param_groups"][0]
        self.lr, self.betas, self.eps = float(g["lr"]), tuple(g["betas"]), float(g["eps"])
        steps = set()
        with torch.no_grad():
            for i, (p, o) in enumerate(zip(self.params, self.offsets)):
                st = sd["state"].get(i)
                if st is None:
                    continue
                n = p.numel()
                self.exp_avg[o : o + n].copy_(st["exp_avg"].reshape(-1))
                self.exp_avg_sq[o : o + n].copy_(st["exp_avg_sq"].reshape(-1))
                steps.add(int(float(st["step"])))
        assert len(steps) <= 1, "per-parameter step counts differ; not an Adam state this optimiser can hold"
        self.step_count = steps.pop() if steps else 0
