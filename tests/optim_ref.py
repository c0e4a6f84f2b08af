"""config.grad_clip = "agc" and config.optimizer = "laprop" restated on the CPU (not a test): per-tensor adaptive gradient
clipping (Brock et al. 2021, as DreamerV3 applies it) and the LaProp update (Ziyin et al. 2020).  The reference has no
counterpart, so DESIGN.md 6p is the specification and this file is its executable form:

 * `config`                        the keys and their defaults;
 * `agc_coef`, `agc_coefs`         unorm = |g|, upper = clip max(pmin, |p|), coef = 1 if unorm <= upper else upper / unorm;
 * `global_coef`                   oracle.repo_oracle.clip_grad_norm's coefficient, operation for operation;
 * `rule_step`                     one Adam or LaProp step on a list of tensors, in the dtype of the tensors; the Adam
                                   branch is oracle.repo_oracle.Adam.step's sequence of torch operations;
 * `update`                        clip + step over a list of tensors (the kernels' float64 reference, and, run on float32
                                   tensors, the CPU evaluation whose error the GPU bound is measured against);
 * `CHUNK`, `PARTS_MAX_BLOCKS`, `FINISH_THREADS`, `STEP_MAX_BLOCKS`, `WAVE`   csrc/optim.hip's launch geometry (the GPU
                                   suite checks them against repo_agc_geometry() and takes its sizes from them);
 * `layout`                        FlatAdam's offsets for a list of tensor sizes;
 * `RuleOpt`                       oracle.repo_oracle.Adam with the rule as an argument ("adam": the parent's step itself);
 * `OracleRules`, `OracleRulesCombined`   OracleAgent / OracleTwoHotSlowPcont with the three optimisers swapped for RuleOpt
                                   and the module-level repo_oracle.clip_grad_norm replaced for the duration of their calls.

tests/test_optim_rules_cpu.py ties this file to oracle.repo_oracle; tests/test_optim_rules_gpu.py holds the kernels and whole
updates of the HIP agents to it."""
import contextlib
import math

import torch

from oracle import repo_oracle as ro
from tests import twohot_ref as th

CHUNK = 4096               # kAgcChunk: elements per chunk
PARTS_MAX_BLOCKS = 1024    # kAgcMaxBlocks: above it a block of the norm pass takes several chunks
FINISH_THREADS = 256       # kAgcFinishThreads: the finishing block; a 64-lane wave per segment
STEP_MAX_BLOCKS = 2048     # kStepMaxBlocks: above it the step strides
WAVE = 64                  # chunks of one segment summed per pass of its wave
LAPROP_EPS = 1e-20
BETAS = (0.9, 0.999)


def config(cfg):
    """(grad_clip, agc_clip, agc_pmin, optimizer, eps) with the defaults of DESIGN.md 6p."""
    rule = getattr(cfg, "optimizer", "adam")
    eps = getattr(cfg, "optimizer_eps", LAPROP_EPS if rule == "laprop" else 1e-8)
    return (getattr(cfg, "grad_clip", "norm"), float(getattr(cfg, "agc_clip", 0.3)), float(getattr(cfg, "agc_pmin", 1e-3)),
            rule, float(eps))


def layout(sizes):
    """-> (offsets, padded length): every tensor starts at a multiple of 4 floats (FlatAdam)."""
    offsets, off = [], 0
    for n in sizes:
        offsets.append(off)
        off += (n + 3) // 4 * 4
    return offsets, off


def agc_coef(g, p, clip, pmin):
    """-> (coef, unorm, upper) as 0-d tensors of g's dtype.  A NaN norm gives a NaN coefficient."""
    unorm, pnorm = torch.linalg.vector_norm(g), torch.linalg.vector_norm(p)
    upper = clip * torch.maximum(pnorm, torch.as_tensor(pmin, dtype=pnorm.dtype))    # (maximum carries a NaN through)
    coef = torch.where(unorm <= upper, torch.ones_like(unorm), upper / unorm)
    return coef, unorm, upper


def agc_coefs(grads, params, clip, pmin):
    """-> (coefs, ratios = unorm / upper) as lists of floats, from float64 copies."""
    coefs, ratios = [], []
    for g, p in zip(grads, params):
        c, un, up = agc_coef(g.detach().double(), p.detach().double(), clip, pmin)
        coefs.append(float(c))
        ratios.append(float(un / up))
    return coefs, ratios


def global_coef(grads, max_norm):
    """oracle.repo_oracle.clip_grad_norm's (coefficient, total norm), the same operations."""
    total = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(g) for g in grads]))
    return torch.clamp(max_norm / (total + 1e-6), max=1.0), total


@torch.no_grad()
def rule_step(ps, gs, ms, vs, t, lr, rule="adam", betas=BETAS, eps=None, us=None):
    """Step number t (1-based) of `rule` on the (already clipped) gradients, in place.  us: a list that receives LaProp's u."""
    b1, b2 = betas
    if eps is None:
        eps = LAPROP_EPS if rule == "laprop" else 1e-8
    bc1, bc2 = 1 - b1 ** t, 1 - b2 ** t
    for p, g, m, v in zip(ps, gs, ms, vs):
        if rule == "adam":      # oracle.repo_oracle.Adam.step
            m.mul_(b1).add_(g, alpha=1 - b1)
            v.mul_(b2).addcmul_(g, g, value=1 - b2)
            denom = (v.sqrt() / math.sqrt(bc2)).add_(eps)
            p.addcdiv_(m, denom, value=-(lr / bc1))
        else:
            assert rule == "laprop", rule
            v.mul_(b2).addcmul_(g, g, value=1 - b2)
            denom = (v.sqrt() / math.sqrt(bc2)).add_(eps)
            u = g / denom
            m.mul_(b1).add_(u, alpha=1 - b1)
            p.add_(m, alpha=-(lr / bc1))
            if us is not None:
                us.append(u)


@torch.no_grad()
def update(ps, gs, ms, vs, t, lr, rule="adam", clip="norm", max_norm=100.0, agc_clip=0.3, agc_pmin=1e-3, betas=BETAS,
           eps=None):
    """clip + step in the tensors' dtype; ps, ms, vs change in place, gs is left alone.  clip: "none", "norm" or "agc".
    -> dict(coefs (one per tensor), total (the pre-clip global norm), clipped (tensors with coef < 1))."""
    gs = [g.clone() for g in gs]
    total = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(g) for g in gs]))
    if clip == "agc":
        coefs = [agc_coef(g, p, agc_clip, agc_pmin)[0] for g, p in zip(gs, ps)]
    elif clip == "norm":
        coefs = [global_coef(gs, max_norm)[0]] * len(gs)
    else:
        assert clip == "none", clip
        coefs = [torch.ones((), dtype=gs[0].dtype)] * len(gs)
    for g, c in zip(gs, coefs):
        g.mul_(c)
    rule_step(ps, gs, ms, vs, t, lr, rule, betas, eps)
    return dict(coefs=[float(c) for c in coefs], total=float(total), clipped=sum(1 for c in coefs if float(c) < 1.0))


class RuleOpt(ro.Adam):
    """oracle.repo_oracle.Adam with the update rule as an argument: "adam" IS the parent's step."""

    def __init__(self, params, lr, rule="adam", eps=None):
        super().__init__(params, lr, eps=(LAPROP_EPS if rule == "laprop" else 1e-8) if eps is None else eps)
        self.rule = rule

    @torch.no_grad()
    def step(self):
        if self.rule == "adam":
            return super().step()
        self.t += 1
        live = [(p, p.grad, m, v) for p, m, v in zip(self.params, self.m, self.v) if p.grad is not None]
        rule_step(*zip(*live), self.t, self.lr, self.rule, (self.b1, self.b2), self.eps)


class _Rules:
    """Swaps the three optimisers of the class behind it for RuleOpt and, for the duration of train_dynamics and
    train_actor_critic, the module-level repo_oracle.clip_grad_norm for the clip cfg.grad_clip asks for.  With the keys
    absent both are the parent's own.  Under "agc", self.last["<group>_coefs" / "_ratios" / "_clipped"] hold every
    tensor's coefficient, its unorm / upper, and the number of tensors with coef < 1 (a tensor without a gradient: 1, 0)."""

    def _init_rules(self, cfg):
        self.clip_mode, self.agc_clip, self.agc_pmin, self.rule, eps = config(cfg)
        for name in ("model_opt", "actor_opt", "value_opt"):
            old = getattr(self, name)
            assert type(old) is ro.Adam and old.t == 0, name
            setattr(self, name, RuleOpt(old.params, old.lr, self.rule, eps))

    def _group(self, params):
        for name in ("model", "actor", "value"):
            if params is getattr(self, f"{name}_params"):
                return name
        raise AssertionError("clip_grad_norm on a parameter list that is none of the agent's groups")

    @contextlib.contextmanager
    def _clip_swapped(self):
        orig = ro.clip_grad_norm

        @torch.no_grad()
        def clip(params, max_norm):
            if self.clip_mode != "agc":
                return orig(params, max_norm)
            name = self._group(params)
            grads = [torch.zeros_like(p) if p.grad is None else p.grad for p in params]
            total = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(g) for g in grads]))
            coefs, ratios = agc_coefs(grads, params, self.agc_clip, self.agc_pmin)
            for p, c in zip(params, coefs):
                if p.grad is not None:
                    p.grad.mul_(c)
            self.last[f"{name}_coefs"], self.last[f"{name}_ratios"] = coefs, ratios
            self.last[f"{name}_clipped"] = sum(1 for c in coefs if c < 1.0)
            return total

        ro.clip_grad_norm = clip
        try:
            yield
        finally:
            ro.clip_grad_norm = orig

    def train_dynamics(self, *a, **kw):
        with self._clip_swapped():
            return super().train_dynamics(*a, **kw)

    def train_actor_critic(self, *a, **kw):
        with self._clip_swapped():
            return super().train_actor_critic(*a, **kw)


class OracleRules(_Rules, ro.OracleAgent):
    """OracleAgent with cfg.grad_clip / cfg.optimizer and their keys."""

    def __init__(self, cfg, action_size, params=None, seed=7):
        super().__init__(cfg, action_size, params=params, seed=seed)
        self._init_rules(cfg)


class OracleRulesCombined(_Rules, th.OracleTwoHotSlowPcont):
    """The same over the combined configuration of 6k - 6o (pcont, slow target, "both", return_norm, two-hot)."""

    def __init__(self, cfg, action_size, **kw):
        super().__init__(cfg, action_size, **kw)
        self._init_rules(cfg)
