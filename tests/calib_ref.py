"""Plain-torch restatement of CalibratedRePo's own arithmetic (reference common/models/gans.py:56-156, mlps.py:11-32 and the
loss lines of algorithms/repo/repo_adapt.py:426-482), written the way tests/inv_dyn_ref.py is: from the mathematics, on
float64 leaves under autograd (the gradient penalty with create_graph=True), noise explicit, and every LeakyReLU / ReLU
input recorded in `pre` (the bottleneck sample `lat` included) so that a test can assert min |pre| >= PRE_MARGIN before
it compares.  tests/test_calib_cpu.py ties it to the reference's own modules.

make_disc_params / make_tau_params are the seeded parameter sets of the discriminator and the density-ratio model, shared
by the golden generator (which loads them into the reference's modules) and the GPU tests: no weights are committed."""
import math
from collections import OrderedDict

import numpy as np
import torch
import torch.nn.functional as F

from tests.act_ref import PRE_MARGIN, min_abs_pre  # noqa: F401  (re-exported for the tests)

DISC_SEED = 31
TAU_SEED = 37
SLOPE = 0.01   # nn.LeakyReLU()'s default
# what the goldens' configuration adds to oracle/fixtures.py:default_config (experiments/adapt_repo.py:172-190's defaults,
# a small calibration ring, random calibration actions)
CALIB_CFG = dict(inv_dynamics=True, inv_dynamics_lr=3e-4, inv_dynamics_hidden_size=64, calibration_mode="simple_pair",
                 calibration_buffer_size=64, expert_calib_data=False, calib_time_limit=500, aln_coef=1.0, dyn_coef=1.0,
                 calib_coef=1.0, f_lr=3e-4, f_latent_size=64, f_target_kl=0.1, f_hidden_size=256, tau_lr=5e-5, u_lr=5e-3,
                 init_u=1e-4, source_dir="", offline_truncate_size=1000000)


def _mlp_params(prefix, dims, rs, out):
    for i, (fan_in, fan_out) in enumerate(zip(dims[:-1], dims[1:])):
        k = 1.0 / np.sqrt(float(fan_in))
        out[f"{prefix}layers.{2 * i}.weight"] = rs.uniform(-k, k, size=(fan_out, fan_in)).astype(np.float32)
        out[f"{prefix}layers.{2 * i}.bias"] = rs.uniform(-k, k, size=(fan_out,)).astype(np.float32)


def make_disc_params(E, Hf, Z, n_hidden=4, seed=DISC_SEED):
    """OrderedDict(name -> float32 ndarray) in the discriminator's state_dict order: encoder.layers.{0,2,..}.{weight,bias},
    fc.{weight,bias}; uniform(-k, k) with k = fan_in ** -0.5 (the recipe of oracle/fixtures.py:make_params)."""
    rs = np.random.RandomState(seed)
    out = OrderedDict()
    _mlp_params("encoder.", [E] + [Hf] * n_hidden + [2 * Z], rs, out)
    k = 1.0 / np.sqrt(float(Z))
    out["fc.weight"] = rs.uniform(-k, k, size=(1, Z)).astype(np.float32)
    out["fc.bias"] = rs.uniform(-k, k, size=(1,)).astype(np.float32)
    return out


def make_tau_params(E, Hf, n_hidden=4, seed=TAU_SEED):
    """The density-ratio model log_tau = MLP(E, [Hf] * n_hidden, 1): layers.{0,2,..}.{weight,bias}."""
    rs = np.random.RandomState(seed)
    out = OrderedDict()
    _mlp_params("", [E] + [Hf] * n_hidden + [1], rs, out)
    return out


def _n_linear(p, prefix):
    return sum(1 for k in p if k.startswith(prefix + "layers.") and k.endswith(".weight"))


def mlp(p, x, act, pre=None, prefix=""):
    """Linear layers `prefix`layers.{0,2,..}; `act` ("relu" / "leaky") after all but the last."""
    n = _n_linear(p, prefix)
    h = x
    for i in range(n):
        h = F.linear(h, p[f"{prefix}layers.{2 * i}.weight"], p[f"{prefix}layers.{2 * i}.bias"])
        if i < n - 1:
            if pre is not None:
                pre.append(h.detach())
            h = F.relu(h) if act == "relu" else torch.where(h > 0, h, SLOPE * h)
    return h


def disc_forward(p, x, eps, pre=None):
    """-> (d (N,), mean, logstd): z = encoder(x) = [mean | logstd], lat = mean + eps exp(logstd), d = fc(leaky(lat))."""
    z = mlp(p, x, "leaky", pre, "encoder.")
    Z = z.shape[1] // 2
    mean, logstd = z[:, :Z], z[:, Z:]
    lat = mean + eps * torch.exp(logstd)
    if pre is not None:
        pre.append(lat.detach())
    d = F.linear(torch.where(lat > 0, lat, SLOPE * lat), p["fc.weight"], p["fc.bias"])
    return d[:, 0], mean, logstd


def kl_prior_rows(mean, logstd):
    """KL(N(mean, exp(logstd)^2) || N(0, 1)) per row."""
    return (-logstd + 0.5 * (torch.exp(2 * logstd) + mean ** 2)).sum(1) - 0.5 * mean.shape[1]


def bce(d, target):
    """mean binary cross entropy of the logits d against a constant target in {0, 1}."""
    return (F.softplus(-d) if target else F.softplus(d)).mean()


def disc_losses(p, x_real, x_fake, eps_real, eps_fake, beta, tau=None, target_kl=0.1, gp_weight=1.0, pre=None):
    """The four losses of one discriminator step and the zero-centred gradient penalty on the real rows:
    -> dict(real, fake, kl, kl_loss, gp); their sum real + fake + kl_loss + gp is what the step minimises."""
    x_real = x_real.detach().clone().requires_grad_(True)
    d_real, m_r, s_r = disc_forward(p, x_real, eps_real, pre)
    d_fake, m_f, s_f = disc_forward(p, x_fake.detach(), eps_fake, pre)
    if tau is None:
        real, fake = bce(d_real, 1), bce(d_fake, 0)
    else:
        real, fake = -(tau.detach() * d_real).mean(), (d_fake + 0.25 * d_fake ** 2).mean()
    kl = 0.5 * (kl_prior_rows(m_r, s_r).mean() + kl_prior_rows(m_f, s_f).mean())
    g, = torch.autograd.grad(d_real.sum(), x_real, create_graph=True)
    gp = gp_weight * g.pow(2).sum(1).mean()
    return dict(real=real, fake=fake, kl=kl, kl_loss=beta * (kl - target_kl), gp=gp, d_real=d_real, d_fake=d_fake)


def beta_step(beta, kl, beta_lr=5e-3, target_kl=0.1):
    return max(float(beta) + beta_lr * (float(kl) - target_kl), 0.0)


def adam_first_step(p, g, lr, eps=1e-8):
    """torch.optim.Adam's first step from zero moments: the bias corrections cancel, p - lr g / (|g| + eps)."""
    return p - lr * g / (g.abs() + eps)


def generator_loss(d_tgt, support):
    """The alignment loss of the encoder on the discriminator's output for target embeddings."""
    return -(d_tgt + 0.25 * d_tgt ** 2).mean() if support else bce(d_tgt, 1)


def calib_loss(tgt, src):
    """-Normal(tgt, 1).log_prob(src).mean() over all elements."""
    return 0.5 * ((tgt - src) ** 2).mean() + 0.5 * math.log(2 * math.pi)


def tau_losses(tau, d_src, u):
    """-> (tau_loss = mean(tau d_src) + u mean(tau - 1) with u a constant, u_loss = -u mean(tau - 1) with tau a constant)."""
    c = (tau - 1).mean()
    return (tau * d_src.detach()).mean() + u.detach() * c, -u * c.detach()


def make_calib_inputs(L, B, A, Z, u):
    """The seeded inputs of calibration step `u` of the goldens: four uint8 frame batches (L, B, 3, 64, 64) -- source
    replay, target replay and the two halves of the paired frames -- and the four (L B, Z) noise draws in draw order."""
    from oracle import fixtures as fx

    frames = {k: fx.make_batch(L, B, A, seed=s + u)[0] for k, s in
              (("aln_src", 11), ("aln_tgt", 21), ("cal_src", 31), ("cal_tgt", 41))}
    rs = np.random.RandomState(201 + u)
    noise = OrderedDict((k, rs.standard_normal((L * B, Z)).astype(np.float32))
                        for k in ("disc_real", "disc_fake", "disc_tgt", "disc_src"))
    return frames, noise
