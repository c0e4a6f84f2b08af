"""VDBDiscriminator (reference common/models/gans.py:56-156): the variational-bottleneck discriminator CalibratedRePo aligns
its target encoder with, on HIP kernels.

    x (N, E) -> encoder = MLP(E, hidden_dims, 2Z, act="LeakyReLU") -> [mean | logstd]
    lat = mean + eps * exp(logstd);  d = fc(LeakyReLU(lat))

State-dict keys (`encoder.layers.{0,2,..}.{weight,bias}`, `fc.{weight,bias}`), construction order and initialisation are
the reference's.  The dense chain runs on ops.gemm / ops.gemm_wgrad with the LeakyReLU epilogues
(functional.leaky_chain_*), everything behind it on csrc/vdb.hip: the bottleneck head with the prior KL, the four losses,
the head's reverse pass, the dual step on `beta` and the zero-centred gradient penalty with its second-order parameter
gradient.  `beta` is a one-element device tensor from the start (the reference's float becomes a tensor
after the first step); `train` reads nothing back.

Differences a caller sees: the module is built ON its device (`device=`; FlatAdam lays the parameters out in one flat
buffer, which a later .to() would rebind); noise is explicit (`eps`) or drawn in-kernel from a Philox (seed, offset) pair
(`noise`), as everywhere in this package; `train` returns a DiscLosses -- the reference's dict, read lazily.
"""
import torch
import torch.nn as nn

from ... import functional as Fn
from ... import ops
from .mlps import MLP


class _Saved:
    """One forward pass, kept for its reverse pass."""
    __slots__ = ("x", "hid", "z", "lat", "d", "kl", "eps", "noise")


class DiscLosses:
    """VDBDiscriminator.train's loss_info: five device scalars and what turns them into the reference's five floats.
    `buf` = [real loss sum, fake loss sum, kl, sum |g|^2, beta]; reading a key synchronises (once)."""
    KEYS = ("real_loss", "fake_loss", "kl", "gp", "beta")

    def __init__(self, buf, scales):
        self.buf, self.scales, self._host = buf, scales, None

    def values(self, host=None):
        host = self.buf.tolist() if host is None else host
        return {k: v * s for k, v, s in zip(self.KEYS, host, self.scales)}

    def __getitem__(self, k):
        if self._host is None:
            self._host = self.values()
        return self._host[k]

    def keys(self):
        return self.KEYS


class VDBDiscriminator(nn.Module):
    def __init__(self, input_dim, hidden_dims, latent_dim, lr=1e-4, init_beta=0.1, beta_lr=5e-3, target_kl=0.1,
                 gp_weight=1.0, device=None):
        super().__init__()
        self.latent_dim = latent_dim
        self.encoder = MLP(input_dim, hidden_dims, 2 * self.latent_dim, act="LeakyReLU")
        self.act = nn.LeakyReLU()
        self.fc = nn.Linear(self.latent_dim, 1)
        dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        super().to(dev)
        from ...algorithms.repo.models.utils import FlatAdam   # (here: algorithms.repo imports this module)

        self.optimizer = FlatAdam(list(self.parameters()), lr=lr)   # no clipping: the reference steps with plain Adam.step
        self.beta = torch.full((1,), float(init_beta), dtype=torch.float32, device=dev)
        self.beta_lr = beta_lr
        self.target_kl = target_kl
        self.gp_weight = gp_weight
        # in-kernel noise of calls that are given neither `eps` nor `noise`: this module's own Philox stream
        self.noise_seed = int(torch.initial_seed()) & 0x7FFFFFFFFFFFFFFF
        self._noise_counter = 0

    def to(self, *args, **kwargs):
        raise RuntimeError("VDBDiscriminator is built on its device (device=...): its parameters are views of the flat "
                           "buffer of its FlatAdam")

    # ------------------------------------------------------------------ passes
    def plist(self):
        return self.encoder.plist() + [self.fc.weight, self.fc.bias]

    def _pg(self):
        ps = self.plist()
        return [p.detach() for p in ps], [p.grad for p in ps]

    def _draw(self, n):
        off = self._noise_counter
        self._noise_counter += int(n)
        return self.noise_seed, off

    def fwd(self, x, eps=None, noise=None, want_kl=True):
        """x (N, E) -> the saved pass (d (N,), z = [mean | logstd], lat, kl = sum of the rows' prior KL)."""
        p, _ = self._pg()
        sv = _Saved()
        sv.x = x
        sv.eps = eps
        sv.noise = noise if (noise is not None or eps is not None) else self._draw(x.shape[0] * self.latent_dim)
        sv.z, sv.hid = Fn.leaky_chain_fwd(p[:-2], x)
        sv.lat, sv.d, sv.kl = ops.vdb_head_fwd(sv.z, p[-2].view(-1), p[-1], eps=eps, noise=sv.noise or (0, 0), want_kl=want_kl)
        return sv

    def bwd(self, sv, dd, kl_coef=0.0, extra=None, train=True, accumulate=True, dx=None):
        """The reverse pass of `fwd` from dd = dL/dd (N,): parameter gradients (train) and / or the input gradient dx."""
        p, g = self._pg()
        dz = ops.vdb_head_bwd(sv.z, sv.lat, p[-2].view(-1), dd, eps=sv.eps, noise=sv.noise or (0, 0),
                              beta=self.beta if kl_coef else None, kl_coef=kl_coef, extra=extra,
                              dfc_w=g[-2].view(-1) if train else None, dfc_b=g[-1] if train else None, accumulate=accumulate)
        return Fn.leaky_chain_bwd(p[:-2], sv.x, sv.hid, dz, dparams=g[:-2] if train else None, accumulate=accumulate, dx=dx)

    def input_grad(self, sv, dd):
        """dL/dx (N, E) through the frozen discriminator: how an encoder is trained against it."""
        dx = torch.empty_like(sv.x)
        return self.bwd(sv, dd, train=False, dx=dx)

    @torch.no_grad()
    def forward(self, x, deterministic=False, eps=None, noise=None):
        x = x.float().contiguous()
        if deterministic:
            eps = torch.zeros(x.shape[0], self.latent_dim, dtype=torch.float32, device=x.device)
        sv = self.fwd(x, eps=eps, noise=noise, want_kl=False)
        return sv.d.view(-1, 1), sv.z[:, : self.latent_dim], sv.z[:, self.latent_dim:]

    def _grad_penalty(self, sv, out=None):
        """Adds the penalty's parameter gradient (all but its logstd upstream, which is returned for the reverse pass) and
        returns (sum_n |g_n|^2, extra).  DESIGN.md 6h."""
        p, g = self._pg()
        n = sv.x.shape[0]
        fcw = p[-2].view(-1)
        delta = ops.vdb_gp_delta(sv.z, sv.lat, fcw, eps=sv.eps, noise=sv.noise or (0, 0))
        dpre = []                                        # pre-activation gradients of layers L .. 1 of d(sum d)/dx
        gx = torch.empty_like(sv.x)
        Fn.leaky_chain_bwd(p[:-2], sv.x, sv.hid, delta, dparams=None, dx=gx, keep=dpre)
        dpre.reverse()                                   # [layer 1, ..., layer L]
        sq = ops.vdb_gp_norm(gx, 2.0 * self.gp_weight / n, out=out)      # gx is now ghat = 2 gp_weight g / N
        L = len(dpre)
        a = gx
        for l in range(L):
            ops.gemm_wgrad(dpre[l], a, dW=g[2 * l], accumulate=True, want_bias=False)
            last = l == L - 1
            a = ops.gemm(a, p[2 * l], transb=True, epi=ops.EPI_NONE if last else ops.EPI_MUL_DLEAKY,
                         aux=None if last else sv.hid[l])
        extra = ops.vdb_gp_head(a, sv.z, sv.lat, fcw, g[-2].view(-1), eps=sv.eps, noise=sv.noise or (0, 0), accumulate=True)
        return sq, extra

    def loss_and_grad(self, x_real, x_fake, tau=None, eps=None, noise=None, penalty=True):
        """The losses of gans.py:94-119 and the gradient of their sum in self.optimizer.grad (zeroed first).  -> (buf, svr,
        svf): buf = [real loss sum, fake loss sum, -, sum_n |g_n|^2 (0 without the penalty), -].  penalty=False leaves the
        gradient penalty out of value and gradient (the tests compare that part at the first-order tolerance)."""
        x_real, x_fake = x_real.detach().float().contiguous(), x_fake.detach().float().contiguous()
        nr, nf = x_real.shape[0], x_fake.shape[0]
        eps = (None, None) if eps is None else eps
        noise = (None, None) if noise is None else noise
        self.optimizer.zero_grad()
        svr = self.fwd(x_real, eps=eps[0], noise=noise[0])
        svf = self.fwd(x_fake, eps=eps[1], noise=noise[1])
        buf = torch.zeros(5, dtype=torch.float32, device=x_real.device)
        if tau is None:
            _, ddr = ops.vdb_loss(svr.d, ops.VDB_BCE1, 1.0 / nr, out=buf[0:1])
            _, ddf = ops.vdb_loss(svf.d, ops.VDB_BCE0, 1.0 / nf, out=buf[1:2])
        else:
            _, ddr = ops.vdb_loss(svr.d, ops.VDB_NEG_TAU, 1.0 / nr, tau=tau.detach().float().contiguous().view(-1), out=buf[0:1])
            _, ddf = ops.vdb_loss(svf.d, ops.VDB_CHI, 1.0 / nf, out=buf[1:2])
        extra = None
        if penalty:
            _, extra = self._grad_penalty(svr, out=buf[3:4])
        self.bwd(svr, ddr, kl_coef=0.5 / nr, extra=extra)
        self.bwd(svf, ddf, kl_coef=0.5 / nf)
        return buf, svr, svf

    def train(self, x_real, x_fake, tau=None, eps=None, noise=None):
        """gans.py:90-136 (this shadows nn.Module.train, as the reference does).  x_real (Nr, E), x_fake (Nf, E) detached;
        tau (Nr,) or None = the JS form.  eps: (eps_real, eps_fake) tensors; noise: ((seed, off), (seed, off)); neither: this
        module's own Philox stream.  One plain Adam step, then the dual step on beta; nothing is read back."""
        buf, svr, svf = self.loss_and_grad(x_real, x_fake, tau, eps, noise)
        nr, nf = svr.x.shape[0], svf.x.shape[0]
        self.optimizer.step()
        ops.vdb_beta_step(self.beta, svr.kl, nr, svf.kl, nf, self.beta_lr, self.target_kl, kl_out=buf[2:3])
        buf[4:5].copy_(self.beta)
        return DiscLosses(buf, (1.0 / nr, 1.0 / nf, 1.0, self.gp_weight / nr, 1.0))

    def _bce_with_logits(self, d_out, target, reduction="mean"):
        """F.binary_cross_entropy_with_logits(d_out, full(target)) as a device scalar (target 0 or 1)."""
        d = d_out.detach().float().contiguous().view(-1)
        s, _ = ops.vdb_loss(d, ops.VDB_BCE1 if target else ops.VDB_BCE0, want_grad=False)
        return s[0] / d.numel() if reduction == "mean" else s[0]
