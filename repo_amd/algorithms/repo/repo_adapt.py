"""Test-time adaptation of a trained RePo agent: FinetunedRePo (its ENCODER only, on target-domain replay) and
CalibratedRePo (a target encoder aligned with the frozen source encoder through a VDB discriminator and paired frames).

Reference: `FinetunedRePo`, /root/reference/algorithms/repo/repo_adapt.py:26-127 (driven by experiments/adapt_repo.py:220):
the source agent's world model, reward head, actor and critic stay frozen; on target-domain replay the encoder is
trained to keep the reward predictable and the posterior close to the (frozen) prior -- reward NLL + beta * (KL -
target_kl), the full KL gradient through both arguments (repo_adapt.py:63-76) -- with the same dual ascent on log_beta as
RePo.  Here: encoder forward, the observe scan, the reward head's input gradient, the KL reduction, the reverse scan (for
its gradient into the embeddings; the frozen weights' gradients it also forms are discarded) and the encoder backward,
all on the update's kernels; one Adam over the encoder's slice of the model buffer (`FlatAdam.view`).

`CalibratedRePo` (repo_adapt.py:136-596), calibration_mode="simple_pair": the frozen source encoder embeds source-domain
replay and the source half of paired calibration frames; the target encoder is trained so that a variational-bottleneck
discriminator (common/models/gans.py, csrc/vdb.hip) cannot tell its embeddings of target replay from the source's
(alignment_mode "js" -- anything but "support" -- or "support": the chi-squared form against a learned density ratio
tau = exp(log_tau) with its dual variable u) and so that its embeddings of the target half of the paired frames match the
source's (a unit-variance Normal NLL).  One plain Adam step (no clipping) on the encoder's slice of the model buffer.
Not built, each raising NotImplementedError by name: calibration_mode="pair" (the 3 B-row frozen scan with the
inverse-dynamics loss), disag_model, pixel_obs=False, a data-parallel job.  DESIGN.md 6h.
"""
import glob
import os

import numpy as np
import torch

from ... import functional as Fn
from ... import ops
from ...common.buffers import CalibrationBuffer, SequenceReplayBuffer
from ...common.models.gans import VDBDiscriminator
from ...common.models.mlps import MLP
from ...common.utils import preprocess, to_np, to_torch
from .dreamer import LOG_2PI
from .models.encoder import Encoder
from .models.utils import FlatAdam
from .repo import RePo


class FinetunedRePo(RePo):
    _BUILDS_SYMBOLIC = False   # pixel_obs=False: train_encoder runs the conv encoder's passes (the reference pins uint8 frames)

    def build_models(self, config, env):
        super().build_models(config, env)
        n_enc = len(list(self.encoder.parameters()))
        self.encoder_optimizer = FlatAdam.view(self.model_optimizer, n_enc, lr=config.model_lr)
        self._scratch_gr = None
        self._enc_log = None
        self._enc_host = torch.empty(8, dtype=torch.float32).pin_memory()

    def train_encoder(self, obs, actions, rewards, nonterms):
        """repo_adapt.py:31-94.  obs (L,B,3,64,64) float32 in [-1,1] or uint8."""
        c, dev = self.c, self.device
        obs, actions, rewards, nonterms = self._prep_batch(obs, actions, rewards, nonterms)
        L, B = obs.shape[:2]
        T = L - 1
        rows = T * B
        grow = self._global_rows(rows)
        D, S = c.belief_size, c.state_size
        frames = obs[1:].reshape(rows, *obs.shape[2:])
        pe, ge = self._pg(self.encoder)
        embeds, enc_saved = Fn.encoder_fwd(pe, frames)
        pr, _ = self._pg(self.transition_model)
        b0, s0 = self._zero_state(B)
        sv = ops.rssm_observe_fwd(
            pr, b0, s0, actions[:-1].contiguous(), nonterms[:-1].reshape(T, B).contiguous(), embeds.view(T, B, -1),
            self._noise("obs_prior", (T, B, S)), self._noise("obs_post", (T, B, S)), self.transition_model.min_std_dev,
            noise=self._draw(2 * T * B * S), act=self.transition_model.act)
        feat = sv.featx[1:].reshape(rows, D + S)
        # reward NLL through the frozen head: only its input gradient
        pw, _ = self._pg(self.reward_model)
        r_pred, r_hid = ops.mlp_fwd(pw, feat, act=self.reward_model.act)
        rew_sums, drew = ops.scalar_nll(r_pred.view(-1), rewards[:-1].reshape(-1).contiguous(),
                                        nonterms[:-1].reshape(-1).contiguous(), 1.0 / grow)
        dfeat = torch.empty(rows, D + S, device=dev)
        ops.mlp_bwd(pw, feat, r_hid, drew.view(rows, 1), dparams=None, dx=dfeat, act=self.reward_model.act)
        # beta * KL(post || prior), gradient through BOTH arguments: the balanced form with alpha = 1/2, scale 2
        kl_sum, klg = ops.kl_balance(sv.prior_mean, sv.prior_std, sv.post_mean, sv.post_std, 0, 0.5, self.log_beta, 0.0,
                                     2.0 / grow)
        if self._scratch_gr is None:
            self._scratch_gr = [torch.empty_like(t) for t in pr]   # gradients of the frozen filter: discarded
        dembeds = torch.empty(rows, c.embedding_size, device=dev)
        ops.rssm_observe_bwd(pr, sv, self._scratch_gr, dfeat=dfeat, dpm=klg[0], dps=klg[1], dqm=klg[2], dqs=klg[3],
                             dembeds=dembeds, min_std=self.transition_model.min_std_dev)
        Fn.encoder_bwd(pe, frames, enc_saved, dembeds, ge, side=self._wgrad_side(B))
        opt = self.encoder_optimizer
        self._take_status()   # both scans are behind us on this stream: the step and the dual step skip on a fault
        self._allreduce(opt.grad)
        opt.clip_and_step(c.grad_clip_norm)
        kl_global = kl_sum
        if self.dp is not None:
            kl_global = kl_sum.clone()
            self._allreduce(kl_global)
        bo = self.beta_optimizer
        bo.step_count += 1
        ops.dual_step(self.log_beta, bo.exp_avg, bo.exp_avg_sq, kl_global, grow, c.target_kl, bo.lr, bo.step_count,
                      betas=bo.betas, eps=bo.eps, out=self._dual_out, skip=self._ustatus)
        # logging: one asynchronous copy, read when first needed
        self._flush_enc_log()
        buf = torch.cat([rew_sums, self._dual_out, opt.sqnorm, self._ustatus.view(torch.float32)])
        self._allreduce_scalars(buf, n_sum=2)
        self._enc_host[:8].copy_(buf, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(dev))
        self._enc_log = (ev, grow, self._restore_point)

    def _flush_enc_log(self):
        if self._enc_log is None:
            return
        ev, grow, restore = self._enc_log
        self._enc_log = None
        ev.synchronize()
        self._raise_update_fault(int(self._enc_host[7:8].view(torch.int32).item()), restore)
        rsq, rmask, kl_div, kl_loss, beta_loss, beta, gsq = self._enc_host[:7].tolist()
        reward_loss = (rsq + 0.5 * LOG_2PI * rmask) / grow
        out = {"train/reward_loss": reward_loss, "train/kl_loss": kl_loss, "train/kl_div": kl_div,
               "train/encoder_loss": reward_loss + kl_loss, "train/beta": beta, "train/beta_loss": beta_loss}
        self._last_scalars = out
        self.last_grad_norms = {"encoder": max(gsq, 0.0) ** 0.5}
        for k, v in out.items():
            self.logger.record(k, v)

    @property
    def last_scalars(self):
        self._flush_enc_log()
        return self._last_scalars

    def train_agent(self):
        """repo_adapt.py:96-107: `train_steps` encoder steps on fresh target-domain batches."""
        c = self.c
        B, L = c.batch_size, c.chunk_size
        for _ in range(c.train_steps):
            obs, actions, rewards, dones = self.buffer.sample_to_device(B, L, self.device)
            self.train_encoder(obs, actions, rewards, 1.0 - dones.float())
        self._flush_enc_log()

    def train(self):
        self.load_source_models()
        super().train()

    def load_source_models(self):
        """repo_adapt.py:113-126: the source agent's six modules from `source_dir/models.pt` (reference key layout)."""
        path = os.path.join(self.c.source_dir, "models.pt")
        if os.path.exists(path):
            ckpt = torch.load(path, map_location=self.device, weights_only=False)
            print(f"Loaded checkpoint from {path}")
            for name in ("encoder", "transition_model", "obs_model", "reward_model", "actor_model", "value_model"):
                self._load_module(getattr(self, name), ckpt[name])


class CalibratedRePo(RePo):
    _BUILDS_SYMBOLIC = False   # pixel_obs=False: the calibration frames are paired pixel frames (uint8, 6 channels)
    _LOG_KEYS = ("f_loss_src", "f_loss_tgt", "f_kl", "aln_loss", "calib_loss", "encoder_loss")
    _LOG_KEYS_SUPPORT = ("tau_loss", "tau_mean", "u_value")

    def __init__(self, config, env, eval_env, calib_env, logger):
        assert config.disag_model or config.inv_dynamics
        super().__init__(config, env, eval_env, logger)
        self.calib_env = calib_env
        self.calib_buffer = CalibrationBuffer(
            config.calibration_buffer_size, calib_env.observation_space.shape, calib_env.action_space.shape,
            obs_type=np.uint8)
        self.src_buffer = SequenceReplayBuffer(
            config.replay_size, env.observation_space.shape, env.action_space.shape,
            obs_type=np.uint8 if config.pixel_obs else np.float32)
        if getattr(config, "replay_on_device", True):
            self.calib_buffer.enable_device_mirror(self.device)
            self.src_buffer.enable_device_mirror(self.device)

    def build_models(self, config, env):
        super().build_models(config, env)
        dev = self.device
        # the reference deep-copies the encoder (repo_adapt.py:156); here its tensors are views of the model's flat buffer,
        # so a FRESH module takes the values -- built under a forked generator: like the copy, it draws nothing from
        # torch's stream, and the modules below initialise as the reference's do under the same seed
        with torch.random.fork_rng(devices=[]):
            self.src_encoder = Encoder(self._symbolic, env.observation_space.shape, config.embedding_size,
                                       config.cnn_activation_function).to(dev)
        self._load_module(self.src_encoder, self.encoder.state_dict())
        for p in self.src_encoder.parameters():
            p.requires_grad_(False)
        n_enc = len(list(self.encoder.parameters()))
        self.encoder_optimizer = FlatAdam.view(self.model_optimizer, n_enc, lr=config.model_lr)
        hidden_dims = [config.f_hidden_size] * 4
        self.disc = VDBDiscriminator(input_dim=config.embedding_size, hidden_dims=hidden_dims,
                                     latent_dim=config.f_latent_size, lr=config.f_lr, target_kl=config.f_target_kl,
                                     device=dev)
        self.log_tau = MLP(config.embedding_size, hidden_dims, 1).to(dev)
        self.tau_optimizer = FlatAdam(self.log_tau.parameters(), lr=config.tau_lr)
        self.u = torch.tensor(float(config.init_u), device=dev, requires_grad=True)
        self.u_optimizer = FlatAdam([self.u], lr=config.u_lr)
        self._cal_log = None
        self._cal_host = torch.empty(20, dtype=torch.float32).pin_memory()

    def _noise_stride(self):
        """The discriminator's passes of one calibration step draw up to 4 L B Z normals on top of an update's."""
        c = self.c
        per_update = super()._noise_stride() + 4 * c.chunk_size * c.batch_size * c.f_latent_size
        return 1 << max(int(per_update) - 1, 1).bit_length()

    # ------------------------------------------------------------------ acting with the source encoder
    @torch.no_grad()
    def expert_update_latent_and_select_action(self, belief, posterior_state, action, obs, explore=False):
        """repo_adapt.py:174-195: one filtering step on the SOURCE encoder's embedding of a source-view frame."""
        self.synchronize()
        embed = self.src_encoder(obs)
        outs = self.transition_model.observe(belief, posterior_state, action.unsqueeze(0), embed.unsqueeze(0))
        belief, posterior_state = outs[0].squeeze(0), outs[4].squeeze(0)
        action = self.actor_model.get_action(belief, posterior_state, det=not explore)
        if explore:
            action = torch.clamp(action + torch.randn_like(action) * self.c.action_noise, -1, 1)
        return belief, posterior_state, action

    def collect_calibration_data(self, expert):
        """repo_adapt.py:197-243: `calibration_buffer_size` paired transitions -- the source agent acting on the source
        view (expert) or random actions; the paired frame goes to the calibration ring, its target half to the replay ring."""
        print("Collecting calibration trajectories")
        env, c = self.calib_env, self.c
        obs = env.reset()
        if expert:
            belief, posterior_state, action_tensor = self.init_latent_and_action()
            timestep = 0
        for _ in range(c.calibration_buffer_size):
            if expert:
                obs_tensor = to_torch(preprocess(obs[:3][None]), device=self.device)
                belief, posterior_state, action_tensor = self.expert_update_latent_and_select_action(
                    belief, posterior_state, action_tensor, obs_tensor, False)
                action = to_np(action_tensor)[0]
            else:
                action = env.action_space.sample()
            next_obs, reward, done, info = env.step(action)
            if expert:
                timestep += 1
                if timestep == c.calib_time_limit:
                    done = True
                    timestep = 0
            self.calib_buffer.push(obs, action, reward, done)
            self.buffer.push(obs[3:], action, reward, done)
            obs = next_obs
            if done:
                obs = env.reset()
                if expert:
                    belief, posterior_state, action_tensor = self.init_latent_and_action()

    # ------------------------------------------------------------------ the calibration step
    def _eps(self, key, n, z):
        """One discriminator pass's noise: (explicit tensor, None) from the injected source / torch, or (None, (seed,
        offset)) = drawn in the kernel from the agent's Philox stream."""
        t = self._noise(key, (n, z))
        return (t, None) if t is not None else (None, self._draw(n * z))

    def simple_pair_calibration(self):
        """repo_adapt.py:400-482.  Three batches, drawn in the reference's order (source replay, target replay, paired)."""
        B, L, dev = self.c.batch_size, self.c.chunk_size, self.device
        aln_src = self.src_buffer.sample_to_device(B, L, dev)[0]
        aln_tgt = self.buffer.sample_to_device(B, L, dev)[0]
        cal_src, cal_tgt = self.calib_buffer.sample_to_device(B, L, dev)[:2]
        self.calibration_step(aln_src, aln_tgt, cal_src, cal_tgt)

    def calibration_step(self, aln_src_obs, aln_tgt_obs, cal_src_obs, cal_tgt_obs):
        """The arithmetic of simple_pair_calibration on four (L, B, 3, 64, 64) device batches (uint8, or float32 in [-1, 1]):
        ALL L frames of each chunk are embedded.  Noise draws, in order: disc_real, disc_fake, disc_tgt, then disc_src
        (support mode), each (L B, Z)."""
        if self.dp is not None:
            raise NotImplementedError("CalibratedRePo: a data-parallel calibration step is not built")
        c = self.c
        support = c.alignment_mode == "support"
        L, B = aln_src_obs.shape[:2]
        N, E, Z = L * B, c.embedding_size, c.f_latent_size

        def frames(o):
            assert o.dtype in (torch.uint8, torch.float32), o.dtype
            return o.reshape(N, *o.shape[2:]).contiguous()

        ps, _ = self._pg(self.src_encoder)
        pe, ge = self._pg(self.encoder)
        f_at, f_ct = frames(aln_tgt_obs), frames(cal_tgt_obs)
        aln_src, _ = Fn.encoder_fwd(ps, frames(aln_src_obs))
        aln_tgt, sv_at = Fn.encoder_fwd(pe, f_at)
        cal_src, _ = Fn.encoder_fwd(ps, frames(cal_src_obs))
        cal_tgt, sv_ct = Fn.encoder_fwd(pe, f_ct)
        # alignment: tau BEFORE the discriminator's step, d_tgt AFTER it (the updated discriminator, a fresh draw)
        tau = None
        if support:
            lt, lt_hid = self.log_tau.fwd(aln_src)
            _, tau, _ = ops.vdb_tau(lt.view(-1), want_tau=True)
        (e_r, n_r), (e_f, n_f) = self._eps("disc_real", N, Z), self._eps("disc_fake", N, Z)
        info = self.disc.train(aln_src, aln_tgt, tau, eps=(e_r, e_f), noise=(n_r, n_f))
        e_t, n_t = self._eps("disc_tgt", N, Z)
        sv = self.disc.fwd(aln_tgt, eps=e_t, noise=n_t, want_kl=False)
        aln_sum, dd = ops.vdb_loss(sv.d, ops.VDB_NEG_CHI if support else ops.VDB_BCE1, c.aln_coef / N)
        d_aln = self.disc.input_grad(sv, dd)
        # calibration: -Normal(cal_tgt, 1).log_prob(cal_src).mean() over all N E elements
        cal_sums, d_cal = ops.scalar_nll(cal_tgt.view(-1), cal_src.view(-1), None, c.calib_coef / (N * E))
        # the encoder: two batches into one gradient, a plain Adam step (repo_adapt.py:451-454: no clipping)
        Fn.encoder_bwd(pe, f_at, sv_at, d_aln, ge, accumulate=False)
        Fn.encoder_bwd(pe, f_ct, sv_ct, d_cal.view(N, E), ge, accumulate=True)
        eo = self.encoder_optimizer
        ops.grad_sqnorm(eo.grad, out=eo.sqnorm)   # logged only
        eo.step()
        parts = [info.buf, aln_sum, cal_sums[:1], eo.sqnorm, ops.grad_sqnorm(self.disc.optimizer.grad)]
        if support:
            # the density ratio (repo_adapt.py:463-478): a fourth pass on the source embeddings, then log_tau and u step
            e_s, n_s = self._eps("disc_src", N, Z)
            svs = self.disc.fwd(aln_src, eps=e_s, noise=n_s, want_kl=False)
            tau_sums, _, dlt = ops.vdb_tau(lt.view(-1), d=svs.d, u=self.u.detach().view(1), want_grad=True)
            to, uo = self.tau_optimizer, self.u_optimizer
            self.log_tau.bwd(aln_src, lt_hid, dlt.view(N, 1), dparams=[p.grad for p in self.log_tau.plist()])
            ops.grad_sqnorm(to.grad, out=to.sqnorm)
            u_old = self.u.detach().view(1).clone()
            to.step()
            torch.mul(tau_sums[1:2], -1.0 / N, out=uo.grad[:1])   # d(-u mean(tau - 1)) / du
            uo.step()
            parts += [tau_sums, u_old, self.u.detach().view(1), to.sqnorm]
        # logging: one asynchronous copy, read when first needed
        self._flush_cal_log()
        buf = torch.cat(parts)
        self._cal_host[: buf.numel()].copy_(buf, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        self._cal_log = (ev, info.scales, N, E, support)

    def _flush_cal_log(self):
        if self._cal_log is None:
            return
        ev, scales, N, E, support = self._cal_log
        self._cal_log = None
        ev.synchronize()
        h = self._cal_host.tolist()
        c = self.c
        f = {k: v * s for k, v, s in zip(("real", "fake", "kl", "gp", "beta"), h[:5], scales)}
        aln, calib = h[5] / N, h[6] / (N * E) + 0.5 * LOG_2PI
        out = {"train/f_loss_src": f["real"], "train/f_loss_tgt": f["fake"], "train/f_kl": f["kl"], "train/aln_loss": aln,
               "train/calib_loss": calib, "train/encoder_loss": c.aln_coef * aln + c.calib_coef * calib}
        self.last_grad_norms = {"encoder": max(h[7], 0.0) ** 0.5, "disc": max(h[8], 0.0) ** 0.5}
        self.last_disc_scalars = {"gp": f["gp"], "beta": f["beta"]}
        if support:
            tau_d, tau_m1, u_old, u_new, tsq = h[9:14]
            out["train/tau_loss"] = tau_d / N + u_old * tau_m1 / N
            out["train/tau_mean"] = 1.0 + tau_m1 / N
            out["train/u_value"] = u_new
            self.last_grad_norms["log_tau"] = max(tsq, 0.0) ** 0.5
        self._last_scalars = out
        for k, v in out.items():
            self.logger.record(k, v)

    @property
    def last_scalars(self):
        self._flush_cal_log()
        return self._last_scalars

    def train_agent(self):
        """repo_adapt.py:484-491."""
        mode = self.c.calibration_mode
        if mode == "pair":
            raise NotImplementedError('calibration_mode="pair" (the frozen 3 B-row scan with the inverse-dynamics loss) is '
                                      'not built; "simple_pair" is')
        if mode != "simple_pair":
            raise ValueError("Unsupported calibration mode")
        for _ in range(self.c.train_steps):
            self.simple_pair_calibration()
        self._flush_cal_log()

    def train(self):
        """repo_adapt.py:493-545: load the source agent and its replay, collect the paired frames, then interleave
        target-domain environment steps with calibration steps (the step counter advances BEFORE its periods are
        checked, as in the reference's loop)."""
        from .rollout import EpisodeDriver

        c = self.c
        self.load_source_models()
        self.load_source_data()
        if c.calibration_mode in ("pair", "simple_pair"):
            self.collect_calibration_data(expert=c.expert_calib_data)
        periodic = ((c.train_every, self.train_agent), (c.eval_every, self.eval_agent),
                    (c.checkpoint_every, self.save_checkpoint), (c.log_every, self._dump_log))
        driver = EpisodeDriver(self, self.env, explore=True)
        driver.begin()
        while self.step < c.num_steps:
            tr = driver.advance()
            self.buffer.push(tr.obs, tr.action, tr.reward, tr.done)
            if tr.done:
                driver.report("train")
                driver.begin()
            self.step += 1
            for period, job in periodic:
                if self.step % period == 0:
                    job()

    def load_source_models(self):
        """repo_adapt.py:547-564: both encoders start from the source agent's; the reward head is NOT loaded (the
        reference does not load it either)."""
        path = os.path.join(self.c.source_dir, "models.pt")
        if os.path.exists(path):
            ckpt = torch.load(path, map_location=self.device, weights_only=False)
            print(f"Loaded model from {path}")
            self._load_module(self.src_encoder, ckpt["encoder"])
            for name in ("encoder", "transition_model", "obs_model", "actor_model", "value_model"):
                self._load_module(getattr(self, name), ckpt[name])
            if self._inv_dyn and "inv_dynamics" in ckpt:
                self._load_module(self.inv_dynamics, ckpt["inv_dynamics"])

    def load_source_data(self):
        """repo_adapt.py:566-596: every `buffer*.npz` under source_dir becomes the source ring (adopt_offline)."""
        paths = list(glob.glob(os.path.join(self.c.source_dir, "buffer*.npz")))
        self.src_buffer.adopt_offline(paths, self.c.offline_truncate_size)
        for path in paths:
            print(f"Loaded buffer from {path}")
