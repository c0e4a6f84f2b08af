"""Test-time adaptation of a trained RePo agent: FinetunedRePo (its ENCODER only, on target-domain replay) and
CalibratedRePo (a target encoder aligned with the frozen source encoder through a VDB discriminator and paired frames).

Reference: `FinetunedRePo`, /root/reference/algorithms/repo/repo_adapt.py:26-127 (driven by experiments/adapt_repo.py:220):
the source agent's world model, reward head, actor and critic stay frozen; on target-domain replay the encoder is
trained to keep the reward predictable and the posterior close to the (frozen) prior -- reward NLL + beta * (KL -
target_kl), the full KL gradient through both arguments (repo_adapt.py:63-76) -- with the same dual ascent on log_beta as
RePo.  Here: encoder forward, the observe scan, the reward head's input gradient, the KL reduction, the reverse scan (for
its gradient into the embeddings; the frozen weights' gradients it also forms are discarded) and the encoder backward,
all on the update's kernels; one Adam over the encoder's slice of the model buffer (`FlatAdam.view`).

`CalibratedRePo` (repo_adapt.py:136-596): the frozen source encoder embeds source-domain replay and the source half of
paired calibration frames; the target encoder is trained so that a variational-bottleneck discriminator
(common/models/gans.py, csrc/vdb.hip) cannot tell its embeddings of target replay from the source's (alignment_mode "js"
-- anything but "support" -- or "support": the chi-squared form against a learned density ratio tau = exp(log_tau) with
its dual variable u) and
 * calibration_mode="simple_pair": so that its embeddings of the target half of the paired frames match the source's (a
   unit-variance Normal NLL);
 * calibration_mode="pair" (repo_adapt.py:245-398): through the FROZEN world model's latents -- the frozen
   inverse-dynamics model must explain the target trajectories (dyn_loss) and the transitions from a source latent to the
   paired target latent (calib_loss); the gradient reaches the encoder through a reverse scan that forms no weight
   gradient (repo_rssm_observe_bwd_frozen).  DESIGN.md 6i.
One plain Adam step (no clipping) on the encoder's slice of the model buffer.
Not built, each raising NotImplementedError by name: disag_model (so "pair" runs the reference's inv_dynamics branch
only), pixel_obs=False, a data-parallel job.  DESIGN.md 6h, 6i.
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
    _BUILDS_PCONT = False   # pcont=True: train_encoder has no imagination to discount; built for Dreamer and RePo
    _BUILDS_SLOW_VALUE = False   # slow_value_target=True: built and tested for Dreamer and RePo
    _BUILDS_ACTOR_GRAD = False   # actor_grad="reinforce" / "both": built and tested for Dreamer and RePo
    _BUILDS_RETURN_NORM = False   # return_norm=True: built and tested for Dreamer and RePo
    _BUILDS_VALUE_DIST = False   # value_dist="twohot": built and tested for Dreamer and RePo
    _BUILDS_OPTIM_RULES = False   # grad_clip="agc" / optimizer="laprop": built and tested for Dreamer and RePo
    _BUILDS_REWARD_DIST = False   # reward_dist="twohot": built and tested for Dreamer and RePo
    _BUILDS_OBS_SYMLOG = False   # obs_symlog=True: built and tested for Dreamer and RePo on state vectors
    _BUILDS_KL_SCALES = False   # kl_dyn_scale / kl_rep_scale: built and tested for Dreamer
    _BUILDS_VALUE_SLOW_REG = False   # value_slow_reg > 0: built and tested for Dreamer and RePo
    _BUILDS_BIN_SPACE = False   # value_bin_space / reward_bin_space="symexp": built and tested for Dreamer and RePo
    _BUILDS_SYMBOLIC = False   # pixel_obs=False: train_encoder runs the conv encoder's passes (the reference pins uint8 frames)
    _BUILDS_CONV_PRECISION = False   # conv_precision="high": built and tested for Dreamer and RePo

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
    _BUILDS_PCONT = False   # pcont=True: built and tested for Dreamer and RePo
    _BUILDS_SLOW_VALUE = False   # slow_value_target=True: built and tested for Dreamer and RePo
    _BUILDS_ACTOR_GRAD = False   # actor_grad="reinforce" / "both": built and tested for Dreamer and RePo
    _BUILDS_RETURN_NORM = False   # return_norm=True: built and tested for Dreamer and RePo
    _BUILDS_VALUE_DIST = False   # value_dist="twohot": built and tested for Dreamer and RePo
    _BUILDS_OPTIM_RULES = False   # grad_clip="agc" / optimizer="laprop": built and tested for Dreamer and RePo
    _BUILDS_REWARD_DIST = False   # reward_dist="twohot": built and tested for Dreamer and RePo
    _BUILDS_OBS_SYMLOG = False   # obs_symlog=True: built and tested for Dreamer and RePo on state vectors
    _BUILDS_KL_SCALES = False   # kl_dyn_scale / kl_rep_scale: built and tested for Dreamer
    _BUILDS_VALUE_SLOW_REG = False   # value_slow_reg > 0: built and tested for Dreamer and RePo
    _BUILDS_BIN_SPACE = False   # value_bin_space / reward_bin_space="symexp": built and tested for Dreamer and RePo
    _BUILDS_SYMBOLIC = False   # pixel_obs=False: the calibration frames are paired pixel frames (uint8, 6 channels)
    _BUILDS_CONV_PRECISION = False   # conv_precision="high": built and tested for Dreamer and RePo
    _LOG_KEYS = ("f_loss_src", "f_loss_tgt", "f_kl", "aln_loss", "calib_loss", "encoder_loss")
    _LOG_KEYS_PAIR = ("dyn_loss",)
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
        """The discriminator's passes of one calibration step draw up to 4 L B Z normals on top of an update's; the
        "pair" step's scans over its 3 B columns draw 2 T 3B S more."""
        c = self.c
        per_update = super()._noise_stride() + 4 * c.chunk_size * c.batch_size * c.f_latent_size
        if c.calibration_mode == "pair":
            per_update += 2 * (c.chunk_size - 1) * 3 * c.batch_size * self.transition_model.state_size
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
        L, B = aln_src_obs.shape[:2]
        N, E = L * B, c.embedding_size
        ps, _ = self._pg(self.src_encoder)
        pe, ge = self._pg(self.encoder)
        f_at, f_ct = self._frames(aln_tgt_obs), self._frames(cal_tgt_obs)
        aln_src, _ = Fn.encoder_fwd(ps, self._frames(aln_src_obs))
        aln_tgt, sv_at = Fn.encoder_fwd(pe, f_at)
        cal_src, _ = Fn.encoder_fwd(ps, self._frames(cal_src_obs))
        cal_tgt, sv_ct = Fn.encoder_fwd(pe, f_ct)
        al = self._alignment(aln_src, aln_tgt)
        # calibration: -Normal(cal_tgt, 1).log_prob(cal_src).mean() over all N E elements
        cal_sums, d_cal = ops.scalar_nll(cal_tgt.view(-1), cal_src.view(-1), None, c.calib_coef / (N * E))
        # the encoder: two batches into one gradient, a plain Adam step (repo_adapt.py:451-454: no clipping)
        Fn.encoder_bwd(pe, f_at, sv_at, al["d_aln"], ge, accumulate=False)
        Fn.encoder_bwd(pe, f_ct, sv_ct, d_cal.view(N, E), ge, accumulate=True)
        eo = self.encoder_optimizer
        ops.grad_sqnorm(eo.grad, out=eo.sqnorm)   # logged only
        eo.step()
        parts = [al["info"].buf, al["aln_sum"], cal_sums[:1], eo.sqnorm, ops.grad_sqnorm(self.disc.optimizer.grad)]
        parts += self._support_tail(aln_src, al)
        self._queue_cal_log(parts, al["info"].scales, N, E, None)

    @staticmethod
    def _frames(o):
        assert o.dtype in (torch.uint8, torch.float32), o.dtype
        return o.reshape(o.shape[0] * o.shape[1], *o.shape[2:]).contiguous()

    def _alignment(self, aln_src, aln_tgt):
        """The alignment half of both calibration modes on the (N, E) embeddings of source and target replay
        (repo_adapt.py:296-313 = 426-443): tau BEFORE the discriminator's step, d_tgt AFTER it (the updated discriminator,
        a fresh draw).  -> the discriminator's info, the loss sum and d_aln = aln_coef d aln_loss / d aln_tgt (N, E)."""
        c = self.c
        support = c.alignment_mode == "support"
        N, Z = aln_src.shape[0], c.f_latent_size
        tau = lt = lt_hid = None
        if support:
            lt, lt_hid = self.log_tau.fwd(aln_src)
            _, tau, _ = ops.vdb_tau(lt.view(-1), want_tau=True)
        (e_r, n_r), (e_f, n_f) = self._eps("disc_real", N, Z), self._eps("disc_fake", N, Z)
        info = self.disc.train(aln_src, aln_tgt, tau, eps=(e_r, e_f), noise=(n_r, n_f))
        e_t, n_t = self._eps("disc_tgt", N, Z)
        sv = self.disc.fwd(aln_tgt, eps=e_t, noise=n_t, want_kl=False)
        aln_sum, dd = ops.vdb_loss(sv.d, ops.VDB_NEG_CHI if support else ops.VDB_BCE1, c.aln_coef / N)
        return dict(info=info, aln_sum=aln_sum, d_aln=self.disc.input_grad(sv, dd), lt=lt, lt_hid=lt_hid)

    def _support_tail(self, aln_src, al):
        """Support mode, behind the encoder's step: the density ratio (repo_adapt.py:379-398 = 463-478) -- a fourth pass
        on the source embeddings, then log_tau and u step.  -> its log parts (none in js mode)."""
        if self.c.alignment_mode != "support":
            return []
        N, Z = aln_src.shape[0], self.c.f_latent_size
        lt, lt_hid = al["lt"], al["lt_hid"]
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
        return [tau_sums, u_old, self.u.detach().view(1), to.sqnorm]

    def _queue_cal_log(self, parts, scales, N, E, pair):
        """Logging: one asynchronous copy, read when first needed.  pair: None, or the "pair" step's restore point (its
        parts then hold two (NLL sum, selected rows) pairs and end with the scans' status word)."""
        self._flush_cal_log()
        buf = torch.cat(parts)
        self._cal_host[: buf.numel()].copy_(buf, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.device))
        self._cal_log = (ev, scales, N, E, self.c.alignment_mode == "support", pair, buf.numel())

    def pair_calibration(self):
        """repo_adapt.py:245-269.  The same three batches in the same order, with the actions and dones of the target
        replay and of the paired ring."""
        B, L, dev = self.c.batch_size, self.c.chunk_size, self.device
        aln_src = self.src_buffer.sample_to_device(B, L, dev)[0]
        aln_tgt, aln_act, _, aln_done = self.buffer.sample_to_device(B, L, dev)
        cal_src, cal_tgt, cal_act, _, cal_done = self.calib_buffer.sample_to_device(B, L, dev)
        self.pair_calibration_step(aln_src, aln_tgt, aln_act, 1.0 - aln_done.float(), cal_src, cal_tgt, cal_act,
                                   1.0 - cal_done.float())

    def pair_calibration_step(self, aln_src_obs, aln_tgt_obs, aln_actions, aln_nonterms, cal_src_obs, cal_tgt_obs,
                              cal_actions, cal_nonterms):
        """The arithmetic of pair_calibration (repo_adapt.py:271-398, the inv_dynamics branch) on device batches: four
        (L, B, 3, 64, 64) frame batches, actions (L, B, A) and nonterms (L, B, 1) of the target replay and of the paired
        ring.  The reference's one scan over the 3 B columns [cal_src | cal_tgt | aln_tgt] runs as two -- its rows are
        independent: forward only over cal_src (no gradient path: frozen encoder, frozen filter), forward and the frozen
        reverse over [cal_tgt | aln_tgt].  Noise, in order: cal_prior, cal_post (T, 3 B, S) in the reference's column
        order, then the discriminator's draws as in calibration_step.  DESIGN.md 6i."""
        if self.dp is not None:
            raise NotImplementedError("CalibratedRePo: a data-parallel calibration step is not built")
        if not self._inv_dyn:
            raise NotImplementedError('calibration_mode="pair" is built on the inverse-dynamics model (inv_dynamics=True); '
                                      "the disag_model ensemble is not built")
        c = self.c
        self._update_seq += 1
        self._restore_point = (self._update_seq, self._noise_counter, [(o, o.step_count) for o in self._steppers()])
        L, B = aln_src_obs.shape[:2]
        N, E = L * B, c.embedding_size
        assert L >= 3, "the inverse-dynamics rows need chunks of three frames at least"
        aln_actions, cal_actions = aln_actions.float().contiguous(), cal_actions.float().contiguous()
        aln_nonterms, cal_nonterms = aln_nonterms.float().reshape(L, B), cal_nonterms.float().reshape(L, B)
        ps, _ = self._pg(self.src_encoder)
        pe, ge = self._pg(self.encoder)
        f_at, f_ct = self._frames(aln_tgt_obs), self._frames(cal_tgt_obs)
        aln_src, _ = Fn.encoder_fwd(ps, self._frames(aln_src_obs))
        aln_tgt, sv_at = Fn.encoder_fwd(pe, f_at)
        cal_src, _ = Fn.encoder_fwd(ps, self._frames(cal_src_obs))
        cal_tgt, sv_ct = Fn.encoder_fwd(pe, f_ct)
        lat = self._latent_losses(cal_src.view(L, B, E), cal_tgt.view(L, B, E), aln_tgt.view(L, B, E), cal_actions,
                                  cal_nonterms, aln_actions, aln_nonterms)
        # the two forward scans and the reverse one are behind us on this stream: the encoder's step (and log_tau's and
        # u's) skips on a fault.  The discriminator's optimiser and its beta live on self.disc and do step
        self._take_status()
        al = self._alignment(aln_src, aln_tgt)
        # -- the encoder: aln_tgt takes the alignment gradient on all L frames and the scan's on frames 1..L-1, cal_tgt
        # the scan's alone (frame 0: zeros)
        d_at = al["d_aln"].view(L, B, E)
        d_at[1:] += lat["d_aln_tgt"]
        Fn.encoder_bwd(pe, f_at, sv_at, d_at.view(N, E), ge, accumulate=False)
        Fn.encoder_bwd(pe, f_ct, sv_ct, lat["d_cal_tgt"].view(N, E), ge, accumulate=True)
        eo = self.encoder_optimizer
        ops.grad_sqnorm(eo.grad, out=eo.sqnorm)   # logged only
        eo.step()
        parts = [al["info"].buf, al["aln_sum"], lat["dyn_sums"], lat["cal_sums"], eo.sqnorm,
                 ops.grad_sqnorm(self.disc.optimizer.grad)]
        parts += self._support_tail(aln_src, al)
        parts.append(self._ustatus.view(torch.float32))
        self._queue_cal_log(parts, al["info"].scales, N, E, self._restore_point)

    def _latent_losses(self, cal_src, cal_tgt, aln_tgt, cal_actions, cal_nonterms, aln_actions, aln_nonterms):
        """dyn_coef dyn_loss + calib_coef calib_loss of the "pair" step from the (L, B, E) embeddings, actions (L, B, A)
        and nonterms (L, B): the two scans, both losses through the frozen inverse-dynamics model, and the way back to
        the embeddings.  -> dyn_sums, cal_sums (each [NLL sum over the selected rows, selected rows]), d_cal_tgt (L, B, E)
        with frame 0 zero, d_aln_tgt (T, B, E) for frames 1..L-1.  cal_src has no gradient path: its scan is never
        reversed."""
        c, dev, tm, inv = self.c, self.device, self.transition_model, self.inv_dynamics
        L, B, E = cal_src.shape
        T, D, S = L - 1, c.belief_size, c.state_size
        F_, Nr = D + S, (T - 1) * B
        # -- the scans (repo_adapt.py:271-294), one after the other on this stream: the column-split engine's exchange
        # buffer and the status word are shared
        pr, _ = self._pg(tm)
        eps_p, eps_q = self._noise("cal_prior", (T, 3 * B, S)), self._noise("cal_post", (T, 3 * B, S))
        cut = lambda e, lo, hi: None if e is None else e[:, lo:hi].contiguous()   # noqa: E731
        draw = (lambda n: self._draw(n)) if eps_p is None else (lambda n: (0, 0))
        emb = lambda e: e[1:]   # noqa: E731
        b0, s0 = self._zero_state(B)
        sv_s = ops.rssm_observe_fwd(pr, b0, s0, cal_actions[:-1], cal_nonterms[:-1], emb(cal_src), cut(eps_p, 0, B),
                                    cut(eps_q, 0, B), tm.min_std_dev, noise=draw(2 * T * B * S), act=tm.act)
        b0, s0 = self._zero_state(2 * B)
        sv_t = ops.rssm_observe_fwd(pr, b0, s0, torch.cat((cal_actions[:-1], aln_actions[:-1]), 1),
                                    torch.cat((cal_nonterms[:-1], aln_nonterms[:-1]), 1),
                                    torch.cat((emb(cal_tgt), emb(aln_tgt)), 1), cut(eps_p, B, 3 * B), cut(eps_q, B, 3 * B),
                                    tm.min_std_dev, noise=draw(2 * T * 2 * B * S), act=tm.act)
        lat_s, lat_ct, lat_at = sv_s.featx[1:], sv_t.featx[1:, :B], sv_t.featx[1:, B:]
        # -- both losses through the frozen inverse-dynamics model in one chain: rows [dyn | calib]
        x = torch.empty(2 * Nr, F_ + D, device=dev)
        ops.inv_dyn_pack_pair(lat_at, lat_at, D, out=x[:Nr])     # [aln belief_t | aln post_t | aln belief_t+1]
        ops.inv_dyn_pack_pair(lat_s, lat_ct, D, out=x[Nr:])      # [src belief_t | src post_t | tgt belief_t+1]
        pi, _ = self._pg(inv)
        raw, hid = ops.mlp_fwd(pi, x, act=inv.act)
        draw_ = torch.empty_like(raw)
        A = aln_actions.shape[2]
        dyn_sums, _ = ops.normal_nll_rows(raw[:Nr], aln_actions[1:-1].reshape(Nr, A), aln_nonterms[1:-1].reshape(Nr),
                                          inv.min_std_dev, draw=draw_[:Nr])
        cal_sums, _ = ops.normal_nll_rows(raw[Nr:], cal_actions[1:-1].reshape(Nr, A), cal_nonterms[1:-1].reshape(Nr),
                                          inv.min_std_dev, draw=draw_[Nr:])
        dx = torch.empty_like(x)
        ops.mlp_bwd(pi, x, hid, draw_, dparams=None, dx=dx, act=inv.act)
        # -- the coefficients enter where the rows' gradients go back to the latents; then the frozen reverse scan
        dfeat = torch.empty(T, 2 * B, F_, device=dev)
        ops.inv_dyn_unpack_pair(None, dx[Nr:], D, dfeat[:, :B], 0.0, c.calib_coef)
        ops.inv_dyn_unpack_pair(dx[:Nr], dx[:Nr], D, dfeat[:, B:], c.dyn_coef, c.dyn_coef)
        dembeds = torch.empty(T, 2 * B, E, device=dev)
        ops.rssm_observe_bwd(pr, sv_t, None, dfeat=dfeat, dembeds=dembeds, min_std=tm.min_std_dev)
        d_ct = torch.empty(L, B, E, device=dev)
        d_ct[0].zero_()   # frame 0 never enters the scan
        d_ct[1:] = dembeds[:, :B]
        return dict(dyn_sums=dyn_sums, cal_sums=cal_sums, d_cal_tgt=d_ct, d_aln_tgt=dembeds[:, B:])

    def _flush_cal_log(self):
        if self._cal_log is None:
            return
        ev, scales, N, E, support, pair, n = self._cal_log
        self._cal_log = None
        ev.synchronize()
        h = self._cal_host.tolist()
        c = self.c
        f = {k: v * s for k, v, s in zip(("real", "fake", "kl", "gp", "beta"), h[:5], scales)}
        aln = h[5] / N
        out = {"train/f_loss_src": f["real"], "train/f_loss_tgt": f["fake"], "train/f_kl": f["kl"], "train/aln_loss": aln}
        if pair is None:
            calib = h[6] / (N * E) + 0.5 * LOG_2PI
            out.update({"train/calib_loss": calib, "train/encoder_loss": c.aln_coef * aln + c.calib_coef * calib})
            h = h[7:]
        else:
            try:
                self._raise_update_fault(int(self._cal_host[n - 1 : n].view(torch.int32).item()), pair)
            except Exception as fault:  # noqa: BLE001  (RepoHipError)
                raise type(fault)(f"{fault} -- of this calibration step the discriminator's own step (its Adam step and "
                                  "beta) stands: it is not among the agent's optimisers") from None
            # no selected row: the gradient was exact zeros and the log says nan, as the reference's mean over no rows
            dyn, calib = (h[i] / h[i + 1] if h[i + 1] > 0 else float("nan") for i in (6, 8))
            out.update({"train/dyn_loss": dyn, "train/calib_loss": calib,
                        "train/encoder_loss": c.aln_coef * aln + c.dyn_coef * dyn + c.calib_coef * calib})
            h = h[10:]
        self.last_grad_norms = {"encoder": max(h[0], 0.0) ** 0.5, "disc": max(h[1], 0.0) ** 0.5}
        self.last_disc_scalars = {"gp": f["gp"], "beta": f["beta"]}
        if support:
            tau_d, tau_m1, u_old, u_new, tsq = h[2:7]
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
        if mode not in ("pair", "simple_pair"):
            raise ValueError("Unsupported calibration mode")
        step = self.pair_calibration if mode == "pair" else self.simple_pair_calibration
        for _ in range(self.c.train_steps):
            step()
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
