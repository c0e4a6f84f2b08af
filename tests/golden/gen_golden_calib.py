#!/usr/bin/env python3
"""Golden vectors of the REFERENCE's CalibratedRePo (algorithms/repo/repo_adapt.py:136-596) on the CPU:

    python tests/golden/gen_golden_calib.py [--out DIR]

writes calib_js_tiny.npz (alignment_mode="js") and calib_support_tiny.npz (alignment_mode="support"): two
simple_pair_calibration steps at (L, B, A) = (8, 4, 6) with inv_dynamics=True, calibration_mode="simple_pair" and the
reference's discriminator widths (256 / 64).  Results only: per step the logged scalars, the discriminator's beta, u, and
the gradient norms of encoder, discriminator and log_tau, each taken as its optimiser steps; after the last step the parameter checksums of the three.

All inputs are seeded: the six modules from fx.make_params (the source encoder seed 7, the target encoder seed 9),
tests/calib_ref.py's make_disc_params / make_tau_params, and its make_calib_inputs for the frame batches the three buffers
hand out (stand-in buffers: the rings themselves are compared in tests/test_calib_cpu.py) and the noise, which is served
through the NoiseFeeder in draw order: real, fake, target, then source in support mode."""
import os
import sys
from collections import OrderedDict

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as gg  # noqa: E402  (puts the repository root on sys.path and reads --out)

from tests import calib_ref as cr  # noqa: E402

fx = gg.fx
L, B, H, A, N_UPDATES = 8, 4, 5, 6, 2
CALIB_CFG = cr.CALIB_CFG


class FixedBuffer:
    """Stands in for a ring: sample() hands out the step's seeded batch."""

    def __init__(self):
        self.batch = None

    def sample(self, batch_size, seq_len):
        assert self.batch[0].shape[:2] == (seq_len, batch_size)
        return self.batch


class PairedEnv(gg.FakeEnv):
    def __init__(self, A):
        super().__init__(A)
        self.observation_space = gg.FakeSpace((6, 64, 64))


def load_seeded(algo):
    params = fx.make_params(A, seed=7)
    gg.load_params(algo, params)
    algo.src_encoder.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in params["encoder"].items()})
    tgt = fx.make_params(A, seed=9)["encoder"]
    algo.encoder.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in tgt.items()})
    c = algo.c
    for mod, p in ((algo.disc, cr.make_disc_params(c.embedding_size, c.f_hidden_size, c.f_latent_size)),
                   (algo.log_tau, cr.make_tau_params(c.embedding_size, c.f_hidden_size))):
        assert list(mod.state_dict().keys()) == list(p.keys())
        mod.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in p.items()})


def record_norm_at_step(optimizer, module, norms, name):
    """The gradient norm of `module` as its optimiser steps.  Read after the whole calibration step it would be another
    quantity for the discriminator: the reference never zeroes the gradients the encoder's and the density ratio's
    backward passes leave in the discriminator's parameters (they are zeroed by its next train call)."""
    step = optimizer.step

    def hooked(*a, **k):
        norms[name] = float(np.sqrt(sum(float((p.grad.double() ** 2).sum()) for p in module.parameters())))
        return step(*a, **k)

    optimizer.step = hooked


def run_calib_case(Calibrated, mode, feeder, out_path):
    cfg = fx.default_config(algo="repo_calibrate", batch_size=B, chunk_size=L, horizon=H, alignment_mode=mode, **CALIB_CFG)
    logger = gg.RecLogger()
    algo = Calibrated(cfg, gg.FakeEnv(A), gg.FakeEnv(A), PairedEnv(A), logger)
    load_seeded(algo)
    algo.src_buffer, algo.buffer, algo.calib_buffer = FixedBuffer(), FixedBuffer(), FixedBuffer()
    support = mode == "support"
    modules = ("encoder", "disc") + (("log_tau",) if support else ())
    norms = {}
    for name, opt in (("encoder", algo.encoder_optimizer), ("disc", algo.disc.optimizer), ("log_tau", algo.tau_optimizer)):
        record_norm_at_step(opt, getattr(algo, name), norms, name)
    g = OrderedDict()
    g["meta"] = np.array([L, B, H, A, N_UPDATES], dtype=np.int64)
    scalar_keys = None
    for u in range(N_UPDATES):
        frames, noise = cr.make_calib_inputs(L, B, A, cfg.f_latent_size, u)
        _, actions, rewards, dones = fx.make_batch(L, B, A, seed=51 + u)
        algo.src_buffer.batch = (frames["aln_src"], actions, rewards, dones)
        algo.buffer.batch = (frames["aln_tgt"], actions, rewards, dones)
        algo.calib_buffer.batch = (frames["cal_src"], frames["cal_tgt"], actions, rewards, dones)
        feeder.queue = [noise[k] for k in ("disc_real", "disc_fake", "disc_tgt") + (("disc_src",) if support else ())]
        logger.kv.clear()
        norms.clear()
        algo.simple_pair_calibration()
        assert sorted(norms) == sorted(modules)
        assert not feeder.queue, "noise left over: the draw order differs"
        keys = sorted(logger.kv.keys())
        scalar_keys = scalar_keys or keys
        assert keys == scalar_keys and ("train/tau_loss" in keys) == support
        g[f"u{u}/scalars"] = np.array([logger.kv[k] for k in keys], dtype=np.float64)
        g[f"u{u}/disc_beta"] = np.array(float(algo.disc.beta), dtype=np.float64)
        g[f"u{u}/u"] = np.array(float(algo.u.detach()), dtype=np.float64)
        g[f"u{u}/grad_norms"] = np.array([norms[m] for m in modules], dtype=np.float64)
        print(f"  [{os.path.basename(out_path)}] step {u}: "
              + " ".join(f"{k.split('/')[-1]}={logger.kv[k]:.6g}" for k in keys), flush=True)
    g["scalar_keys"] = np.array(scalar_keys)
    g["grad_norm_modules"] = np.array(modules)
    names, sums, abssums = [], [], []
    for mod in ("encoder", "disc", "log_tau", "src_encoder"):
        for k, v in getattr(algo, mod).state_dict().items():
            names.append(f"{mod}.{k}")
            sums.append(float(v.double().sum()))
            abssums.append(float(v.double().abs().sum()))
    g["param_names"], g["param_sums"], g["param_abssums"] = (np.array(names), np.array(sums, dtype=np.float64),
                                                             np.array(abssums, dtype=np.float64))
    np.savez_compressed(out_path, **g)
    print(f"wrote {out_path} ({os.path.getsize(out_path)} bytes)")


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    gg.import_reference()
    from algorithms.repo import CalibratedRePo

    feeder = gg.NoiseFeeder()
    gg.install_patches(feeder, {"clip_calls": [], "total_norms": []})
    for mode in ("js", "support"):
        run_calib_case(CalibratedRePo, mode, feeder, os.path.join(gg.OUT, f"calib_{mode}_tiny.npz"))


if __name__ == "__main__":
    main()
