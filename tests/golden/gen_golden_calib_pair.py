#!/usr/bin/env python3
"""Golden vectors of the REFERENCE's CalibratedRePo with calibration_mode="pair" (algorithms/repo/repo_adapt.py:245-398, the
inv_dynamics branch) on the CPU:

    python tests/golden/gen_golden_calib_pair.py [--out DIR]

writes calib_pair_js_tiny.npz (alignment_mode="js") and calib_pair_support_tiny.npz (alignment_mode="support"): two
pair_calibration steps at (L, B, A) = (8, 4, 6) with tests/calib_ref.py's CALIB_CFG.  Results only: per step the logged
scalars (train/dyn_loss among them), the discriminator's beta, u, and the gradient norms of encoder, discriminator and
log_tau, each taken as its optimiser steps; after the last step the parameter checksums of those three, of the source
encoder and of the inverse-dynamics model (which the step must leave as it found them).

All inputs are seeded as in gen_golden_calib.py; on top of them the inverse-dynamics parameters come from
tests/inv_dyn_ref.py:make_inv_params (the module's default initialisation would not be reproducible on the other side) and
tests/calib_pair_ref.py:make_pair_inputs gives the aligned batch and the paired batch actions and dones of their own and
the scan's noise.  The NoiseFeeder is queued in draw order: prior_0, post_0, ..., prior_{T-1}, post_{T-1} over the 3 B
columns [cal_src | cal_tgt | aln_tgt], then real, fake, target and, in support mode, source."""
import os
import sys
from collections import OrderedDict

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as gg  # noqa: E402  (puts the repository root on sys.path and reads --out)
import gen_golden_calib as gc  # noqa: E402

from tests import calib_pair_ref as cp  # noqa: E402
from tests import calib_ref as cr  # noqa: E402
from tests.inv_dyn_ref import make_inv_params  # noqa: E402

fx = gg.fx
L, B, H, A, N_UPDATES = 8, 4, 5, 6, 2
MODULES = ("encoder", "disc", "log_tau", "src_encoder", "inv_dynamics")


def run_pair_case(Calibrated, mode, feeder, out_path):
    cfg = fx.default_config(algo="repo_calibrate", batch_size=B, chunk_size=L, horizon=H, alignment_mode=mode,
                            **{**cr.CALIB_CFG, "calibration_mode": "pair"})
    logger = gg.RecLogger()
    algo = Calibrated(cfg, gg.FakeEnv(A), gg.FakeEnv(A), gc.PairedEnv(A), logger)
    gc.load_seeded(algo)
    inv = make_inv_params(cfg.belief_size, cfg.state_size, A, cfg.inv_dynamics_hidden_size)
    assert list(algo.inv_dynamics.state_dict().keys()) == list(inv.keys())
    algo.inv_dynamics.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in inv.items()})
    algo.src_buffer, algo.buffer, algo.calib_buffer = gc.FixedBuffer(), gc.FixedBuffer(), gc.FixedBuffer()
    support = mode == "support"
    modules = ("encoder", "disc") + (("log_tau",) if support else ())
    norms = {}
    for name, opt in (("encoder", algo.encoder_optimizer), ("disc", algo.disc.optimizer), ("log_tau", algo.tau_optimizer)):
        gc.record_norm_at_step(opt, getattr(algo, name), norms, name)
    g = OrderedDict()
    g["meta"] = np.array([L, B, H, A, N_UPDATES], dtype=np.int64)
    scalar_keys = None
    T = L - 1
    for u in range(N_UPDATES):
        frames, noise = cr.make_calib_inputs(L, B, A, cfg.f_latent_size, u)
        pair, scan_noise = cp.make_pair_inputs(L, B, A, cfg.state_size, u)
        for k in ("aln_dones", "cal_dones"):   # both masks select some rows and drop others
            n_sel, n_rows = cp.selected(1 - pair[k])
            assert 0 < n_sel < n_rows, (k, u, n_sel, n_rows)
        algo.src_buffer.batch = (frames["aln_src"], None, None, None)
        algo.buffer.batch = (frames["aln_tgt"], pair["aln_actions"], None, pair["aln_dones"])
        algo.calib_buffer.batch = (frames["cal_src"], frames["cal_tgt"], pair["cal_actions"], None, pair["cal_dones"])
        feeder.queue = [scan_noise[k][t] for t in range(T) for k in ("cal_prior", "cal_post")]
        feeder.queue += [noise[k] for k in ("disc_real", "disc_fake", "disc_tgt") + (("disc_src",) if support else ())]
        logger.kv.clear()
        norms.clear()
        algo.pair_calibration()
        assert sorted(norms) == sorted(modules)
        assert not feeder.queue, "noise left over: the draw order differs"
        assert all(p.grad is None for p in algo.transition_model.parameters())   # frozen: not even a gradient
        keys = sorted(logger.kv.keys())
        scalar_keys = scalar_keys or keys
        assert keys == scalar_keys and ("train/tau_loss" in keys) == support and "train/dyn_loss" in keys
        g[f"u{u}/scalars"] = np.array([logger.kv[k] for k in keys], dtype=np.float64)
        g[f"u{u}/disc_beta"] = np.array(float(algo.disc.beta), dtype=np.float64)
        g[f"u{u}/u"] = np.array(float(algo.u.detach()), dtype=np.float64)
        g[f"u{u}/grad_norms"] = np.array([norms[m] for m in modules], dtype=np.float64)
        print(f"  [{os.path.basename(out_path)}] step {u}: "
              + " ".join(f"{k.split('/')[-1]}={logger.kv[k]:.6g}" for k in keys), flush=True)
    g["scalar_keys"] = np.array(scalar_keys)
    g["grad_norm_modules"] = np.array(modules)
    names, sums, abssums = [], [], []
    for mod in MODULES:
        for k, v in getattr(algo, mod).state_dict().items():
            names.append(f"{mod}.{k}")
            sums.append(float(v.double().sum()))
            abssums.append(float(v.double().abs().sum()))
    for k, v in inv.items():   # no optimiser applies the gradient the inverse-dynamics model collects
        assert np.array_equal(algo.inv_dynamics.state_dict()[k].numpy(), v), k
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
        run_pair_case(CalibratedRePo, mode, feeder, os.path.join(gg.OUT, f"calib_pair_{mode}_tiny.npz"))


if __name__ == "__main__":
    main()
