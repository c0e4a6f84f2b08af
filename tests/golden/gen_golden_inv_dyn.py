#!/usr/bin/env python3
"""Golden vectors of the REFERENCE's RePo and Dreamer with inv_dynamics=True, at the tiny shapes of repo_tiny.npz /
dreamer_relu_tiny.npz, for the same number of updates and from the same seeds:

    python tests/golden/gen_golden_inv_dyn.py [--out DIR]

writes repo_invdyn_tiny.npz (RePo, elu, inv_dynamics_hidden_size=512) and dreamer_invdyn_tiny.npz (Dreamer,
dense_activation_function="relu", inv_dynamics_hidden_size=100).  Results only: the keys of the tiny fixtures, plus per
update the pre-clip total norm of the inverse-dynamics gradient (u*/inv_dynamics_norm) and, after the last update, the
checksums of its parameters (inv_param_*).  The module's parameters come from tests/inv_dyn_ref.py:make_inv_params.

The update loop is this file's own: with the auxiliary the reference's clip_grad_norm_ calls of one update are model,
inv_dynamics, actor, value, and gen_golden.py:run_case indexes them by position.  The auxiliary is detached from the
world model and draws no noise, so everything the tiny fixtures also hold must come out unchanged
(tests/test_golden_inv_dyn_recipe.py)."""
import os
import sys
from collections import OrderedDict

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as gg  # noqa: E402  (puts the repository root on sys.path and reads --out)

from tests.inv_dyn_ref import make_inv_params  # noqa: E402

fx = gg.fx


def run_inv_case(Algo, algo_name, L, B, H, A, n_updates, feeder, record, out_path, **over):
    cfg = fx.default_config(algo=algo_name, batch_size=B, chunk_size=L, horizon=H, inv_dynamics=True,
                            inv_dynamics_lr=3e-4, **over)
    logger = gg.RecLogger()
    algo = Algo(cfg, gg.FakeEnv(A), gg.FakeEnv(A), logger)
    gg.load_params(algo, fx.make_params(A, seed=7))
    inv = make_inv_params(cfg.belief_size, cfg.state_size, A, cfg.inv_dynamics_hidden_size)
    assert list(algo.inv_dynamics.state_dict().keys()) == list(inv.keys())
    algo.inv_dynamics.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in inv.items()})
    T = L - 1
    g = OrderedDict()
    g["meta"] = np.array([L, B, H, A, n_updates], dtype=np.int64)
    g["inv_hidden"] = np.array(cfg.inv_dynamics_hidden_size, dtype=np.int64)
    scalar_keys = None
    for u in range(n_updates):
        obs_u8, actions, rewards, dones = fx.make_batch(L, B, A, seed=11 + u)
        selected = int((1 - dones)[1:-1].sum())
        assert 0 < selected < (T - 1) * B, selected   # the mask selects some rows and drops some
        noise = fx.make_noise(L, B, H, A, seed=101 + u)
        feeder.load(noise, T, H)
        record["clip_calls"].clear()
        record["total_norms"].clear()
        logger.kv.clear()
        beliefs, post = algo.train_dynamics(torch.from_numpy(fx.preprocess_u8(obs_u8)), torch.from_numpy(actions),
                                            torch.from_numpy(rewards), torch.from_numpy(1 - dones))
        algo.train_actor_critic(beliefs.flatten(0, 1), post.flatten(0, 1))
        assert not feeder.queue, "noise left over: draw order differs from SURVEY 8c"
        keys = sorted(logger.kv.keys())
        scalar_keys = scalar_keys or keys
        assert keys == scalar_keys and "train/inv_dyn_loss" in keys
        g[f"u{u}/scalars"] = np.array([logger.kv[k] for k in keys], dtype=np.float64)
        if hasattr(algo, "log_beta"):
            g[f"u{u}/log_beta"] = np.array(algo.log_beta.item(), dtype=np.float64)
        # clip_grad_norm_ calls of one update: model, inv_dynamics, actor, value
        model, inv_c, actor, value = record["clip_calls"]
        assert len(inv_c) == len(list(algo.inv_dynamics.parameters()))
        tn = record["total_norms"]
        g[f"u{u}/total_norms"] = np.array([tn[0], tn[2], tn[3]], dtype=np.float64)
        g[f"u{u}/inv_dynamics_norm"] = np.array(tn[1], dtype=np.float64)
        mn = gg.module_norms(algo, model, "model")
        mn.update(gg.module_norms(algo, actor, "actor_model"))
        mn.update(gg.module_norms(algo, value, "value_model"))
        g[f"u{u}/module_grad_norms"] = np.array([mn[m] for m in fx.MODULES], dtype=np.float64)
        g[f"u{u}/beliefs"] = beliefs.numpy().copy()
        g[f"u{u}/posterior_states"] = post.numpy().copy()
        print(f"  [{os.path.basename(out_path)}] update {u}: "
              + " ".join(f"{k.split('/')[-1]}={logger.kv[k]:.6g}" for k in keys), flush=True)
    g["scalar_keys"] = np.array(scalar_keys)

    def checksums(mods):
        names, sums, abssums = [], [], []
        for mod in mods:
            for k, v in getattr(algo, mod).state_dict().items():
                names.append(f"{mod}.{k}")
                sums.append(float(v.double().sum()))
                abssums.append(float(v.double().abs().sum()))
        return np.array(names), np.array(sums, dtype=np.float64), np.array(abssums, dtype=np.float64)

    g["param_names"], g["param_sums"], g["param_abssums"] = checksums(fx.MODULES)
    g["inv_param_names"], g["inv_param_sums"], g["inv_param_abssums"] = checksums(("inv_dynamics",))
    np.savez_compressed(out_path, **g)
    print(f"wrote {out_path} ({os.path.getsize(out_path)} bytes)")


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    Dreamer, RePo, _ = gg.import_reference()
    feeder = gg.NoiseFeeder()
    record = {"clip_calls": [], "total_norms": []}
    gg.install_patches(feeder, record)
    run_inv_case(RePo, "repo", 8, 4, 5, 6, 3, feeder, record, os.path.join(gg.OUT, "repo_invdyn_tiny.npz"),
                 inv_dynamics_hidden_size=512)
    run_inv_case(Dreamer, "dreamer", 8, 4, 5, 6, 3, feeder, record, os.path.join(gg.OUT, "dreamer_invdyn_tiny.npz"),
                 dense_activation_function="relu", inv_dynamics_hidden_size=100)


if __name__ == "__main__":
    main()
