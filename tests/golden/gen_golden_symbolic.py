#!/usr/bin/env python3
"""Golden vectors of the REFERENCE's RePo and Dreamer on state-vector observations (pixel_obs=False), at the tiny shapes
of repo_tiny.npz / dreamer_tiny.npz (L = 8, B = 4, H = 5, A = 6) with 17-float observations, for the same number of
updates and from the same seeds:

    python tests/golden/gen_golden_symbolic.py [--out DIR]

writes repo_symbolic_tiny.npz (RePo, cnn_activation_function="relu") and dreamer_symbolic_tiny.npz (Dreamer,
cnn_activation_function="elu": the symbolic modules take the config's cnn activation).  Results only: the keys of the tiny
fixtures.  The symbolic encoder's and decoder's parameters and the observation vectors come from
tests/symbolic_ref.py (make_symbolic_params, make_obs); every other module's parameters, the actions, rewards, dones and
the noise are the existing goldens' (oracle/fixtures.py: make_params / make_batch / make_noise with the same seeds)."""
import os
import sys
from collections import OrderedDict

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as gg  # noqa: E402  (puts the repository root on sys.path and reads --out)

from tests.symbolic_ref import make_obs, make_symbolic_params  # noqa: E402

fx = gg.fx
OBS = 17


class VectorEnv:
    def __init__(self, A, obs):
        self.observation_space = gg.FakeSpace((obs,))
        self.action_space = gg.FakeSpace((A,))


def symbolic_params(cfg, A, obs):
    """fx.make_params with the conv encoder / decoder replaced by the seeded symbolic ones."""
    params = fx.make_params(A, seed=7)
    params.update(make_symbolic_params(obs, cfg.belief_size, cfg.state_size, cfg.embedding_size))
    return params


def run_symbolic_case(Algo, algo_name, L, B, H, A, obs, n_updates, feeder, record, out_path, **over):
    cfg = fx.default_config(algo=algo_name, batch_size=B, chunk_size=L, horizon=H, pixel_obs=False, **over)
    logger = gg.RecLogger()
    algo = Algo(cfg, VectorEnv(A, obs), VectorEnv(A, obs), logger)
    gg.load_params(algo, symbolic_params(cfg, A, obs))
    T = L - 1
    g = OrderedDict()
    g["meta"] = np.array([L, B, H, A, n_updates], dtype=np.int64)
    g["obs_size"] = np.array(obs, dtype=np.int64)
    scalar_keys = None
    for u in range(n_updates):
        _, actions, rewards, dones = fx.make_batch(L, B, A, seed=11 + u)
        vec = make_obs(L, B, obs, seed=11 + u)
        noise = fx.make_noise(L, B, H, A, seed=101 + u)
        feeder.load(noise, T, H)
        record["clip_calls"].clear()
        record["total_norms"].clear()
        logger.kv.clear()
        beliefs, post = algo.train_dynamics(torch.from_numpy(vec), torch.from_numpy(actions), torch.from_numpy(rewards),
                                            torch.from_numpy(1 - dones))
        algo.train_actor_critic(beliefs.flatten(0, 1), post.flatten(0, 1))
        assert not feeder.queue, "noise left over: draw order differs from SURVEY 8c"
        keys = sorted(logger.kv.keys())
        scalar_keys = scalar_keys or keys
        assert keys == scalar_keys
        g[f"u{u}/scalars"] = np.array([logger.kv[k] for k in keys], dtype=np.float64)
        if hasattr(algo, "log_beta"):
            g[f"u{u}/log_beta"] = np.array(algo.log_beta.item(), dtype=np.float64)
        g[f"u{u}/total_norms"] = np.array(record["total_norms"], dtype=np.float64)
        mn = gg.module_norms(algo, record["clip_calls"][0], "model")
        mn.update(gg.module_norms(algo, record["clip_calls"][1], "actor_model"))
        mn.update(gg.module_norms(algo, record["clip_calls"][2], "value_model"))
        g[f"u{u}/module_grad_norms"] = np.array([mn[m] for m in fx.MODULES], dtype=np.float64)
        g[f"u{u}/beliefs"] = beliefs.numpy().copy()
        g[f"u{u}/posterior_states"] = post.numpy().copy()
        print(f"  [{os.path.basename(out_path)}] update {u}: "
              + " ".join(f"{k.split('/')[-1]}={logger.kv[k]:.6g}" for k in keys), flush=True)
    g["scalar_keys"] = np.array(scalar_keys)
    names, sums, abssums = [], [], []
    for mod in fx.MODULES:
        for k, v in getattr(algo, mod).state_dict().items():
            names.append(f"{mod}.{k}")
            sums.append(float(v.double().sum()))
            abssums.append(float(v.double().abs().sum()))
    g["param_names"], g["param_sums"], g["param_abssums"] = np.array(names), np.array(sums), np.array(abssums)
    np.savez_compressed(out_path, **g)
    print(f"wrote {out_path} ({os.path.getsize(out_path)} bytes)")


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    Dreamer, RePo, _ = gg.import_reference()
    feeder = gg.NoiseFeeder()
    record = {"clip_calls": [], "total_norms": []}
    gg.install_patches(feeder, record)
    run_symbolic_case(RePo, "repo", 8, 4, 5, 6, OBS, 3, feeder, record, os.path.join(gg.OUT, "repo_symbolic_tiny.npz"))
    run_symbolic_case(Dreamer, "dreamer", 8, 4, 5, 6, OBS, 3, feeder, record,
                      os.path.join(gg.OUT, "dreamer_symbolic_tiny.npz"), cnn_activation_function="elu")


if __name__ == "__main__":
    main()
