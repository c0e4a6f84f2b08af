#!/usr/bin/env python3
"""Golden vectors of the REFERENCE's RePo and Dreamer with dense_activation_function="relu", at the tiny shapes of
repo_tiny.npz / dreamer_tiny.npz and for the same number of updates:

    python tests/golden/gen_golden_act.py [--out DIR]

writes repo_relu_tiny.npz and dreamer_relu_tiny.npz (results only, the keys of the ELU fixtures).  Everything but the
config comes from gen_golden.py: seeded parameters / batches / noise, the noise feeder, the recorded quantities."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as gg  # noqa: E402  (puts the repository root on sys.path and reads --out)


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    Dreamer, RePo, _ = gg.import_reference()
    feeder = gg.NoiseFeeder()
    record = {"clip_calls": [], "total_norms": []}
    gg.install_patches(feeder, record)
    base = gg.fx.default_config

    def relu_config(**over):
        return base(**dict(over, dense_activation_function="relu"))

    gg.fx.default_config = relu_config   # run_case builds its config through it
    try:
        gg.run_case(RePo, "repo", 8, 4, 5, 6, 3, True, feeder, record, os.path.join(gg.OUT, "repo_relu_tiny.npz"))
        gg.run_case(Dreamer, "dreamer", 8, 4, 5, 6, 3, True, feeder, record, os.path.join(gg.OUT, "dreamer_relu_tiny.npz"))
    finally:
        gg.fx.default_config = base


if __name__ == "__main__":
    main()
