#!/usr/bin/env python3
"""Golden vectors of the REFERENCE's agents at embedding_size != 1024, on the CPU, at the tiny shapes
(L, B, H, A) = (8, 4, 5, 6) of the existing tiny fixtures and from the same seeds:

    python tests/golden/gen_golden_embed.py [--out DIR]

    repo_embed250_tiny.npz      RePo, E = 250, 3 updates
    dreamer_embed64_tiny.npz    Dreamer, E = 64, 3 updates
    tia_embed250_tiny.npz       TIA, E = 250, 2 updates
    mt_repo_embed250_tiny.npz   MultitaskRePo, E = 250, C = 3, 2 updates (mt_repo_tiny.npz's beta settings)
    finetune_embed250_tiny.npz  FinetunedRePo.train_encoder, E = 250, 3 updates
    calib_js_embed250_tiny.npz  CalibratedRePo, simple_pair, alignment_mode="js", E = 250, 2 steps
    calib_pair_{js,support}_embed250_tiny.npz   CalibratedRePo, calibration_mode="pair", both alignment modes, E = 250,
                                2 steps each

Results only, with the keys of the fixtures those loops already write.  The loops are gen_golden.py's,
gen_golden_calib.py's and gen_golden_calib_pair.py's own run_* functions, unedited: they read their configuration and
parameters through the module global `fx`, which this process replaces by tests/embed_ref.py:FixturesAt(E) -- oracle.fixtures with
embedding_size = E in default_config and embed_ref.make_params (the encoder's fc 1024 -> E behind conv4) for
make_params."""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import gen_golden as gg  # noqa: E402  (puts the repository root on sys.path and reads --out)
import gen_golden_calib as gc  # noqa: E402
import gen_golden_calib_pair as gp  # noqa: E402

from tests.embed_ref import FixturesAt  # noqa: E402


def at(E):
    gg.fx = gc.fx = gp.fx = FixturesAt(E)


def main():
    torch.manual_seed(0)
    torch.set_num_threads(8)
    Dreamer, RePo, TIA = gg.import_reference()
    from algorithms.repo import CalibratedRePo

    feeder = gg.NoiseFeeder()
    record = {"clip_calls": [], "total_norms": []}
    gg.install_patches(feeder, record)
    out = lambda name: os.path.join(gg.OUT, name)  # noqa: E731

    at(250)
    gg.run_case(RePo, "repo", 8, 4, 5, 6, 3, True, feeder, record, out("repo_embed250_tiny.npz"))
    at(64)
    gg.run_case(Dreamer, "dreamer", 8, 4, 5, 6, 3, True, feeder, record, out("dreamer_embed64_tiny.npz"))
    at(250)
    gg.run_tia_case(TIA, 8, 4, 5, 6, 2, feeder, record, out("tia_embed250_tiny.npz"))
    gg.run_mt_case("repo_multitask", 8, 4, 5, 6, 3, 2, feeder, record, out("mt_repo_embed250_tiny.npz"),
                   init_beta=0.05, target_kl=0.3, beta_lr=1e-2)
    gg.run_finetune_case(8, 4, 6, 3, feeder, record, out("finetune_embed250_tiny.npz"))
    gc.run_calib_case(CalibratedRePo, "js", feeder, out("calib_js_embed250_tiny.npz"))
    for mode in ("js", "support"):
        gp.run_pair_case(CalibratedRePo, mode, feeder, out(f"calib_pair_{mode}_embed250_tiny.npz"))


if __name__ == "__main__":
    main()
