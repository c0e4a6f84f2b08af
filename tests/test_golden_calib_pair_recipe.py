"""The "pair" calibration goldens' recipe must stay runnable (as tests/test_golden_calib_recipe.py for the simple_pair ones):
gen_golden_calib_pair.py is re-run against the reference checkout into a temp dir and must reproduce the committed
fixtures.  And the fixtures hold what the GPU test reads: both alignment modes, two steps, the reference's log keys with
train/dyn_loss among them, and the checksums of the inverse-dynamics model."""
import os

import numpy as np
import pytest

from tests.test_golden_recipe import GOLDEN, _run, _same_npz

pytestmark = pytest.mark.skipif(not os.path.isdir("/root/reference/algorithms"),
                                reason="needs the reference checkout (build container only)")

FILES = ["calib_pair_js_tiny.npz", "calib_pair_support_tiny.npz"]
KEYS = ["train/aln_loss", "train/calib_loss", "train/dyn_loss", "train/encoder_loss", "train/f_kl", "train/f_loss_src",
        "train/f_loss_tgt"]
SUPPORT_KEYS = ["train/tau_loss", "train/tau_mean", "train/u_value"]


def test_calib_pair_generator_reproduces_committed_fixtures(tmp_path):
    _run("gen_golden_calib_pair.py", tmp_path)
    made = sorted(f for f in os.listdir(tmp_path) if f.endswith(".npz"))
    assert made == FILES
    for f in made:
        _same_npz(tmp_path / f, os.path.join(GOLDEN, f))


@pytest.mark.parametrize("fname", FILES)
def test_calib_pair_goldens_hold_results_only_and_the_reference_keys(fname):
    path = os.path.join(GOLDEN, fname)
    assert os.path.getsize(path) < (1 << 20)
    g = np.load(path)
    support = "support" in fname
    keys = [str(k) for k in g["scalar_keys"]]
    assert keys == sorted(KEYS + (SUPPORT_KEYS if support else []))
    assert [str(m) for m in g["grad_norm_modules"]] == ["encoder", "disc"] + (["log_tau"] if support else [])
    n = int(g["meta"][4])
    assert n == 2
    for u in range(n):
        s = dict(zip(keys, g[f"u{u}/scalars"]))
        assert np.isfinite(g[f"u{u}/scalars"]).all() and np.isfinite(g[f"u{u}/grad_norms"]).all()
        assert (g[f"u{u}/grad_norms"] > 0).all() and float(g[f"u{u}/disc_beta"]) > 0
        want = s["train/aln_loss"] + s["train/dyn_loss"] + s["train/calib_loss"]   # CALIB_CFG: all three coefficients 1
        assert abs(s["train/encoder_loss"] - want) <= 1e-6 * abs(want)
        assert s["train/dyn_loss"] != s["train/calib_loss"]
    assert any(str(k).startswith("inv_dynamics.") for k in g["param_names"])
    assert max(v.size for v in (g[k] for k in g.files)) < 200   # names, scalars and checksums: no tensors
