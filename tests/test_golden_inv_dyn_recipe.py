"""The inverse-dynamics goldens' recipe must stay runnable (as tests/test_golden_act_recipe.py for the relu ones):
gen_golden_inv_dyn.py is re-run against the reference checkout into a temp dir and must reproduce the committed fixtures.
And the auxiliary must perturb nothing: it is detached from the world model and draws no noise, so every scalar, latent,
gradient norm and parameter checksum the new goldens share with the fixtures of the same configuration WITHOUT the
auxiliary (repo_tiny.npz, dreamer_relu_tiny.npz) equals them."""
import os

import numpy as np
import pytest

from tests.test_golden_recipe import GOLDEN, _run, _same_npz

pytestmark = pytest.mark.skipif(not os.path.isdir("/root/reference/algorithms"),
                                reason="needs the reference checkout (build container only)")

PAIRS = [("repo_invdyn_tiny.npz", "repo_tiny.npz"), ("dreamer_invdyn_tiny.npz", "dreamer_relu_tiny.npz")]


def test_inv_dyn_generator_reproduces_committed_fixtures(tmp_path):
    _run("gen_golden_inv_dyn.py", tmp_path)
    made = sorted(f for f in os.listdir(tmp_path) if f.endswith(".npz"))
    assert made == sorted(f for f, _ in PAIRS)
    for f in made:
        _same_npz(tmp_path / f, os.path.join(GOLDEN, f))


@pytest.mark.parametrize("fname,base", PAIRS)
def test_inv_dyn_goldens_equal_the_fixtures_without_the_auxiliary(fname, base):
    a, b = np.load(os.path.join(GOLDEN, fname)), np.load(os.path.join(GOLDEN, base))
    assert set(b.files) <= set(a.files), sorted(set(b.files) - set(a.files))
    assert np.array_equal(a["meta"], b["meta"])
    ka, kb = [str(k) for k in a["scalar_keys"]], [str(k) for k in b["scalar_keys"]]
    assert sorted(set(ka) - set(kb)) == ["train/inv_dyn_loss"] and set(kb) <= set(ka)
    assert np.array_equal(a["param_names"], b["param_names"])
    compared = 0
    for k in b.files:
        if k in ("meta", "scalar_keys", "param_names"):
            continue
        x, y = a[k], b[k]
        if k.endswith("/scalars"):
            x = np.array([x[ka.index(n)] for n in kb])
            assert np.isfinite(a[k][ka.index("train/inv_dyn_loss")])
        np.testing.assert_allclose(x, y, rtol=1e-12, atol=1e-12, err_msg=f"{fname}:{k}")
        compared += 1
    n_updates = int(a["meta"][4])
    assert compared >= 5 * n_updates + 2, compared   # scalars, two latents, two kinds of norms per update; checksums
