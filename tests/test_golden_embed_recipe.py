"""The embedding-size goldens' recipe must stay runnable (as tests/test_golden_inv_dyn_recipe.py for its fixtures):
gen_golden_embed.py is re-run against the reference checkout into a temp dir and must reproduce the committed fixtures."""
import os

import pytest

from tests.test_golden_recipe import GOLDEN, _run, _same_npz

pytestmark = pytest.mark.skipif(not os.path.isdir("/root/reference/algorithms"),
                                reason="needs the reference checkout (build container only)")

FIXTURES = ["calib_js_embed250_tiny.npz", "calib_pair_js_embed250_tiny.npz", "calib_pair_support_embed250_tiny.npz",
            "dreamer_embed64_tiny.npz", "finetune_embed250_tiny.npz",
            "mt_repo_embed250_tiny.npz", "repo_embed250_tiny.npz", "tia_embed250_tiny.npz"]


def test_embed_generator_reproduces_committed_fixtures(tmp_path):
    _run("gen_golden_embed.py", tmp_path)
    made = sorted(f for f in os.listdir(tmp_path) if f.endswith(".npz"))
    assert made == FIXTURES
    for f in made:
        _same_npz(tmp_path / f, os.path.join(GOLDEN, f))
