"""The relu goldens' recipe must stay runnable (as tests/test_golden_recipe.py for the ELU ones): gen_golden_act.py is
re-run against the reference checkout into a temp dir and must reproduce the committed fixtures."""
import os

import pytest

from tests.test_golden_recipe import GOLDEN, _run, _same_npz

pytestmark = pytest.mark.skipif(not os.path.isdir("/root/reference/algorithms"),
                                reason="needs the reference checkout (build container only)")


def test_relu_update_generator_reproduces_committed_fixtures(tmp_path):
    _run("gen_golden_act.py", tmp_path)
    made = sorted(f for f in os.listdir(tmp_path) if f.endswith(".npz"))
    assert made == ["dreamer_relu_tiny.npz", "repo_relu_tiny.npz"]
    for f in made:
        _same_npz(tmp_path / f, os.path.join(GOLDEN, f))
