"""The state-vector goldens' recipe must stay runnable (as tests/test_golden_inv_dyn_recipe.py for the inverse-dynamics
ones): gen_golden_symbolic.py is re-run against the reference checkout into a temp dir and must reproduce the committed
fixtures.  And the fixtures keep the layout of the pixel ones they stand beside (repo_tiny.npz, dreamer_tiny.npz): the
same keys, shapes and logged scalars, with the symbolic modules' six tensors in place of the conv stacks'."""
import os

import numpy as np
import pytest

from tests.test_golden_recipe import GOLDEN, _run, _same_npz

needs_ref = pytest.mark.skipif(not os.path.isdir("/root/reference/algorithms"),
                               reason="needs the reference checkout (build container only)")

PAIRS = [("repo_symbolic_tiny.npz", "repo_tiny.npz"), ("dreamer_symbolic_tiny.npz", "dreamer_tiny.npz")]


@needs_ref
def test_symbolic_generator_reproduces_committed_fixtures(tmp_path):
    _run("gen_golden_symbolic.py", tmp_path)
    made = sorted(f for f in os.listdir(tmp_path) if f.endswith(".npz"))
    assert made == sorted(f for f, _ in PAIRS)
    for f in made:
        _same_npz(tmp_path / f, os.path.join(GOLDEN, f))


@pytest.mark.parametrize("fname,base", PAIRS)
def test_symbolic_goldens_keep_the_layout_of_the_pixel_ones(fname, base):
    a, b = np.load(os.path.join(GOLDEN, fname)), np.load(os.path.join(GOLDEN, base))
    assert os.path.getsize(os.path.join(GOLDEN, fname)) < (1 << 20)
    assert set(a.files) == set(b.files) | {"obs_size"}
    assert np.array_equal(a["meta"], b["meta"]) and int(a["obs_size"]) == 17
    assert [str(k) for k in a["scalar_keys"]] == [str(k) for k in b["scalar_keys"]]
    for k in b.files:
        if k != "param_names" and not k.startswith("param_"):
            assert a[k].shape == b[k].shape, k
            assert a[k].dtype.kind in "US" or np.isfinite(a[k]).all(), k
    sym = [f"{m}.fc{i}.{w}" for m in ("encoder", "obs_model") for i in (1, 2, 3) for w in ("weight", "bias")]
    names = [str(n) for n in a["param_names"]]
    assert [n for n in names if n.startswith(("encoder.", "obs_model."))] == sym
    rest = lambda ns: [str(n) for n in ns if not str(n).startswith(("encoder.", "obs_model."))]  # noqa: E731
    assert rest(a["param_names"]) == rest(b["param_names"])
