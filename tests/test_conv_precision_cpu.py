"""conv_precision without a GPU: the model of tests/conv_precision_ref.py stays inside its derived bound against float64 on
the inputs the GPU tests use; the library's setter (thread-local, returns the previous mode, refuses unknown values) and the
REPO_CONV_PRECISION variable (a fresh process per value: it is read once); the Python names."""
import os
import subprocess
import sys
import threading

import pytest
import torch

from tests import conv_precision_ref as ref
from tests import test_conv_engines_gpu as ce
from tests import test_conv_precision_gpu as cp
from tests.util import ROOT

E_BADARG, E_ENV = -1, -6


def test_split2_restates_the_kernels_rounding():
    """Round to nearest even on 8 significand bits, twice; the residual after two parts is below u^2 |a|."""
    x = torch.tensor([1.0 + 2.0 ** -8, 1.0 + 3 * 2.0 ** -8, 1.0 + 2.0 ** -8 + 2.0 ** -20, -3.1415927, 1e-20, 65504.0])
    a1, a2 = ref.split2(x)
    assert a1[0] == 1.0 and a1[1] == 1.0 + 2.0 ** -6          # ties go to the even neighbour: no truncation
    assert a1[2] == 1.0 + 2.0 ** -7                           # above the tie: up
    g = torch.Generator().manual_seed(0)
    y = torch.randn(1 << 16, generator=g) * torch.pow(2.0, torch.randint(-20, 20, (1 << 16,), generator=g).float())
    b1, b2 = ref.split2(y)
    yd = y.double()
    assert bool(((yd - b1.double()).abs() <= ref.U * yd.abs()).all())
    assert bool(((yd - b1.double() - b2.double()).abs() <= ref.U ** 2 * yd.abs()).all())
    assert torch.equal(b1.to(torch.bfloat16).float(), b1) and torch.equal(b2.to(torch.bfloat16).float(), b2)


def test_cases_reach_every_bf16_engine_the_mirrors_can_select():
    """Every (layer, pass, engine, frame type) the imported mirrors send to a bf16 engine has its smallest listed count and a
    ragged one; none is the workload's count."""
    reached = {(c.layer, c.kind, c.engine, c.u8) for c in cp.CASES}
    want = set()
    for layer, kind, engine in ce.selectable():
        if engine in cp.BF_ENGINES[kind]:
            want.add((layer, kind, engine, False))
    for layer in ce.U8_LAYERS:
        if ce.TABLE[layer].down_bf_u8:
            want.add((layer, "down", "Bf16", True))
    want -= {(layer, kind, engine, False) for layer, kind, engine in ce.NOT_REACHABLE}
    # the 3-channel layers' float frames have no bf16 engine: selectable() lists Bf16 for them through the uint8 plan only
    want -= {(layer, "down", "Bf16", False) for layer in ce.U8_LAYERS}
    assert reached == want, (sorted(want - reached), sorted(reached - want))
    for key in reached:
        counts = sorted(c.nimg for c in cp.CASES if (c.layer, c.kind, c.engine, c.u8) == key)
        assert len(counts) == 2 and ce.FULL[key[0]] not in counts, (key, counts)
    mins = {(c.layer, c.kind, c.engine): c.nimg for c in reversed(cp.CASES)}
    assert mins[(1, "down", "Bf16")] == 3 and mins[(1, "down", "Tcd")] == 32 and mins[(1, "up", "Tconv")] == 4
    assert all(cp.engine_at(c.kind, c.layer, c.nimg, c.epi, c.u8) == c.engine for c in cp.CASES)


@pytest.mark.parametrize("c", cp.CASES, ids=cp.case_id)
def test_model_is_inside_the_derived_bound(c):
    """|model - exact| <= K_HIGH * sum |a||b| (K_HIGH_U8 for uint8 frames) componentwise, in float64, and the model is NOT
    the exact product (the bound is not vacuous: the worst component uses a visible part of it)."""
    torch.set_num_threads(8)
    d = ce.Data(c.layer, c.nimg)
    hb = ce.geo(c.layer)[2]
    if c.kind == "down":
        model, exact, bound = ref.down_u8(d.u8, d.w) if c.u8 else ref.down(d.big0, d.w)
    elif c.kind == "up":
        model, exact, bound = ref.up(d.small0, d.w, hb)
    else:
        model, exact, bound = ref.wgrad(d.small_w, d.big0, tuple(d.w.shape))
    if c.u8:
        # the product the kernel forms is x w' with the bytes x and w' = float32(2 w / 255) (+ the folded bias): the bound is on
        # ITS truncation.  Against `exact` (float32 frames, unscaled weights) the fp32 roundings of the frame, of w' and of the
        # folded bias add a few 2^-24 sum |x||w|: part of the fp32 allowance the GPU test gives both modes.
        own = ref.down_u8_own_exact(d.u8, d.w)
        assert float((own - exact).abs().max()) < 1e-6 * float(exact.abs().max())
        exact = own
    err = (model - exact).abs()
    assert bool((err <= bound).all()), float((err - bound).max())
    assert float(err.max()) > 0.0, "the model is the exact product: the bound says nothing"


def test_nll_model_is_inside_the_derived_bound():
    h3, w, _, _ = cp._nll_inputs(5, True)
    model, exact, bound = ref.up(h3, w, 64)
    assert bool(((model - exact).abs() <= bound).all())


# ----------------------------------------------------------------------------- the library's switch (no device needed)
@pytest.fixture
def lib():
    from repo_amd._lib import lib as load

    return load()


def test_abi_version_is_14(lib):
    assert lib.repo_abi_version() == 14


def test_setter_returns_the_previous_mode_and_refuses_unknown_values(lib):
    start = lib.repo_conv_precision(0)
    assert start in (0, 1)
    try:
        assert lib.repo_conv_precision(1) == 0
        assert lib.repo_conv_precision(1) == 1
        for bad in (2, -1, 7):
            assert lib.repo_conv_precision(bad) == E_BADARG
            assert lib.repo_conv_precision(1) == 1, "a refused value changed the mode"
        assert lib.repo_conv_precision(0) == 1
        assert lib.repo_conv_precision(0) == 0
    finally:
        lib.repo_conv_precision(start)


def test_python_names_and_thread_locality():
    from repo_amd import ops

    start = ops.set_conv_precision("highest")
    assert ops.get_conv_precision() == "highest"
    assert ops.set_conv_precision("high") == "highest"
    try:
        assert ops.get_conv_precision() == "high"
        seen = {}
        t = threading.Thread(target=lambda: seen.setdefault("mode", ops.get_conv_precision()))
        t.start()
        t.join()
        assert seen["mode"] == cp.DEFAULT, "the setting leaked into another thread"
        with ops.conv_precision("highest"):
            assert ops.get_conv_precision() == "highest"
        assert ops.get_conv_precision() == "high"
        snap = ops.debug_snapshot()
        assert snap[-1] == 1
        with ops.conv_precision("highest"), ops.debug_scope(snap):
            assert ops.get_conv_precision() == "high"
    finally:
        assert ops.set_conv_precision("highest") == "high"
    for bad in ("tf32", "HIGH", "", None, 1):
        with pytest.raises(ValueError, match='"highest" or "high"'):
            ops.set_conv_precision(bad)
        with pytest.raises(ValueError, match='"highest" or "high"'):
            with ops.conv_precision(bad):
                pass
    assert ops.get_conv_precision() == "highest"
    ops.set_conv_precision(start)


def _child(value, code):
    env = dict(os.environ, REPO_CONV_PRECISION=value)
    return subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=120)


def test_environment_variable_sets_the_initial_mode():
    r = _child("high", "from repo_amd import ops; print(ops.get_conv_precision(), ops.set_conv_precision('highest'), "
                       "ops.get_conv_precision())")
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == ["high", "high", "highest"]


def test_unknown_name_in_the_environment_variable_is_an_error_that_names_it():
    code = ("from repo_amd._lib import lib; L = lib(); rc = L.repo_conv_precision(1); "
            "print(rc, L.repo_strerror(rc).decode())\n"
            "from repo_amd import ops\n"
            "try:\n    ops.get_conv_precision()\nexcept Exception as e:\n    print(type(e).__name__, e)")
    r = _child("tf32", code)
    assert r.returncode == 0, r.stderr
    first, second = r.stdout.strip().splitlines()
    assert first.split()[0] == str(E_ENV) and "REPO_CONV_PRECISION" in first and "tf32" in first, first
    assert second.startswith("RepoHipError") and "tf32" in second, second
