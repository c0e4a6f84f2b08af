"""config.grad_clip = "agc" and config.optimizer = "laprop" on the GPU: repo_agc_coef and repo_optim_step
against tests/optim_ref.py's float64 restatement over every layout regime, the skip word and the argument checks; whole
updates of RePo and Dreamer against OracleRules (tied to OracleAgent by tests/test_optim_rules_cpu.py); the default path;
checkpoints, pipelining, and the families that refuse.

Bounds.
  Squared norms (per tensor and global): tests/test_reductions_gpu.py's -- |got - sum| / sum|terms| <= FTOL = 1e-5.
  Coefficients: coef = clip * max(pmin, sqrt(P)) / sqrt(G) where it is not 1.  P and G are sums of non-negative terms, so
    the bound above is their RELATIVE error; a square root halves a relative error, the quotient adds the two halves: FTOL
    from the sums.  On top come the roundings of the two roots, the maximum's operand clip (given as float32, the reference
    takes the same value), the product and the quotient: 5 of 2^-24.  COEF_TOL = FTOL + 8 * 2^-24 relative.  Inputs keep
    every tensor's unorm / upper at least 2 % away from 1 (asserted on the reference), so the clipped SET is exact.
  The step, after k steps: |p - p64| <= k * (2^-24 * max|p| + R * 2^-24 * U * lr).  As
    tests/test_reductions_gpu.py::test_clip_adam_against_float64_adam derives for Adam: the subtraction p <- fl(p - x)
    rounds once at the magnitude of p; x = lr_bc1 * q carries the roundings of its operands, R = 16 of them, relative to
    a quantity of magnitude U.  Adam: q = m' / (sqrt(v') / sqrt(bc2) + eps), |m_hat / sqrt(v_hat)| < U = 4 asserted on the
    reference.  LaProp: q = m', m' = b1 m + (1 - b1) u, u = g' / (sqrt(v') / sqrt(bc2) + eps) -- the coefficient (3), v'
    (3, halved by the root), the root, the scaling, the sum, the quotient (1 each), then m' (3), lr_bc1 and the product (1
    each): 14 again, on |m_hat| <= max|u| <= sqrt((1 - b2^t) / (1 - b2)) <= sqrt(3) < U = 2 for t <= 3, asserted on the
    reference.  Under the coefficient TABLE the coefficient is not 3 roundings but the two reduction trees: a thread adds
    at most 4 groups of 4 squares (7 + 4 roundings), the wave 6 levels, the block 4 partials, then a lane at most
    ceil(chunks / 64) partials and the wave 6 more -- under 32 roundings per sum for the layouts here, halved by the root,
    two sums: R = 16 + 32 = 48.
  Beside the derived bound stands a measured one: the same formulas evaluated in float32 by torch on the CPU, before any
  GPU run, and the limit is max(derived, 3 * that error) (DESIGN.md 6p lists both numbers).
  Gradients are exactly 0 or at least 1e-12 in magnitude (g^2 underflows below about 1e-19).
  Updates: tests/test_pcont_gpu.py::test_update_matches_oracle's -- scalars 1e-3, flat gradients 1e-3, per-tensor gradients
  5e-3; per-tensor coefficients 5e-3; clipped counts equal; parameters by tests/test_oracle_golden.py's per-tensor checksums;
  second moments per tensor 1e-2 (twice the gradient's 5e-3: a square)."""
import functools
import math

import numpy as np
import pytest
import torch

from oracle import fixtures as fx
from oracle import repo_oracle as ro
from tests import optim_ref as orf
from tests import pcont_ref as pr
from tests import test_actor_grad_gpu as tag
from tests import test_slow_value_gpu as tsv
from tests import test_update_gpu as tu
from tests import twohot_ref as th
from tests.util import has, l2err, log, relerr, rnd, traced

pytestmark = pytest.mark.gpu

E_BADARG, E_SHAPE, E_ALIGN = -1, -2, -3   # include/repo_hip.h
F32 = np.float32
FTOL = 1e-5
COEF_TOL = FTOL + 8 * 2.0 ** -24
BETAS = (float(F32(0.9)), float(F32(0.999)))
LR = 1e-2
CLIP, PMIN = float(F32(0.3)), float(F32(1e-3))
PAD, SENT, GUARD = 1e3, -777.0, 16
C = orf.CHUNK
PARTS_KERNEL, FINISH_KERNEL, STEP_KERNEL = r"\bagc_parts_kernel\b", r"\bagc_finish_kernel\b", r"\boptim_step_kernel\b"
OLD_KERNELS = (r"\bsqnorm_kernel\b", r"\bsqnorm_final_kernel\b", r"\bclip_adam_kernel\b", r"\bclip_adam_target_kernel\b")


@pytest.fixture(autouse=True)
def _poison_lds():
    """Start every test from NaN-filled LDS on all CUs: reads of never-written LDS cannot hide."""
    from repo_amd._lib import lib

    assert lib().repo_debug_poison_lds(torch.cuda.current_stream().cuda_stream) == 0
    yield


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from repo_amd import ops as o

    return o


def dev(t):
    return t.cuda()


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_geometry_is_the_restatements(ops):
    assert ops.agc_geometry() == (orf.CHUNK, orf.PARTS_MAX_BLOCKS, orf.FINISH_THREADS, orf.STEP_MAX_BLOCKS)
    assert orf.CHUNK % 4 == 0 and orf.FINISH_THREADS % orf.WAVE == 0


# ----------------------------------------------------------------------------- 1. norms and coefficients
LAYOUTS = {
    "padding": [1, 2, 3, 4, 5],
    "chunks": [C - 1, C, C + 1, 3 * C + 5],
    "more chunks than lanes": [7, (orf.WAVE + 1) * C + 3, 2],          # one segment's wave strides its chunks
    "300 segments": [1] * 300,                                          # more segments than the finishing block's threads
    "alone": [1000],
    "past the grid cap": [600 * C + 1, 5, (orf.PARTS_MAX_BLOCKS - 590) * C + 7],   # more chunks than blocks
}
RATIOS = (0.25, 4.0, 0.7, 1.5, 0.97, 1.03)


def flat_inputs(sizes, seed, ratios=RATIOS, zero_p=(), zero_g=()):
    """Flat float32 parameter and gradient buffers in FlatAdam's layout, padding filled with PAD, each tensor's gradient
    scaled so that unorm / upper is ratios[s % len] (tensors in zero_p / zero_g are all zero) -> (p, g, offsets, n)."""
    rs = np.random.RandomState(seed)
    offsets, n = orf.layout(sizes)
    p, g = torch.full((n,), PAD, dtype=torch.float32), torch.full((n,), PAD, dtype=torch.float32)
    for s, (o, k) in enumerate(zip(offsets, sizes)):
        ps, gs = rnd(rs, k, scale=0.3), rnd(rs, k)
        gs[gs == 0] = 1.0
        if s in zero_p:
            ps.zero_()
        upper = CLIP * max(PMIN, float(ps.double().norm()))
        gs = (gs.double() * (ratios[s % len(ratios)] * upper / float(gs.double().norm()))).float()
        if s in zero_g:
            gs.zero_()
        p[o : o + k], g[o : o + k] = ps, gs
    return p, g, offsets, n


def reference(p, g, offsets, sizes):
    """float64 per-tensor squared norms, coefficients, ratios from the float32 buffers' own elements."""
    G = [g[o : o + k].double() for o, k in zip(offsets, sizes)]
    P = [p[o : o + k].double() for o, k in zip(offsets, sizes)]
    coefs, ratios = orf.agc_coefs(G, P, CLIP, PMIN)
    return G, P, coefs, ratios


class Bands:
    """norms, coef and stats as views of one buffer filled with SENT, GUARD floats between and around them."""

    def __init__(self, nseg):
        a = GUARD
        b = a + 2 * nseg + GUARD
        c = b + nseg + GUARD
        self.buf = torch.full((c + 2 + GUARD,), SENT, dtype=torch.float32, device="cuda")
        self.norms, self.coef, self.stats = self.buf[a : a + 2 * nseg], self.buf[b : b + nseg], self.buf[c : c + 2]
        self.mask = torch.ones_like(self.buf, dtype=torch.bool)
        for lo, k in ((a, 2 * nseg), (b, nseg), (c, 2)):
            self.mask[lo : lo + k] = False

    def intact(self):
        return bool((self.buf[self.mask] == SENT).all())


def check_coef_case(ops, what, sizes, p, g, offsets, n):
    G, P, coefs, ratios = reference(p, g, offsets, sizes)
    assert all(abs(r - 1.0) >= 0.02 for r in ratios), (what, "a tensor within 2 % of its threshold")
    tables = ops.AgcTables(offsets, sizes, n, torch.device("cuda"))
    assert tables.nchunk == sum(-(-k // C) for k in sizes) and tables.nseg == len(sizes)
    pd, gd = dev(p), dev(g)
    out = Bands(len(sizes))
    _, names = traced(lambda: ops.agc_coef(tables, pd, gd, CLIP, PMIN, out.norms, out.coef, out.stats))
    assert has(names, PARTS_KERNEL) and has(names, FINISH_KERNEL) and len(names) == 2, names
    assert out.intact(), (what, "a write outside the outputs")
    norms, coef, stats = out.norms.cpu(), out.coef.cpu(), out.stats.cpu()
    worst_s = worst_c = 0.0
    for s in range(len(sizes)):
        for got, terms in ((norms[2 * s], G[s] ** 2), (norms[2 * s + 1], P[s] ** 2)):
            if float(terms.sum()) == 0.0:
                assert float(got) == 0.0, (what, s, "a zero tensor's norm (the padding's sentinel would show)")
            else:
                worst_s = max(worst_s, tsum_err(got, terms))
        worst_c = max(worst_c, abs(float(coef[s]) - coefs[s]) / coefs[s])
        assert (float(coef[s]) < 1.0) == (coefs[s] < 1.0) and (coefs[s] < 1.0 or float(coef[s]) == 1.0), (what, s)
    total = torch.cat(G) ** 2
    e_tot = tsum_err(stats[0], total)
    clean = gd.clone()
    keep = torch.zeros(n, dtype=torch.bool)
    for o, k in zip(offsets, sizes):
        keep[o : o + k] = True
    clean[~keep.cuda()] = 0.0
    e_old = abs(float(stats[0]) - float(ops.grad_sqnorm(clean))) / max(float(total.sum()), 1e-300)
    log(f"agc_coef {what}: {len(sizes)} tensors, {tables.nchunk} chunks; norms {worst_s:.2e}, coefficients {worst_c:.2e}, "
        f"global {e_tot:.2e}, against grad_sqnorm {e_old:.2e}; clipped {int(stats[1])}")
    assert worst_s <= FTOL and worst_c <= COEF_TOL and e_tot <= FTOL and e_old <= FTOL, what
    assert float(stats[1]) == sum(1 for c in coefs if c < 1.0), what
    again = Bands(len(sizes))
    ops.agc_coef(tables, pd, gd, CLIP, PMIN, again.norms, again.coef, again.stats)
    assert same_bits(again.buf, out.buf), (what, "two runs differ in bits")


def tsum_err(got, terms):
    terms = terms.detach().double()
    return abs(float(got) - terms.sum().item()) / (terms.abs().sum().item() + 1e-300)


@pytest.mark.parametrize("name", list(LAYOUTS))
def test_norms_and_coefficients(ops, name):
    sizes = LAYOUTS[name]
    if name == "past the grid cap":
        assert sum(-(-k // C) for k in sizes) > orf.PARTS_MAX_BLOCKS
    if name == "more chunks than lanes":
        assert -(-sizes[1] // C) > orf.WAVE
    if name == "300 segments":
        assert len(sizes) > orf.FINISH_THREADS
    check_coef_case(ops, name, sizes, *flat_inputs(sizes, len(sizes) + sizes[0]))


def test_zero_tensors(ops):
    """An all-zero parameter tensor (the pmin branch: 6o's zero-initialised head), an all-zero gradient (coef = 1), both."""
    sizes = [10, 11, 12, 13, 3]
    p, g, offsets, n = flat_inputs(sizes, 5, ratios=(4.0, 1.5, 0.25, 4.0, 0.25), zero_p=(0, 2, 4), zero_g=(1, 2))
    _, _, coefs, _ = reference(p, g, offsets, sizes)
    assert abs(coefs[0] - 0.25) < 1e-6 and coefs[1] == coefs[2] == 1.0 and coefs[4] == 1.0
    check_coef_case(ops, "zero tensors", sizes, p, g, offsets, n)


def test_nan_norm_gives_nan_coefficient(ops):
    sizes = [5, 6, 7]
    p, g, offsets, n = flat_inputs(sizes, 6)
    g[offsets[0] + 1] = float("nan")
    p[offsets[1] + 2] = float("nan")
    tables = ops.AgcTables(offsets, sizes, n, torch.device("cuda"))
    _, coef, stats = ops.agc_coef(tables, dev(p), dev(g), CLIP, PMIN)
    coef = coef.cpu()
    assert math.isnan(float(coef[0])) and math.isnan(float(coef[1])) and math.isfinite(float(coef[2]))
    assert math.isnan(float(stats[0])) and float(stats[1]) == (1.0 if float(coef[2]) < 1 else 0.0)


# ----------------------------------------------------------------------------- 2. the step
BIG = {"none": 524547, "norm": 524547, "agc": (orf.STEP_MAX_BLOCKS + 1) * C + 3}
MODE = {"none": 0, "norm": 1, "agc": 2}


def step_bound(k, pmax, R, U, lr=LR):
    return k * (2.0 ** -24 * pmax + R * 2.0 ** -24 * U * lr)


def step_gradients(rs, sizes, offsets, n, step, clip, p64):
    """A flat gradient (zero padding, a fifth of the elements exactly zero, nothing below 1e-12 otherwise).  "agc": tensor s is
    scaled to unorm / upper = (0.3, 1.7, 5)[(s + step) % 3] against the reference's current parameters, so a three-tensor layout
    sees three coefficients, one of them exactly 1; "norm" / "none": small, and large at step 2 (the global clip bites)."""
    g = torch.zeros(n, dtype=torch.float32)
    for s, (o, k) in enumerate(zip(offsets, sizes)):
        gs = rnd(rs, k, scale=5.0 if step == 2 else 0.01)
        if k > 4:
            gs[::5] = 0.0
        gs[(gs != 0) & (gs.abs() < 1e-6)] = 1e-6
        if k == 1:      # a single draw may not land on its side of max_norm
            gs = gs.sign() * (5.0 if step == 2 else 0.01)
        if clip == "agc":
            upper = CLIP * max(PMIN, float(p64[s].norm()))
            gs = (gs.double() * ((0.3, 1.7, 5.0)[(s + step) % 3] * upper / float(gs.double().norm()))).float()
        assert bool(((gs == 0) | (gs.abs() >= 1e-12)).all())
        g[o : o + k] = gs
    return g


@pytest.mark.parametrize("sizes", [[1], [257], "big", [5, 300, C + 3]], ids=["1", "257", "big", "three"])
@pytest.mark.parametrize("clip", ["none", "norm", "agc"])
@pytest.mark.parametrize("rule", ["adam", "laprop"])
def test_step_against_float64(ops, rule, clip, sizes):
    """Three steps against optim_ref.update in float64 (module docstring: the bound, and the float32 CPU evaluation that is
    recorded first)."""
    sizes = [BIG[clip]] if sizes == "big" else sizes
    offsets, n = orf.layout(sizes)
    if len(sizes) == 1 and sizes[0] > 257:
        blocks = -(-sizes[0] // C) if clip == "agc" else -(-n // 256)
        assert blocks > orf.STEP_MAX_BLOCKS
    rs = np.random.RandomState(sum(sizes) + MODE[clip])
    p0 = [rnd(rs, k, scale=0.3) for k in sizes]
    max_norm = float(F32(math.sqrt(sum(sizes))))
    eps = float(F32(orf.LAPROP_EPS if rule == "laprop" else 1e-8))
    U, R = (4.0, 16) if rule == "adam" else (2.0, 16)
    R += 32 if clip == "agc" else 0
    kw = dict(rule=rule, clip=clip, max_norm=max_norm, agc_clip=CLIP, agc_pmin=PMIN, betas=BETAS, eps=eps)
    # the float64 reference and the float32 CPU evaluation, all three steps, before anything runs on the GPU
    p64, m64, v64 = ([x.double().clone() for x in p0], [torch.zeros(k, dtype=torch.float64) for k in sizes],
                     [torch.zeros(k, dtype=torch.float64) for k in sizes])
    p32, m32, v32 = [x.clone() for x in p0], [torch.zeros(k) for k in sizes], [torch.zeros(k) for k in sizes]
    grads, want, cpu_err = [], [], []
    for step in (1, 2, 3):
        g = step_gradients(rs, sizes, offsets, n, step, clip, p64)
        gl = [g[o : o + k] for o, k in zip(offsets, sizes)]
        info = orf.update(p64, [x.double() for x in gl], m64, v64, step, LR, **kw)
        orf.update(p32, gl, m32, v32, step, LR, **kw)
        bc1, bc2 = 1 - BETAS[0] ** step, 1 - BETAS[1] ** step
        if rule == "adam":
            mag = max(float(((m / bc1) / (v / bc2).sqrt().clamp(min=1e-300)).abs().max()) for m, v in zip(m64, v64))
        else:
            mag = max(float((m / bc1).abs().max()) for m in m64)
        assert mag < U, (step, mag)
        if clip == "agc" and len(sizes) == 3:
            assert sorted(round(c, 3) for c in info["coefs"]) == [0.2, round(1 / 1.7, 3), 1.0], info["coefs"]
        if clip == "norm":
            assert (info["clipped"] > 0) == (step == 2), (step, info)
        grads.append(g)
        want.append(([x.clone() for x in p64], [x.clone() for x in m64], [x.clone() for x in v64], info))
        cpu_err.append(max(float((a.double() - b).abs().max()) for a, b in zip(p32, p64)))
    # the GPU
    flat = lambda xs: torch.cat([torch.cat([x.float(), torch.zeros((-len(x)) % 4)]) for x in xs])
    p, m, v = dev(flat(p0)), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    tables = ops.AgcTables(offsets, sizes, n, torch.device("cuda")) if clip == "agc" else None
    for step, g, (wp, wm, wv, info), ce in zip((1, 2, 3), grads, want, cpu_err):
        gd = dev(g)
        sq = ops.grad_sqnorm(gd) if clip == "norm" else None
        if clip == "agc":
            _, coef, stats = ops.agc_coef(tables, p, gd, CLIP, PMIN)
            assert float(stats[1]) == info["clipped"]
        _, names = traced(lambda: ops.optim_step(p, gd, m, v, LR, step, rule, MODE[clip], sq, max_norm, tables, None, BETAS, eps))
        assert has(names, STEP_KERNEL) and len(names) == 1 and not any(has(names, k) for k in OLD_KERNELS), names
        pc, mc, vc = p.cpu(), m.cpu(), v.cpu()
        e = max(float((pc[o : o + k].double() - w).abs().max()) for o, k, w in zip(offsets, sizes, wp))
        derived = step_bound(step, max(float(w.abs().max()) for w in wp), R, U)
        limit = max(derived, 3 * ce)
        em = relerr(torch.cat([mc[o : o + k] for o, k in zip(offsets, sizes)]), torch.cat(wm))
        ev = relerr(torch.cat([vc[o : o + k] for o, k in zip(offsets, sizes)]), torch.cat(wv))
        log(f"optim_step {rule} {clip} sizes={sizes} step {step}: max |p - p64| {e:.2e} (derived {derived:.2e}, float32 on the "
            f"CPU {ce:.2e}, limit {limit:.2e}); relerr m {em:.2e} v {ev:.2e}")
        assert e <= limit, (rule, clip, sizes, step, e, limit)
        assert em < FTOL and ev < FTOL
    # the padding lanes carried a zero gradient: parameters and moments there are still zero
    pad = torch.ones(n, dtype=torch.bool)
    for o, k in zip(offsets, sizes):
        pad[o : o + k] = False
    assert not p.cpu()[pad].any() and not m.cpu()[pad].any() and not v.cpu()[pad].any()


@pytest.mark.parametrize("n", [1, 257, 524547])
def test_adam_through_the_new_launch_is_clip_adam_in_bits(ops, n):
    p0, g, m0, v0, _ = tsv.kernel_inputs(n, n)
    sq = ops.grad_sqnorm(g)
    assert float(sq) > 1.0
    for mode, sqn in ((1, sq), (0, None)):
        a = [p0.clone(), m0.clone(), v0.clone()]
        ops.clip_adam(a[0], g, a[1], a[2], sqn, 1.0, LR, 2, betas=BETAS)
        b = [p0.clone(), m0.clone(), v0.clone()]
        ops.optim_step(b[0], g, b[1], b[2], LR, 2, "adam", mode, sqn, 1.0, betas=BETAS)
        assert not same_bits(a[0], p0)
        for x, y, what in zip(a, b, "pmv"):
            assert same_bits(x, y), (what, n, mode)


def _table_case(ops, seed=3):
    sizes = [5, 300, C + 3]
    p, g, offsets, n = flat_inputs(sizes, seed, ratios=(0.3, 1.7, 5.0))
    pad = torch.ones(n, dtype=torch.bool)
    for o, k in zip(offsets, sizes):
        pad[o : o + k] = False
    p[pad], g[pad] = 0.0, 0.0
    rs = np.random.RandomState(seed)
    m0, v0, t0 = rnd(rs, n, scale=0.1), rnd(rs, n, scale=0.1).abs(), rnd(rs, n, scale=0.3)
    tables = ops.AgcTables(offsets, sizes, n, torch.device("cuda"))
    pd, gd = dev(p), dev(g)
    ops.agc_coef(tables, pd, gd, CLIP, PMIN)
    return tables, pd, gd, dev(m0), dev(v0), dev(t0)


@pytest.mark.parametrize("fraction", [1.0, 0.5])
@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("rule", ["adam", "laprop"])
def test_target_variant(ops, rule, mode, fraction):
    """Parameters and moments: the plain variant's bits.  The target: inside tests/test_slow_value_gpu.py's MIX_BOUND."""
    tables, p0, g, m0, v0, t0 = _table_case(ops)
    sq = ops.grad_sqnorm(g)
    kw = dict(rule=rule, clip_mode=mode, sqnorm=sq if mode == 1 else None, max_norm=1.0, tables=tables if mode == 2 else None,
              betas=BETAS, eps=1e-8 if rule == "adam" else 1e-20)
    a = [p0.clone(), m0.clone(), v0.clone()]
    ops.optim_step(a[0], g, a[1], a[2], LR, 2, **kw)
    b = [p0.clone(), m0.clone(), v0.clone(), t0.clone()]
    _, names = traced(lambda: ops.optim_step(b[0], g, b[1], b[2], LR, 2, target=b[3], fraction=fraction, **kw))
    assert has(names, STEP_KERNEL) and len(names) == 1, names
    assert not same_bits(a[0], p0)
    for x, y, what in zip(a, b, "pmv"):
        assert same_bits(x, y), (what, rule, mode)
    if fraction == 1.0:
        assert same_bits(b[3], b[0])
    else:
        tsv.mix_check(b[3], t0, b[0], fraction, f"optim_step {rule} mode {mode} fraction={fraction:g}")


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("rule", ["adam", "laprop"])
def test_skip_word(ops, rule, mode):
    tables, p0, g, m0, v0, t0 = _table_case(ops, 4)
    sq = ops.grad_sqnorm(g)
    runs = []
    for skip in (None, torch.zeros(1, dtype=torch.int32, device="cuda"), torch.full((1,), 4, dtype=torch.int32, device="cuda")):
        bufs = [p0.clone(), m0.clone(), v0.clone(), t0.clone()]
        ops.optim_step(bufs[0], g, bufs[1], bufs[2], LR, 3, rule, mode, sq if mode == 1 else None, 1.0,
                       tables if mode == 2 else None, None, BETAS, 1e-8, skip, bufs[3], 0.5)
        runs.append(bufs)
    none, zero, four = runs
    assert all(not same_bits(x, y) for x, y in zip(none, (p0, m0, v0, t0))), "the step writes all four buffers"
    assert all(same_bits(x, y) for x, y in zip(none, zero)), "skip word 0 is no skip word"
    assert all(same_bits(x, y) for x, y in zip(four, (p0, m0, v0, t0))), "a non-zero skip word: nothing is written"


def test_argument_errors(ops):
    from repo_amd._lib import lib

    tables, p, g, m, v, t = _table_case(ops, 5)
    n, st = p.numel(), torch.cuda.current_stream().cuda_stream
    keep = [x.clone() for x in (p, m, v, t)]
    out = Bands(tables.nseg)
    P = lambda x: None if x is None else x.data_ptr()

    def coef(n_=n, nseg=tables.nseg, nchunk=tables.nchunk, chunks=tables.chunks, first=tables.seg_first, pp=p, gg=g, clip=0.3,
             pmin=1e-3, parts=tables.parts, norms=out.norms, co=out.coef, stats=out.stats, shift=0):
        return lib().repo_agc_coef(n_, nseg, nchunk, P(chunks), P(first), P(pp) + shift if pp is not None else None, P(gg),
                                   clip, pmin, P(parts), P(norms), P(co), P(stats), st)

    for bad in (dict(n_=0), dict(n_=2 ** 31), dict(nseg=0), dict(nchunk=tables.nseg - 1), dict(nchunk=n + 1)):
        assert coef(**bad) == E_SHAPE, bad
    for name in ("chunks", "first", "pp", "gg", "parts", "norms", "co", "stats"):
        assert coef(**{name: None}) == E_BADARG, name
    for bad in (dict(clip=0.0), dict(clip=-1.0), dict(clip=float("inf")), dict(clip=float("nan")), dict(pmin=0.0),
                dict(pmin=float("nan"))):
        assert coef(**bad) == E_BADARG, bad
    assert coef(shift=4) == E_ALIGN
    assert lib().repo_agc_geometry(None, None, None, None) == E_BADARG

    def step(n_=n, pp=p, gg=g, mm=m, vv=v, rule=1, mode=2, sq=None, nseg=tables.nseg, nchunk=tables.nchunk,
             chunks=tables.chunks, co=tables.coef, step_=1, target=None, fraction=0.5, shift=0):
        return lib().repo_optim_step(n_, P(pp), P(gg), P(mm), P(vv), rule, mode, P(sq), 1.0, nseg, nchunk,
                                     P(chunks) + shift if chunks is not None else None, P(co), LR, BETAS[0], BETAS[1], 1e-8,
                                     step_, None, P(target), fraction, st)

    for bad in (dict(n_=0), dict(step_=0), dict(nseg=0), dict(nchunk=tables.nseg - 1), dict(nchunk=n + 1)):
        assert step(**bad) == E_SHAPE, bad
    for name in ("pp", "gg", "mm", "vv", "chunks", "co"):
        assert step(**{name: None}) == E_BADARG, name
    for bad in (dict(rule=2), dict(rule=-1), dict(mode=3), dict(mode=-1), dict(mode=1, sq=None), dict(target=t, fraction=0.0),
                dict(target=t, fraction=1.5), dict(target=t, fraction=float("nan"))):
        assert step(**bad) == E_BADARG, bad
    assert step(shift=4) == E_ALIGN
    torch.cuda.synchronize()
    assert all(same_bits(x, y) for x, y in zip((p, m, v, t), keep)) and out.intact(), "a refused call launches nothing"
    assert step(target=t, fraction=1.0) == 0
    torch.cuda.synchronize()
    assert same_bits(t, p) and not same_bits(p, keep[0])


def test_flat_adam_picks_the_path_and_view_stays_adam(ops):
    from repo_amd.algorithms.repo.models.utils import FlatAdam

    rs = np.random.RandomState(8)
    shapes = [(5,), (30, 10), (C + 3,)]

    def build(**kw):
        return FlatAdam([torch.nn.Parameter(rnd(rs, *s, scale=0.3).cuda()) for s in shapes], lr=LR, **kw)

    every = (PARTS_KERNEL, FINISH_KERNEL, STEP_KERNEL) + OLD_KERNELS
    for kw in (dict(), dict(rule="laprop"), dict(grad_clip="agc"), dict(rule="laprop", grad_clip="agc")):
        opt = build(**kw)
        target = opt.flat.clone()
        opt.track_target(target, 2, 0.5)
        for step in (1, 2):
            for gv in opt.gviews:    # (through the views: the padding keeps its zero gradient)
                gv.copy_(dev(rnd(rs, *gv.shape, scale=3.0)))
            before = target.clone()
            counts = tsv.counted(lambda: opt.clip_and_step(1.0))[1]
            if "grad_clip" in kw:
                expect = (PARTS_KERNEL, FINISH_KERNEL, STEP_KERNEL)
            else:
                expect = OLD_KERNELS[:2] + ((STEP_KERNEL,) if kw else (OLD_KERNELS[3] if step == 2 else OLD_KERNELS[2],))
            for k in every:
                assert tsv.n_launches(counts, k) == (1 if k in expect else 0), (kw, step, k, counts)
            assert same_bits(target, before) == (step == 1), (kw, step)
        if "grad_clip" in kw:
            want = float((opt.grad.double() ** 2).sum())
            assert abs(float(opt.sqnorm) - want) <= FTOL * want and opt.sqnorm.data_ptr() == opt.agc.stats.data_ptr()
            assert 0 <= float(opt.agc_count) <= 3
            view = FlatAdam.view(opt, 2, lr=LR)
            assert view.rule == "adam" and view.grad_clip == "norm" and view.agc is None and view.eps == (opt.eps if opt.rule == "adam" else 1e-8)


# ----------------------------------------------------------------------------- 3. whole updates against the oracle
L_, B_, H_, A_ = 10, 5, 6, 6
SMALL_CLIP = 0.004    # 0.01 and 0.006 leave a tensor within 2 % of its threshold in one of the two updates
GROUPS = {0.3: ("model", "value"), SMALL_CLIP: ("model", "actor")}   # the groups with clipped AND unclipped tensors
COMBINED_CLIP = 0.05  # the combined configuration's actor and value gradients are larger: both groups clip both ways here


@functools.lru_cache(maxsize=None)
def plain_first_update(algo):
    """The plain oracle's moments after the first update at the fixture seeds: computed once, shared, left unchanged."""
    cfg = fx.default_config(algo=algo, batch_size=B_, chunk_size=L_, horizon=H_)
    plain = ro.OracleAgent(cfg, A_, params=fx.make_params(A_, 7))
    plain.update(*fx.make_batch(L_, B_, A_, seed=60), fx.make_noise(L_, B_, H_, A_, seed=160))
    return {name: (torch.cat([x.reshape(-1) for x in getattr(plain, f"{name}_opt").m]),
                   torch.cat([x.reshape(-1) for x in getattr(plain, f"{name}_opt").v])) for name in ("model", "actor", "value")}


def check_optimisers(agent, oracle, names, tag, agc, clip_groups, first):
    """Coefficients, clipped counts, second moments and parameter checksums of the optimisers in `names`."""
    for name in names:
        opt, oo = getattr(agent, f"{name}_optimizer"), getattr(oracle, f"{name}_opt")
        if agc:
            ratios, want = oracle.last[f"{name}_ratios"], oracle.last[f"{name}_coefs"]
            assert all(abs(r - 1.0) >= 0.02 for r in ratios), (tag, name, "a tensor within 2 % of its threshold", ratios)
            if name in clip_groups:
                assert 0 < oracle.last[f"{name}_clipped"] < len(want), (tag, name, oracle.last[f"{name}_clipped"])
            got = opt.agc.coef.cpu().tolist()
            worst = max(abs(a - b) / b for a, b in zip(got, want))
            count = agent.last_scalars[f"train/agc_clipped_{name}"]
            log(f"{tag} {name}: coefficients worst {worst:.2e}; clipped {count:.0f} of {len(want)} (oracle "
                f"{oracle.last[f'{name}_clipped']}); nearest unorm / upper {min(ratios, key=lambda r: abs(r - 1)):.4f}")
            assert worst < 5e-3, (tag, name, worst)
            assert count == oracle.last[f"{name}_clipped"] == float(opt.agc_count), (tag, name)
        for q, o, v_o, m_o in zip(opt.params, opt.offsets, oo.v, oo.m):
            k = q.numel()
            ev = l2err(opt.exp_avg_sq[o : o + k], v_o)
            assert ev < 1e-2, (tag, name, tuple(q.shape), "second moment", ev)
            if first:   # |m| is sign-free: (1 - b1) |g'| under Adam, (1 - b1) on every non-zero gradient under LaProp
                am, wm = float(opt.exp_avg[o : o + k].abs().sum()), float(m_o.abs().sum())
                assert abs(am - wm) <= 1e-2 * wm + 1e-12, (tag, name, tuple(q.shape), "first moment", am, wm)
    ptol = 2e-4 if agent.c.algo == "repo" else 1e-3     # tests/test_oracle_golden.py's per-tensor checksums
    for mod in fx.MODULES:
        for k, v in getattr(agent, mod).state_dict().items():
            a, w = v.double().cpu(), oracle.p[mod][k].detach().double()
            assert abs(float(a.abs().sum() - w.abs().sum())) <= ptol * float(w.abs().sum()) + 1e-7, (tag, mod, k)
            assert abs(float(a.sum() - w.sum())) <= ptol * float(w.abs().sum()) + 1e-7, (tag, mod, k)


@pytest.mark.parametrize("clip,rule,agc_clip", [("agc", "adam", 0.3), ("norm", "laprop", None), ("agc", "laprop", 0.3),
                                                ("agc", "laprop", SMALL_CLIP)])
@pytest.mark.parametrize("algo", ["repo", "dreamer"])
def test_update_matches_oracle(algo, clip, rule, agc_clip):
    over = dict(grad_clip=clip, optimizer=rule)
    if agc_clip is not None:
        over["agc_clip"] = agc_clip
    agent, cfg = tu.make_agent(algo, L_, B_, H_, A_, **over)
    oracle = orf.OracleRules(cfg, A_, params=fx.make_params(A_, 7))
    agc = clip == "agc"
    assert agent.model_optimizer.rule == rule == oracle.rule and (agent.model_optimizer.agc is not None) == agc
    assert agent.model_optimizer.eps == oracle.model_opt.eps == (1e-20 if rule == "laprop" else 1e-8)
    tag_ = f"[oracle rules {algo} {clip} {rule} {agc_clip}]"
    for u in range(2):
        batch, host = tu.dev_batch(L_, B_, A_, 60 + u, u8=(u == 0))
        agent.noise_source, nz = tu.dev_noise(L_, B_, H_, A_, 160 + u)
        with tu.grad_snapshots(agent) as snap:
            beliefs, post = agent.train_dynamics(batch[0], batch[1], batch[2], 1.0 - batch[3])
            agent.train_actor_critic(beliefs.flatten(0, 1), post.flatten(0, 1))
        _, _, oscal = oracle.update(*host, nz)
        tag.check_against_oracle(agent, oracle, oscal, snap, ("model", "actor", "value"), f"{tag_} update {u}")
        assert not agent.logger.nonfinite
        assert ("train/agc_clipped_model" in agent.last_scalars) == agc
        torch.cuda.synchronize()
        check_optimisers(agent, oracle, ("model", "actor", "value"), f"{tag_} update {u}", agc, GROUPS.get(agc_clip, ()), u == 0)
        if u == 0:
            # the switched-on update is another update: on the same inputs the oracle's moments are not the plain oracle's.
            # (The PARAMETERS of a first step cannot tell: from zero moments Adam and LaProp both move every element by
            # lr * sign(g), whatever the clip.)
            plain = plain_first_update(algo)
            diffs = {}
            for name in ("model", "actor", "value"):
                oo = getattr(oracle, f"{name}_opt")
                diffs[name] = (l2err(torch.cat([x.reshape(-1) for x in oo.m]), plain[name][0]),
                               l2err(torch.cat([x.reshape(-1) for x in oo.v]), plain[name][1]))
            log(f"{tag_} moments against the plain oracle's (m, v): {diffs}")
            assert max(diffs["model"]) > 1e-2 and max(max(d) for d in diffs.values()) > 1e-2, diffs
        with torch.no_grad():   # the oracle takes the agent's parameters: the second update is compared at the same point
            for m in fx.MODULES:
                for k, v in getattr(agent, m).state_dict().items():
                    oracle.p[m][k].copy_(v.cpu())
            if algo == "repo":
                oracle.log_beta.copy_(agent.log_beta.cpu().reshape(oracle.log_beta.shape))


def test_combined_with_every_other_switch():
    """pcont, a slow target from another seed, "both" at mix 0.1, return_norm, the two-hot critic and inv_dynamics under
    ("agc", "laprop"): the actor-critic half against OracleRulesCombined from the agent's own latents and post-model-step
    parameters, over two steps; the model and the inverse-dynamics optimiser's coefficients and clipped counts against
    float64 from their own buffers."""
    K = 31
    torch.manual_seed(0)     # (the inverse-dynamics module keeps its default initialisation)
    agent, cfg = tu.make_agent("repo", L_, B_, H_, A_, value_dist="twohot", value_bins=K, value_bin_low=-5.0, value_bin_high=5.0,
                               actor_grad="both", actor_grad_mix=0.1, pcont=True, slow_value_target=True, slow_value_update=2,
                               slow_value_fraction=0.5, return_norm=True, return_norm_decay=0.5, return_norm_limit=1e-3,
                               inv_dynamics=True, inv_dynamics_lr=3e-4, inv_dynamics_hidden_size=64, grad_clip="agc",
                               optimizer="laprop", agc_clip=COMBINED_CLIP)
    agent._load_module(agent.value_model, tsv.torch_sd(th.make_twohot_value_params(K)))
    head = pr.make_pcont_params(cfg.belief_size, cfg.state_size, cfg.hidden_size)
    agent._load_module(agent.pcont_model, tsv.torch_sd(head))
    slow = th.make_twohot_value_params(K, seed=th.TWOHOT_SLOW_SEED)
    tsv.load_target(agent, slow)
    oracle = orf.OracleRulesCombined(cfg, A_, params=th.twohot_params(A_, K), pcont_params=head, slow_params=slow)
    assert oracle.rule == "laprop" and oracle.clip_mode == "agc" and oracle.th_on and oracle.rn_on
    io = agent.inv_dynamics_optimizer
    assert io.rule == "laprop" and io.agc is not None and agent.value_optimizer.target is not None
    for u in range(2):
        batch, _ = tu.dev_batch(L_, B_, A_, 60 + u)
        agent.noise_source, nz = tu.dev_noise(L_, B_, H_, A_, 160 + u)
        with tu.grad_snapshots(agent, ("model", "actor", "value", "inv_dynamics")) as snap:
            pi, pm = io.flat.clone(), agent.model_optimizer.flat.clone()
            beliefs, post = agent.train_dynamics(batch[0], batch[1], batch[2], 1.0 - batch[3])
            torch.cuda.synchronize()
            with torch.no_grad():
                for m in ("transition_model", "reward_model", "actor_model", "value_model", "pcont_model"):
                    for k, v in getattr(agent, m).state_dict().items():
                        oracle.p[m][k].copy_(v.cpu())
                for k, v in agent.slow_value_model.state_dict().items():
                    oracle.slow[k] = v.cpu().clone()
                oracle.value_opt.t = agent.value_optimizer.step_count
            agent.train_actor_critic(beliefs.flatten(0, 1), post.flatten(0, 1))
        t = {k: torch.as_tensor(v) for k, v in nz.items()}
        oscal = oracle.train_actor_critic(beliefs.flatten(0, 1).cpu(), post.flatten(0, 1).cpu(), t["img_act"],
                                          t["img_prior"], t["entropy"])
        assert all(np.isfinite(v) for v in agent.last_scalars.values()) and not agent.logger.nonfinite
        tag.check_against_oracle(agent, oracle, oscal, snap, ("actor", "value"), f"[rules combined] update {u}")
        for name in ("actor", "value"):
            opt = getattr(agent, f"{name}_optimizer")
            ratios, want = oracle.last[f"{name}_ratios"], oracle.last[f"{name}_coefs"]
            assert all(abs(r - 1.0) >= 0.02 for r in ratios), (name, ratios)
            worst = max(abs(a - b) / b for a, b in zip(opt.agc.coef.cpu().tolist(), want))
            log(f"[rules combined] update {u} {name}: coefficients worst {worst:.2e}, clipped {oracle.last[f'{name}_clipped']}; "
                f"unorm / upper {sorted(round(r, 4) for r in ratios)}")
            assert worst < 5e-3 and agent.last_scalars[f"train/agc_clipped_{name}"] == oracle.last[f"{name}_clipped"]
        for name in ("actor", "value"):
            assert 0 < oracle.last[f"{name}_clipped"] < len(oracle.last[f"{name}_coefs"]), (name, oracle.last[f"{name}_clipped"])
        # the model and the inverse-dynamics group, for which this configuration has no oracle class: coefficients and
        # clipped counts against float64 from the group's own pre-step parameters and snapshot gradient
        for name, before in (("model", pm), ("inv_dynamics", pi)):
            opt = getattr(agent, f"{name}_optimizer")
            gs, ps = snap[name].cpu(), before.cpu()
            P = [ps[o : o + q.numel()] for o, q in zip(opt.offsets, opt.params)]
            G = [gs[o : o + q.numel()] for o, q in zip(opt.offsets, opt.params)]
            coefs, ratios = orf.agc_coefs(G, P, float(F32(COMBINED_CLIP)), PMIN)
            worst = max(abs(a - b) / b for a, b in zip(opt.agc.coef.cpu().tolist(), coefs))
            count = sum(1 for c in coefs if c < 1.0)
            log(f"[rules combined] update {u} {name}: coefficients worst {worst:.2e}, clipped {count} of {len(coefs)}; "
                f"unorm / upper {sorted(round(r, 4) for r in ratios)}")
            assert all(abs(r - 1.0) >= 0.02 for r in ratios), (name, "a tensor within 2 % of its threshold", ratios)
            assert worst <= COEF_TOL, (name, worst)
            assert agent.last_scalars[f"train/agc_clipped_{name}"] == count == float(opt.agc_count), name
            assert 0 < count < len(coefs), (name, count)
    assert "train/agc_clipped_inv_dynamics" in agent.last_scalars


# ----------------------------------------------------------------------------- 4. the default path, traces
def _run_updates(agent, n, L=8, B=4, H=5, A=6):
    for u in range(n):
        batch, _ = tu.dev_batch(L, B, A, 11 + u)
        agent.noise_source, _ = tu.dev_noise(L, B, H, A, 101 + u)
        agent.update(batch)
    return agent.last_scalars


def test_default_path_is_untouched():
    L, B, H, A = 8, 4, 5, 6
    plain, cfg = tu.make_agent("repo", L, B, H, A)
    assert not any(hasattr(cfg, k) for k in ("grad_clip", "optimizer", "agc_clip", "agc_pmin", "optimizer_eps"))
    named, _ = tu.make_agent("repo", L, B, H, A, grad_clip="norm", optimizer="adam", agc_clip=0.01, agc_pmin=1.0)
    for agent in (plain, named):
        assert not agent._agc and agent.model_optimizer.rule == "adam" and agent.model_optimizer.agc is None
    for u in range(2):      # every scalar after each update, not only behind the last
        scalars = []
        for agent in (plain, named):
            batch, _ = tu.dev_batch(L, B, A, 11 + u)
            agent.noise_source, _ = tu.dev_noise(L, B, H, A, 101 + u)
            agent.update(batch)
            scalars.append(dict(agent.last_scalars))
        assert scalars[0] == scalars[1] and all(np.isfinite(v) for v in scalars[0].values()), u
    torch.cuda.synchronize()
    for name in ("model", "actor", "value"):
        a, b = getattr(named, f"{name}_optimizer"), getattr(plain, f"{name}_optimizer")
        assert same_bits(a.flat, b.flat) and same_bits(a.exp_avg, b.exp_avg) and same_bits(a.exp_avg_sq, b.exp_avg_sq), name
    assert named.last_scalars == plain.last_scalars and not any("agc" in k for k in plain.last_scalars)
    batch, _ = tu.dev_batch(L, B, A, 13)
    noise, _ = tu.dev_noise(L, B, H, A, 103)
    for agent in (plain, named):
        agent.noise_source = noise

        def three_updates(agent=agent):
            for _ in range(3):
                agent.update(batch)

        _, counts = tsv.counted(three_updates)
        assert tsv.n_launches(counts, OLD_KERNELS[0]) == 9 == tsv.n_launches(counts, OLD_KERNELS[1]), counts
        assert tsv.n_launches(counts, OLD_KERNELS[2]) == 9, counts
        for k in (PARTS_KERNEL, FINISH_KERNEL, STEP_KERNEL):
            assert tsv.n_launches(counts, k) == 0, (k, counts)


@pytest.mark.parametrize("clip,rule", [("agc", "adam"), ("norm", "laprop"), ("agc", "laprop")])
def test_switched_on_trace(clip, rule):
    """Three updates, three optimisers: at most three optimiser launches per step, the new kernels among them."""
    L, B, H, A = 8, 4, 5, 6
    agent, _ = tu.make_agent("dreamer", L, B, H, A, grad_clip=clip, optimizer=rule)
    batch, _ = tu.dev_batch(L, B, A, 13)
    agent.noise_source, _ = tu.dev_noise(L, B, H, A, 103)

    def three_updates():
        for _ in range(3):
            agent.update(batch)

    _, counts = tsv.counted(three_updates)
    assert tsv.n_launches(counts, STEP_KERNEL) == 9, counts
    assert tsv.n_launches(counts, OLD_KERNELS[2]) == 0 == tsv.n_launches(counts, OLD_KERNELS[3]), counts
    agc = 9 if clip == "agc" else 0
    assert tsv.n_launches(counts, PARTS_KERNEL) == agc == tsv.n_launches(counts, FINISH_KERNEL), counts
    assert tsv.n_launches(counts, OLD_KERNELS[0]) == 9 - agc == tsv.n_launches(counts, OLD_KERNELS[1]), counts
    assert all(np.isfinite(v) for v in agent.last_scalars.values())


# ----------------------------------------------------------------------------- 5. checkpoints, pipelining, refusals
def test_checkpoint_round_trip_continuation_and_mismatch():
    L, B, H, A = 8, 4, 5, 6
    over = dict(grad_clip="agc", optimizer="laprop")
    agent, _ = tu.make_agent("dreamer", L, B, H, A, **over)
    _run_updates(agent, 1)
    torch.cuda.synchronize()
    ck = agent.get_param_dict()
    for name in ("model", "actor", "value"):
        group = ck[f"{name}_optimizer"]["param_groups"][0]
        assert group["optimizer"] == "laprop" and group["eps"] == 1e-20
        assert not any("agc" in str(k) for k in group), "AGC is stateless: no key"
        assert list(ck[f"{name}_optimizer"]["state"][0]) == ["step", "exp_avg", "exp_avg_sq"]
    fresh, _ = tu.make_agent("dreamer", L, B, H, A, seed=8, **over)
    fresh.load_param_dict(ck)
    for a in (agent, fresh):
        a.noise_source = None
        a.seed_noise(5)
        a._noise_counter = 0
    b2, _ = tu.dev_batch(L, B, A, 12)
    for a in (agent, fresh):
        a.update(b2)
    torch.cuda.synchronize()
    for name in ("model", "actor", "value"):
        x, y = getattr(agent, f"{name}_optimizer"), getattr(fresh, f"{name}_optimizer")
        assert same_bits(x.flat, y.flat) and same_bits(x.exp_avg, y.exp_avg) and same_bits(x.exp_avg_sq, y.exp_avg_sq), name
    assert agent.last_scalars == fresh.last_scalars
    # across the rules, both ways: a ValueError naming the key before anything -- a weight, a moment, the step -- is taken
    def state(a):
        opts = (a.model_optimizer, a.actor_optimizer, a.value_optimizer)
        return ([o.flat.clone() for o in opts] + [o.exp_avg.clone() for o in opts] + [o.exp_avg_sq.clone() for o in opts],
                a.step, [o.step_count for o in opts])

    def unchanged(a, kept):
        now = state(a)
        return all(same_bits(x, y) for x, y in zip(now[0], kept[0])) and now[1:] == kept[1:]

    adam, _ = tu.make_agent("dreamer", L, B, H, A, seed=9, grad_clip="agc")
    _run_updates(adam, 1)
    torch.cuda.synchronize()
    lap_ck, adam_ck = dict(agent.get_param_dict(), step=123), dict(adam.get_param_dict(), step=77)
    assert "optimizer" not in adam_ck["model_optimizer"]["param_groups"][0]
    assert not same_bits(adam.model_optimizer.flat, agent.model_optimizer.flat) and adam.step not in (123, 77)
    for target, ck_ in ((adam, lap_ck), (fresh, adam_ck)):
        kept = state(target)
        with pytest.raises(ValueError, match="optimizer"):
            target.load_param_dict(ck_)
        torch.cuda.synchronize()
        assert unchanged(target, kept), "a refused load takes nothing from the checkpoint"
    # one optimiser entry of the other rule among matching ones is enough, whichever it is
    mixed = dict(lap_ck, value_optimizer=adam_ck["value_optimizer"])
    kept = state(fresh)
    with pytest.raises(ValueError, match="optimizer"):
        fresh.load_param_dict(mixed)
    assert unchanged(fresh, kept)


def test_two_seeded_agents_are_bit_equal():
    L, B, H, A = 8, 4, 5, 6
    batches = [tu.dev_batch(L, B, A, 300 + i)[0] for i in range(3)]
    finals = []
    for _ in range(2):
        agent, _cfg = tu.make_agent("repo", L, B, H, A, grad_clip="agc", optimizer="laprop")
        agent.seed_noise(99)
        for b in batches:
            agent.update(b, join=False)
        agent.synchronize()
        torch.cuda.synchronize()
        assert all(np.isfinite(v) for v in agent.last_scalars.values())
        opts = (agent.model_optimizer, agent.actor_optimizer, agent.value_optimizer)
        finals.append([o.flat.clone() for o in opts] + [o.exp_avg.clone() for o in opts] + [o.agc.out.clone() for o in opts]
                      + [torch.tensor([agent.last_scalars[k] for k in sorted(agent.last_scalars)])])
    for a, b in zip(*finals):
        assert same_bits(a, b)


@pytest.mark.parametrize("over", [dict(grad_clip="agc"), dict(optimizer="laprop"), dict(grad_clip="agc", optimizer="laprop")])
@pytest.mark.parametrize("family", ["FinetunedRePo", "CalibratedRePo", "TIA", "MultitaskDreamer", "MultitaskRePo"])
def test_other_families_refuse(family, over):
    from tests import test_pcont_gpu as tp

    build = tp._family_builders()[family]
    with pytest.raises(NotImplementedError, match="grad_clip"):
        build(**over)
    if len(over) == 2:
        agent = build(grad_clip="norm", optimizer="adam")
        assert type(agent).__name__ == family and agent.model_optimizer.rule == "adam" and agent.model_optimizer.agc is None


@pytest.mark.parametrize("over,key", [(dict(grad_clip="global"), "grad_clip"), (dict(optimizer="sgd"), "optimizer"),
                                      (dict(grad_clip="agc", agc_clip=0.0), "agc_clip"),
                                      (dict(grad_clip="agc", agc_pmin=float("nan")), "agc_pmin"),
                                      (dict(optimizer="laprop", optimizer_eps=-1.0), "optimizer_eps")])
@pytest.mark.parametrize("algo", ["repo", "dreamer"])
def test_out_of_range_keys_raise(algo, over, key):
    with pytest.raises(ValueError, match=key):
        tu.make_agent(algo, 8, 4, 5, 6, **over)
