"""Every entry point of csrc/multitask.hip on its own, against the float64 statement of tests/mt_ref.py, at each grid regime,
plane size and layer geometry, with proof of which kernels ran.

Regimes (tests/mt_ref.py mirrors each grid; tests/test_mt_ref_cpu.py asserts that every case below is where its id says):
 * film_fwd_kernel, P >= 64: a wave per plane, min(8192, ceil(planes / 4)) blocks -- one plane, P = 64 | 65 | 961, exactly 8192
   blocks, 32769 planes (wave 0 alone takes a second pass) and 65540 (waves 0..3 a third); P < 64: a lane per element,
   min(8192, ceil(planes P / 256)) -- P = 1, 63, 4 and 2097200 elements (48 over the cap);
 * film_bwd_kernel<false|true>: a wave per plane, min(16384, ceil(planes / 4)) -- P = 1, 63 | 64 | 65, 961, exactly 16384 blocks
   (65536 planes), 65535 (the last wave idle), 65537 (one plane on a second pass), 131073 (one on a third).  The capped
   cases carry 1 + gamma = 0.5 on every plane but 0, 65535, 65536 and planes - 1, which carry 2 (beta = 0): both products
   are exact, dy is held BITWISE, and a plane index carried wrongly into a later pass shows as a factor 4;
 * film_exact_kernel: a block per plane, min(4096, planes); S = the k-slices per pixel (mt_ref.film_exact_slices).  Dense,
   convolution and transposed convolution at geometries of no layer of the project: S clamped to 3 and 7 (256 / S does not
   divide 256: threads with sl >= S), K = 1, the four-accumulator loop with and without its tail, the tail alone, two pixel
   batches, odd KS and HB, a 1 x 1 input of the transpose, uint8 input, per-channel | per-element | no bias, and 65792
   planes (17 passes of film_exact, two of film_bwd) with gated-off planes on the first pass, on both sides of 4096, on
   film_bwd's second pass and at planes - 1 -- and at planes - 1 alone;
 * film_tables_kernel: min(4096, ceil(nimg 2 total / 256)) -- 1, 2, 3 and 4 layers, ldfilm = and > 2 total, nimg = 1, 9, 1093
   (the encoder list: 233 elements over the cap) and 2500 (the workload: three passes);
 * kl_tasks_kernel: min(512, ceil(rows / 4)) blocks of four waves, a row per wave -- 1 row, 2048 (512 blocks, one pass), 2049
   (one row on a second pass; S = 1 and S = 64), 6145 (one on a fourth); one-hot tasks with one task absent, and real-valued
   task rows; mt_final_sum_kernel's sums are reduce_ref.fixed_order_sum of the partials BIT FOR BIT (it is
   final_sum_kernel's loop: 256 threads stride the row, block_sum);
 * dual_step_tasks_kernel: C = 1, 3, 13, five steps with carried moments.

Every output comes from the conftest's NaN-filled torch.empty: "every element written" is isfinite(...).all().  dfilm starts
as a sentinel that must survive bit for bit outside the two (n, C) blocks; ld = 2C + 24 with the blocks in the middle of the
row, beta below gamma when C is odd.

Tolerances (u = 2^-24; none is tuned to the kernels):
 * film_fwd per element: |got - want| <= 2^-23 (|(1 + gamma) y| + |beta|): a rounding of 1 + gamma, one of the FMA, and slack;
   the ReLU is 1-Lipschitz, so it holds across the kink;
 * dy per element: <= 2^-23 |dh (1 + gamma)|;
 * d gamma, d beta summed from y / dh: <= (ceil(P / 64) + 8) u sum |terms|, the lane's chain plus the six butterfly steps;
 * the gamma gradient of recomputed (gated-off) planes, the KL gradients and sums, the dual step's scalars: the convention
   of tests/test_vdb_kernels_gpu.py -- 8 x the error of mt_ref's statement run in float32 on the CPU against its float64 self
   on the same inputs, the largest over the group's cases (`measure_f32()`; tests/test_mt_ref_cpu.py holds the table F32 to
   it; the statement adds term by term in a fixed order -- mt_ref.film_layer_y_seq, seq_sum, reduce_ref.fixed_order_sum -- so
   that the figure does not depend on a host's convolution, matrix product or vectorised sum), and never above the figure
   tests/test_mt_gpu.py asserts for the same quantity: 1e-5 (gated and recovered d gamma, d beta; max error over max |want|),
   2e-5 (KL gradients, relerr), FTOL (sums, against sum |terms|; scalars, relative).
   The factor 8 covers another summation order, FMA contraction and the device's expf / logf;
 * log_beta after k steps: k (2^-24 |log_beta| + 2^-18 lr) per entry (tests/test_reductions_gpu.py derives it), and the
   reference's own step is more than 100 times that."""
import ctypes
import functools
import math

import numpy as np
import pytest
import torch

from tests import mt_ref as mr
from tests import reduce_ref as rr
from tests.test_reductions_gpu import F32 as f32, FTOL, dev, same_bits
from tests.util import has, log, relerr, rnd, traced

pytestmark = pytest.mark.gpu

SENT = -12345.0
U = 2.0 ** -24
ENC_CHANNELS, DEC_CHANNELS = [32, 64, 128, 256], [128, 64, 32]      # models/conditional.py (asserted in the CPU tests)

FWD_CASES = [(1, 1, 64), (3, 5, 65), (2, 3, 961), (128, 256, 64), (3, 10923, 64), (5, 13108, 64),
             (1, 1, 1), (2, 3, 63), (4, 256, 4), (7, 11984, 25)]
BWD_SMALL = [(1, 1, 1), (2, 3, 63), (2, 3, 64), (2, 3, 65), (2, 3, 961)]
BWD_CAP = [(256, 256, 4), (257, 255, 4), (1, 65537, 4), (3, 43691, 4)]
BWD_CASES = BWD_SMALL + BWD_CAP
MARKED = (0, 65535, 65536, -1)        # the planes of a capped case that carry 1 + gamma = 2, beta = 0

# repo_film_bwd_h with a description: (kind, dims, uint8 input); dims as the module docstring of mt_ref.film_layer_y
DENSE_SMALL = [(3, 7, 5, 4), (3, 1, 5, 25), (2, 70, 3, 25), (2, 1024, 4, 25)]             # (n, K, C, P)
DENSE_BIG = (257, 7, 256, 4)
DOWN_CASES = [((3, 3, 5, 10, 4), False), ((3, 3, 5, 10, 4), True), ((2, 21, 4, 10, 4), False), ((2, 70, 4, 10, 4), False),
              ((2, 5, 3, 9, 3), False), ((2, 4, 3, 36, 4), True)]                          # (n, CB, CS, HB, KS), uint8
UP_CASES = [(2, 6, 5, 4, 5), (2, 6, 5, 4, 6), (3, 7, 4, 1, 4), (2, 9, 3, 8, 6)]            # (n, CS, CB, HS, KS)
BIASES = ["channel", "element", "none"]
GATED = (-1.0, -1.0 + 1e-4, -1.0 - 1e-4)          # 1 + gamma in {0, +-1e-4}: recomputed
RECOVERED = (-0.95, -1.05)                        # 1 + gamma = +-0.05: recovered from h
BIG_GATED_PLANES = (0, 4095, 4096, 65536, -1)

EXACT_CASES = ([(mr.DENSE, d, False, b, "std") for d in DENSE_SMALL for b in BIASES]
               + [(mr.DENSE, DENSE_BIG, False, b, "std") for b in BIASES] + [(mr.DENSE, DENSE_BIG, False, "channel", "last")]
               + [(mr.CONV_DOWN, d, u8, "channel", "std") for d, u8 in DOWN_CASES]
               + [(mr.CONV_UP, d, False, "channel", "std") for d in UP_CASES])

TABLE_CASES = ([(n, ch, wide) for ch in ([1], [5, 3], ENC_CHANNELS, DEC_CHANNELS) for n in (1, 9) for wide in (False, True)]
               + [(1093, ENC_CHANNELS, False), (2500, ENC_CHANNELS, True)])

KL_CASES = [(1, 30, 1, False), (2048, 30, 3, False), (2049, 1, 3, False), (2049, 64, 13, False), (6145, 30, 13, False),
            (2049, 64, 13, True)]                 # (rows, S, C, real-valued task rows)
DUAL_CS = [1, 3, 13]
DUAL_LR, DUAL_ROWS, DUAL_STEPS = 1e-2, 100, 5
BETAS = (f32(0.9), f32(0.999))

# group -> the error of mt_ref's float32 statement against its float64 self, the largest over the group's cases
# (measure_f32() recomputes it); metrics as the bounds of the module docstring
F32 = {"gated_dense": 3.3e-07, "gated_down": 5.5e-07, "gated_up": 2.1e-07, "kl_grads": 2.5e-07, "kl_sums": 1.2e-07,
       "dual_scalars": 2.7e-07}
FIGURE = {"gated_dense": 1e-5, "gated_down": 1e-5, "gated_up": 1e-5, "kl_grads": 2e-5, "kl_sums": FTOL, "dual_scalars": FTOL}


def bound(name):
    return min(FIGURE[name], 8.0 * F32[name])


# --------------------------------------------------------------------------------------------------------------- inputs
def offsets(C):
    """(ld, gamma_off, beta_off): both blocks inside a wider row; beta BELOW gamma when C is odd."""
    return (2 * C + 24, 5, C + 19) if C % 2 == 0 else (2 * C + 24, C + 11, 3)


def plane_block(film, off, C):
    return film[:, off:off + C]


def _away_from_gate(gamma):
    """Push 1 + gamma out of (-0.1, 0.1): recovering y from h loses eps |beta| / |(1 + gamma) y| (csrc/multitask.hip), and the
    planes near the gate have tests of their own."""
    g1 = 1 + gamma
    near = g1.abs() < 0.1
    gamma[near] = torch.where(g1[near] < 0, torch.tensor(-1.1), torch.tensor(-0.9))
    return gamma


@functools.lru_cache(maxsize=None)
def film_inputs(n, C, P, marked=False):
    """y, film (gamma ~ 0.5 N(0, 1) kept away from -1, beta ~ 0.5 N(0, 1)), the two offsets and an upstream gradient.
    marked: 1 + gamma = 0.5 on every plane but MARKED, where it is 2 with beta = 0."""
    rs = np.random.RandomState(n * 1000 + C + P)
    ld, goff, boff = offsets(C)
    y, up = rnd(rs, n, C, P), rnd(rs, n, C, P)
    film = rnd(rs, n, ld, scale=0.5)
    _away_from_gate(plane_block(film, goff, C))
    if marked:
        gam = torch.full((n * C,), -0.5)
        bet = plane_block(film, boff, C).reshape(-1).clone()
        for pl in MARKED:
            if pl < n * C:
                gam[pl], bet[pl] = 1.0, 0.0
        plane_block(film, goff, C).copy_(gam.view(n, C))
        plane_block(film, boff, C).copy_(bet.view(n, C))
    return y, film, goff, boff, up


def exact_geometry(kind, dims):
    """-> (n, C, P, geo as the ABI takes it, outer reduction length)."""
    if kind == mr.DENSE:
        n, K, C, P = dims
        return n, C, P, (K, 0, 0, 0), K
    if kind == mr.CONV_DOWN:
        n, CB, CS, HB, KS = dims
        HS = (HB - KS) // 2 + 1
        return n, CS, HS * HS, (CB, CS, HB, KS), CB
    n, CS, CB, HS, KS = dims
    HB = 2 * (HS - 1) + KS
    return n, CB, HB * HB, (CB, CS, HB, KS), CS


def gated_planes(planes, mode, rs):
    """{plane: gamma} of the special planes of an exact case."""
    if mode == "last":
        return {planes - 1: GATED[0]}
    if mode == "none":        # the same planes, all recovered: a call without a gated-off plane
        return {p: RECOVERED[i % 2] for i, p in enumerate(gated_planes(planes, "std", rs))}
    if planes > 60000:
        sp = {p % planes: GATED[i % 3] for i, p in enumerate(BIG_GATED_PLANES)}
        sp.update({1: RECOVERED[0], 4097: RECOVERED[1], 65537: RECOVERED[0]})
        return sp
    pick = rs.choice(planes, size=5, replace=False)
    return {int(p): v for p, v in zip(pick, GATED + RECOVERED)}


@functools.lru_cache(maxsize=None)
def exact_case(kind, dims, u8=False, bias_mode="channel", gate="std"):
    """A layer (x, w, bias), its float64 output y, a FiLM row per image with beta > 0 (a gated-off plane is ACTIVE: h = beta)
    and the special planes of gated_planes(), h = relu((1 + gamma) y + beta) rounded to float32, and dh = a random
    cotangent masked by h > 0."""
    n, C, P, geo, outer = exact_geometry(kind, dims)
    rs = np.random.RandomState(100 * sum((i + 1) * d for i, d in enumerate(dims)) + 10 * kind + int(u8))
    if kind == mr.DENSE:
        K = dims[1]
        x, w = rnd(rs, n, K), rnd(rs, K, C * P, scale=3.0 / math.sqrt(K))      # y ~ 3 N(0, 1): the ReLU is live against beta > 0
        bias = {"channel": rnd(rs, C), "element": rnd(rs, C * P), "none": None}[bias_mode]
        geo = (K, int(bias_mode == "element"), 0, 0)
    else:
        CB, CS, HB, KS = geo
        HS = (HB - KS) // 2 + 1
        hin, cin = (HB, CB) if kind == mr.CONV_DOWN else (HS, CS)
        x = torch.from_numpy(rs.randint(0, 256, (n, cin, hin, hin)).astype(np.uint8)) if u8 else rnd(rs, n, cin, hin, hin)
        taps = KS * KS if kind == mr.CONV_DOWN else ((KS + 1) // 2) ** 2
        w = rnd(rs, CS, CB, KS, KS, scale=(5.0 if u8 else 3.0) / math.sqrt(cin * taps))
        bias = rnd(rs, C)
    y64 = mr.film_layer_y(kind, geo, x, w, bias).reshape(n, C, P)
    ld, goff, boff = offsets(C)
    film = rnd(rs, n, ld, scale=0.5)
    _away_from_gate(plane_block(film, goff, C))
    plane_block(film, boff, C).copy_(plane_block(film, boff, C).abs() + 0.2)
    gam = plane_block(film, goff, C).reshape(-1).clone()
    special = gated_planes(n * C, gate, np.random.RandomState(n * C))
    for pl, v in special.items():
        gam[pl] = v
    plane_block(film, goff, C).copy_(gam.view(n, C))
    h = mr.film_fwd(y64, film, goff, boff)[0].float().contiguous()
    dh = (rnd(rs, n, C, P) * (h > 0)).contiguous()
    return dict(kind=kind, geo=geo, n=n, C=C, P=P, outer=outer, x=x, w=w, bias=bias, y64=y64, film=film, goff=goff, boff=boff,
                h=h, dh=dh, special=special)


def is_gated(film, goff, C):
    """The kernel's decision, on the kernel's float32 1 + gamma."""
    return np.abs(np.float32(1.0) + plane_block(film, goff, C).numpy()) < np.float32(mr.FILM_EXACT_BELOW)


def gated_err(got_g, want_g, gated):
    """max |got - want| over the gated-off planes / max |want| over all planes."""
    got_g, want_g = got_g.double().cpu(), want_g.double().cpu()
    return float(((got_g - want_g).abs() * gated).max() / want_g.abs().max())


def exact_f32_err(c):
    """The float32 statement of the gated-off planes' gamma gradient: the layer in float32 and d gamma = sum dh * y, both added
    term by term in a fixed order (mt_ref.film_layer_y_seq, seq_sum), so that every host measures the same figure."""
    y32 = mr.film_layer_y_seq(c["kind"], c["geo"], c["x"], c["w"], c["bias"]).reshape(c["n"], c["C"], c["P"])
    want = mr.film_bwd(c["dh"], c["y64"], c["film"], c["goff"], c["boff"])[1]
    gated = torch.from_numpy(is_gated(c["film"], c["goff"], c["C"]))
    return gated_err(mr.seq_sum(c["dh"] * y32, 2), want, gated)


@functools.lru_cache(maxsize=None)
def kl_inputs(rows, S, C, real):
    """pm, qm ~ N(0, 1), ps, qs = |N(0, 1)| + 0.2, log_beta ~ U(-3, -1); tasks one-hot with task C - 1 absent (C > 1), or
    real-valued rows ~ 0.5 N(0, 1); alpha, target, scale as the float32 values the kernel receives."""
    rs = np.random.RandomState(rows + 100 * S + C + 7 * real)
    pm, qm = rnd(rs, rows, S), rnd(rs, rows, S)
    ps, qs = rnd(rs, rows, S).abs() + 0.2, rnd(rs, rows, S).abs() + 0.2
    if real:
        tasks = rnd(rs, rows, C, scale=0.5)
    else:
        tasks = torch.from_numpy(np.eye(C, dtype=np.float32)[rs.randint(0, max(C - 1, 1), rows)])
    lb = torch.from_numpy(rs.uniform(-3, -1, C).astype(np.float32))
    return pm, ps, qm, qs, f32(5 / 6), lb, tasks, f32(0.7), f32(1.0 / rows)


def f32_sums(terms):
    """The column sums of the float32 statement's terms, in the device's fixed order: reproducible on every host."""
    t = terms.numpy()
    return torch.from_numpy(np.array([rr.fixed_order_sum(t[:, v]) for v in range(t.shape[1])], dtype=np.float32))


def kl_errs(sums, grads, ref):
    """(the largest sum_err over the 3 + C sums, the largest relerr over the four gradients) against ref = mr.kl_tasks()."""
    terms, g64 = ref
    sums = sums.detach().double().cpu().reshape(-1)
    es = max(abs(sums[v].item() - terms[:, v].sum().item()) / (terms[:, v].abs().sum().item() + 1e-300) for v in range(terms.shape[1]))
    return es, max(relerr(g.reshape(w.shape), w) for g, w in zip(grads, g64))


@functools.lru_cache(maxsize=None)
def dual_inputs(C):
    """log_beta ~ U(-3, -1) and five (3 + C) rows of sums: every third task sees a negative violation, the others a positive one,
    task 0 changes sides at steps 2 and 4; task 1 (C > 1) has a zero gradient throughout."""
    rs = np.random.RandomState(40 + C)
    lb = torch.from_numpy(rs.uniform(-3, -1, C).astype(np.float32))
    sums = torch.from_numpy(rs.uniform(0.5, 3.0, (DUAL_STEPS, 3 + C)).astype(np.float32)) * DUAL_ROWS
    sign = torch.tensor([-1.0 if i % 3 == 2 else 1.0 for i in range(C)])
    sums[:, 3:] *= sign
    sums[1, 3] *= -1
    sums[3, 3] *= -1
    if C > 1:
        sums[:, 4] = 0.0
    return lb, sums


def dual_run(C, dtype):
    """mt_ref.dual_step_tasks carried over the five steps at `dtype`: -> [(log_beta, m, v, scalars) per step]."""
    lb0, sums = dual_inputs(C)
    lb, m, v = lb0.to(dtype), torch.zeros(C, dtype=dtype), torch.zeros(C, dtype=dtype)
    out = []
    for k in range(DUAL_STEPS):
        lb, m, v, sc = mr.dual_step_tasks(lb, m, v, sums[k], DUAL_ROWS, DUAL_LR, BETAS[0], BETAS[1], 1e-8, k + 1, dtype=dtype)
        out.append((lb, m, v, sc))
    return out


def scalar_err(got, want):
    got, want = got.detach().double().cpu(), want.double()
    return float(((got - want).abs() / want.abs().clamp_min(1e-300)).max())


def measure_f32():
    """The table F32, recomputed."""
    out = {k: 0.0 for k in F32}
    for kind, dims, u8, b, gate in EXACT_CASES:
        key = {mr.DENSE: "gated_dense", mr.CONV_DOWN: "gated_down", mr.CONV_UP: "gated_up"}[kind]
        out[key] = max(out[key], exact_f32_err(exact_case(kind, dims, u8, b, gate)))
    for case in KL_CASES:
        a = kl_inputs(*case)
        t32, g32 = mr.kl_tasks(*a, dtype=torch.float32)
        es, eg = kl_errs(f32_sums(t32), g32, mr.kl_tasks(*a))
        out["kl_sums"], out["kl_grads"] = max(out["kl_sums"], es), max(out["kl_grads"], eg)
    for C in DUAL_CS:
        for lo, hi in zip(dual_run(C, torch.float32), dual_run(C, torch.float64)):
            out["dual_scalars"] = max(out["dual_scalars"], scalar_err(lo[3], hi[3]))
    return out


# -------------------------------------------------------------------------------------------------------------- helpers
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


K_FWD, K_TABLES, K_EXACT = r"\bfilm_fwd_kernel\b", r"\bfilm_tables_kernel\b", r"\bfilm_exact_kernel\b"
K_BWD_Y, K_BWD_H = r"\bfilm_bwd_kernel<(false|\(bool\)0)>", r"\bfilm_bwd_kernel<(true|\(bool\)1)>"
K_KL, K_KL_SUM, K_DUAL = r"\bkl_tasks_kernel\b", r"\bmt_final_sum_kernel\b", r"\bdual_step_tasks_kernel\b"


def device():
    return torch.device("cuda", torch.cuda.current_device())


def sentinel_like(film):
    return torch.full(film.shape, SENT, dtype=torch.float32, device="cuda")


def outside_kept(dfilm, goff, boff, C):
    mask = torch.ones(dfilm.shape, dtype=torch.bool, device=dfilm.device)
    mask[:, goff:goff + C] = False
    mask[:, boff:boff + C] = False
    return bool((dfilm[mask] == SENT).all())


def written(*ts):
    return all(bool(torch.isfinite(t).all()) for t in ts)


def within(got, want, tol):
    """Every |got - want| <= tol (elementwise tensors, float64 on the host); -> (ok, the largest |got - want| / tol)."""
    e = (got.detach().double().cpu().reshape(want.shape) - want).abs()
    ratio = (e / tol.clamp_min(1e-300)).max().item()
    return bool((e <= tol).all()), ratio


def sum_tol(P, sabs):
    return (-(-P // 64) + 8) * U * sabs


def fwd_id(n, C, P):
    b = mr.film_fwd_blocks(n * C, P)
    return f"n{n}-C{C}-P{P}-{'wave' if P >= 64 else 'elem'}-{b}blk-{mr.film_fwd_passes(n * C, P)}pass"


def bwd_id(n, C, P):
    return f"n{n}-C{C}-P{P}-{mr.film_bwd_blocks(n * C)}blk-{mr.film_bwd_passes(n * C)}pass"


def exact_id(case):
    kind, dims, u8, b, gate = case
    n, C, P, geo, outer = exact_geometry(kind, dims)
    S, batches, main, tail, idle = mr.film_exact_loops(kind, geo, P)
    name = {mr.DENSE: "dense", mr.CONV_DOWN: "down", mr.CONV_UP: "up"}[kind]
    return (f"{name}-{'x'.join(map(str, dims))}{'-u8' if u8 else ''}-bias_{b}-gate_{gate}-P{P}-S{S}-{batches}batch-main{main}-tail{tail}"
            f"-{mr.film_exact_passes(n * C)}pass")


# ------------------------------------------------------------------------------------------------------------- film_fwd
@pytest.mark.parametrize("n,C,P", FWD_CASES, ids=[fwd_id(*c) for c in FWD_CASES])
def test_film_fwd_at_each_grid_regime_and_plane_size(ops, n, C, P):
    y, film, goff, boff, _ = film_inputs(n, C, P)
    want, mag = mr.film_fwd(y, film, goff, boff)
    yd, fd = dev(y), dev(film)
    h, names = traced(lambda: ops.film_fwd(yd, fd, goff, boff))
    assert has(names, K_FWD), names
    assert written(h), "an output element was left unwritten"
    ok, r = within(h, want, 2.0 ** -23 * mag)
    log(f"film_fwd {fwd_id(n, C, P)}: largest |h - h64| / (2^-23 (|(1 + gamma) y| + |beta|)) = {r:.3f}")
    assert ok, (n, C, P, r)
    assert same_bits(ops.film_fwd(yd, fd, goff, boff), h), "two calls differ"


# ------------------------------------------------------------------------------------------------------------- film_bwd
@pytest.mark.parametrize("n,C,P", BWD_CASES, ids=[bwd_id(*c) for c in BWD_CASES])
def test_film_bwd_and_bwd_h_kind0_at_each_grid_regime(ops, n, C, P):
    """repo_film_bwd on the saved y and repo_film_bwd_h (no description) on h = film_fwd(y), the same dh."""
    marked = (n, C, P) in BWD_CAP
    y, film, goff, boff, up = film_inputs(n, C, P, marked)
    yd, fd = dev(y), dev(film)
    h = ops.film_fwd(yd, fd, goff, boff)
    dh = (dev(up) * (h > 0)).contiguous()
    dy64, dg64, db64, sg, sb = mr.film_bwd(dh.cpu(), y, film, goff, boff)
    dfa = sentinel_like(film)
    dya, names = traced(lambda: ops.film_bwd(dh, yd, fd, goff, boff, dfa))
    assert has(names, K_BWD_Y) and not has(names, K_BWD_H) and not has(names, K_EXACT), names
    assert written(dya, dfa) and outside_kept(dfa, goff, boff, C)
    ok_y, ry = within(dya, dy64, 2.0 ** -23 * dy64.abs())
    ok_g, rg = within(plane_block(dfa, goff, C), dg64, sum_tol(P, sg))
    ok_b, rb = within(plane_block(dfa, boff, C), db64, sum_tol(P, sb))
    log(f"film_bwd {bwd_id(n, C, P)}: error / bound: dy {ry:.3f} d gamma {rg:.3f} d beta {rb:.3f}")
    assert ok_y and ok_g and ok_b, (n, C, P, ry, rg, rb)
    if marked:   # 1 + gamma is 0.5 or 2: the product is exact, and a wrong plane is a factor 4
        g = (1 + plane_block(fd, goff, C)).reshape(n, C, 1)
        assert sorted(g.unique().tolist()) == [0.5, 2.0] and same_bits(dya, dh * g)
    dfb = sentinel_like(film)
    dyb, names = traced(lambda: ops.film_bwd_h(dh, h, fd, goff, boff, dfb))
    assert has(names, K_BWD_H) and not has(names, K_BWD_Y) and not has(names, K_EXACT), names
    assert written(dyb, dfb) and outside_kept(dfb, goff, boff, C)
    assert same_bits(dya, dyb), "dy of the two entry points differs"
    assert same_bits(plane_block(dfa, boff, C), plane_block(dfb, boff, C)), "d beta of the two entry points differs"
    eg = relerr(plane_block(dfb, goff, C), plane_block(dfa, goff, C))
    log(f"film_bwd_h kind 0 {bwd_id(n, C, P)}: d gamma from the recovered y against the saved y: relerr {eg:.2e}")
    assert eg < 2e-5, (n, C, P, eg)


# ------------------------------------------------------------------------------------- film_bwd_h with a layer description
def run_exact(ops, c, exact=True, **kw):
    """-> (dy, dfilm, kernel names) of one repo_film_bwd_h call on the case's data."""
    x = c["x"].cuda() if c["x"].dtype == torch.uint8 else dev(c["x"])
    desc = None
    if exact:
        which = c["geo"] if c["kind"] != mr.DENSE else (c["geo"][0], bool(c["geo"][1]))
        desc = (c["kind"], which, x, dev(c["w"]), None if c["bias"] is None else dev(c["bias"]))
    dfilm = sentinel_like(c["film"])
    dh, h, fd = dev(c["dh"]), dev(c["h"]), dev(c["film"])
    dy, names = traced(lambda: ops.film_bwd_h(dh, h, fd, c["goff"], c["boff"], dfilm, exact=desc, **kw))
    return dy, dfilm, names


def check_exact(c, dy, dfilm, names, what, key):
    n, C, P, goff, boff = c["n"], c["C"], c["P"], c["goff"], c["boff"]
    assert has(names, K_BWD_H) and has(names, K_EXACT), names
    assert written(dy, dfilm) and outside_kept(dfilm, goff, boff, C), what
    dy64, dg64, db64, sg, sb = mr.film_bwd(c["dh"], c["y64"], c["film"], goff, boff)
    gated = torch.from_numpy(is_gated(c["film"], goff, C))
    got_g, got_b = plane_block(dfilm, goff, C), plane_block(dfilm, boff, C)
    ok_y, ry = within(dy, dy64, 2.0 ** -23 * dy64.abs())
    ok_b, rb = within(got_b, db64, sum_tol(P, sb))
    eg, er = gated_err(got_g, dg64, gated), gated_err(got_g, dg64, ~gated)
    eb = float((got_b.double().cpu() - db64).abs().max() / db64.abs().max())
    log(f"film_bwd_h {what}: gated d gamma {eg:.2e} (float32 statement {exact_f32_err(c):.2e}, bound {bound(key):.1e}) "
        f"recovered {er:.2e} d beta {eb:.2e}; error / bound: dy {ry:.3f} d beta {rb:.3f}")
    assert ok_y and ok_b, (what, ry, rb)
    assert eg <= bound(key) and er < 1e-5 and eb < 1e-5, (what, eg, er, eb)


@pytest.mark.parametrize("case", EXACT_CASES, ids=[exact_id(c) for c in EXACT_CASES])
def test_film_bwd_h_recomputes_gated_off_planes_at_any_geometry(ops, case):
    kind = case[0]
    c = exact_case(*case)
    dy, dfilm, names = run_exact(ops, c)
    key = {mr.DENSE: "gated_dense", mr.CONV_DOWN: "gated_down", mr.CONV_UP: "gated_up"}[kind]
    check_exact(c, dy, dfilm, names, exact_id(case), key)
    dy2, dfilm2, _ = run_exact(ops, c)
    assert same_bits(dy, dy2) and same_bits(dfilm, dfilm2), "two calls differ"


@pytest.mark.parametrize("order", ["ABA", "BAB"])
def test_film_bwd_h_epoch_word_between_calls_with_and_without_gated_planes(ops, order):
    """A has gated-off planes, B has the same planes at 1 + gamma = +-0.05; on one stream, in both orders.  Every call is
    judged on its own.  The A calls exercise the word: a call that failed to stamp it with its own epoch (the word then holds
    B's or an earlier A's) would skip the recomputation and miss the reference; each A is also bit-equal to the first.  The B
    calls show the per-plane gate of film_exact_kernel, not the word: it re-reads 1 + gamma per plane, so without a
    gated-off plane it writes nothing whatever the word holds, and B is bit-equal to what kind 0 writes."""
    case = (mr.CONV_DOWN, (3, 3, 5, 10, 4), False, "channel")
    A, B = exact_case(*case, "std"), exact_case(*case, "none")
    C = A["C"]
    assert is_gated(A["film"], A["goff"], C).any() and not is_gated(B["film"], B["goff"], C).any()
    _, b0, names0 = run_exact(ops, B, exact=False)
    assert not has(names0, K_EXACT)
    first = None
    for i, which in enumerate(order):
        c = A if which == "A" else B
        dy, dfilm, names = run_exact(ops, c)
        check_exact(c, dy, dfilm, names, f"epoch {order}[{i}]={which}", "gated_down")
        if which == "B":
            assert same_bits(dfilm, b0), (order, i, "a call without gated-off planes is not what kind 0 writes")
        elif first is None:
            first = dfilm
        else:
            assert same_bits(dfilm, first), (order, i)


@pytest.mark.parametrize("case", [(mr.DENSE, (3, 7, 5, 4), False, "channel", "std"), (mr.DENSE, DENSE_BIG, False, "element", "std"),
                                  (mr.CONV_UP, (2, 9, 3, 8, 6), False, "channel", "std")], ids=exact_id)
def test_film_bwd_h_without_an_epoch_word_equals_the_call_with_it(ops, case):
    c = exact_case(*case)
    assert is_gated(c["film"], c["goff"], c["C"]).any()
    dy, dfilm, _ = run_exact(ops, c)
    dy0, dfilm0, names = run_exact(ops, c, epoch_word=False)
    assert has(names, K_BWD_H) and has(names, K_EXACT), names
    assert same_bits(dy, dy0) and same_bits(dfilm, dfilm0)
    b = exact_case(*case[:4], "none")     # ... and without a gated-off plane the walk writes nothing
    _, k0, _ = run_exact(ops, b, exact=False)
    _, k1, _ = run_exact(ops, b, epoch_word=False)
    assert same_bits(k0, k1)


# ---------------------------------------------------------------------------------------------------------- film_tables
def table_id(case):
    n, ch, wide = case
    tot = sum(ch)
    return (f"n{n}-ch{'_'.join(map(str, ch))}-ld{'wide' if wide else 'tight'}-{mr.film_tables_blocks(n, tot)}blk-"
            f"{mr.film_tables_passes(n, tot)}pass")


@pytest.mark.parametrize("case", TABLE_CASES, ids=table_id)
def test_film_tables_any_layer_list_pitch_and_grid(ops, case):
    n, ch, wide = case
    tot = sum(ch)
    ld = 2 * tot + (7 if wide else 0)
    film = rnd(np.random.RandomState(n + tot), n, ld, scale=0.5)
    flat, views = mr.film_tables(film[:, :2 * tot], ch)
    fd = dev(film)
    tabs, names = traced(lambda: ops.film_tables(fd, ch))
    assert has(names, K_TABLES), names
    assert len(tabs) == len(ch)
    for l, (got, want) in enumerate(zip(tabs, views)):
        assert got.shape == want.shape and torch.equal(got.cpu(), want), (case, l)
    assert torch.equal(torch.cat([t.reshape(-1) for t in tabs]).cpu(), flat)
    assert same_bits(fd, dev(film))


# ----------------------------------------------------------------------------------------------------- kl_balance_tasks
def kl_id(case):
    rows, S, C, real = case
    return f"rows{rows}-S{S}-C{C}-{'real' if real else 'onehot'}-{mr.kl_tasks_blocks(rows)}blk-{mr.kl_tasks_passes(rows)}pass"


@pytest.mark.parametrize("case", KL_CASES, ids=kl_id)
def test_kl_balance_tasks_at_each_grid_regime(ops, case):
    rows, S, C, real = case
    a = kl_inputs(*case)
    ref = mr.kl_tasks(*a)
    pm, ps, qm, qs, alpha, lb, tasks, target, scale = a
    d = [dev(t) for t in (pm, ps, qm, qs)]
    lbd, td = dev(lb), dev(tasks)
    blocks, nv = mr.kl_tasks_blocks(rows), 3 + C
    ws = ops.workspace(ops.lib().repo_kl_balance_tasks_workspace_bytes(), device())   # fetched BEFORE the call: it is served from it
    area = ws[:ws.numel() // 4 * 4].view(torch.float32)
    area.fill_(float("nan"))
    (sums, g), names = traced(lambda: ops.kl_balance_tasks(*d, alpha, lbd, td, target, scale))
    assert has(names, K_KL) and has(names, K_KL_SUM), names
    assert written(sums, *g)
    fin = torch.isfinite(area.cpu())
    k = nv * blocks
    assert bool(fin[:k].all()) and not bool(fin[k:].any()), ("finite partials", int(fin.sum()), "expected", k)
    parts = area[:k].cpu().view(nv, blocks).numpy()
    want = torch.from_numpy(np.array([rr.fixed_order_sum(parts[v]) for v in range(nv)], dtype=np.float32))
    assert torch.equal(sums.cpu(), want), ("not the fixed-order sum of its partials", sums.tolist(), want.tolist())
    es, eg = kl_errs(sums, g, ref)
    t32, g32 = mr.kl_tasks(*a, dtype=torch.float32)
    fs, fg = kl_errs(f32_sums(t32), g32, ref)
    log(f"kl_balance_tasks {kl_id(case)}: sums {es:.2e} (float32 statement {fs:.2e}, bound {bound('kl_sums'):.1e}); "
        f"gradients {eg:.2e} (float32 statement {fg:.2e}, bound {bound('kl_grads'):.1e})")
    assert es <= bound("kl_sums") and eg <= bound("kl_grads"), (case, es, eg)
    if not real and C > 1:
        assert sums[3 + C - 1].item() == 0.0      # the absent task
    area.fill_(float("nan"))
    sums2, none = ops.kl_balance_tasks(*d, alpha, lbd, td, target, scale, want_grads=False)
    assert none is None and same_bits(sums2, sums)
    assert int(torch.isfinite(area).sum()) == k
    for got, keep in zip(d + [lbd, td], (pm, ps, qm, qs, lb, tasks)):
        assert same_bits(got, dev(keep))


# ------------------------------------------------------------------------------------------------------ dual_step_tasks
@pytest.mark.parametrize("C", DUAL_CS)
def test_dual_step_tasks_five_steps_with_carried_moments(ops, C):
    lb0, sums = dual_inputs(C)
    ref = dual_run(C, torch.float64)
    lo = dual_run(C, torch.float32)
    lb, m, v = dev(lb0), torch.zeros(C, device="cuda"), torch.zeros(C, device="cuda")
    zero = 1 if C > 1 else None
    beta_bits = None
    for k in range(DUAL_STEPS):
        sd = dev(sums[k])
        out, names = traced(lambda: ops.dual_step_tasks(lb, m, v, sd, DUAL_ROWS, DUAL_LR, BETAS, 1e-8, k + 1))
        assert has(names, K_DUAL), names
        assert written(out)
        want_lb, want_m, want_v, want_sc = ref[k]
        e = (lb.double().cpu() - want_lb).abs()
        bnd = (k + 1) * (U * want_lb.abs() + 2.0 ** -18 * DUAL_LR)
        es, fs = scalar_err(out, want_sc), scalar_err(lo[k][3], want_sc)
        log(f"dual_step_tasks C={C} step {k + 1}: largest |log_beta - ref| / bound {float((e / bnd).max()):.3f}; scalars {es:.2e} "
            f"(float32 statement {fs:.2e}, bound {bound('dual_scalars'):.1e})")
        assert bool((e <= bnd).all()), (C, k, e.tolist(), bnd.tolist())
        assert es <= bound("dual_scalars"), (C, k, es)
        if zero is not None:      # a task without a row in the batch: its variable never moves, and its beta stays exp of it
            assert same_bits(lb[zero], dev(lb0)[zero]) and m[zero].item() == 0.0 and v[zero].item() == 0.0
            beta_bits = out[3 + zero].clone() if beta_bits is None else beta_bits
            assert same_bits(out[3 + zero], beta_bits)
    assert relerr(m, ref[-1][1]) < FTOL and relerr(v, ref[-1][2]) < FTOL
    # apply = 0 and a non-zero skip word: the scalars are written, the variable and its moments are not
    sd = dev(sums[2])
    want_sc = mr.dual_step_tasks(lb.cpu(), m.cpu(), v.cpu(), sums[2], DUAL_ROWS, DUAL_LR, BETAS[0], BETAS[1], 1e-8, 6, apply=False)[3]
    for kw in (dict(apply=False), dict(skip=torch.full((1,), 2, dtype=torch.int32, device="cuda"))):
        keep = [lb.clone(), m.clone(), v.clone()]
        out = ops.dual_step_tasks(lb, m, v, sd, DUAL_ROWS, DUAL_LR, BETAS, 1e-8, 6, **kw)
        assert all(same_bits(x, y) for x, y in zip((lb, m, v), keep)), kw
        assert written(out) and scalar_err(out, want_sc) <= bound("dual_scalars"), kw
    # a zero skip word changes nothing against no skip word
    s1, s2 = [lb.clone(), m.clone(), v.clone()], [lb.clone(), m.clone(), v.clone()]
    o1 = ops.dual_step_tasks(*s1, sd, DUAL_ROWS, DUAL_LR, BETAS, 1e-8, 6)
    o2 = ops.dual_step_tasks(*s2, sd, DUAL_ROWS, DUAL_LR, BETAS, 1e-8, 6, skip=torch.zeros(1, dtype=torch.int32, device="cuda"))
    assert same_bits(o1, o2) and all(same_bits(x, y) for x, y in zip(s1, s2))
    moved = [i for i in range(C) if i != zero]
    assert not same_bits(s1[0][moved], lb[moved])


# ------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_write_nothing(ops):
    E_BADARG, E_SHAPE, E_WS = -1, -2, -4       # include/repo_hip.h
    L, st = ops.lib(), torch.cuda.current_stream().cuda_stream
    p = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    filled = lambda *s: torch.full(s, SENT, device="cuda")  # noqa: E731
    i64 = lambda *v: (ctypes.c_int64 * 4)(*v)  # noqa: E731
    rs = np.random.RandomState(5)
    # ---- the three FiLM passes: n = 2, C = 5, a 4 x 4 plane = the stride-2 convolution of (3, 10, 10) with KS = 4
    n, C, P, ld = 2, 5, 16, 34
    src, film = dev(rnd(rs, n, C, 25)), dev(rnd(rs, n, ld))      # (room for the 5 x 5 plane one refused call names)
    out, dfilm = filled(n, C, 25), filled(n, ld)
    x, x8 = dev(rnd(rs, n, 3, 10, 10)), torch.zeros(n, 3, 10, 10, dtype=torch.uint8, device="cuda")
    w, bias = dev(rnd(rs, 5, 3, 4, 4)), dev(rnd(rs, 5))
    word = torch.zeros(1, dtype=torch.int32, device="cuda")
    down = i64(3, 5, 10, 4)

    def fwd(P_=P, ld_=ld, goff=3, boff=20):
        return L.repo_film_fwd(n, C, P_, p(src), p(film), ld_, goff, boff, p(out), st)

    def bwd(P_=P, ld_=ld, goff=3, boff=20):
        return L.repo_film_bwd(n, C, P_, p(src), p(src), p(film), ld_, goff, boff, p(out), p(dfilm), st)

    def bwd_h(P_=P, ld_=ld, goff=3, boff=20, kind=1, geo=down, x_=x, u8=0, wd=word, epoch=7, C_=C):
        return L.repo_film_bwd_h(n, C_, P_, p(src), p(src), p(film), ld_, goff, boff, p(out), p(dfilm), kind, geo, p(x_), u8, p(w),
                                 p(bias), p(wd), epoch, st)

    for call in (fwd, bwd, bwd_h):
        assert call(P_=0) == E_SHAPE
        assert call(goff=ld - C + 1) == E_SHAPE and call(boff=ld - C + 1) == E_SHAPE      # goff + C > ld
        assert call(goff=3, boff=7) == E_SHAPE and call(goff=7, boff=3) == E_SHAPE        # overlapping blocks
        assert call(goff=-1) == E_SHAPE
    assert bwd_h(kind=4) == E_BADARG and bwd_h(kind=-1) == E_BADARG
    assert bwd_h(epoch=0) == E_BADARG                                                   # a word with epoch 0
    assert bwd_h(kind=3, geo=i64(3, 0, 0, 0), x_=x8, u8=1) == E_SHAPE                   # dense with uint8 input
    assert bwd_h(geo=i64(3, 4, 10, 4)) == E_SHAPE                                       # C != CS
    assert bwd_h(geo=i64(3, 5, 12, 4)) == E_SHAPE                                       # P != HS^2
    assert bwd_h(geo=i64(3, 5, 3, 4)) == E_SHAPE                                        # HB < KS
    assert bwd_h(x_=None) == E_BADARG                                                   # no input with a description
    assert bwd_h(kind=2, geo=i64(5, 3, 4, 2), x_=x8, u8=1) == E_SHAPE                   # the transpose with uint8 input
    # the transpose: HB = 2 (HS - 1) + KS.  HB = 5, KS = 2 describes no layer (P = 25 is its plane); HB = 4, KS = 2 does
    assert bwd_h(kind=2, geo=i64(5, 3, 5, 2), P_=25) == E_SHAPE
    torch.cuda.synchronize()
    assert bool((out == SENT).all()) and bool((dfilm == SENT).all()) and int(word.item()) == 0, "a refused call wrote an output"
    assert bwd_h() == 0 and bwd_h(kind=2, geo=i64(5, 3, 4, 2)) == 0 and fwd() == 0 and bwd() == 0     # ... and the valid calls are taken
    torch.cuda.synchronize()
    assert not bool((out.view(-1)[:n * C * P] == SENT).any())
    # ---- repo_film_tables
    tab = filled(n * ld)
    ch = lambda *v: (ctypes.c_int * len(v))(*v)  # noqa: E731
    assert L.repo_film_tables(n, 0, ch(5), p(film), ld, p(tab), st) == E_SHAPE
    assert L.repo_film_tables(n, 5, ch(1, 1, 1, 1, 1), p(film), ld, p(tab), st) == E_SHAPE
    assert L.repo_film_tables(n, 2, ch(5, 0), p(film), ld, p(tab), st) == E_SHAPE
    assert L.repo_film_tables(n, 2, ch(9, 9), p(film), 35, p(tab), st) == E_SHAPE          # ldfilm < 2 * total
    assert L.repo_film_tables(0, 1, ch(5), p(film), ld, p(tab), st) == E_SHAPE
    assert L.repo_film_tables(n, 1, ch(5), None, ld, p(tab), st) == E_BADARG
    # ---- repo_kl_balance_tasks
    rows, S, Ct = 9, 30, 3
    a = [dev(t) if torch.is_tensor(t) else t for t in kl_inputs(rows, S, Ct, False)]
    pm, ps, qm, qs, alpha, lb, tasks, target, scale = a
    g, sums = [filled(rows, S) for _ in range(4)], filled(3 + Ct)
    nb = L.repo_kl_balance_tasks_workspace_bytes()
    assert nb == (3 + mr.MAX_TASKS) * mr.KL_TASKS_CAP * 4
    ws = ops.workspace(nb, device())
    wsf = ws[:nb].view(torch.float32)
    wsf.fill_(SENT)

    def kl(S_=S, C_=Ct, pm_=pm, tasks_=tasks, sums_=sums, nbytes=nb):
        return L.repo_kl_balance_tasks(rows, S_, C_, p(pm_), p(ps), p(qm), p(qs), alpha, p(lb), p(tasks_), target, scale, p(g[0]),
                                       p(g[1]), p(g[2]), p(g[3]), p(sums_), p(ws), nbytes, st)

    assert kl(S_=0) == E_SHAPE and kl(S_=65) == E_SHAPE and kl(C_=0) == E_SHAPE and kl(C_=14) == E_SHAPE
    assert kl(nbytes=nb - 1) == E_WS
    assert kl(pm_=None) == E_BADARG and kl(tasks_=None) == E_BADARG and kl(sums_=None) == E_BADARG
    # ---- repo_dual_step_tasks
    lbv, mv, vv, sc = filled(14), filled(14), filled(14), filled(17)

    def dual(C_=3, step=1, lb_=lbv):
        return L.repo_dual_step_tasks(C_, p(lb_), p(mv), p(vv), p(sums), 100, 1e-2, 0.9, 0.999, 1e-8, step, 1, p(sc), None, st)

    assert dual(step=0) == E_SHAPE and dual(C_=14) == E_SHAPE and dual(C_=0) == E_SHAPE and dual(lb_=None) == E_BADARG
    torch.cuda.synchronize()
    for t in (tab, sums, wsf, lbv, mv, vv, sc, *g):
        assert bool((t == SENT).all()), "a refused call wrote an output"
    assert kl() == 0
    torch.cuda.synchronize()
    assert written(sums, *g) and not bool((sums == SENT).any())
