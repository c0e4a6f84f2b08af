"""Every dense weight-gradient engine where its plan sends it, with proof that it ran.

csrc/gemm.hip's wgrad_plan / wgrad_group_plan choose among four engines -- one bf16x6 product (bgemm.h), the transposing
row-range kernel (wgrad_tr.h), the direct row-range kernel (wgrad_direct.h) and split-K on 64 x 64 tiles (vgemm.h) -- and
the last three end in a slab reduce.  The plans are mirrored in Python below; a CPU test holds the expected-engine column
of every case table against the mirror, and every GPU case proves from a device trace that the C side made the same
choice.  References are float64 on the CPU (dY^T X, or autograd of the head / the scan); tolerances are the project's
(TOL relative to the largest element for ops.gemm_wgrad, GTOL normwise per tensor through mlp_bwd and rssm_observe_bwd).
Destinations that are stored start as NaN, destinations that are accumulated into start at a constant, strided ones keep
their guard columns bit for bit, operand pad columns hold NaN, and a second call reproduces the first bit for bit.
"""
import itertools
from collections import namedtuple

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests.test_widths_gpu import BY_ID, W, g64, observe_ref, params64
from tests.util import DENSE_WGRAD_KERNELS, has, l2err, log, relerr, rnd, traced

TOL = 1e-5
GTOL = 1e-4
E = 1024
TR, DIRECT, TILE1, TILEG, BF16, RED1, REDG = DENSE_WGRAD_KERNELS


# ----------------------------------------------------------------------------- the plans, in Python
K_MAX_BUF_ELEMS = 1 << 29
WD_MAX_JOBS, WD_MAX_SPLITS, MAX_GROUP_JOBS = 8, 128, 8
BG_MIN_TILES = 150


def _cdiv(a, b):
    return -(-a // b)


def wgrad_splits(rows, N, K):
    tiles = _cdiv(N, 64) * _cdiv(K + 1, 64)
    return min(max(min(_cdiv(768, tiles), _cdiv(rows, 64)), 1), 1024)


def wgrad_direct_ok(rows, N, K, lddy, ldx):
    return (rows >= 4096 and 192 < N <= 224 and N % 4 == 0 and lddy % 4 == 0 and K >= 1 and K + 1 <= 256
            and rows * lddy < K_MAX_BUF_ELEMS and rows * ldx < K_MAX_BUF_ELEMS)


def wgrad_tr_ok(rows, N, K, lddy, ldx):
    return (rows >= 4096 and 192 < N <= 208 and N % 4 == 0 and lddy % 4 == 0 and K >= 128 and K + 1 <= 240
            and rows * lddy < K_MAX_BUF_ELEMS and rows * ldx < K_MAX_BUF_ELEMS)


def bgemm_ok(M, N, K, a_kc, lda, b_kc, ldb, aligned=True):
    return (M >= 512 and N >= 512 and K >= 128 and _cdiv(M, 128) * _cdiv(N, 128) >= BG_MIN_TILES and lda % 4 == 0
            and ldb % 4 == 0 and aligned and (a_kc or M % 4 == 0) and (b_kc or N % 4 == 0))


def single_engine(M, N, K, lddy, ldx, has_db, bgemm=True, aligned=True):
    """repo_gemm_wgrad: ("bf16", 1) -- dW = dY^T X as dense_plan(1, 0, N, K, M) runs it -- or ("tile", splits)."""
    if not has_db and bgemm and bgemm_ok(N, K, M, False, lddy, False, ldx, aligned):
        return "bf16", 1
    return "tile", wgrad_splits(M, N, K)


GroupPlan = namedtuple("GroupPlan", "plain use_tr dsplits engines")


def group_plan(jobs, bgemm=True):
    """wgrad_group_plan over jobs (rows, N, K, lddy, ldx), each with a bias gradient."""
    n = len(jobs)
    if n == 1 or n > MAX_GROUP_JOBS or any(min(j[:3]) <= 0 for j in jobs):
        return GroupPlan(True, False, 0, [single_engine(*j, True, bgemm)[0] for j in jobs])
    dk = [wgrad_direct_ok(*j) for j in jobs]
    use_tr = bgemm and all(not d or wgrad_tr_ok(*j) for d, j in zip(dk, jobs))
    ndirect = min(sum(dk), WD_MAX_JOBS)
    dsplits = min((128 if use_tr else 256) // ndirect, WD_MAX_SPLITS) if ndirect else 0
    engines, taken = [], 0
    for d in dk:
        rowrange = d and dsplits > 0 and taken < WD_MAX_JOBS
        engines.append(("tr" if use_tr else "direct") if rowrange else "tile")
        taken += rowrange
    return GroupPlan(False, use_tr, dsplits, engines)


def plan_kernels(plan):
    """The weight-gradient kernels a group plan launches."""
    if plan.plain:
        return {BF16} if set(plan.engines) == {"bf16"} else {TILE1, RED1}
    return {{"tr": TR, "direct": DIRECT, "tile": TILEG}[e] for e in plan.engines} | {REDG}


def _blk(k):
    return (k + 15) // 16


def head_fused(in_dim, hidden, out_dim, L):
    return L in (4, 5) and _blk(in_dim) == 15 and _blk(hidden) == 13 and hidden % 4 == 0 and out_dim <= 16


def head_jobs(rows, in_dim, hidden, out_dim, L):
    return [(rows, out_dim if l == L - 1 else hidden, in_dim if l == 0 else hidden, out_dim if l == L - 1 else hidden,
             in_dim if l == 0 else hidden) for l in range(L)]


def head_plan(rows, in_dim, hidden, out_dim, L, bgemm):
    """mlp_bwd: the fused head hands its layers to the group; any other head goes layer by layer through repo_gemm_wgrad."""
    jobs = head_jobs(rows, in_dim, hidden, out_dim, L)
    if head_fused(in_dim, hidden, out_dim, L):
        return group_plan(jobs, bgemm)
    return GroupPlan(True, False, 0, [single_engine(*j, True, bgemm)[0] for j in jobs])


def obs_jobs(R, D, Hd, S, A):
    """csrc/rssm.hip obs_wgrad_jobs."""
    F_, X = D + S, S + A
    return [(R, 2 * S, Hd, 2 * S, Hd), (R, 2 * S, Hd, 2 * S, Hd), (R, Hd, D, Hd, F_), (R, Hd, D, Hd, F_),
            (R, 3 * D, D, 3 * D, D), (R, 3 * D, D, 3 * D, F_), (R, D, X, D, X)]


# ----------------------------------------------------------------------------- the case tables
# Single jobs: (id, M, N, K, bias gradient, lead columns of dY / X inside their wider buffers, both row pitches a
# multiple of 4, expected engine, expected splits).  One 64 x 64 tile -> wgrad_splits = ceil(M / 64): M picks the split
# count and with it the four-chain reduce's tail length (splits % 4).
S = namedtuple("S", "id M N K db lead_y lead_x quad engine splits")
SINGLE = [
    S("one-split", 50, 60, 36, True, 1, 3, False, "tile", 1),
    S("splits-2-k1-64", 100, 64, 63, True, 2, 1, False, "tile", 2),          # K + 1 = 64 and N = 64: exactly one tile
    S("splits-3-k64-n65", 190, 65, 64, True, 3, 2, False, "tile", 3),        # 2 x 2 tiles: the second column tile holds only the bias column
    S("splits-4", 250, 60, 36, True, 4, 4, True, "tile", 4),
    S("splits-5", 317, 64, 64, True, 1, 1, False, "tile", 5),
    S("no-bias-on-tiles", 190, 65, 64, False, 3, 2, False, "tile", 3),
    S("bf16-smallest", 128, 516, 3716, False, 4, 8, True, "bf16", 1),
    S("bf16-shape-odd-lead", 128, 516, 3716, False, 1, 8, True, "tile", 2),  # a misaligned dY keeps the same sizes on tiles
    S("bf16-shape-with-bias", 128, 516, 3716, True, 4, 8, True, "tile", 2),
]
SINGLE_BY_ID = {c.id: c for c in SINGLE}


def _single_ld(c):
    """Row pitches of the wider buffers: a multiple of 4 for `quad` cases, odd otherwise."""
    pitch = lambda lead, cols: (lead + cols + 8) // 4 * 4 if c.quad else (lead + cols + 5) | 1  # noqa: E731
    return pitch(c.lead_y, c.N), pitch(c.lead_x, c.K)


HEADS = list(itertools.product((196, 208), (225, 239, 240), (1, 16), (2, 5)))   # hidden, in_dim, out_dim, layers
HEAD_ROWS = (4095, 4096, 4097)


def head_expected(rows, in_dim, hidden, out_dim, L, bgemm):
    """The expected-engine column of the head cases, written out: below 4096 rows or on a two-layer head everything is
    split-K tiles (in a group if fused); from 4096 rows the four wide layers of the fused head take the transposing
    kernel, except with the bf16x6 engines off or at in_dim = 240 (K + 1 = 241: past its 15 column tiles), where they take
    the direct one.  The out_dim-row layer always stays on tiles."""
    if L == 2:
        return {TILE1, RED1}
    if rows < 4096:
        return {TILEG, REDG}
    return {TR if bgemm and in_dim < 240 else DIRECT, TILEG, REDG}


# the observe scan's width rows (tests/test_widths_gpu.py) at T x B = 8 x 515 = 4120 rows, and the widest N the direct
# kernel takes; expected row-range kernel of jobs 2, 3 and 6 (None: no job of the group passes wgrad_direct_ok)
OBS_T, OBS_B = 8, 515
OBS_WIDTHS = dict(BY_ID)
OBS_WIDTHS["n-224"] = W("n-224", 224, 224, 32, 6, "row", "per-step", "per-step", False, False)
OBS_CASES = [("default", DIRECT, 3), ("widest-pad", DIRECT, 3), ("hidden-ne-belief", DIRECT, 3), ("belief-not-quad", TR, 2),
             ("max-width", None, 0), ("n-224", DIRECT, 3)]


def test_case_tables_match_the_plan_mirror():
    """CPU-side: every expected engine / split count of the tables above is what the mirrored plans select, and the
    bf16x6 case is the smallest shape they send there."""
    for c in SINGLE:
        ldy, ldx = _single_ld(c)
        aligned = c.lead_y % 4 == 0 and c.lead_x % 4 == 0
        assert single_engine(c.M, c.N, c.K, ldy, ldx, c.db, True, aligned) == (c.engine, c.splits), c.id
        assert ldy != c.N and ldx != c.K and (ldy % 4 == 0 and ldx % 4 == 0) == c.quad, c.id
    assert sorted({c.splits % 4 for c in SINGLE if c.engine == "tile" and c.splits > 1}) == [0, 1, 2, 3]
    # the smallest bf16x6 product: the fewest rows, and the fewest outputs N x K among the tile grids that reach 150
    # (an output extent of t tiles is at least 128 (t - 1) + 4: a multiple of 4 past the last full tile, and >= 512)
    ext = lambda t: max(128 * (t - 1) + 4, 512)  # noqa: E731
    best = min(((ext(a) * ext(b), ext(a), ext(b)) for a in range(1, 160) for b in range(1, 160) if a * b >= BG_MIN_TILES))
    c = SINGLE_BY_ID["bf16-smallest"]
    assert (c.N, c.K) in {(best[1], best[2]), (best[2], best[1])} and c.M == 128
    for M, N, K in ((c.M - 1, c.N, c.K), (c.M, c.N - 4, c.K), (c.M, c.N, c.K - 4), (c.M, c.N + 1, c.K)):
        assert single_engine(M, N, K, N + 4 & ~3, K + 4 & ~3, False)[0] == "tile", (M, N, K)
    assert single_engine(c.M, c.N, c.K, 528, 3728, False, bgemm=False)[0] == "tile"
    # heads
    for (hidden, in_dim, out_dim, L), rows, bgemm in itertools.product(HEADS, HEAD_ROWS, (True, False)):
        plan = head_plan(rows, in_dim, hidden, out_dim, L, bgemm)
        assert plan_kernels(plan) == head_expected(rows, in_dim, hidden, out_dim, L, bgemm), (hidden, in_dim, out_dim, L, rows, bgemm)
        if L == 5 and rows >= 4096:
            assert plan.engines[:4] == ["tr" if bgemm and in_dim < 240 else "direct"] * 4 and plan.engines[4] == "tile"
            assert plan.dsplits == (32 if plan.use_tr else 64)
    assert head_fused(240, 208, 16, 5) and head_fused(225, 196, 1, 4) and not head_fused(240, 208, 16, 6)
    assert not head_fused(240, 208, 16, 2)   # 4 and 5 layers are all the fused head is instantiated for
    # the scan's group
    for wid, kernel, ndirect in OBS_CASES:
        w = OBS_WIDTHS[wid]
        plan = group_plan(obs_jobs(OBS_T * OBS_B, w.D, w.Hd, w.S, w.A))
        want = {TILEG, REDG} | ({kernel} if kernel else set())
        assert plan_kernels(plan) == want, wid
        rowrange = [i for i, e in enumerate(plan.engines) if e != "tile"]
        assert rowrange == ([2, 3, 6] if ndirect == 3 else [2, 3] if ndirect == 2 else []), (wid, plan)
        assert plan.dsplits == ((128 if plan.use_tr else 256) // ndirect if ndirect else 0)
    # 2450 rows, the largest any other test gives the scan, stays on tiles; 4096 is the first row count that does not
    assert set(group_plan(obs_jobs(2450, 200, 200, 30, 6)).engines) == {"tile"}
    assert set(group_plan(obs_jobs(4095, 200, 200, 30, 6)).engines) == {"tile"}
    assert group_plan(obs_jobs(4096, 200, 200, 30, 6)).engines.count("direct") == 3
    # the embedding's share of fc_embed_belief_posterior runs alone, without a bias column, and stays on tiles
    assert single_engine(OBS_T * OBS_B, 224, E, 224, E, False)[0] == "tile"
    # the edges of the two predicates
    assert wgrad_direct_ok(4096, 224, 255, 224, 255) and not wgrad_direct_ok(4096, 228, 200, 228, 200)
    assert not wgrad_direct_ok(4096, 192, 200, 192, 200) and not wgrad_direct_ok(4096, 200, 256, 200, 256)
    assert wgrad_tr_ok(4096, 208, 239, 208, 239) and not wgrad_tr_ok(4096, 208, 240, 208, 240)
    assert not wgrad_tr_ok(4096, 212, 200, 212, 200) and not wgrad_tr_ok(4096, 200, 127, 200, 127)
    assert wgrad_splits(2450, 200, 230) == 39 and wgrad_splits(50, 60, 200) == 1 and wgrad_splits(10 ** 6, 1, 1) == 768


# ----------------------------------------------------------------------------- GPU fixtures and helpers
@pytest.fixture(autouse=True)
def _poison_lds(request):
    """Start every GPU test from NaN-filled LDS on all CUs: reads of never-written LDS cannot hide."""
    if "gpu" in request.keywords:
        from repo_amd._lib import lib

        assert lib().repo_debug_poison_lds(torch.cuda.current_stream().cuda_stream) == 0
    yield


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from repo_amd import ops as o

    return o


@pytest.fixture
def bgemm():
    """Set repo_debug_bgemm for the test; restored after it."""
    from repo_amd._lib import lib

    prev = lib().repo_debug_bgemm(1)
    lib().repo_debug_bgemm(prev)
    yield lambda on: lib().repo_debug_bgemm(int(on))
    lib().repo_debug_bgemm(prev)


def dev(t):
    return t.detach().float().cuda().contiguous()


def assert_wgrad_kernels(names, expected, what, ignore=()):
    """Of the weight-gradient kernels, exactly `expected` ran (`ignore`: kernels that other products of the same call may
    launch too)."""
    ran = {k for k in DENSE_WGRAD_KERNELS if has(names, k)}
    assert ran - set(ignore) == set(expected) - set(ignore), (what, sorted(ran), sorted(expected), names)
    log(f"{what}: weight-gradient kernels " + " + ".join(sorted(k.replace("\\b", "").replace("[^,]*", "") for k in expected)))


def bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def sliced(t, lead, ld, fill=float("nan")):
    """t as columns [lead, lead + cols) of a device buffer of row pitch ld whose other columns hold `fill`."""
    wide = torch.full((max(t.shape[0], 1), ld), fill)
    wide[: t.shape[0], lead : lead + t.shape[1]] = t
    return wide.cuda()[: t.shape[0], lead : lead + t.shape[1]]


class CarvedWorkspace:
    """Stands in for ops.workspace: every request gets EXACTLY its bytes, 256-byte aligned, out of a buffer of its own
    that is otherwise filled with a pattern; intact() checks the pattern around every request."""
    GUARD, PATTERN = 1 << 20, 0xA5

    def __init__(self):
        self.given = []

    def __call__(self, nbytes, device):
        nbytes = int(nbytes)
        buf = torch.empty(2 * self.GUARD + (nbytes + 255) // 256 * 256, dtype=torch.uint8, device=device)
        buf.fill_(self.PATTERN)
        assert buf.data_ptr() % 256 == 0
        self.given.append((buf, nbytes))
        return buf[self.GUARD : self.GUARD + nbytes]

    def intact(self):
        torch.cuda.synchronize()
        assert self.given and all(nb > 0 for _, nb in self.given), [nb for _, nb in self.given]
        return all(bool((buf[: self.GUARD] == self.PATTERN).all()) and bool((buf[self.GUARD + nb :] == self.PATTERN).all())
                   for buf, nb in self.given)


# ----------------------------------------------------------------------------- one job: ops.gemm_wgrad
_SINGLE_REF = {}


def _single_operands(c):
    if c.id not in _SINGLE_REF:
        rs = np.random.RandomState(c.M + 3 * c.N + 7 * c.K)
        dY, X = rnd(rs, c.M, c.N), rnd(rs, c.M, c.K)
        _SINGLE_REF[c.id] = (dY, X, dY.double().t() @ X.double(), dY.double().sum(0))
    return _SINGLE_REF[c.id]


def _run_single(ops, c, accumulate, trace=True):
    """One ops.gemm_wgrad into the middle columns of a wider dW: returns (dW view, its whole buffer, db, kernel names)."""
    dY, X, _, _ = _single_operands(c)
    ldy, ldx = _single_ld(c)
    fill = 2.0 if accumulate else float("nan")
    wide = torch.full((c.N, c.K + 11), fill).cuda()
    db = torch.full((c.N,), 3.0 if accumulate else float("nan")).cuda() if c.db else None
    dYd, Xd = sliced(dY, c.lead_y, ldy), sliced(X, c.lead_x, ldx)
    call = lambda: ops.gemm_wgrad(dYd, Xd, dW=wide[:, 4 : 4 + c.K], db=db, accumulate=accumulate, want_bias=c.db)  # noqa: E731
    if trace:
        _, names = traced(call)
    else:
        call()
        names = None
    return wide[:, 4 : 4 + c.K], wide, db, names


@pytest.mark.gpu
@pytest.mark.parametrize("cid", [c.id for c in SINGLE])
def test_single_job_engine_and_value(ops, cid):
    """ops.gemm_wgrad at the smallest shapes that reach one split, each tail length of the reduce's four chains, a
    product of exactly one tile, a bias-only column tile, N = 64 / 65, no bias gradient, and the bf16x6 product (and the
    same sizes kept off it by a misaligned operand or a bias gradient).  Operands are column slices at lead offsets that
    are no multiple of 4 floats and odd row pitches (the tile engine's loads need 4-byte alignment only), their pad
    columns NaN; dW is a column slice of a wider buffer."""
    c = SINGLE_BY_ID[cid]
    _, _, want, want_b = _single_operands(c)
    expected = {BF16} if c.engine == "bf16" else {TILE1, RED1}
    for accumulate in (False, True):
        what = f"gemm_wgrad {cid} {c.M}x{c.N}x{c.K} accumulate={int(accumulate)}"
        base = 2.0 if accumulate else 0.0
        dW, wide, db, names = _run_single(ops, c, accumulate)
        assert_wgrad_kernels(names, expected, what)
        guard = torch.full((c.N, 4), 2.0 if accumulate else float("nan"))
        assert torch.equal(bits(wide[:, :4]), bits(guard)) and torch.equal(bits(wide[:, 4 + c.K :]), bits(guard.repeat(1, 2)[:, :7])), what
        e1 = relerr(dW, want + base)
        e2 = relerr(db, want_b + 3.0 * accumulate) if c.db else 0.0
        log(f"{what}: dW {e1:.2e} db {e2:.2e}")
        assert e1 < TOL and e2 < TOL, (what, e1, e2)
        dW2, _, db2, _ = _run_single(ops, c, accumulate, trace=False)
        assert torch.equal(dW2, dW) and (not c.db or torch.equal(db2, db)), what


@pytest.mark.gpu
@pytest.mark.parametrize("accumulate", [False, True])
def test_single_job_without_rows(ops, accumulate):
    """repo_gemm_wgrad at M = 0 into a strided dW: zeros where it stores, nothing where it accumulates; the guard columns
    stay as they were."""
    from repo_amd._lib import lib

    N, K, ld = 5, 7, 12
    dY, X = torch.zeros(1, N).cuda(), torch.zeros(1, K).cuda()
    fill = 2.0 if accumulate else float("nan")
    wide, db = torch.full((N, ld), fill).cuda(), torch.full((N,), fill).cuda()
    dW = wide[:, 3 : 3 + K]
    rc = lib().repo_gemm_wgrad(0, N, K, dY.data_ptr(), N, X.data_ptr(), K, dW.data_ptr(), ld, db.data_ptr(), int(accumulate),
                               None, 0, torch.cuda.current_stream().cuda_stream)
    assert rc == 0
    torch.cuda.synchronize()
    want = torch.full((N, ld), fill)
    if not accumulate:
        want[:, 3 : 3 + K] = 0.0
    assert torch.equal(bits(wide), bits(want))
    assert torch.equal(db.cpu(), torch.full((N,), 2.0 if accumulate else 0.0))
    log(f"gemm_wgrad M=0 accumulate={int(accumulate)}: no kernel, dW and db exact")


# ----------------------------------------------------------------------------- groups through mlp_bwd
_HEAD_X = {}


def _head_case(hidden, in_dim, out_dim, L, rows):
    """Parameters (fp32 on the device, float64 leaves), input and upstream gradient of a head, and its float64 gradients."""
    rs = np.random.RandomState(hidden + 3 * in_dim + 7 * out_dim + 11 * L)
    dims = [in_dim] + [hidden] * (L - 1) + [out_dim]
    p32 = []
    for l in range(L):
        p32 += [rnd(rs, dims[l + 1], dims[l], scale=dims[l] ** -0.5), rnd(rs, dims[l + 1], scale=0.1)]
    if in_dim not in _HEAD_X:
        _HEAD_X[in_dim] = rnd(np.random.RandomState(in_dim), max(HEAD_ROWS), in_dim)
    x = _HEAD_X[in_dim][:rows]
    up = rnd(rs, max(HEAD_ROWS), out_dim, scale=0.1)[:rows]
    p64 = [t.double().requires_grad_(True) for t in p32]
    h = x.double()
    for l in range(L):
        h = F.linear(h, p64[2 * l], p64[2 * l + 1])
        if l < L - 1:
            h = F.elu(h)
    grads = torch.autograd.grad((h * up.double()).sum(), p64)
    return [t.cuda() for t in p32], x.cuda(), up.cuda(), grads


def _run_head(ops, p, x, hid, up, accumulate, trace=True):
    dp = [torch.full_like(t, 0.5 if accumulate else float("nan")) for t in p]
    call = lambda: ops.mlp_bwd(p, x, hid, up, dparams=dp, accumulate_w=accumulate, dx=None)  # noqa: E731
    names = traced(call)[1] if trace else call()
    return dp, names


@pytest.mark.gpu
@pytest.mark.parametrize("hidden,in_dim,out_dim,L", HEADS)
def test_head_group_engines_and_values(ops, bgemm, hidden, in_dim, out_dim, L):
    """mlp_bwd's weight gradients at 4095 rows (every job on tiles), 4096 (the first row count of the row-range kernels)
    and 4097 (an odd count: the last row pair is half empty), with the bf16x6 engines on and off, stored and accumulated:
    every parameter gradient against float64 autograd, the kernels that ran against head_expected.  Where the transposing
    kernel ran, its worst error over the tensors it produced may not exceed the fp32 direct kernel's on the same operands
    by more than 25 % (the rule of test_bgemm_matches_fp64_and_the_fp32_engine)."""
    for rows in HEAD_ROWS:
        p, x, up, grads = _head_case(hidden, in_dim, out_dim, L, rows)
        bgemm(1)
        _, hid = ops.mlp_fwd(p, x)
        worst = {}
        for bg, accumulate in itertools.product((1, 0), (False, True)):
            what = f"mlp_bwd hidden={hidden} in={in_dim} out={out_dim} L={L} rows={rows} bgemm={bg} accumulate={int(accumulate)}"
            bgemm(bg)
            dp, names = _run_head(ops, p, x, hid, up, accumulate)
            expected = head_expected(rows, in_dim, hidden, out_dim, L, bool(bg))
            assert_wgrad_kernels(names, expected, what, ignore=(BF16,))
            errs = [l2err(g, w + (0.5 if accumulate else 0.0)) for g, w in zip(dp, grads)]
            log(f"{what}: " + " ".join(f"{'dW' if i % 2 == 0 else 'db'}{i // 2 + 1} {e:.2e}" for i, e in enumerate(errs)))
            for i, e in enumerate(errs):
                assert e < GTOL, (what, i, e)
            dp2, _ = _run_head(ops, p, x, hid, up, accumulate, trace=False)
            assert all(torch.equal(a, b) for a, b in zip(dp, dp2)), what
            if not accumulate:
                worst[bg] = (max(errs[: 2 * (L - 1)]), expected)
        if TR in worst[1][1]:
            assert DIRECT in worst[0][1]
            log(f"mlp_bwd hidden={hidden} in={in_dim} out={out_dim} L={L} rows={rows}: worst row-range error bf16x6 "
                f"{worst[1][0]:.2e} fp32 MFMA {worst[0][0]:.2e}")
            assert worst[1][0] <= 1.25 * worst[0][0] + 1e-9, (rows, worst)


# ----------------------------------------------------------------------------- groups through rssm_observe_bwd
_OBS = {}


def _observe_case(ops, wid):
    """The scan at T x B = 8 x 515 on the row engine: forward on the device once, float64 gradients once."""
    if wid in _OBS:
        return _OBS[wid]
    w = OBS_WIDTHS[wid]
    T, B, D, Sd, A = OBS_T, OBS_B, w.D, w.S, w.A
    rs = np.random.RandomState(len(wid) + D)
    p64, p = params64(w, "transition_model")
    act = torch.from_numpy(rs.uniform(-1, 1, (T, B, A))).float().double()
    non = torch.from_numpy((rs.uniform(size=(T, B, 1)) > 0.2).astype(np.float64))
    emb = g64(rs, T, B, E).clamp_min(0).requires_grad_(True)
    b0, s0 = g64(rs, B, D, scale=0.3).requires_grad_(True), g64(rs, B, Sd).requires_grad_(True)
    e1, e2 = g64(rs, T, B, Sd), g64(rs, T, B, Sd)
    outs, _ = observe_ref(p64, b0, s0, act, emb, non, e1, e2)
    ups = [g64(rs, *o.shape, scale=0.1) for o in outs]
    sum((o * u).sum() for o, u in zip(outs, ups)).backward()
    up = dict(dfeat=dev(torch.cat([ups[0], ups[4]], 2)), dprior_state=dev(ups[1]), dpm=dev(ups[2]), dps=dev(ups[3]),
              dqm=dev(ups[5]), dqs=dev(ups[6]))
    sv = ops.rssm_observe_fwd(p, dev(b0), dev(s0), dev(act), dev(non), dev(emb), dev(e1), dev(e2), 0.1)
    assert not sv.cs
    want = {f"d{k}": v.grad for k, v in p64.items()}
    want.update(dembeds=emb.grad, dprev_belief=b0.grad, dprev_state=s0.grad)
    _OBS[wid] = (w, p, sv, up, want)
    return _OBS[wid]


def _run_observe_bwd(ops, case, accumulate, trace=True):
    w, p, sv, up, _ = case
    dp = [torch.full_like(t, 0.25 if accumulate else float("nan")) for t in p]
    nan = lambda *s: torch.full(s, float("nan")).cuda()  # noqa: E731
    demb, dpb, dps_ = nan(OBS_T, OBS_B, E), nan(OBS_B, w.D), nan(OBS_B, w.S)
    call = lambda: ops.rssm_observe_bwd(p, sv, dp, dembeds=demb, dprev_belief=dpb, dprev_state=dps_, accumulate=accumulate, **up)  # noqa: E731
    names = traced(call)[1] if trace else call()
    return dp + [demb, dpb, dps_], names


@pytest.mark.gpu
@pytest.mark.parametrize("wid,kernel,ndirect", OBS_CASES, ids=[c[0] for c in OBS_CASES])
def test_observe_group_engines_and_values(ops, monkeypatch, wid, kernel, ndirect):
    """rssm_observe_bwd at 4120 rows: jobs 2, 3 and 6 of its group pass wgrad_direct_ok, and job 6 (K = S + A < 128) keeps
    the whole group off the transposing kernel -- three jobs per launch of the direct one, the last with two of its eight
    waves at work, reading X at a row pitch of 36 / 33 / 38 floats; job 3 writes into the (Hd, D + E) weight; jobs 2 and 3
    read beliefs at a row pitch of D + S from one time step into featx.  Every parameter gradient, dembeds, dprev_belief
    and dprev_state against float64 autograd, stored and accumulated."""
    monkeypatch.setenv("REPO_SCAN_CS", "0")
    case = _observe_case(ops, wid)
    want = case[4]
    expected = {TILEG, REDG, TILE1, RED1} | ({kernel} if kernel else set())
    for accumulate in (False, True):
        what = f"observe_bwd {wid} T={OBS_T} B={OBS_B} accumulate={int(accumulate)}"
        got, names = _run_observe_bwd(ops, case, accumulate)
        assert_wgrad_kernels(names, expected, what, ignore=(BF16,))
        errs = {n: l2err(g, t + (0.25 if accumulate and i < 14 else 0.0)) for i, (g, (n, t)) in enumerate(zip(got, want.items()))}
        log(f"{what}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))
        for n, e in errs.items():
            assert e < GTOL, (what, n, e)
        again, _ = _run_observe_bwd(ops, case, accumulate, trace=False)
        assert all(torch.equal(a, b) for a, b in zip(got, again)), what


# ----------------------------------------------------------------------------- workspace bounds
@pytest.mark.gpu
@pytest.mark.parametrize("which", ["single", "head", "observe"])
def test_plans_stay_inside_the_bytes_they_ask_for(ops, monkeypatch, bgemm, which):
    """ops.workspace hands out one growing buffer, so a plan that wrote past repo_*_workspace_bytes would go unseen: here
    each request gets exactly its bytes out of a patterned buffer.  The pattern survives and the results do not change."""
    if which == "single":
        c = SINGLE_BY_ID["splits-5"]
        run = lambda: [t for t in _run_single(ops, c, False, trace=False)[:3]]  # noqa: E731
    elif which == "head":
        p, x, up, _ = _head_case(208, 240, 16, 5, 4097)
        _, hid = ops.mlp_fwd(p, x)
        run = lambda: _run_head(ops, p, x, hid, up, False, trace=False)[0]  # noqa: E731
    else:
        monkeypatch.setenv("REPO_SCAN_CS", "0")
        case = _observe_case(ops, "default")
        run = lambda: _run_observe_bwd(ops, case, False, trace=False)[0]  # noqa: E731
    bgemm(1)
    first = run()
    carved = CarvedWorkspace()
    monkeypatch.setattr(ops, "workspace", carved)
    second = run()
    assert carved.intact(), which
    assert all(torch.equal(bits(a), bits(b)) for a, b in zip(first, second)), which
    log(f"workspace bounds {which}: requests {[nb for _, nb in carved.given]} bytes, pattern intact, results bit-equal")
