"""config.return_norm on the GPU: repo_return_scale's two order statistics held to EQUALITY with a sort of
the same float32 array at every regime of its walk, its running average and scale against float64, the guard, the error
codes, the device-scalar multiplier of the gradients, whole updates of RePo and Dreamer against
tests/return_norm_ref.py's OracleReturnNorm (tied to OracleActorGrad and autograd by tests/test_return_norm_cpu.py), the
configuration in which the key must change nothing, checkpoints, the families that refuse, and determinism.

Bounds.  Order statistics: equality.  State: 3 * 2^-24 * (|d lo| + |(1 - d) lo_b|), three float32 roundings.  scale and
1 / scale: 2 ulp of the values recomputed from the kernel's own state.  Updates: the project's own -- scalars 1e-3, flat
gradients 1e-3, per-tensor gradients 5e-3."""
import math

import numpy as np
import pytest
import torch

from oracle import fixtures as fx
from tests import pcont_ref as pr
from tests import return_norm_ref as rn
from tests import slow_value_ref as sv
from tests import test_actor_grad_gpu as tag
from tests import test_update_gpu as tu
from tests.util import has, log, traced

pytestmark = pytest.mark.gpu

E_BADARG, E_SHAPE, E_WS_TOO_SMALL = -1, -2, -4   # include/repo_hip.h
NEW_KERNELS = ("return_scale_kernel", "return_scale_finish_kernel", "scale_by_kernel",
               r"tanh_normal_reinforce_kernel<\s*true\s*>")
T, P = rn.SEL_THREADS, rn.SEL_PER_TRIP
SIZES = [1, 2, 3, 63, 64, 65, 255, 256, 257, T - 1, T, T + 1, P - 1, P, P + 1, 2 * P + 3]


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


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _ulp(x):
    return float(np.spacing(np.float32(abs(x))))


def _is_inv_of_old_state(v):
    """1 / max(1.0, 3.0 - 0.5) of the guard cases' state, to the 2 ulp asked of the inverse."""
    return abs(float(v) - 0.4) <= 2 * _ulp(0.4)


# ----------------------------------------------------------------------------- 1. regimes
def test_grid_regimes(ops):
    """One workgroup of T threads walks x in trips of P elements.  Below T some threads (below 64: some lanes of the only
    busy wave) hold nothing; from T to P every thread holds 1 .. P / T elements of ONE trip; above P the walk loops, and
    its last trip is partial unless the size is a multiple of P.  The constants are the library's own."""
    assert ops.return_scale_geometry() == (T, P)
    regimes = [rn.regime(n) for n in SIZES]
    assert {"partial-wave", "one-trip", "stride"} == set(regimes)
    for edge in (64, 256, T, P):   # one size on each side of every boundary, and the boundary itself
        assert {edge - 1, edge, edge + 1} <= set(SIZES)
    assert rn.regime(T - 1) == "partial-wave" and rn.regime(T) == "one-trip" == rn.regime(P) and rn.regime(P + 1) == "stride"
    assert SIZES[-1] > 2 * P and SIZES[-1] % P != 0 and SIZES[-1] % T != 0     # three trips, the last one ragged
    assert {1, 2, 3, 255, 256, 257} <= set(SIZES)


# ----------------------------------------------------------------------------- 2. the order statistics: equality
KINDS = ("normal", "equal", "two-values", "ascending", "descending", "last-bit", "specials")


def _input(kind, n):
    rs = np.random.RandomState(n % 9973 + 17 * KINDS.index(kind))
    if kind == "normal":
        x = rs.standard_normal(n)
    elif kind == "equal":
        x = np.full(n, 1.37)
    elif kind == "two-values":
        x = np.where(rs.uniform(size=n) < 0.3, -2.5, 0.75)
    elif kind == "ascending":
        x = np.sort(rs.standard_normal(n))
    elif kind == "descending":
        x = np.sort(rs.standard_normal(n))[::-1].copy()
    elif kind == "last-bit":   # 1.0 and its float32 neighbours: the keys differ in the last digit of the last pass only
        base = np.float32(1.0).view(np.int32)
        return (base + rs.randint(-3, 4, n).astype(np.int32)).view(np.float32)
    else:   # mixed signs with both zeros, denormals and both infinities
        pool = np.array([0.0, -0.0, 1e-45, -1e-45, 1e-40, -1e-40, np.inf, -np.inf, 1.0, -1.0, 3.4e38, -3.4e38, 1e-38,
                         -1e-38], dtype=np.float32)
        x = np.where(rs.uniform(size=n) < 0.5, pool[rs.randint(0, len(pool), n)], rs.standard_normal(n).astype(np.float32))
    return np.asarray(x, dtype=np.float32)


def _rank_cases(n):
    return sorted({(0, n - 1), (n // 3, n // 3), rn.ranks(n, 0.05, 0.95)})


@pytest.mark.parametrize("n", SIZES)
def test_order_statistics_equal_the_sorted_array(ops, n):
    state = torch.zeros(2, device="cuda")
    for kind in KINDS:
        x = torch.from_numpy(_input(kind, n))
        xd = x.cuda()
        srt = torch.sort(x).values
        for k_lo, k_hi in _rank_cases(n):
            a = ops.return_scale(xd, k_lo, k_hi, 0.99, 1.0, state, update_state=False)
            b = ops.return_scale(xd, k_lo, k_hi, 0.99, 1.0, state, update_state=False)
            ah = a.cpu()
            want = (srt[k_lo], srt[k_hi])
            assert bool(ah[0] == want[0]) and bool(ah[1] == want[1]), (kind, n, k_lo, k_hi, ah[:2].tolist(), want)
            assert torch.equal(_bits(a), _bits(b)), (kind, n, "two runs differ")
            assert ah[2] == 1.0 and ah[3] == 1.0          # update_state = 0 on a zero state: the limit
    assert torch.equal(_bits(state), torch.zeros(2, dtype=torch.int32)), "update_state = 0 wrote the state"


def test_the_nominal_size(ops):
    """The flagship update's 14 x 2450 returns, through a 2-D view as the agent passes them."""
    x = torch.from_numpy(_input("normal", 14 * 2450) * 3.0 + 5.0).reshape(14, 2450)
    k_lo, k_hi = rn.ranks(x.numel(), 0.05, 0.95)
    state = torch.zeros(2, device="cuda")
    out = ops.return_scale(x.cuda(), k_lo, k_hi, 0.99, 1.0, state, update_state=False).cpu()
    lo, hi = rn.order_stats(x, k_lo, k_hi)
    assert bool(out[0] == lo) and bool(out[1] == hi)


# ----------------------------------------------------------------------------- 3. the running average, scale and inverse
def _check_epilogue(prior, out, after, d, limit, updated, tag):
    """prior, after: the state's float32 values before and after; out: the four outputs."""
    lo_b, hi_b, scale, inv = (float(v) for v in out)
    if updated:
        want, _, _ = rn.ema_scale(prior, lo_b, hi_b, d, limit)
        for got, w, p, b in zip(after, want, prior, (lo_b, hi_b)):
            bound = 3 * 2.0 ** -24 * (abs(d * p) + abs((1.0 - d) * b))
            log(f"{tag}: state got {got:.9g} float64 {w:.9g} err {abs(got - w):.2e} bound {bound:.2e}")
            assert abs(got - w) <= bound, (tag, got, w, bound)
    else:
        assert tuple(after) == tuple(prior), (tag, after, prior)
    s_want = max(limit, float(after[1]) - float(after[0]))
    assert abs(scale - s_want) <= 2 * _ulp(s_want), (tag, scale, s_want)
    assert abs(inv - 1.0 / s_want) <= 2 * _ulp(1.0 / s_want), (tag, inv, 1.0 / s_want)


def test_ten_chained_steps_from_zero_state(ops):
    n = 257
    d, limit = float(np.float32(0.99)), float(np.float32(1e-3))
    k_lo, k_hi = rn.ranks(n, 0.05, 0.95)
    state = torch.zeros(2, device="cuda")
    skip0 = torch.zeros(1, dtype=torch.int32, device="cuda")
    for step in range(10):
        x = torch.from_numpy(np.random.RandomState(step).standard_normal(n).astype(np.float32) * (1.0 + step) + 0.5 * step)
        prior = tuple(state.cpu().tolist())
        out = ops.return_scale(x.cuda(), k_lo, k_hi, d, limit, state, skip=skip0 if step % 2 else None).cpu()
        lo, hi = rn.order_stats(x, k_lo, k_hi)
        assert bool(out[0] == lo) and bool(out[1] == hi)
        _check_epilogue(prior, out.tolist(), tuple(state.cpu().tolist()), d, limit, True, f"return_scale step {step}")
    assert state[1] - state[0] > limit


def test_decay_zero_and_the_finish_entry(ops):
    """decay 0: the state becomes the batch statistics themselves.  repo_return_scale_finish on the statistics a
    repo_return_scale(update_state = 0) wrote gives the bits the one-call form gives."""
    n = 1025
    x = torch.from_numpy(_input("normal", n)).cuda()
    k_lo, k_hi = rn.ranks(n, 0.05, 0.95)
    st = torch.tensor([0.25, 0.75], device="cuda")
    out = ops.return_scale(x, k_lo, k_hi, 0.0, 1e-3, st)
    assert torch.equal(_bits(st), _bits(out[:2]))
    for d in (0.0, 0.5, float(np.float32(0.99))):
        one, two = torch.tensor([0.25, 0.75], device="cuda"), torch.tensor([0.25, 0.75], device="cuda")
        a = ops.return_scale(x, k_lo, k_hi, d, 1e-3, one)
        b = ops.return_scale(x, k_lo, k_hi, d, 1e-3, two, update_state=False)
        assert torch.equal(_bits(two), _bits(torch.tensor([0.25, 0.75])))
        _check_epilogue((0.25, 0.75), b.cpu().tolist(), (0.25, 0.75), d, 1e-3, False, f"update_state=0 d={d}")
        c = ops.return_scale_finish(b[:2].clone(), d, 1e-3, two)
        assert torch.equal(_bits(a), _bits(c)) and torch.equal(_bits(one), _bits(two)), d


def test_capture_in_a_graph(ops):
    """The select and the in-place scale capture: two replays advance the state as two eager calls do."""
    n = 4097
    x = torch.from_numpy(_input("normal", n)).cuda()
    k_lo, k_hi = rn.ranks(n, 0.05, 0.95)
    eager, st = torch.zeros(2, device="cuda"), torch.zeros(2, device="cuda")
    g0 = torch.from_numpy(_input("normal", 300)).cuda()
    ge, gg = g0.clone(), g0.clone()

    def step(state, grad):
        out = ops.return_scale(x, k_lo, k_hi, 0.5, 1e-3, state)
        ops.scale_by(out[3:4], grad)
        return (out,)

    graph, outs, keep = ops.capture_graph(lambda: step(st, gg))
    st.zero_()      # (the warm-up runs of the capture have stepped both)
    gg.copy_(g0)
    for _ in range(2):
        graph.replay()
        want = step(eager, ge)[0]
    torch.cuda.synchronize()
    assert torch.equal(_bits(outs[0]), _bits(want)) and torch.equal(_bits(st), _bits(eager)) and torch.equal(_bits(gg), _bits(ge))
    assert float(st[1] - st[0]) > 1e-3
    del keep


# ----------------------------------------------------------------------------- 4. the guard
def _guard_case(ops, x, k_lo, k_hi, skip=None):
    st = torch.tensor([0.5, 3.0], device="cuda")
    out = ops.return_scale(x.cuda(), k_lo, k_hi, 0.5, 1.0, st, skip=skip).cpu()
    return out, st.cpu()


def test_guard(ops):
    n = 257
    base = torch.from_numpy(_input("normal", n))
    old = torch.tensor([0.5, 3.0])
    k5, k95 = rn.ranks(n, 0.05, 0.95)
    assert k95 < n - 1
    # a NaN at a selected rank (it sorts last: rank n - 1), and an infinity at one
    for bad, k_lo, k_hi in ((float("nan"), 0, n - 1), (float("inf"), 0, n - 1), (float("-inf"), 0, n - 1)):
        x = base.clone()
        x[100] = bad
        out, st = _guard_case(ops, x, k_lo, k_hi)
        assert torch.equal(_bits(st), _bits(old)), bad
        sel = out[0] if bad == float("-inf") else out[1]
        assert (math.isnan(float(sel)) if bad != bad else float(sel) == bad), (bad, out.tolist())
        _check_epilogue((0.5, 3.0), out.tolist(), (0.5, 3.0), 0.5, 1.0, False, f"guard {bad}")
        assert _is_inv_of_old_state(out[3])
    # a non-zero skip word
    out, st = _guard_case(ops, base, k5, k95, skip=torch.tensor([4], dtype=torch.int32, device="cuda"))
    assert torch.equal(_bits(st), _bits(old)) and _is_inv_of_old_state(out[3])
    lo, hi = rn.order_stats(base, k5, k95)
    assert bool(out[0] == lo) and bool(out[1] == hi)       # the statistics are still reported
    # ... and a zero one updates
    out, st = _guard_case(ops, base, k5, k95, skip=torch.zeros(1, dtype=torch.int32, device="cuda"))
    _check_epilogue((0.5, 3.0), out.tolist(), tuple(st.tolist()), 0.5, 1.0, True, "skip word 0")
    assert not torch.equal(_bits(st), _bits(old))
    # a NaN that no rank selects: it sorts last, above the 95 % rank -- the update is the one of the finite elements' ranks
    x = base.clone()
    x[7] = float("nan")
    out, st = _guard_case(ops, x, k5, k95)
    lo, hi = rn.order_stats(x, k5, k95)
    assert math.isfinite(float(hi)) and bool(out[0] == lo) and bool(out[1] == hi)
    _check_epilogue((0.5, 3.0), out.tolist(), tuple(st.tolist()), 0.5, 1.0, True, "unselected NaN")
    assert not torch.equal(_bits(st), _bits(old)) and torch.isfinite(st).all()


@pytest.mark.parametrize("n", [1, 257, P + 1])
def test_all_nan_terminates_and_leaves_the_state(ops, n):
    x = torch.full((n,), float("nan"))
    x[::2] = -x[::2]      # both sign bits
    k_lo, k_hi = rn.ranks(n, 0.05, 0.95)
    out, st = _guard_case(ops, x, k_lo, k_hi)
    assert torch.isnan(out[:2]).all() and torch.equal(_bits(st), _bits(torch.tensor([0.5, 3.0])))
    assert float(out[2]) == 2.5 and _is_inv_of_old_state(out[3])


# ----------------------------------------------------------------------------- 5. error codes
def test_error_codes(ops):
    from repo_amd._lib import lib

    n = 16
    x, st, out = torch.zeros(n, device="cuda"), torch.zeros(2, device="cuda"), torch.zeros(4, device="cuda")
    ws = ops.reduce_ws(x.device)
    s = torch.cuda.current_stream().cuda_stream
    need = lib().repo_reduce_workspace_bytes()
    call = lib().repo_return_scale
    tail = (0.99, 1.0, st.data_ptr(), out.data_ptr(), 1, None, ws.data_ptr(), ws.numel(), s)
    assert call(0, x.data_ptr(), 0, 0, *tail) == E_SHAPE and call(-1, x.data_ptr(), 0, 0, *tail) == E_SHAPE
    assert call(n, x.data_ptr(), -1, 3, *tail) == E_SHAPE and call(n, x.data_ptr(), 0, n, *tail) == E_SHAPE
    assert call(n, x.data_ptr(), 5, 4, *tail) == E_SHAPE and call(2 ** 31, x.data_ptr(), 0, 1, *tail) == E_SHAPE
    assert call(n, None, 0, n - 1, *tail) == E_BADARG
    assert call(n, x.data_ptr(), 0, n - 1, 0.99, 1.0, None, out.data_ptr(), 1, None, ws.data_ptr(), ws.numel(), s) == E_BADARG
    assert call(n, x.data_ptr(), 0, n - 1, 0.99, 1.0, st.data_ptr(), None, 1, None, ws.data_ptr(), ws.numel(), s) == E_BADARG
    assert call(n, x.data_ptr(), 0, n - 1, 0.99, 1.0, st.data_ptr(), out.data_ptr(), 1, None, ws.data_ptr(), need - 1, s) \
        == E_WS_TOO_SMALL
    assert call(n, x.data_ptr(), 0, n - 1, 0.99, 1.0, st.data_ptr(), out.data_ptr(), 1, None, None, need, s) == E_WS_TOO_SMALL
    assert call(n, x.data_ptr(), 0, n - 1, *tail) == 0 and call(n, x.data_ptr(), 4, 4, *tail) == 0
    fin = lib().repo_return_scale_finish
    for null in range(3):
        ptrs = [out.data_ptr(), st.data_ptr(), out.data_ptr()]
        ptrs[null] = None
        assert fin(ptrs[0], 0.99, 1.0, ptrs[1], ptrs[2], 1, None, s) == E_BADARG
    sc = lib().repo_scale_by
    assert sc(0, x.data_ptr(), None, None, out.data_ptr(), s) == E_SHAPE
    assert sc(2 ** 31, x.data_ptr(), None, None, out.data_ptr(), s) == E_SHAPE
    assert sc(n, None, None, None, out.data_ptr(), s) == E_BADARG and sc(n, x.data_ptr(), None, None, None, s) == E_BADARG
    assert sc(n, x.data_ptr(), None, None, out.data_ptr(), s) == 0
    torch.cuda.synchronize()
    assert torch.equal(_bits(st), torch.zeros(2, dtype=torch.int32))     # x is all zeros: the state stayed zero


# ----------------------------------------------------------------------------- 6. the multiplier
@pytest.mark.parametrize("rows,A", [(5, 6), (2731, 6)])
def test_reinforce_with_a_device_multiplier(ops, rows, A):
    from repo_amd._lib import lib

    mean, std, eps, ret, base, w = (torch.from_numpy(a).cuda() for a in tag._kernel_inputs(rows, A))
    gscale = -0.9 / rows
    sums, dm, ds = ops.tanh_normal_reinforce(mean, std, eps, ret, base, w, gscale=gscale)
    # gmul = NULL through the new entry point: the old kernel, the same bits
    dm0, ds0, sums0 = torch.empty_like(dm), torch.empty_like(ds), torch.empty_like(sums)
    ws = ops.reduce_ws(mean.device)
    assert lib().repo_tanh_normal_reinforce_gmul(rows, A, mean.data_ptr(), std.data_ptr(), eps.data_ptr(), 0, 0,
                                                 ret.data_ptr(), base.data_ptr(), w.data_ptr(), gscale, None, dm0.data_ptr(),
                                                 ds0.data_ptr(), sums0.data_ptr(), ws.data_ptr(), ws.numel(),
                                                 torch.cuda.current_stream().cuda_stream) == 0
    for a, b in ((dm0, dm), (ds0, ds), (sums0, sums)):
        assert torch.equal(_bits(a), _bits(b))
    # a power of two is exact
    q = torch.tensor([0.25], device="cuda")
    sums4, dm4, ds4 = ops.tanh_normal_reinforce(mean, std, eps, ret, base, w, gscale=gscale, gmul=q)
    assert torch.equal(_bits(sums4), _bits(sums)), "the sums do not depend on the multiplier"
    assert torch.equal(dm4, 0.25 * dm) and torch.equal(ds4, 0.25 * ds) and float(dm.abs().max()) > 0
    one = torch.ones(1, device="cuda")
    _, dm1, ds1 = ops.tanh_normal_reinforce(mean, std, eps, ret, base, w, gscale=gscale, gmul=one)
    assert torch.equal(_bits(dm1), _bits(dm)) and torch.equal(_bits(ds1), _bits(ds))


@pytest.mark.parametrize("N", [7, 300])
def test_scale_by_on_the_returns_gradients(ops, N):
    Hm = 5
    rs = np.random.RandomState(N)
    r, v, c = (torch.from_numpy(rs.standard_normal((Hm, N)).astype(np.float32)).cuda() for _ in range(3))
    q = torch.tensor([0.25], device="cuda")
    _, dr, dv, _ = ops.lambda_return(r, v, 0.99, 0.95, -1.0 / ((Hm - 1) * N))
    want = (0.25 * dr, 0.25 * dv)
    ops.scale_by(q, dr, dv)
    assert torch.equal(dr, want[0]) and torch.equal(dv, want[1]) and float(dr.abs().max()) > 0
    _, _, dr, dv, dc, _ = ops.lambda_return_disc(r, v, c, 0.95, -1.0 / ((Hm - 1) * N), disc_is_logit=True)
    want = (0.25 * dr, 0.25 * dv, 0.25 * dc)
    keep = dv.clone()
    ops.scale_by(q, dr, dv, dc)
    assert all(torch.equal(a, b) for a, b in zip((dr, dv, dc), want)) and float(dc.abs().max()) > 0
    ops.scale_by(torch.ones(1, device="cuda"), dr, dv, dc)
    assert torch.equal(_bits(dv), _bits(0.25 * keep))
    big = torch.from_numpy(rs.standard_normal(1024 * 256 + 5).astype(np.float32)).cuda()   # past the grid: the stride loop
    want = 0.25 * big
    ops.scale_by(q, big)
    assert torch.equal(big, want)


# ----------------------------------------------------------------------------- 7. whole updates against the oracle
ON = {"return_norm": True, "return_norm_decay": 0.5, "return_norm_limit": 1e-3}
NEW_KEYS = ("train/return_scale", "train/return_lo", "train/return_hi")


def _check_scale_is_the_range(oracle, tag_):
    batch, scale, inv = oracle.last["return_norm"]
    lo, hi = oracle.rn_state
    log(f"{tag_} oracle: batch lo/hi {batch[0]:.6g} {batch[1]:.6g} state {lo:.6g} {hi:.6g} scale {scale:.6g} inv {inv:.6g}")
    assert scale == hi - lo > 10 * 1e-3, "the scale is to be the percentile range, not the limit"
    assert abs(inv - 1.0) > 0.5, "a multiplier an agent that ignored the key could not match"


@pytest.mark.parametrize("name,mix", [("dynamics", None), ("reinforce", None), ("both", 0.1)])
@pytest.mark.parametrize("algo", ["repo", "dreamer"])
def test_update_matches_oracle(algo, name, mix):
    L, B, H, A = 10, 5, 6, 6
    over = dict(ON, actor_grad=name)
    if mix is not None:
        over["actor_grad_mix"] = mix
    agent, cfg = tu.make_agent(algo, L, B, H, A, **over)
    oracle = rn.OracleReturnNorm(cfg, A, params=fx.make_params(A, 7))
    assert oracle.rn_on and agent._return_norm and (oracle.rn_decay, oracle.rn_limit) == (0.5, 1e-3)
    for u in range(2):
        batch, host = tu.dev_batch(L, B, A, 60 + u, u8=(u == 0))
        agent.noise_source, nz = tu.dev_noise(L, B, H, A, 160 + u)
        with tu.grad_snapshots(agent) as snap:
            beliefs, post = agent.train_dynamics(batch[0], batch[1], batch[2], 1.0 - batch[3])
            agent.train_actor_critic(beliefs.flatten(0, 1), post.flatten(0, 1))
        prior = oracle.rn_state
        _, _, oscal = oracle.update(*host, nz)
        assert set(NEW_KEYS) <= set(oscal) and (u == 0 or prior != (0.0, 0.0))
        _check_scale_is_the_range(oracle, f"[oracle return_norm {algo} {name}] update {u}")
        tag.check_against_oracle(agent, oracle, oscal, snap, ("model", "actor", "value"),
                                 f"[oracle return_norm {algo} {name}] update {u}")
        st = agent._return_state.cpu().tolist()
        assert st == [agent.last_scalars["train/return_lo"], agent.last_scalars["train/return_hi"]]
        torch.cuda.synchronize()
        with torch.no_grad():   # the oracle takes the agent's parameters: the second update is compared at the same point
            for m in fx.MODULES:
                for k, v in getattr(agent, m).state_dict().items():
                    oracle.p[m][k].copy_(v.cpu())
            if algo == "repo":
                oracle.log_beta.copy_(agent.log_beta.cpu().reshape(oracle.log_beta.shape))


def test_with_pcont_and_slow_value_target():
    """pcont, a slow target from another seed and "both" at mix 0.1: the actor-critic half against
    OracleReturnNormSlowPcont from the agent's own latents and post-model-step parameters, as 6m's combined case does, over
    two steps.  The statistics are of the unweighted returns; the weights stay on the objective."""
    from tests import test_slow_value_gpu as tsv

    L, B, H, A = 10, 5, 6, 6
    agent, cfg = tu.make_agent("repo", L, B, H, A, pcont=True, slow_value_target=True, slow_value_update=2,
                               slow_value_fraction=0.5, actor_grad="both", actor_grad_mix=0.1, **ON)
    head = pr.make_pcont_params(cfg.belief_size, cfg.state_size, cfg.hidden_size)
    agent._load_module(agent.pcont_model, tsv.torch_sd(head))
    slow = sv.make_slow_params(cfg.belief_size, cfg.state_size, cfg.hidden_size)
    tsv.load_target(agent, slow)
    oracle = rn.OracleReturnNormSlowPcont(cfg, A, params=fx.make_params(A, 7), pcont_params=head, slow_params=slow)
    assert oracle.mix == 0.1 == agent._actor_mix and oracle.rn_on
    for u in range(2):
        batch, _ = tu.dev_batch(L, B, A, 60 + u)
        agent.noise_source, nz = tu.dev_noise(L, B, H, A, 160 + u)
        with tu.grad_snapshots(agent) as snap:
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
        wts = oracle.last["weights"]
        assert float(wts.min()) < 0.9 and float(wts[0].min()) == 1.0
        _check_scale_is_the_range(oracle, f"[return_norm combined] update {u}")
        tag.check_against_oracle(agent, oracle, oscal, snap, ("actor", "value"), f"[return_norm combined] update {u}")


# ----------------------------------------------------------------------------- 8. inert when it should be
def _run_updates(agent, L, B, H, A, n):
    for u in range(n):
        batch, _ = tu.dev_batch(L, B, A, 11 + u)
        agent.noise_source, _ = tu.dev_noise(L, B, H, A, 101 + u)
        agent.update(batch)
    return agent.last_scalars


@pytest.mark.parametrize("name", ["dynamics", "both"])
def test_limit_one_on_small_returns_changes_no_bit(name):
    """limit = 1.0 and imagined returns whose 5-95 % range stays below 1 (asserted from the oracle, on the CPU): inv is
    exactly 1.0 and the update -- parameters, Adam moments, every scalar the key-off agent logs -- is the key-off update bit
    for bit.  The multiplications all happen: by 1.0f."""
    L, B, H, A = 8, 4, 5, 6
    off, cfg_off = tu.make_agent("repo", L, B, H, A, actor_grad=name)
    on, cfg = tu.make_agent("repo", L, B, H, A, actor_grad=name, return_norm=True)
    assert on._return_norm and on._rn_limit == 1.0 and not off._return_norm
    oracle = rn.OracleReturnNorm(cfg, A, params=fx.make_params(A, 7))
    for u in range(2):
        _, host = tu.dev_batch(L, B, A, 11 + u)
        _, nz = tu.dev_noise(L, B, H, A, 101 + u)
        oracle.update(*host, nz)
        (lo_b, hi_b), scale, inv = oracle.last["return_norm"]
        assert hi_b - lo_b < 0.5 and (scale, inv) == (1.0, 1.0), (lo_b, hi_b)     # (0.5: far from the float32 agent's doubt)
    for agent in (off, on):
        _run_updates(agent, L, B, H, A, 2)
    torch.cuda.synchronize()
    for opt in ("model", "actor", "value"):
        a, b = getattr(on, f"{opt}_optimizer"), getattr(off, f"{opt}_optimizer")
        assert torch.equal(_bits(a.flat), _bits(b.flat)) and torch.equal(_bits(a.exp_avg), _bits(b.exp_avg)), opt
        assert torch.equal(_bits(a.exp_avg_sq), _bits(b.exp_avg_sq)), opt
    assert set(on.last_scalars) == set(off.last_scalars) | set(NEW_KEYS)
    for k, v in off.last_scalars.items():
        assert on.last_scalars[k] == v, k
    assert on.last_scalars["train/return_scale"] == 1.0
    st = on._return_state.cpu()
    assert 0.0 < float(st[1] - st[0]) < 1.0 and float(st[1]) == on.last_scalars["train/return_hi"]


def test_key_absent_launches_nothing_new():
    from tests import test_slow_value_gpu as tsv

    L, B, H, A = 8, 4, 5, 6
    batch, _ = tu.dev_batch(L, B, A, 13)
    noise, _ = tu.dev_noise(L, B, H, A, 103)
    for over in ({}, {"return_norm": False}, {"actor_grad": "both"}):
        agent, cfg = tu.make_agent("repo", L, B, H, A, **over)
        assert not agent._return_norm and not hasattr(agent, "_return_state")
        agent.noise_source = noise
        _, names = traced(lambda: agent.update(batch))
        assert has(names, "lambda_return_kernel")
        for k in NEW_KERNELS:
            assert not has(names, k), (over, k, names)
        assert not set(NEW_KEYS) & set(agent.last_scalars)
    # ... and the names would show: the switched-on agent launches them.  (Three updates and fill kernels behind them: a
    # trace can lose the events of its tail, tests/test_slow_value_gpu.py::counted.)
    on, _ = tu.make_agent("repo", L, B, H, A, actor_grad="both", return_norm=True)
    on.noise_source = noise

    def three_updates():
        for _ in range(3):
            on.update(batch)

    _, names = tsv.counted(three_updates)
    for k in ("return_scale_kernel", "scale_by_kernel", NEW_KERNELS[3]):
        assert has(names, k), (k, names)
    assert not has(names, "return_scale_finish_kernel")      # the data-parallel path's


# ----------------------------------------------------------------------------- 9. checkpoints, refusals, determinism
def test_checkpoint_round_trip():
    L, B, H, A = 8, 4, 5, 6
    agent, _ = tu.make_agent("dreamer", L, B, H, A, **ON)
    assert torch.equal(_bits(agent._return_state), torch.zeros(2, dtype=torch.int32))
    _run_updates(agent, L, B, H, A, 1)
    torch.cuda.synchronize()
    ck = agent.get_param_dict()
    st = ck["return_norm"]
    assert st.shape == (2,) and st.dtype == torch.float32 and float(st[1] - st[0]) > 0
    assert st.data_ptr() != agent._return_state.data_ptr()
    fresh, _ = tu.make_agent("dreamer", L, B, H, A, seed=8, **ON)
    fresh.load_param_dict(ck)
    assert torch.equal(_bits(fresh._return_state), _bits(st))
    # an agent without the key writes no entry and reads past one; a checkpoint without the entry leaves the state
    plain, _ = tu.make_agent("dreamer", L, B, H, A)
    assert "return_norm" not in plain.get_param_dict()
    plain.load_param_dict(ck)
    ck.pop("return_norm")
    fresh.load_param_dict(ck)
    assert torch.equal(_bits(fresh._return_state), _bits(st))
    # both continue alike
    for a in (agent, fresh):
        a.noise_source = None     # (the first update ran on injected noise)
        a.seed_noise(5)
        a._noise_counter = 0
    b2, _ = tu.dev_batch(L, B, A, 12)
    for a in (agent, fresh):
        a.update(b2)
    torch.cuda.synchronize()
    assert torch.equal(_bits(agent._return_state), _bits(fresh._return_state))
    assert torch.equal(_bits(agent.actor_optimizer.flat), _bits(fresh.actor_optimizer.flat))


@pytest.mark.parametrize("family", ["FinetunedRePo", "CalibratedRePo", "TIA", "MultitaskDreamer", "MultitaskRePo"])
def test_other_families_refuse(family):
    from tests import test_pcont_gpu as tp

    build = tp._family_builders()[family]
    with pytest.raises(NotImplementedError, match="return_norm"):
        build(return_norm=True)
    agent = build(return_norm=False)
    assert type(agent).__name__ == family and not agent._return_norm


@pytest.mark.parametrize("over", [{"return_norm_decay": 1.0}, {"return_norm_low": 0.95, "return_norm_high": 0.05},
                                  {"return_norm_high": 1.5}, {"return_norm_limit": 0.0},
                                  {"return_norm_limit": float("nan")}])
@pytest.mark.parametrize("algo", ["repo", "dreamer"])
def test_out_of_range_keys_raise(algo, over):
    with pytest.raises(ValueError, match="return_norm"):
        tu.make_agent(algo, 8, 4, 5, 6, return_norm=True, **over)


def test_two_seeded_agents_are_bit_equal():
    L, B, H, A = 8, 4, 5, 6
    batches = [tu.dev_batch(L, B, A, 300 + i)[0] for i in range(3)]
    finals = []
    for _ in range(2):
        agent, _cfg = tu.make_agent("dreamer", L, B, H, A, actor_grad="both", **ON)
        agent.seed_noise(99)
        for b in batches:
            agent.update(b, join=False)
        agent.synchronize()
        torch.cuda.synchronize()
        assert all(np.isfinite(v) for v in agent.last_scalars.values())
        finals.append([o.flat.clone() for o in (agent.model_optimizer, agent.actor_optimizer, agent.value_optimizer)]
                      + [agent._return_state.clone(),
                         torch.tensor([agent.last_scalars[k] for k in NEW_KEYS + ("train/actor_loss",)])])
    for a, b in zip(*finals):
        assert torch.equal(_bits(a), _bits(b))
    assert float(finals[0][3][1] - finals[0][3][0]) > 1e-3
