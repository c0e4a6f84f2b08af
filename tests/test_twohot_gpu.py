"""config.value_dist = "twohot" on the GPU: the three repo_twohot_* kernels against tests/twohot_ref.py's
float64 restatement at every regime of their launch, every width class and both access paths; special returns; the error
codes; the head's dense chain at out_dim = K; whole updates of RePo and Dreamer against OracleTwoHot (tied to
OracleReturnNorm and autograd by tests/test_twohot_cpu.py); the zero initialisation; the configuration in which the key must
change nothing; checkpoints, the families that refuse, and determinism.

Bounds, in units of 2^-24 times a normaliser, 64 units each (a float32 torch evaluation of the same formulas
on the CPU stays under 9 / 9 / 21-33 / 2.6 / 2.4 units in this order; 64 is at least twice the largest and leaves room for
the device's expf / log1pf):
    m                      max|b|
    v                      (|v| + 1) max|b|
    decode-reverse dz      |g| (|v| + 1) max|b|
    loss dz                scale w (1 + pos)
    per-row CE             (1 + pos) |logp_k0 - logp_k0+1| + 1 + |logp_k0| + |logp_k0+1|
the sums are held to the per-row bound summed.  Updates: the project's own -- scalars 1e-3, flat gradients 1e-3, per-tensor
gradients 5e-3."""
import math

import numpy as np
import pytest
import torch

from oracle import fixtures as fx
from tests import pcont_ref as pr
from tests import test_actor_grad_gpu as tag
from tests import test_update_gpu as tu
from tests import twohot_ref as th
from tests.util import has, l2err, log, traced

pytestmark = pytest.mark.gpu

E_BADARG, E_SHAPE, E_WS_TOO_SMALL = -1, -2, -4   # include/repo_hip.h
NEW_KERNELS = ("twohot_decode_kernel", "twohot_decode_bwd_kernel", "twohot_nll_kernel")
UNIT, LIMIT = 2.0 ** -24, 64.0
LOW, HIGH = -20.0, 20.0
SIZES = th.regime_sizes()
ONE_PER_REGIME = [3, 5, th.ROWS_PER_BLOCK * th.LAST_BLOCK_MAX_GRID + 1, th.ROWS_PER_BLOCK * th.MAX_BLOCKS + 1]
WIDTHS = [2, 3, 63, 64, 65, 255, 256, 257, 1024]
GUARD, SENT = 64, -777.0
WORST = {}


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


def _roundup4(K):
    return (K + 3) // 4 * 4


def _pitches(K):
    return [K, _roundup4(K), _roundup4(K) + 4]


class Banded:
    """A (rows, K) view at pitch ld inside a flat buffer filled with `fill`, GUARD + shift floats in front and GUARD behind:
    `intact()` tells whether everything outside the view's rows x K elements still holds the fill."""

    def __init__(self, rows, K, ld, fill, shift=0):
        self.n = (rows - 1) * ld + K
        self.off = GUARD + shift
        self.buf = torch.full((self.off + self.n + GUARD,), fill, dtype=torch.float32, device="cuda")
        self.fill = fill
        self.view = self.buf.as_strided((rows, K), (ld, 1), self.off)
        self.mask = torch.ones_like(self.buf, dtype=torch.bool)
        self.mask.as_strided((rows, K), (ld, 1), self.off).fill_(False)

    def intact(self):
        out = self.buf[self.mask]
        return bool((out == self.fill).all()) if self.fill == self.fill else bool(torch.isnan(out).all())


def _inputs(rows, K, lscale, seed):
    rs = np.random.RandomState(seed)
    z = (rs.standard_normal((rows, K)) * lscale).astype(np.float32)
    R = (rs.standard_normal(rows) * 50.0).astype(np.float32)
    R[::7] *= 1e4
    w = rs.uniform(0.05, 1.0, rows).astype(np.float32)
    g = rs.standard_normal(rows).astype(np.float32)
    return tuple(torch.from_numpy(a) for a in (z, R, w, g))


def _note(name, ratio):
    WORST[name] = max(WORST.get(name, 0.0), float(ratio))
    return float(ratio)


def _kernel_case(ops, rows, K, ld, lscale, weighted, with_gmul, low=LOW, high=HIGH, shift=0, per_row_ce=False):
    """All three kernels on one input against float64; logits and every output sit between guard bands (the logits' of
    NaN: a read outside a row poisons the result; the outputs' of a sentinel that must survive)."""
    z, R, w, g = _inputs(rows, K, lscale, 1000 * K + rows)
    tagc = f"rows={rows} K={K} ld={ld} scale={lscale} w={weighted} gmul={with_gmul} shift={shift} [{low},{high}]"
    zin = Banded(rows, K, ld, float("nan"), shift)
    zin.view.copy_(z)
    z64, R64, w64, g64 = z.double(), R.double(), w.double(), g.double()
    bmax = max(abs(low), abs(high))
    # -- decode
    vout = Banded(rows, 1, 1, SENT)
    v, m = ops.twohot_decode(zin.view, low, high, out=vout.view, want_mean=True)
    v_ref, m_ref, _ = th.decode(z64, low, high)
    assert vout.intact(), tagc
    r_m = _note("m", ((m.cpu().double() - m_ref).abs() / (UNIT * bmax)).max())
    r_v = _note("v", ((v.cpu().double().reshape(-1) - v_ref).abs() / (UNIT * (v_ref.abs() + 1.0) * bmax)).max())
    assert r_m <= LIMIT and r_v <= LIMIT, (tagc, r_m, r_v)
    # -- decode, reverse
    gm = torch.tensor([0.25], device="cuda") if with_gmul else None
    dout = Banded(rows, K, ld, SENT, shift)
    ops.twohot_decode_bwd(zin.view, low, high, g.cuda(), out=dout.view, gmul=gm)
    d_ref = th.decode_bwd(z64, low, high, g64, 0.25 if with_gmul else 1.0)
    norm = UNIT * (g64.abs() * (0.25 if with_gmul else 1.0) * (v_ref.abs() + 1.0) * bmax)[:, None]
    assert dout.intact(), tagc
    r_d = _note("decode_bwd dz", ((dout.view.cpu().double() - d_ref).abs() / norm).max())
    assert r_d <= LIMIT, (tagc, r_d)
    # -- loss
    scale = 1.0 / rows
    wd = w.cuda() if weighted else None
    lout = Banded(rows, K, ld, SENT, shift)
    sums, _ = ops.twohot_nll(zin.view, R.cuda(), wd, low, high, scale, dlogits=lout.view)
    ref = th.nll(z64, R64, w64 if weighted else None, low, high, scale)
    ww = w64 if weighted else torch.ones_like(R64)
    assert lout.intact() and zin.intact(), tagc
    r_l = _note("loss dz", ((lout.view.cpu().double() - ref["dz"]).abs() / (UNIT * scale * ww * (1.0 + ref["pos"]))[:, None]).max())
    assert r_l <= LIMIT, (tagc, r_l)
    hot = ref["hot"]
    row_bound = (1.0 + ref["pos"]) * (hot[:, 0] - hot[:, 1]).abs() + 1.0 + hot[:, 0].abs() + hot[:, 1].abs()
    sh = sums.cpu().double()
    r_s = _note("sum w CE", abs(float(sh[0] - ref["sums"][0])) / float(UNIT * (ww * row_bound).sum()))
    r_w = _note("sum w", abs(float(sh[1] - ref["sums"][1])) / float(UNIT * ww.sum()))
    assert r_s <= LIMIT and r_w <= LIMIT, (tagc, r_s, r_w)
    # the sums do not depend on whether the gradient is asked for
    sums_ng, none = ops.twohot_nll(zin.view, R.cuda(), wd, low, high, scale, want_grad=False)
    assert none is None and torch.equal(_bits(sums_ng), _bits(sums)), tagc
    if per_row_ce:   # a one-hot weight vector reads one row's CE out of the sums
        for r in range(rows):
            e = torch.zeros(rows)
            e[r] = 1.0
            s1, _ = ops.twohot_nll(zin.view, R.cuda(), e.cuda(), low, high, scale, want_grad=False)
            r_c = _note("per-row CE", abs(float(s1[0].cpu().double() - ref["ce"][r])) / float(UNIT * row_bound[r]))
            assert r_c <= LIMIT and float(s1[1]) == 1.0, (tagc, r, r_c)


def _log_worst(where):
    log(f"[twohot {where}] largest ratio to its bound's unit so far: "
        + ", ".join(f"{k} {v:.2f}" for k, v in sorted(WORST.items())) + f" (limit {LIMIT:g})")


# ----------------------------------------------------------------------------- 1. regimes
def test_grid_regimes(ops):
    """One wave per row, ROWS_PER_BLOCK rows per block: below that some waves of the only block hold no row; up to
    LAST_BLOCK_MAX_GRID blocks the launch's last block sums the partials; up to MAX_BLOCKS a follow-up launch does; past
    that the waves loop over rows.  The constants are the library's own."""
    r, g, b = ops.twohot_geometry()
    assert (r, g, b) == (th.ROWS_PER_BLOCK, th.LAST_BLOCK_MAX_GRID, th.MAX_BLOCKS)
    assert {th.regime(n) for n in SIZES} == {"partial-block", "self-finish", "follow-up", "stride"}
    assert {1, 3, 4, 5} <= set(SIZES)
    for edge in (g, b):     # one block below the boundary, the boundary, one row and one block past it
        assert {r * (edge - 1), r * edge, r * edge + 1, r * (edge + 1)} <= set(SIZES)
    assert th.regime(r * g) == "self-finish" and th.regime(r * g + 1) == "follow-up"
    assert th.regime(r * b) == "follow-up" and th.regime(r * b + 1) == "stride"
    assert SIZES[-1] > 2 * r * b and SIZES[-1] % r != 0          # every wave takes three rows, the last trip is ragged
    assert [th.regime(n) for n in ONE_PER_REGIME] == ["partial-block", "self-finish", "follow-up", "stride"]


# ----------------------------------------------------------------------------- 2. the kernels against float64
@pytest.mark.parametrize("K", WIDTHS)
def test_kernels_at_every_width(ops, K):
    """rows = 5 (two blocks, the second with one row): every pitch, logit scale, with and without weights and gmul, and the
    per-row CE; then one size per regime at the rounded-up pitch."""
    for ld in _pitches(K):
        for lscale in (1.0, 5.0, 30.0):
            for weighted, with_gmul in ((False, False), (True, True)):
                _kernel_case(ops, 5, K, ld, lscale, weighted, with_gmul, per_row_ce=(lscale == 5.0 and weighted))
    _kernel_case(ops, 5, K, _roundup4(K), 5.0, True, False)
    _kernel_case(ops, 5, K, _roundup4(K), 5.0, False, True)
    for rows in ONE_PER_REGIME:
        _kernel_case(ops, rows, K, _roundup4(K), 5.0, True, True)
    # a base that is not 16-byte aligned under a pitch that is a multiple of 4: the dword path again
    _kernel_case(ops, 5, K, _roundup4(K), 5.0, True, True, shift=1)
    # narrow bins: most returns clamp to an end bin; and bins that are not symmetric
    _kernel_case(ops, 5, K, _roundup4(K), 5.0, True, False, low=-5.0, high=5.0)
    _kernel_case(ops, 5, K, _roundup4(K), 5.0, True, False, low=-3.0, high=12.0)
    _log_worst(f"K={K}")


@pytest.mark.parametrize("rows", SIZES)
@pytest.mark.parametrize("K", [255, 65])
def test_kernels_at_every_regime(ops, K, rows):
    """K = 255 at ld = 255 leaves every row but the first misaligned; at 256 the 16-byte path runs with a ragged last quad."""
    _kernel_case(ops, rows, K, K, 5.0, True, True)
    _kernel_case(ops, rows, K, _roundup4(K), 5.0, False, False)
    _log_worst(f"K={K} rows={rows}")


def test_two_runs_agree_in_bits(ops):
    rows, K = 4 * 64 + 1, 255
    z, R, w, g = (t.cuda() for t in _inputs(rows, K, 5.0, 3))
    a = ops.twohot_nll(z, R, w, LOW, HIGH, 1.0 / rows)
    b = ops.twohot_nll(z, R, w, LOW, HIGH, 1.0 / rows)
    assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(_bits(a[1]), _bits(b[1]))


# ----------------------------------------------------------------------------- 3. special returns
def test_special_returns(ops):
    K, low, high = 33, -4.0, 4.0          # delta = 0.25: the bins are exact floats, 0 sits on bin 16
    rows = 14
    z, R, w, _ = _inputs(rows, K, 3.0, 77)
    special = {1: float("inf"), 2: float("-inf"), 4: 1e30, 5: -1e30, 7: 0.0, 8: -0.0, 10: float("nan"),
               11: float(np.float32(math.expm1(0.25))), 12: float(-np.float32(math.expm1(1.5)))}
    plain = [r for r in range(rows) if r not in special]
    Rs = R.clone()
    for r, val in special.items():
        Rs[r] = val
    scale = 0.5
    ld = _roundup4(K)
    out_s, out_p = Banded(rows, K, ld, SENT), Banded(rows, K, ld, SENT)
    sums_s, _ = ops.twohot_nll(z.cuda(), Rs.cuda(), w.cuda(), low, high, scale, dlogits=out_s.view)
    sums_p, _ = ops.twohot_nll(z.cuda(), R.cuda(), w.cuda(), low, high, scale, dlogits=out_p.view)
    assert out_s.intact() and out_p.intact(), "something outside the gradient's extents was written"
    ds, dp = out_s.view.cpu(), out_p.view.cpu()
    # the ordinary rows: bit-equal to the run without the special rows
    assert torch.equal(_bits(ds[plain]), _bits(dp[plain]))
    assert torch.isfinite(sums_p).all()
    # the NaN row is NaN, in the gradient and in the CE sum; the weight sum stays finite
    assert torch.isnan(ds[10]).all() and math.isnan(float(sums_s[0])) and float(sums_s[1]) == float(sums_p[1])
    fin = [r for r in range(rows) if r != 10]
    assert torch.isfinite(ds[fin]).all()
    ref = th.nll(z.double(), Rs.double(), w.double(), low, high, scale)
    p = torch.softmax(z.double(), 1)
    unit = UNIT * scale * w.double() * (1.0 + torch.nan_to_num(ref["pos"]))
    err = ((ds.double() - ref["dz"]).abs() / unit[:, None])[fin]
    assert float(err.max()) <= LIMIT, float(err.max())
    # each gradient row sums to 0
    rowsum = (ds.double().sum(1).abs() / unit)[fin]
    log(f"[twohot specials] dz against float64 {float(err.max()):.2f} units, row sums {float(rowsum.max()):.2f} units")
    assert float(rowsum.max()) <= LIMIT
    # the end bins take the whole weight: t = p - dz / (scale w)
    t = p - ds.double() / (scale * w.double())[:, None]
    for r, k in ((1, K - 1), (4, K - 1), (2, 0), (5, 0), (7, 16), (8, 16)):
        hot = torch.zeros(K, dtype=torch.float64)
        hot[k] = 1.0
        assert float((t[r] - hot).abs().max()) <= 1e-5, (r, k)
    # the same rows without a gradient, and a NaN through the weights-free path
    s_ng, _ = ops.twohot_nll(z.cuda(), Rs.cuda(), None, low, high, scale, want_grad=False)
    assert math.isnan(float(s_ng[0])) and float(s_ng[1]) == rows


# ----------------------------------------------------------------------------- 4. error codes
def test_error_codes(ops):
    from repo_amd._lib import lib

    rows, K = 8, 16
    z, d = torch.zeros(rows, K, device="cuda"), torch.zeros(rows, K, device="cuda")
    v, R, g = (torch.zeros(rows, device="cuda") for _ in range(3))
    sums = torch.zeros(2, device="cuda")
    ws = ops.reduce_ws(z.device)
    s = torch.cuda.current_stream().cuda_stream
    need = lib().repo_reduce_workspace_bytes()
    P = lambda t: t.data_ptr()   # noqa: E731
    dec, bwd, nll = lib().repo_twohot_decode, lib().repo_twohot_decode_bwd, lib().repo_twohot_nll

    def c_dec(rows=rows, K=K, z=P(z), ld=K, low=LOW, high=HIGH, v=P(v)):
        return dec(rows, K, z, ld, low, high, v, None, s)

    def c_bwd(rows=rows, K=K, z=P(z), ld=K, low=LOW, high=HIGH, g=P(g), d=P(d), ldd=K):
        return bwd(rows, K, z, ld, low, high, g, d, ldd, None, s)

    def c_nll(rows=rows, K=K, z=P(z), ld=K, R=P(R), low=LOW, high=HIGH, d=P(d), ldd=K, sums=P(sums), ws_=P(ws), nb=ws.numel()):
        return nll(rows, K, z, ld, R, None, low, high, 1.0, d, ldd, sums, ws_, nb, s)

    for call in (c_dec, c_bwd, c_nll):
        assert call() == 0
        assert call(K=1) == E_SHAPE and call(K=1025) == E_SHAPE and call(ld=K - 1) == E_SHAPE
        assert call(rows=0) == E_SHAPE and call(rows=2 ** 31) == E_SHAPE
        assert call(low=5.0, high=5.0) == E_BADARG and call(low=6.0, high=-6.0) == E_BADARG
        assert call(low=float("nan")) == E_BADARG and call(high=float("inf")) == E_BADARG and call(z=None) == E_BADARG
    assert c_dec(v=None) == E_BADARG
    assert c_bwd(g=None) == E_BADARG and c_bwd(d=None) == E_BADARG and c_bwd(ldd=K - 1) == E_SHAPE
    assert c_nll(R=None) == E_BADARG and c_nll(sums=None) == E_BADARG and c_nll(ldd=K - 1) == E_SHAPE
    assert c_nll(d=None, ldd=0) == 0                       # no gradient asked for: its pitch is not read
    assert c_nll(nb=need - 1) == E_WS_TOO_SMALL and c_nll(ws_=None) == E_WS_TOO_SMALL
    geo = lib().repo_twohot_geometry
    assert geo(None, None, None) == E_BADARG
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- 5. the head's dense chain at out_dim = K
@pytest.mark.parametrize("rows", [5, 300])
@pytest.mark.parametrize("K", [255, 64])
def test_mlp_chain_at_the_heads_width(ops, K, rows):
    """in = 230, hidden = 200, three hidden layers, K outputs at the rounded-up pitch, against torch."""
    rs = np.random.RandomState(K + rows)
    head = th.make_twohot_value_params(K, seed=K)
    params = [torch.from_numpy(v) for v in head.values()]
    x = torch.from_numpy(rs.standard_normal((rows, 230)).astype(np.float32))
    dout = torch.from_numpy(rs.standard_normal((rows, K)).astype(np.float32))
    leaf = [q.clone().requires_grad_(True) for q in params]
    xl = x.clone().requires_grad_(True)
    h = xl
    for i in range(3):
        h = torch.nn.functional.elu(torch.nn.functional.linear(h, leaf[2 * i], leaf[2 * i + 1]))
    want = torch.nn.functional.linear(h, leaf[6], leaf[7])
    want.backward(dout)
    dev = [q.cuda() for q in params]
    z = ops.twohot_rows(rows, K, torch.device("cuda"))
    _, hid = ops.mlp_fwd(dev, x.cuda(), out=z)
    e_out = l2err(z, want)
    dz = ops.twohot_rows(rows, K, torch.device("cuda"))
    dz.copy_(dout)
    grads = [torch.zeros_like(q) for q in dev]
    dx = torch.empty(rows, 230, device="cuda")
    ops.mlp_bwd(dev, x.cuda(), hid, dz, dparams=grads, dx=dx)
    e_dx = l2err(dx, xl.grad)
    e_w = [l2err(gq, q.grad) for gq, q in zip(grads, leaf)]
    log(f"[twohot mlp K={K} rows={rows}] out {e_out:.2e} dx {e_dx:.2e} worst dparam {max(e_w):.2e}")
    assert e_out < 1e-3 and e_dx < 1e-3 and max(e_w) < 5e-3
    # the weight-gradient-only form of the critic's chain
    grads2 = [torch.zeros_like(q) for q in dev]
    ops.mlp_bwd(dev, x.cuda(), hid, dz, dparams=grads2, dx=None)
    assert max(l2err(gq, q.grad) for gq, q in zip(grads2, leaf)) < 5e-3


# ----------------------------------------------------------------------------- 6. whole updates against the oracle
def _twohot_agent(algo, L, B, H, A, K, low=-5.0, high=5.0, seed=7, head_seed=th.TWOHOT_SEED, **over):
    from tests import test_slow_value_gpu as tsv

    agent, cfg = tu.make_agent(algo, L, B, H, A, seed=seed, value_dist="twohot", value_bins=K, value_bin_low=low,
                               value_bin_high=high, **over)
    assert agent._twohot and agent._value_bins == K and tuple(agent.value_model.fc4.weight.shape) == (K, cfg.hidden_size)
    agent._load_module(agent.value_model, tsv.torch_sd(th.make_twohot_value_params(K, seed=head_seed)))
    return agent, cfg


@pytest.mark.parametrize("algo,K", [("repo", 31), ("dreamer", 31), ("repo", 255)])
def test_update_matches_oracle(algo, K):
    L, B, H, A = 10, 5, 6, 6
    agent, cfg = _twohot_agent(algo, L, B, H, A, K)
    oracle = th.OracleTwoHot(cfg, A, params=th.twohot_params(A, K))
    assert oracle.th_on and (oracle.th_K, oracle.th_low, oracle.th_high) == (K, -5.0, 5.0)
    for u in range(2):
        batch, host = tu.dev_batch(L, B, A, 60 + u, u8=(u == 0))
        agent.noise_source, nz = tu.dev_noise(L, B, H, A, 160 + u)
        with tu.grad_snapshots(agent) as snap:
            beliefs, post = agent.train_dynamics(batch[0], batch[1], batch[2], 1.0 - batch[3])
            agent.train_actor_critic(beliefs.flatten(0, 1), post.flatten(0, 1))
        _, _, oscal = oracle.update(*host, nz)
        vals = oracle.last["values"]
        log(f"[oracle twohot {algo} K={K}] update {u}: decoded values in [{float(vals.min()):.4g}, {float(vals.max()):.4g}]")
        assert float(vals.abs().max()) > 0.05, "a head whose decoded values are not all ~0"
        tag.check_against_oracle(agent, oracle, oscal, snap, ("model", "actor", "value"),
                                 f"[oracle twohot {algo} K={K}] update {u}")
        assert not agent.logger.nonfinite
        torch.cuda.synchronize()
        with torch.no_grad():   # the oracle takes the agent's parameters: the second update is compared at the same point
            for m in fx.MODULES:
                for k, v in getattr(agent, m).state_dict().items():
                    oracle.p[m][k].copy_(v.cpu())
            if algo == "repo":
                oracle.log_beta.copy_(agent.log_beta.cpu().reshape(oracle.log_beta.shape))


# ----------------------------------------------------------------------------- 7. combined with 6k - 6n
COMBINED = dict(pcont=True, slow_value_target=True, slow_value_update=2, slow_value_fraction=0.5, return_norm=True,
                return_norm_decay=0.5, return_norm_limit=1e-3)


def test_with_pcont_slow_target_both_and_return_norm():
    """pcont, a slow target from another seed, "both" at mix 0.1 and return_norm: the actor-critic half against
    OracleTwoHotSlowPcont from the agent's own latents and post-model-step parameters, over two steps."""
    from tests import test_slow_value_gpu as tsv

    L, B, H, A, K = 10, 5, 6, 6, 31
    agent, cfg = _twohot_agent("repo", L, B, H, A, K, actor_grad="both", actor_grad_mix=0.1, **COMBINED)
    head = pr.make_pcont_params(cfg.belief_size, cfg.state_size, cfg.hidden_size)
    agent._load_module(agent.pcont_model, tsv.torch_sd(head))
    slow = th.make_twohot_value_params(K, seed=th.TWOHOT_SLOW_SEED)
    tsv.load_target(agent, slow)
    assert tuple(agent.slow_value_model.fc4.weight.shape) == (K, cfg.hidden_size)
    oracle = th.OracleTwoHotSlowPcont(cfg, A, params=th.twohot_params(A, K), pcont_params=head, slow_params=slow)
    assert oracle.mix == 0.1 == agent._actor_mix and oracle.rn_on and oracle.th_on
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
        tag.check_against_oracle(agent, oracle, oscal, snap, ("actor", "value"), f"[twohot combined] update {u}")


def test_reinforce_launches_no_decode_reverse():
    """actor_grad = "reinforce": nothing flows through the returns, so the decode's reverse -- the only source of the value
    head's input-gradient chain -- is not launched; the decode and the loss are."""
    from tests import test_slow_value_gpu as tsv

    L, B, H, A = 8, 4, 5, 6
    batch, _ = tu.dev_batch(L, B, A, 13)
    noise, _ = tu.dev_noise(L, B, H, A, 103)
    counts = {}
    for name in ("reinforce", "both"):
        agent, _ = _twohot_agent("repo", L, B, H, A, 31, actor_grad=name)
        agent.noise_source = noise

        def three_updates():
            for _ in range(3):
                agent.update(batch)

        _, names = tsv.counted(three_updates)
        counts[name] = names
        assert has(names, "twohot_decode_kernel") and has(names, "twohot_nll_kernel"), names
        assert all(np.isfinite(v) for v in agent.last_scalars.values())
    assert not has(counts["reinforce"], "twohot_decode_bwd_kernel") and has(counts["both"], "twohot_decode_bwd_kernel")


# ----------------------------------------------------------------------------- 8. zero init
def _fresh(algo, A, seed, **over):
    from repo_amd.algorithms.repo import Dreamer, RePo
    from repo_amd.common.utils import set_gpu_mode

    set_gpu_mode(True)
    cfg = fx.default_config(algo=algo, batch_size=4, chunk_size=8, horizon=5, **over)
    torch.manual_seed(seed)
    return (RePo if algo == "repo" else Dreamer)(cfg, tu.Env(A), tu.Env(A), tu.Logger()), cfg


def test_zero_initialisation(ops):
    L, B, H, A = 8, 4, 5, 6
    inv = dict(inv_dynamics=True, inv_dynamics_lr=3e-4, inv_dynamics_hidden_size=64)
    two, cfg = _fresh("repo", A, 11, value_dist="twohot", **inv)
    plain, _ = _fresh("repo", A, 11, **inv)
    assert two._value_bins == 255 and (two._value_low, two._value_high) == (-20.0, 20.0)
    # everything but the value head's last layer is what the same seed gives the scalar agent -- the module constructed
    # BEHIND the value head (inv_dynamics) included
    for mod in fx.MODULES + ("inv_dynamics",):
        for (k, a), (_, b) in zip(getattr(two, mod).state_dict().items(), getattr(plain, mod).state_dict().items()):
            if mod == "value_model" and k.startswith("fc4"):
                assert not a.any() and tuple(a.shape)[0] == 255 and b.any()
            else:
                assert torch.equal(_bits(a), _bits(b)), (mod, k)
    # the decoded values are exactly 0.0
    pv = [q.detach() for q in two.value_model.plist()]
    x = torch.randn(300, cfg.belief_size + cfg.state_size, device="cuda")
    z = ops.twohot_rows(300, 255, x.device)
    ops.mlp_fwd(pv, x, out=z, act=two.value_model.act)
    v, m = ops.twohot_decode(z, -20.0, 20.0, want_mean=True)
    assert not z.any() and torch.equal(_bits(v), torch.zeros(300, 1, dtype=torch.int32)) and not m.any()
    # the first update is finite and moves the last layer
    batch, _ = tu.dev_batch(L, B, A, 11)
    two.noise_source, _ = tu.dev_noise(L, B, H, A, 101)
    two.update(batch)
    torch.cuda.synchronize()
    sc = two.last_scalars
    assert all(np.isfinite(s) for s in sc.values()) and not two.logger.nonfinite
    assert abs(sc["train/value_loss"] - math.log(255)) < 0.2      # uniform probabilities: CE = log K, whatever the target
    assert two.value_model.fc4.weight.any() and two.value_model.fc4.bias.any()


# ----------------------------------------------------------------------------- 9. the default path is untouched
def _run_updates(agent, L, B, H, A, n):
    for u in range(n):
        batch, _ = tu.dev_batch(L, B, A, 11 + u)
        agent.noise_source, _ = tu.dev_noise(L, B, H, A, 101 + u)
        agent.update(batch)
    return agent.last_scalars


def test_default_path_is_untouched():
    from tests import test_slow_value_gpu as tsv

    L, B, H, A = 8, 4, 5, 6
    plain, cfg = tu.make_agent("repo", L, B, H, A)
    assert not hasattr(cfg, "value_dist") and not hasattr(cfg, "value_bins")
    named, _ = tu.make_agent("repo", L, B, H, A, value_dist="normal", value_bins=31, value_bin_low=-1.0, value_bin_high=1.0)
    for agent in (plain, named):
        assert agent._value_dist == "normal" and not agent._twohot and agent.value_model.bins is None
        _run_updates(agent, L, B, H, A, 2)
    torch.cuda.synchronize()
    for name in ("model", "actor", "value"):
        a, b = getattr(named, f"{name}_optimizer"), getattr(plain, f"{name}_optimizer")
        assert torch.equal(_bits(a.flat), _bits(b.flat)) and torch.equal(_bits(a.exp_avg), _bits(b.exp_avg)), name
        assert torch.equal(_bits(a.exp_avg_sq), _bits(b.exp_avg_sq)), name
    assert named.last_scalars == plain.last_scalars
    batch, _ = tu.dev_batch(L, B, A, 13)
    noise, _ = tu.dev_noise(L, B, H, A, 103)
    for agent in (plain, named):
        agent.noise_source = noise
        _, names = traced(lambda: agent.update(batch))
        assert has(names, "lambda_return_kernel") and has(names, "scalar_nll_kernel")
        for k in NEW_KERNELS:
            assert not has(names, k), (k, names)
    # ... and the names would show: the two-hot agent launches all three (three updates and fill kernels behind them: a
    # trace can lose the events of its tail, tests/test_slow_value_gpu.py::counted)
    on, _ = _twohot_agent("repo", L, B, H, A, 31)
    on.noise_source = noise

    def three_updates():
        for _ in range(3):
            on.update(batch)

    _, names = tsv.counted(three_updates)
    for k in NEW_KERNELS:
        assert has(names, k), (k, names)


# ----------------------------------------------------------------------------- 10. checkpoints, refusals, determinism
def test_checkpoint_round_trip_and_cross_shape_loads():
    L, B, H, A, K = 8, 4, 5, 6, 31
    agent, _ = _twohot_agent("dreamer", L, B, H, A, K, slow_value_target=True, slow_value_update=1, slow_value_fraction=0.5)
    _run_updates(agent, L, B, H, A, 1)
    torch.cuda.synchronize()
    ck = agent.get_param_dict()
    assert tuple(ck["value_model"]["fc4.weight"].shape) == (K, 200) == tuple(ck["slow_value_model"]["fc4.weight"].shape)
    assert not any("twohot" in k or "value_dist" in k for k in ck), "no new checkpoint keys"
    fresh, _ = _twohot_agent("dreamer", L, B, H, A, K, seed=8, head_seed=3, slow_value_target=True, slow_value_update=1,
                             slow_value_fraction=0.5)
    fresh.load_param_dict(ck)
    for a in (agent, fresh):
        a.noise_source = None     # (the first update ran on injected noise)
        a.seed_noise(5)
        a._noise_counter = 0
    b2, _ = tu.dev_batch(L, B, A, 12)
    for a in (agent, fresh):
        a.update(b2)
    torch.cuda.synchronize()
    for name in ("model", "actor", "value"):
        assert torch.equal(_bits(getattr(agent, f"{name}_optimizer").flat), _bits(getattr(fresh, f"{name}_optimizer").flat))
    assert torch.equal(_bits(agent._slow_value_flat), _bits(fresh._slow_value_flat))
    assert agent.last_scalars == fresh.last_scalars
    # the other head's shapes: a ValueError that names the key, in both directions, and for another bin count
    scalar, _ = tu.make_agent("dreamer", L, B, H, A, slow_value_target=True)
    before = scalar.value_model.fc4.weight.detach().clone()
    with pytest.raises(ValueError, match="value_dist"):
        scalar.load_param_dict(ck)
    assert torch.equal(scalar.value_model.fc4.weight.detach(), before) and scalar.step == 0
    with pytest.raises(ValueError, match="value_dist"):
        fresh.load_param_dict(scalar.get_param_dict())
    other, _ = _twohot_agent("dreamer", L, B, H, A, 63, slow_value_target=True)
    with pytest.raises(ValueError, match="value_dist"):
        other.load_param_dict(ck)
    mixed = dict(ck, slow_value_model=scalar.get_param_dict()["slow_value_model"])
    with pytest.raises(ValueError, match="slow_value_model"):
        fresh.load_param_dict(mixed)


@pytest.mark.parametrize("family", ["FinetunedRePo", "CalibratedRePo", "TIA", "MultitaskDreamer", "MultitaskRePo"])
def test_other_families_refuse(family):
    from tests import test_pcont_gpu as tp

    build = tp._family_builders()[family]
    with pytest.raises(NotImplementedError, match="value_dist"):
        build(value_dist="twohot")
    agent = build(value_dist="normal")
    assert type(agent).__name__ == family and not agent._twohot


@pytest.mark.parametrize("over", [{"value_dist": "categorical"}, {"value_bins": 1}, {"value_bins": 1025},
                                  {"value_bins": 31.5}, {"value_bin_low": 5.0, "value_bin_high": -5.0},
                                  {"value_bin_high": float("inf")}, {"value_bin_low": float("nan")}])
@pytest.mark.parametrize("algo", ["repo", "dreamer"])
def test_out_of_range_keys_raise(algo, over):
    with pytest.raises(ValueError, match="value_"):
        tu.make_agent(algo, 8, 4, 5, 6, **dict({"value_dist": "twohot"}, **over))


def test_two_seeded_agents_are_bit_equal():
    L, B, H, A = 8, 4, 5, 6
    batches = [tu.dev_batch(L, B, A, 300 + i)[0] for i in range(3)]
    finals = []
    for _ in range(2):
        agent, _cfg = _twohot_agent("dreamer", L, B, H, A, 255, low=-20.0, high=20.0, actor_grad="both")
        agent.seed_noise(99)
        for b in batches:
            agent.update(b, join=False)
        agent.synchronize()
        torch.cuda.synchronize()
        assert all(np.isfinite(v) for v in agent.last_scalars.values())
        finals.append([o.flat.clone() for o in (agent.model_optimizer, agent.actor_optimizer, agent.value_optimizer)]
                      + [torch.tensor([agent.last_scalars[k] for k in ("train/actor_loss", "train/value_loss")])])
    for a, b in zip(*finals):
        assert torch.equal(_bits(a), _bits(b))
