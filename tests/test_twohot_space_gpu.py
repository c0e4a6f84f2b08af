"""config.value_slow_reg / value_bin_space / reward_bin_space on the GPU: the three repo_twohot_*_x kernels
against tests/twohot_space_ref.py's float64 restatement at every regime of their launch, every width class and both access
paths; the cases that must hold exactly; the error codes; whole updates of RePo and Dreamer against OracleSpace (tied to its
parents and to autograd by tests/test_twohot_space_cpu.py); the configuration in which the keys must change nothing; device
traces, checkpoints, the families that refuse, and determinism.

Bounds of the symexp space, in units of 2^-24 times a normaliser:
    v                      sum_k p_k |B_k|                      (per row)
    decode-reverse dz      |g gmul| sum_k p_k |B_k|             (per row)
    loss dz                scale w ((1 + pos_a) + reg (1 + pos_b))                            (6o's, once per target)
    sum w CE               sum over rows of w ((1 + pos) |logp_k0 - logp_k0+1| + 1 + |logp_k0| + |logp_k0+1|)   (6o's)
    sum w                  sum w
The limit of each is 8 x the worst ratio that the restatement evaluated in float32 on the CPU shows against float64 over the
inputs of the same parametrised case (all its row counts, pitches and offsets): float32 arithmetic alone costs that much, the
device's expf / log1pf / expm1f and its own order of additions get eight times it (DESIGN.md 6q's rule for repo_symlog).  Both
figures are logged per case.  Updates: the project's own -- scalars 1e-3, flat gradients 1e-3, per-tensor gradients 5e-3."""
import math

import numpy as np
import pytest
import torch

from tests import pcont_ref as pr
from tests import test_twohot_gpu as tt
from tests import test_update_gpu as tu
from tests import test_wm_losses_gpu as tw
from tests import twohot_ref as th
from tests import twohot_space_ref as ts
from tests.util import has, log, traced

pytestmark = pytest.mark.gpu

E_BADARG, E_SHAPE, E_WS_TOO_SMALL = -1, -2, -4   # include/repo_hip.h
X_KERNELS = ("twohot_decode_s1_kernel", "twohot_decode_bwd_s1_kernel", r"twohot_nll_kernel<\d, ?(1, ?(false|true|0|1)|0, ?(true|1))>")
UNIT = 2.0 ** -24
LOW, HIGH = -20.0, 20.0
WIDTHS = [2, 3, 31, 64, 65, 255, 256, 1024]
Banded, _bits, _inputs = tt.Banded, tt._bits, tt._inputs
LBHA = tw.LBHA


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


def _row_counts(ops):
    r, g, b = ops.twohot_geometry()
    return sorted({1, 3, r - 1, r, r + 1, g * r, g * r + 1, b * r + 1})


def _variants(K):
    """(ld, base offset in floats): ld = K at an aligned base (the 16-byte path where K is a multiple of 4), ld = K + 1 at a
    base offset by one float (dwords), and the rounded-up pitch where that is neither."""
    out = [(K, 0), (K + 1, 1)]
    r4 = (K + 3) // 4 * 4
    if r4 not in (K, K + 1):
        out.append((r4, 0))
    return out


def _second_target(rows, seed):
    return torch.from_numpy((np.random.RandomState(seed).standard_normal(rows) * 5.0).astype(np.float32))


def _ratios(got, ref, reg, with_gmul, weighted, scale, g, w):
    """The five ratios of `got` (decode v, decode-reverse dz, loss dz, sums3) against the float64 `ref`."""
    gm = 0.25 if with_gmul else 1.0
    ww = w.double() if weighted else torch.ones_like(g.double())
    pB = ref["pB"]
    out = {}
    out["v"] = float(((got["v"].double() - ref["v"]).abs() / (UNIT * pB)).max())
    out["decode_bwd dz"] = float(((got["dv"].double() - ref["dv"]).abs() / (UNIT * g.double().abs() * gm * pB)[:, None]).max())
    n = ref["nll"]
    unit = UNIT * scale * ww * ((1.0 + n["pos"]) + reg * (1.0 + n["pos_b"]))
    out["loss dz"] = float(((got["dz"].double() - n["dz"]).abs() / unit[:, None]).max())
    for name, i, hot, pos in (("sum w CE_a", 0, n["hot"], n["pos"]), ("sum w CE_b", 2, n["hot_b"], n["pos_b"])):
        bound = (1.0 + pos) * (hot[:, 0] - hot[:, 1]).abs() + 1.0 + hot[:, 0].abs() + hot[:, 1].abs()
        out[name] = abs(float(got["sums"][i].double() - n["sums"][i])) / float(UNIT * (ww * bound).sum())
    out["sum w"] = abs(float(got["sums"][1].double() - n["sums"][1])) / float(UNIT * ww.sum())
    return out


def _restate(z, R, Rb, w, g, low, high, reg, with_gmul, weighted, scale, dtype):
    z, R, Rb, w, g = (t.to(dtype) for t in (z, R, Rb, w, g))
    v, _, p = ts.decode(z, low, high, "symexp")
    B = ts.symexp_bins(z.shape[1], low, high, dtype)
    return dict(v=v, pB=(p * B.abs()).sum(1), dv=ts.decode_bwd(z, low, high, g, 0.25 if with_gmul else 1.0, "symexp"),
                nll=ts.nll(z, R, w if weighted else None, low, high, scale, "symexp", target_b=Rb, reg=reg))


def _symexp_case(ops, rows, K, ld, shift, lscale, weighted, with_gmul, reg, low=LOW, high=HIGH):
    """All three kernels in symexp space (the loss with a second target) on one input; logits and every output sit between
    guard bands (the logits' of NaN: a read outside a row poisons the result; the outputs' of a sentinel that must survive).
    -> (the device's ratios, float32-on-the-CPU's ratios)."""
    z, R, w, g = _inputs(rows, K, lscale, 1000 * K + rows)
    Rb = _second_target(rows, 7 * K + rows)
    tagc = f"rows={rows} K={K} ld={ld} shift={shift} scale={lscale} w={weighted} gmul={with_gmul} reg={reg} [{low},{high}]"
    scale = 1.0 / rows
    ref = _restate(z, R, Rb, w, g, low, high, reg, with_gmul, weighted, scale, torch.float64)
    f32 = _restate(z, R, Rb, w, g, low, high, reg, with_gmul, weighted, scale, torch.float32)
    f32 = dict(v=f32["v"], dv=f32["dv"], dz=f32["nll"]["dz"], sums=f32["nll"]["sums"])
    zin = Banded(rows, K, ld, float("nan"), shift)
    zin.view.copy_(z)
    vout = Banded(rows, 1, 1, tt.SENT)
    v, m = ops.twohot_decode(zin.view, low, high, out=vout.view, want_mean=True, space="symexp")
    assert vout.intact() and torch.equal(_bits(v.reshape(-1)), _bits(m)), tagc
    gm = torch.tensor([0.25], device="cuda") if with_gmul else None
    dout = Banded(rows, K, ld, tt.SENT, shift)
    ops.twohot_decode_bwd(zin.view, low, high, g.cuda(), out=dout.view, gmul=gm, space="symexp")
    lout = Banded(rows, K, ld, tt.SENT, shift)
    wd = w.cuda() if weighted else None
    sums, _ = ops.twohot_nll(zin.view, R.cuda(), wd, low, high, scale, dlogits=lout.view, space="symexp",
                             target_b=Rb.cuda(), reg=reg)
    assert dout.intact() and lout.intact() and zin.intact(), tagc
    # the sums do not depend on whether the gradient is asked for
    sums_ng, none = ops.twohot_nll(zin.view, R.cuda(), wd, low, high, scale, want_grad=False, space="symexp",
                                   target_b=Rb.cuda(), reg=reg)
    assert none is None and torch.equal(_bits(sums_ng), _bits(sums)), tagc
    got = dict(v=v.cpu().reshape(-1), dv=dout.view.cpu(), dz=lout.view.cpu(), sums=sums.cpu())
    args = (reg, with_gmul, weighted, scale, g, w)
    return _ratios(got, ref, *args), _ratios(f32, ref, *args), tagc


# ----------------------------------------------------------------------------- 1. the kernels against float64
@pytest.mark.parametrize("K", WIDTHS)
def test_symexp_kernels_at_every_width_and_regime(ops, K):
    rows_all = _row_counts(ops)
    r, g, b = ops.twohot_geometry()
    assert {1, 3, r - 1, r, r + 1, g * r, g * r + 1, b * r + 1} <= set(rows_all)
    dev, cpu = [], []
    for rows in rows_all:
        for i, (ld, shift) in enumerate(_variants(K)):
            d, c, tagc = _symexp_case(ops, rows, K, ld, shift, 5.0, weighted=(i != 1), with_gmul=(i == 0), reg=0.7)
            dev.append((d, tagc))
            cpu.append(c)
    for lscale, low, high in ((1.0, LOW, HIGH), (30.0, LOW, HIGH), (5.0, -5.0, 5.0), (5.0, -3.0, 12.0)):
        d, c, tagc = _symexp_case(ops, 5, K, (K + 3) // 4 * 4, 0, lscale, True, True, 1.0, low, high)
        dev.append((d, tagc))
        cpu.append(c)
    for name in cpu[0]:
        fig32 = max(c[name] for c in cpu)
        worst, where = max((d[name], tagc) for d, tagc in dev)
        log(f"[twohot space K={K}] {name}: float32 on the CPU {fig32:.2f} units, the device {worst:.2f} units "
            f"(limit {8 * fig32:.2f})")
        assert worst <= 8.0 * fig32, (name, worst, fig32, where)


# ----------------------------------------------------------------------------- 2. the cases that hold exactly
@pytest.mark.parametrize("K", [3, 255, 256])
def test_symlog_space_without_a_second_target_is_the_existing_entry_points_in_bits(ops, K):
    from repo_amd._lib import lib

    L = lib()
    s = torch.cuda.current_stream().cuda_stream
    for rows in (5, _row_counts(ops)[-2], _row_counts(ops)[-1]):
        z, R, w, g = (t.cuda() for t in _inputs(rows, K, 5.0, K + rows))
        ld = (K + 3) // 4 * 4
        zz = ops.twohot_rows(rows, K, z.device)
        zz.copy_(z)
        P = lambda t: t.data_ptr()   # noqa: E731
        v0, v1, m0, m1 = (torch.empty(rows, device="cuda") for _ in range(4))
        assert L.repo_twohot_decode(rows, K, P(zz), ld, LOW, HIGH, P(v0), P(m0), s) == 0
        assert L.repo_twohot_decode_x(rows, K, P(zz), ld, LOW, HIGH, 0, P(v1), P(m1), s) == 0
        assert torch.equal(_bits(v0), _bits(v1)) and torch.equal(_bits(m0), _bits(m1))
        d0, d1 = ops.twohot_rows(rows, K, z.device), ops.twohot_rows(rows, K, z.device)
        assert L.repo_twohot_decode_bwd(rows, K, P(zz), ld, LOW, HIGH, P(g), P(d0), ld, None, s) == 0
        assert L.repo_twohot_decode_bwd_x(rows, K, P(zz), ld, LOW, HIGH, 0, P(g), P(d1), ld, None, s) == 0
        assert torch.equal(_bits(d0), _bits(d1))
        ws = ops.reduce_ws(z.device)
        s2, s3 = torch.full((2,), -1.0, device="cuda"), torch.full((3,), -1.0, device="cuda")
        assert L.repo_twohot_nll(rows, K, P(zz), ld, P(R), P(w), LOW, HIGH, 0.5, P(d0), ld, P(s2), P(ws), ws.numel(), s) == 0
        assert L.repo_twohot_nll_x(rows, K, P(zz), ld, P(R), None, 0.3, P(w), LOW, HIGH, 0, 0.5, P(d1), ld, P(s3), P(ws),
                                   ws.numel(), s) == 0
        assert torch.equal(_bits(d0), _bits(d1)) and torch.equal(_bits(s2), _bits(s3[:2])) and float(s3[2]) == 0.0
        # ... and the wrappers route the default arguments to the existing entry points
        _, names = traced(lambda: (ops.twohot_decode(zz, LOW, HIGH), ops.twohot_decode_bwd(zz, LOW, HIGH, g),
                                   ops.twohot_nll(zz, R, w, LOW, HIGH, 0.5)))
        for k in X_KERNELS:
            assert not has(names, k), (k, names)


@pytest.mark.parametrize("space", ts.SPACES)
@pytest.mark.parametrize("K", [31, 255, 1024])
def test_reg_zero_is_the_unpaired_call_in_bits(ops, K, space):
    for rows in (5, _row_counts(ops)[-2], _row_counts(ops)[-1]):
        z, R, w, _ = (t.cuda() for t in _inputs(rows, K, 5.0, K + rows))
        Rb = _second_target(rows, 5).cuda()
        s_one, d_one = ops.twohot_nll(z, R, w, LOW, HIGH, 0.5, space=space)
        s_two, d_two = ops.twohot_nll(z, R, w, LOW, HIGH, 0.5, space=space, target_b=Rb, reg=0.0)
        assert torch.equal(_bits(d_one), _bits(d_two)) and torch.equal(_bits(s_one[:2]), _bits(s_two[:2]))
        assert float(s_two[2]) > 0.0 and (space == "symlog" or float(s_one[2]) == 0.0)


@pytest.mark.parametrize("K", [2, 3, 255, 256])
def test_equal_logits_over_symmetric_bins_decode_to_exactly_zero(ops, K):
    rows = 9
    for level in (0.0, 0.7, -3.0):
        z = ops.twohot_rows(rows, K, torch.device("cuda"))
        z.fill_(level)
        v, m = ops.twohot_decode(z, LOW, HIGH, want_mean=True, space="symexp")
        assert torch.equal(_bits(v), torch.zeros(rows, 1, dtype=torch.int32)) and not m.any()
        d = ops.twohot_decode_bwd(z, LOW, HIGH, torch.ones(rows, device="cuda"), space="symexp")
        assert torch.equal(d.flip(1), -d) and d.any()      # p (B - 0): mirrored like the bins (values: the middle is +-0)


def _device_bins(ops, K, low, high):
    """The kernels' own B_k: a row whose whole probability sits on bin k decodes to it."""
    z = torch.full((K, K), -1e30)
    z.fill_diagonal_(0.0)
    return ops.twohot_decode(z.cuda(), low, high, space="symexp").reshape(-1).cpu()


def test_targets_on_and_around_every_bin(ops):
    """K = 31: a target exactly at B_k gives a one-hot t, read through dlogits = p - t: every column but k holds the bits of p,
    which a run whose (one-hot) target sits on an end bin holds there too.  One float to either side of B_k all but ~2^-20 of
    the weight stays on bin k, and every column outside k - 1 .. k + 1 still holds the bits of p."""
    K, low, high = 31, -5.0, 5.0
    B = _device_bins(ops, K, low, high)
    assert torch.equal(B.flip(0), -B) and float(B[15]) == 0.0      # (values: the middle bin is +-0)
    assert float((B.double() - ts.symexp_bins(K, low, high)).abs().max()) <= 4 * UNIT * float(B[-1])
    z, _, _, _ = _inputs(K, K, 3.0, 9)
    zc = z.cuda()
    p64 = torch.softmax(z.double(), 1)
    # p's bits per column: from the run with every target on the top bin, column K - 1 from the run on the bottom bin
    _, d_hi = ops.twohot_nll(zc, B[-1].expand(K).contiguous().cuda(), None, low, high, 1.0, space="symexp")
    _, d_lo = ops.twohot_nll(zc, B[0].expand(K).contiguous().cuda(), None, low, high, 1.0, space="symexp")
    p_bits = d_hi.cpu().clone()
    p_bits[:, K - 1] = d_lo.cpu()[:, K - 1]
    assert float((p_bits.double() - p64).abs().max()) <= 8 * UNIT
    for name, R in (("on", B), ("below", torch.nextafter(B, torch.full_like(B, -1e30))),
                    ("above", torch.nextafter(B, torch.full_like(B, 1e30)))):
        sums, d = ops.twohot_nll(zc, R.cuda(), None, low, high, 1.0, space="symexp")
        d = d.cpu()
        t = p_bits.double() - d.double()
        assert torch.isfinite(sums).all()
        for k in range(K):
            reach = 0 if name == "on" else 1
            cold = [j for j in range(K) if abs(j - k) > reach]
            assert torch.equal(_bits(d[k, cold]), _bits(p_bits[k, cold])), (name, k)
            assert abs(float(t[k, k]) - 1.0) <= (4 * UNIT if name == "on" else 1e-5), (name, k, float(t[k, k]))
            assert abs(float(t[k].sum()) - 1.0) <= 8 * UNIT, (name, k)


def test_special_targets(ops):
    K, low, high = 33, -4.0, 4.0
    rows = 14
    z, R, w, _ = _inputs(rows, K, 3.0, 77)
    B = _device_bins(ops, K, low, high)
    special = {1: float("inf"), 2: float("-inf"), 4: 1e30, 5: -1e30, 7: 0.0, 8: -0.0, 9: 1e-42, 10: float("nan"),
               11: float(B[20]), 12: float(B[3])}
    plain = [r for r in range(rows) if r not in special]
    Rs = R.clone()
    for r, val in special.items():
        Rs[r] = val
    Rb = _second_target(rows, 3)
    scale, reg = 0.5, 0.7
    ld = (K + 3) // 4 * 4
    out_s, out_p = Banded(rows, K, ld, tt.SENT), Banded(rows, K, ld, tt.SENT)
    kw = dict(space="symexp", target_b=Rb.cuda(), reg=reg)
    sums_s, _ = ops.twohot_nll(z.cuda(), Rs.cuda(), w.cuda(), low, high, scale, dlogits=out_s.view, **kw)
    sums_p, _ = ops.twohot_nll(z.cuda(), R.cuda(), w.cuda(), low, high, scale, dlogits=out_p.view, **kw)
    assert out_s.intact() and out_p.intact(), "something outside the gradient's extents was written"
    ds, dp = out_s.view.cpu(), out_p.view.cpu()
    assert torch.equal(_bits(ds[plain]), _bits(dp[plain])) and torch.isfinite(sums_p).all()
    # the NaN target poisons its own row and sums3[0]; sum w and the second target's sum stay what they were
    assert torch.isnan(ds[10]).all() and math.isnan(float(sums_s[0]))
    assert torch.equal(_bits(sums_s[1:]), _bits(sums_p[1:]))
    fin = [r for r in range(rows) if r != 10]
    assert torch.isfinite(ds[fin]).all()
    # the same through the second target: sums3[2] and the row, not sums3[0]
    Rbn = Rb.clone()
    Rbn[6] = float("nan")
    sums_b, d_b = ops.twohot_nll(z.cuda(), R.cuda(), w.cuda(), low, high, scale, space="symexp", target_b=Rbn.cuda(), reg=reg)
    assert math.isnan(float(sums_b[2])) and torch.equal(_bits(sums_b[:2]), _bits(sums_p[:2]))
    assert torch.isnan(d_b[6]).all() and torch.isfinite(d_b.cpu()[[r for r in range(rows) if r != 6]]).all()
    # the end bins, the middle bin and the bins themselves take the whole weight: t_a = ((1 + reg) p - reg t_b) - dz / (scale w)
    one, _ = ops.twohot_nll(z.cuda(), Rs.cuda(), w.cuda(), low, high, scale, dlogits=out_s.view, space="symexp")
    p = torch.softmax(z.double(), 1)
    t = p - out_s.view.cpu().double() / (scale * w.double())[:, None]
    for r, k in ((1, K - 1), (4, K - 1), (2, 0), (5, 0), (7, 16), (8, 16), (9, 16), (11, 20), (12, 3)):
        hot = torch.zeros(K, dtype=torch.float64)
        hot[k] = 1.0
        assert float((t[r] - hot).abs().max()) <= 1e-5, (r, k)
    assert math.isnan(float(one[0])) and float(one[2]) == 0.0


def test_two_runs_agree_in_bits(ops):
    for rows in (4 * 64 + 1, 4 * 1024 + 1):
        z, R, w, g = (t.cuda() for t in _inputs(rows, 255, 5.0, 3))
        Rb = _second_target(rows, 4).cuda()
        for space in ts.SPACES:
            a = ops.twohot_nll(z, R, w, LOW, HIGH, 1.0 / rows, space=space, target_b=Rb, reg=0.5)
            b = ops.twohot_nll(z, R, w, LOW, HIGH, 1.0 / rows, space=space, target_b=Rb, reg=0.5)
            assert torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(_bits(a[1]), _bits(b[1]))
        a, b = (ops.twohot_decode_bwd(z, LOW, HIGH, g, space="symexp") for _ in range(2))
        assert torch.equal(_bits(a), _bits(b))


def test_error_codes(ops):
    from repo_amd._lib import lib

    rows, K = 8, 16
    z, d = torch.zeros(rows, K, device="cuda"), torch.zeros(rows, K, device="cuda")
    v, R, g = (torch.zeros(rows, device="cuda") for _ in range(3))
    sums = torch.zeros(3, device="cuda")
    ws = ops.reduce_ws(z.device)
    s = torch.cuda.current_stream().cuda_stream
    need = lib().repo_twohot_nll_x_workspace_bytes()
    assert lib().repo_reduce_workspace_bytes() < need <= ws.numel()
    P = lambda t: t.data_ptr()   # noqa: E731
    dec, bwd, nll = lib().repo_twohot_decode_x, lib().repo_twohot_decode_bwd_x, lib().repo_twohot_nll_x

    def c_dec(rows=rows, K=K, z=P(z), ld=K, low=LOW, high=HIGH, space=1, v=P(v)):
        return dec(rows, K, z, ld, low, high, space, v, None, s)

    def c_bwd(rows=rows, K=K, z=P(z), ld=K, low=LOW, high=HIGH, space=1, g=P(g), d=P(d), ldd=K):
        return bwd(rows, K, z, ld, low, high, space, g, d, ldd, None, s)

    def c_nll(rows=rows, K=K, z=P(z), ld=K, R=P(R), Rb=P(R), reg=1.0, low=LOW, high=HIGH, space=1, d=P(d), ldd=K,
              sums=P(sums), ws_=P(ws), nb=ws.numel()):
        return nll(rows, K, z, ld, R, Rb, reg, None, low, high, space, 1.0, d, ldd, sums, ws_, nb, s)

    for call in (c_dec, c_bwd, c_nll):
        for space in (0, 1):
            assert call(space=space) == 0
            assert call(space=space, K=1) == E_SHAPE and call(space=space, K=1025) == E_SHAPE
            assert call(space=space, ld=K - 1) == E_SHAPE
            assert call(space=space, rows=0) == E_SHAPE and call(space=space, rows=2 ** 31) == E_SHAPE
            assert call(space=space, low=5.0, high=5.0) == E_BADARG and call(space=space, low=6.0, high=-6.0) == E_BADARG
            assert call(space=space, low=float("nan")) == E_BADARG and call(space=space, high=float("inf")) == E_BADARG
            assert call(space=space, z=None) == E_BADARG
        assert call(space=2) == E_BADARG and call(space=-1) == E_BADARG
        # bins whose symexp is not a finite float exist in symlog space only
        assert call(space=0, low=-100.0, high=100.0) == 0 and call(space=1, low=-100.0, high=100.0) == E_BADARG
    assert c_dec(v=None) == E_BADARG
    assert c_bwd(g=None) == E_BADARG and c_bwd(d=None) == E_BADARG and c_bwd(ldd=K - 1) == E_SHAPE
    assert c_nll(R=None) == E_BADARG and c_nll(sums=None) == E_BADARG and c_nll(ldd=K - 1) == E_SHAPE
    assert c_nll(Rb=None) == 0 and c_nll(Rb=None, reg=float("nan")) == 0      # reg is not read without a second target
    assert c_nll(reg=-1.0) == E_BADARG and c_nll(reg=float("nan")) == E_BADARG and c_nll(reg=float("inf")) == E_BADARG
    assert c_nll(d=None, ldd=0) == 0                       # no gradient asked for: its pitch is not read
    assert c_nll(nb=need - 1) == E_WS_TOO_SMALL and c_nll(ws_=None) == E_WS_TOO_SMALL
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- 3. whole updates against the oracle
V31 = dict(value_dist="twohot", value_bins=31, value_bin_low=-5.0, value_bin_high=5.0)
V255 = dict(value_dist="twohot", value_bins=255, value_bin_low=-20.0, value_bin_high=20.0)
R31 = dict(reward_dist="twohot", reward_bins=31, reward_bin_low=-5.0, reward_bin_high=5.0)
V3 = dict(value_slow_reg=1.0, slow_value_update=1, slow_value_fraction=0.02)


def _sync_copy(agent, oracle):
    torch.cuda.synchronize()
    if oracle.slow_copy() is not None:
        oracle.set_slow_copy(agent.slow_value_model.state_dict())


def _agent_and_oracle(algo, over, slow_seed=th.TWOHOT_SLOW_SEED):
    from tests import test_slow_value_gpu as tsv

    rK = over.get("reward_bins") if over.get("reward_dist") == "twohot" else None
    agent, cfg, params = tw._pixel_agent(algo, reward_K=rK, **over)
    slow = None
    if agent._slow_copy:
        slow = th.make_twohot_value_params(cfg.value_bins, seed=slow_seed)
        tsv.load_target(agent, slow)
    oracle = ts.OracleSpace(cfg, LBHA[3], params=params, slow_params=slow)
    assert (oracle.sp_reg, oracle.sp_value, oracle.sp_reward) == (agent._value_reg, agent._value_space, agent._reward_space)
    return agent, cfg, oracle


@pytest.mark.parametrize("target", [False, True])
@pytest.mark.parametrize("algo", ["repo", "dreamer"])
def test_value_slow_reg_update_matches_oracle(algo, target):
    agent, cfg, oracle = _agent_and_oracle(algo, dict(V31, slow_value_target=target, **V3))
    assert agent._value_reg == 1.0 and agent._slow_value is target and agent._slow_copy
    assert (getattr(oracle, "slow", None) is not None) is target

    def regularised(u, oscal):
        got = agent.last_scalars
        log(f"[space reg {algo} target={target}] update {u}: value_loss {got['train/value_loss']:.5f} "
            f"value_reg {got['train/value_reg']:.5f} (oracle {oscal['train/value_reg']:.5f})")
        assert oscal["train/value_reg"] > 1e-2 and float(oracle.last["v_slow"].abs().max()) > 0.05
        _sync_copy(agent, oracle)

    tw._two_updates(agent, oracle, algo, False, f"[space reg {algo} target={target}]", regularised)


@pytest.mark.parametrize("algo,head", [("repo", V31), ("dreamer", V31), ("repo", V255)])
def test_value_bin_space_update_matches_oracle(algo, head):
    agent, cfg, oracle = _agent_and_oracle(algo, dict(head, value_bin_space="symexp"))
    assert agent._value_space == "symexp" and not agent._slow_copy

    def decoded(u, oscal):
        vals = oracle.last["values"]
        log(f"[space value {algo} K={cfg.value_bins}] update {u}: decoded values in [{float(vals.min()):.4g}, "
            f"{float(vals.max()):.4g}]")
        assert float(vals.abs().max()) > 0.05, "a head whose decoded values are not all ~0"

    tw._two_updates(agent, oracle, algo, False, f"[space value {algo} K={cfg.value_bins}]", decoded)


@pytest.mark.parametrize("algo", ["repo", "dreamer"])
def test_reward_bin_space_update_matches_oracle(algo):
    agent, cfg, oracle = _agent_and_oracle(algo, dict(R31, reward_bin_space="symexp"))
    assert agent._reward_space == "symexp" and agent._value_space == "symlog"
    tw._two_updates(agent, oracle, algo, False, f"[space reward {algo}]")


def test_all_three_keys_with_pcont_return_norm_and_both():
    """Every key of this change with pcont, return_norm and actor_grad = "both" -- and slow_value_target, which the oracle
    class that carries pcont is built on: the regulariser's target is the returns' own decoded slow value."""
    from tests import test_slow_value_gpu as tsv

    over = dict(V31, **R31, value_bin_space="symexp", reward_bin_space="symexp", value_slow_reg=1.0, pcont=True,
                return_norm=True, return_norm_decay=0.5, return_norm_limit=1e-3, actor_grad="both", actor_grad_mix=0.1,
                slow_value_target=True, slow_value_update=2, slow_value_fraction=0.5)
    agent, cfg, params = tw._pixel_agent("repo", reward_K=31, **over)
    head = pr.make_pcont_params(cfg.belief_size, cfg.state_size, cfg.hidden_size)
    agent._load_module(agent.pcont_model, tsv.torch_sd(head))
    slow = th.make_twohot_value_params(31, seed=th.TWOHOT_SLOW_SEED)
    tsv.load_target(agent, slow)
    oracle = ts.OracleSpaceSlowPcont(cfg, LBHA[3], params=params, pcont_params=head, slow_params=slow)
    assert oracle.sp_on and oracle.wm["rd_on"] and oracle.th_on and oracle.rn_on and oracle.mix == 0.1

    def finite(u, oscal):
        assert all(np.isfinite(v) for v in agent.last_scalars.values()) and "train/value_reg" in agent.last_scalars
        _sync_copy(agent, oracle)

    tw._two_updates(agent, oracle, "repo", False, "[space combined]", finite)


@pytest.mark.parametrize("every", [1, 2])
def test_the_copy_is_stepped_under_value_slow_reg_alone(every):
    """value_slow_reg > 0 with slow_value_target off: the copy exists, is checkpointed, and after the value optimiser's step
    k with k % slow_value_update == 0 it is tests/slow_value_ref.py's slow_mix(old copy, new head, fraction) -- and on
    every other step it stays where it was, in bits.  Bound: the mix is one subtraction, one product and one addition in
    float32, each within half a unit of 2^-24 of |old| + |new|; 4 units."""
    from tests import slow_value_ref as sv
    from tests import test_slow_value_gpu as tsv

    L, B, H, A = 8, 4, 5, 6
    agent, _ = tt._twohot_agent("repo", L, B, H, A, 31, value_slow_reg=1.0, slow_value_update=every, slow_value_fraction=0.02)
    assert not agent._slow_value and agent._slow_copy and "slow_value_model" in agent.get_param_dict()
    tsv.load_target(agent, th.make_twohot_value_params(31, seed=th.TWOHOT_SLOW_SEED))
    for step in (1, 2):
        old = agent._slow_value_flat.clone()
        tt._run_updates(agent, L, B, H, A, 1)
        torch.cuda.synchronize()
        assert agent.value_optimizer.step_count == step
        got, new = agent._slow_value_flat, agent.value_optimizer.flat
        if step % every:
            assert torch.equal(_bits(got), _bits(old)), step
            continue
        want = sv.slow_mix(old.double(), new.double(), 0.02)
        err = ((got.double() - want).abs() / (UNIT * (old.double().abs() + new.double().abs()) + 1e-300)).max()
        log(f"[space copy every={every}] step {step}: the mixed copy against float64 {float(err):.2f} units")
        assert float(err) <= 4.0 and not torch.equal(got, old) and not torch.equal(got, new)


# ----------------------------------------------------------------------------- 4. keys absent, and the device traces
def _opt_state(agent):
    out = []
    for name in ("model", "actor", "value"):
        o = getattr(agent, f"{name}_optimizer")
        out += [o.flat, o.exp_avg, o.exp_avg_sq]
    return [_bits(t) for t in out]


def test_absent_keys_change_nothing():
    from tests import test_slow_value_gpu as tsv

    L, B, H, A = 8, 4, 5, 6
    plain, cfg = tt._twohot_agent("repo", L, B, H, A, 31, **R31)
    for key in ("value_slow_reg", "value_bin_space", "reward_bin_space"):
        assert not hasattr(cfg, key)
    named, _ = tt._twohot_agent("repo", L, B, H, A, 31, value_slow_reg=0, value_bin_space="symlog",
                                reward_bin_space="symlog", **R31)
    assert named._value_bins == 31 and not named._slow_copy and not hasattr(named, "slow_value_model")
    for agent in (plain, named):
        tt._run_updates(agent, L, B, H, A, 2)
    torch.cuda.synchronize()
    for a, b in zip(_opt_state(named), _opt_state(plain)):
        assert torch.equal(a, b)
    assert named.last_scalars == plain.last_scalars and "train/value_reg" not in plain.last_scalars
    batch, _ = tu.dev_batch(L, B, A, 13)
    noise, _ = tu.dev_noise(L, B, H, A, 103)
    for agent in (plain, named):
        agent.noise_source = noise

        def three_updates():
            for _ in range(3):
                agent.update(batch)

        _, names = tsv.counted(three_updates)
        assert has(names, "twohot_decode_kernel") and has(names, "twohot_nll_kernel"), names
        for k in X_KERNELS:
            assert not has(names, k), (k, names)


def test_device_trace_with_the_keys_on():
    """value_slow_reg: ONE cross-entropy launch per critic step (the pair kernel), and without slow_value_target one more
    value-shaped forward and decode; symexp spaces: the _s1 kernels, and no decode reverse under actor_grad = "reinforce"."""
    from tests import test_slow_value_gpu as tsv

    L, B, H, A, n = 8, 4, 5, 6, 3
    batch, _ = tu.dev_batch(L, B, A, 13)
    noise, _ = tu.dev_noise(L, B, H, A, 103)

    def trace(**over):
        agent, _ = tt._twohot_agent("repo", L, B, H, A, 31, **over)
        agent.noise_source = noise
        agent.update(batch)     # (first-use allocations and packs stay out of the trace)

        def updates():
            for _ in range(n):
                agent.update(batch)

        _, names = tsv.counted(updates)
        assert all(np.isfinite(v) for v in agent.last_scalars.values())
        return names

    off = trace()
    on = trace(**V3)
    both = trace(slow_value_target=True, **V3)
    tgt = trace(slow_value_target=True, slow_value_update=1, slow_value_fraction=0.02)
    nll, dec = r"twohot_nll_kernel", r"twohot_decode_kernel"
    for names in (off, on, both, tgt):
        assert tsv.n_launches(names, nll) == n, names          # the value head's only: the reward head is scalar here
    assert tsv.n_launches(on, r"twohot_nll_kernel<\d, ?0, ?(true|1)>") == n == tsv.n_launches(both, r"twohot_nll_kernel<\d, ?0, ?(true|1)>")
    assert tsv.n_launches(on, dec) == tsv.n_launches(off, dec) + n           # the copy's decoded value on the critic's rows
    assert tsv.n_launches(both, dec) == tsv.n_launches(tgt, dec)             # already decoded for the returns: no new forward
    assert sum(on.values()) > sum(off.values())
    sym = trace(value_bin_space="symexp", actor_grad="reinforce")
    assert has(sym, "twohot_decode_s1_kernel") and has(sym, r"twohot_nll_kernel<\d, ?1, ?(false|0)>")
    assert not has(sym, "decode_bwd") and not has(sym, dec)
    dyn = trace(value_bin_space="symexp")
    assert has(dyn, "twohot_decode_bwd_s1_kernel") and not has(dyn, "twohot_decode_bwd_kernel")


# ----------------------------------------------------------------------------- 5. checkpoints, refusals, determinism
def test_checkpoint_round_trip_and_loads_across_spaces():
    L, B, H, A, K = 8, 4, 5, 6, 31
    over = dict(value_bin_space="symexp", reward_bin_space="symexp", **R31, **V3)
    agent, _ = tt._twohot_agent("dreamer", L, B, H, A, K, **over)
    tt._run_updates(agent, L, B, H, A, 1)
    torch.cuda.synchronize()
    ck = agent.get_param_dict()
    assert "slow_value_model" in ck and tuple(ck["slow_value_model"]["fc4.weight"].shape) == (K, 200)
    assert not any("space" in k or "slow_reg" in k for k in ck), "no new checkpoint keys"
    assert not torch.equal(ck["slow_value_model"]["fc4.weight"], ck["value_model"]["fc4.weight"])
    fresh, _ = tt._twohot_agent("dreamer", L, B, H, A, K, seed=8, head_seed=3, **over)
    fresh.load_param_dict(ck)
    for a in (agent, fresh):
        a.noise_source = None     # (the first update ran on injected noise)
        a.seed_noise(5)
        a._noise_counter = 0
    b2, _ = tu.dev_batch(L, B, A, 12)
    for a in (agent, fresh):
        a.update(b2)
    torch.cuda.synchronize()
    for x, y in zip(_opt_state(agent), _opt_state(fresh)):
        assert torch.equal(x, y)
    assert torch.equal(_bits(agent._slow_value_flat), _bits(fresh._slow_value_flat))
    assert agent.last_scalars == fresh.last_scalars
    # a checkpoint written under "symlog" loads under "symexp" (and back): the logits have the same shapes
    log_agent, _ = tt._twohot_agent("dreamer", L, B, H, A, K, **R31)
    tt._run_updates(log_agent, L, B, H, A, 1)
    torch.cuda.synchronize()
    ck_log = log_agent.get_param_dict()
    assert "slow_value_model" not in ck_log
    fresh.load_param_dict(ck_log)          # no slow entry: the copy becomes the value head just loaded
    assert torch.equal(_bits(fresh.value_optimizer.flat), _bits(log_agent.value_optimizer.flat))
    assert torch.equal(_bits(fresh._slow_value_flat), _bits(fresh.value_optimizer.flat))
    fresh.update(b2)
    assert all(np.isfinite(v) for v in fresh.last_scalars.values())
    log_agent.load_param_dict(ck)          # the slow entry of a checkpoint is ignored by an agent without a copy
    log_agent.update(b2)
    assert all(np.isfinite(v) for v in log_agent.last_scalars.values())


@pytest.mark.parametrize("key,over", [("value_slow_reg", dict(value_slow_reg=1.0)),
                                      ("value_bin_space", dict(value_bin_space="symexp")),
                                      ("reward_bin_space", dict(reward_bin_space="symexp"))])
@pytest.mark.parametrize("family", ["FinetunedRePo", "CalibratedRePo", "TIA", "MultitaskDreamer", "MultitaskRePo"])
def test_other_families_refuse(family, key, over):
    from tests import test_pcont_gpu as tp

    build = tp._family_builders()[family]
    with pytest.raises(NotImplementedError, match=key):
        build(**over)


def test_bad_values_raise():
    for over, match in ((dict(value_slow_reg=1.0), "value_slow_reg.*value_dist"),
                        (dict(value_slow_reg=1.0, value_dist="normal"), "value_slow_reg.*value_dist"),
                        (dict(value_slow_reg=-0.5, **V31), "value_slow_reg"),
                        (dict(value_bin_space="symexp"), "value_bin_space.*value_dist"),
                        (dict(reward_bin_space="symexp", **V31), "reward_bin_space.*reward_dist"),
                        (dict(value_bin_space="linear", **V31), "value_bin_space"),
                        (dict(reward_bin_space="log", **R31), "reward_bin_space")):
        for algo in ("repo", "dreamer"):
            with pytest.raises(ValueError, match=match):
                tu.make_agent(algo, 8, 4, 5, 6, **over)


def test_two_seeded_agents_are_bit_equal():
    from tests import test_slow_value_gpu as tsv

    L, B, H, A = 8, 4, 5, 6
    batches = [tu.dev_batch(L, B, A, 300 + i)[0] for i in range(3)]
    finals = []
    for _ in range(2):
        agent, _cfg = tt._twohot_agent("dreamer", L, B, H, A, 255, low=-20.0, high=20.0, actor_grad="both",
                                       value_bin_space="symexp", reward_bin_space="symexp", **dict(R31, reward_bins=255), **V3)
        # (the copy is the construction's clone of a head the helper has since replaced: pin it, as 6l's tests do)
        tsv.load_target(agent, th.make_twohot_value_params(255, seed=th.TWOHOT_SLOW_SEED))
        agent.seed_noise(99)
        for b in batches:
            agent.update(b, join=False)
        agent.synchronize()
        torch.cuda.synchronize()
        assert all(np.isfinite(v) for v in agent.last_scalars.values())
        keys = ("train/actor_loss", "train/value_loss", "train/value_reg")
        finals.append(_opt_state(agent) + [_bits(agent._slow_value_flat),
                                           _bits(torch.tensor([agent.last_scalars[k] for k in keys]))])
    for a, b in zip(*finals):
        assert torch.equal(a, b)
