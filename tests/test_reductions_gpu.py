"""The streaming kernels that close every update -- the reductions of csrc/loss.hip, csrc/optim.hip, channel_sum / relu_mask
of csrc/conv.hip and repo_transpose of csrc/gemm.hip -- at every grid regime, with proof of which kernels ran.

A reduction of loss.hip runs in one of three regimes (tests/reduce_ref.py mirrors each entry point's block count):
at most 64 blocks, where the launch's last block finishes the sum through the ticket word of the workspace header; 65 to
1024 blocks, where `final_sum_kernel` follows; the grid capped at 1024, where blocks stride.  Every case below sits at the
smallest size that reaches its regime (both sides of 64 | 65 included) and goes through the same checks, `reduction()`:
the partial area of the workspace is NaN-filled before the call and holds exactly nvals x blocks finite floats after it
(which pins the mirrored block count), the ticket word is 0 again, the outputs are `reduce_ref.fixed_order_sum` of their row
of partials BIT FOR BIT, every output tensor is finite (conftest hands out NaN-filled torch.empty), and the device trace
lists the reduction's kernel and lists `final_sum_kernel` if and only if blocks > 64.

Values are judged against float64 on the same float32 inputs: a sum by |got - want| <= FTOL * sum|terms| over the
reference's terms (a sum near zero does not inflate the error), elementwise gradients by l2err < GTOL -- FTOL and GTOL are
tests/test_rssm_gpu.py's, with its justification -- and by the tighter figure where an existing test asserts one for the
same quantity.  Bitwise assertions carry no tolerance.
"""
import math

import numpy as np
import pytest
import torch

from oracle import repo_oracle as ro
from tests import reduce_ref as rr
from tests.util import has, l2err, log, relerr, rnd, traced

pytestmark = pytest.mark.gpu

FTOL = 1e-5
GTOL = 1e-4


def F32(x):
    """A Python scalar as the kernel receives it (a C float argument)."""
    return float(np.float32(x))


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
    return t.detach().float().cuda().contiguous()


def bits(t):
    return t.detach().contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def _tensors(x):
    if torch.is_tensor(x):
        yield x
    elif isinstance(x, (tuple, list)):
        for y in x:
            yield from _tensors(y)


def header_word(ws):
    return int(ws[:4].view(torch.int32).item())


def reduction(ops, fn, sums, kernel, blocks, nvals, what, follow_up=None):
    """Run fn() under the checks every reduction case shares (module docstring).  `sums(result)` is the float32 tensor of
    the nvals output scalars; follow_up = (kernel pattern, expected in the trace), loss.hip's rule by default.
    Returns (result, partials as a (nvals, blocks) float32 array)."""
    ws = ops.reduce_ws(torch.device("cuda", torch.cuda.current_device()))
    area = ws[rr.RED_HEADER_BYTES:].view(torch.float32)
    area.fill_(float("nan"))
    res, names = traced(fn)
    assert header_word(ws) == 0, (what, "ticket word not re-armed", header_word(ws))
    a = area.cpu()
    finite = torch.isfinite(a)
    k = nvals * blocks
    assert bool(finite[:k].all()) and not bool(finite[k:].any()), (what, "finite partials", int(finite.sum()), "expected", k)
    parts = a[:k].view(nvals, blocks).numpy()
    want = torch.from_numpy(np.array([rr.fixed_order_sum(parts[v]) for v in range(nvals)], dtype=np.float32))
    got = sums(res).detach().cpu().reshape(-1)
    assert torch.equal(got, want), (what, "not the fixed-order sum of its partials", got.tolist(), want.tolist())
    for t in _tensors(res):
        assert bool(torch.isfinite(t).all()), (what, "an output element was left unwritten", tuple(t.shape))
    assert has(names, rf"\b{kernel}"), (what, names)
    pat, expected = follow_up if follow_up is not None else (r"\bfinal_sum_kernel\b", not rr.finishes_in_launch(blocks))
    assert has(names, pat) == expected, (what, blocks, names)
    return res, parts


def sum_err(got, terms):
    """|got - sum(terms)| / sum|terms| with float64 terms."""
    terms = terms.detach().double()
    return abs(float(got) - terms.sum().item()) / (terms.abs().sum().item() + 1e-300)


# ----------------------------------------------------------------------------------------------------------- kl_balance
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("rows,S", [(1, 30), (2560, 30), (2561, 1), (2561, 64), (41000, 30)])
def test_kl_balance_at_each_grid_regime(ops, rows, S, mode):
    """RePo's balanced KL (mode 0) and Dreamer's free nats (mode 1; a third of the rows under the threshold and, at
    rows = 2561, rows whose KL is exactly free_nats: one element ((qm - pm) / ps)^2 = 4 with qs = ps = 1 gives KL = 2 in
    float32 and float64 alike, every other element 0 -- torch.max hands each side half the gradient there)."""
    blocks = rr.kl_blocks(rows)
    rs = np.random.RandomState(1000 * mode + rows + S)
    pm, qm = rnd(rs, rows, S), rnd(rs, rows, S)
    ps, qs = rnd(rs, rows, S).abs() + 0.1, rnd(rs, rows, S).abs() + 0.1
    fn, alpha, scale = 2.0, F32(5 / 6), F32(1.0 / rows)
    lb = torch.tensor(math.log(0.3), dtype=torch.float32)
    ties = torch.arange(1, rows, 11) if (mode == 1 and rows == 2561) else torch.zeros(0, dtype=torch.long)
    under = torch.zeros(rows, dtype=torch.bool)
    if mode == 1:
        under[2::3] = True
        under[ties] = False
        qm[2::3], qs[2::3] = pm[2::3], ps[2::3]
        pm[ties], ps[ties], qm[ties], qs[ties] = 0.0, 1.0, 0.0, 1.0
        qm[ties, 0] = 2.0
    P = [t.double().requires_grad_(True) for t in (pm, ps, qm, qs)]
    if mode == 0:
        klp = ro.normal_kl(P[2].detach(), P[3].detach(), P[0], P[1]).sum(1)
        klq = ro.normal_kl(P[2], P[3], P[0].detach(), P[1].detach()).sum(1)
        (math.exp(lb.double().item()) * (alpha * klp + (1 - alpha) * klq) * scale).sum().backward()
        terms = klp.detach()
    else:
        kl = ro.normal_kl(P[2], P[3], P[0], P[1]).sum(1)
        assert bool((kl[ties] == fn).all()) and bool((kl[under] < fn).all())
        terms = torch.max(kl, torch.full((1,), fn, dtype=torch.float64))
        (terms * scale).sum().backward()
    args = (dev(pm), dev(ps), dev(qm), dev(qs), mode, alpha, lb.cuda() if mode == 0 else None, fn, scale)
    what = f"kl_balance mode={mode} rows={rows} S={S} blocks={blocks}"
    (out, g), _ = reduction(ops, lambda: ops.kl_balance(*args), lambda r: r[0], "kl_kernel", blocks, 1, what)
    e = sum_err(out.item(), terms)
    gerr = [l2err(gg, t.grad) for gg, t in zip(g, P)]
    log(f"{what}: sum {e:.2e}; l2 d(pm, ps, qm, qs) " + " ".join(f"{x:.2e}" for x in gerr))
    assert e <= FTOL, (what, e)
    for x in gerr:
        assert x < 1e-5, (what, gerr)      # test_rssm_gpu.py::test_losses' figure for these gradients
    if len(ties):
        tie_err = (g[2][ties.cuda()].double().cpu() - P[2].grad[ties]).abs().max().item()
        log(f"{what}: tie rows |d qm| err {tie_err:.2e}")
        assert tie_err < 1e-6 * (2.0 * scale) + 1e-12, tie_err      # test_widths_gpu.py's figure
    (out2, g2), _ = reduction(ops, lambda: ops.kl_balance(*args, want_grads=False), lambda r: r[0], "kl_kernel", blocks, 1,
                              what + " no grads")
    assert g2 == [None] * 4 and same_bits(out2, out), (what, out.item(), out2.item())


# ------------------------------------------------------------------------------------- scalar_nll and normal_entropy
N_FLAT = [1, 1023, 65536, 65537, 1048577]


@pytest.mark.parametrize("n", N_FLAT)
def test_scalar_nll_at_each_grid_regime(ops, n):
    blocks = rr.scalar_nll_blocks(n)
    rs = np.random.RandomState(n)
    pred, tgt = rnd(rs, n), rnd(rs, n)
    mask = torch.from_numpy((rs.uniform(size=n) > 0.3).astype(np.float32))
    scale = F32(0.5)
    p, t, m = dev(pred), dev(tgt), dev(mask)
    d = pred.double() - tgt.double()

    def run(what, mk, **kw):
        return reduction(ops, lambda: ops.scalar_nll(p, t, mk, scale, **kw), lambda r: r[0], "scalar_nll_kernel", blocks, 2,
                         f"scalar_nll n={n} blocks={blocks} {what}")[0]

    sums, dp = run("random mask", m)
    e0, e1 = sum_err(sums[0].item(), 0.5 * d * d * mask.double()), sum_err(sums[1].item(), mask.double())
    eg = relerr(dp, d * mask.double() * scale)
    log(f"scalar_nll n={n} blocks={blocks}: sums {e0:.2e} {e1:.2e}; dpred relerr {eg:.2e}")
    assert e0 <= FTOL and e1 <= FTOL and eg < 1e-6 and l2err(dp, d * mask.double() * scale) < GTOL
    assert sums[1].item() == mask.sum().item()         # a count below 2^24: exact in any order
    sums_ng, dp_ng = run("no grad", m, want_grad=False)
    assert dp_ng is None and same_bits(sums_ng, sums)
    # mask == NULL: every element counts
    sums_n, dp_n = run("mask=None", None)
    e0 = sum_err(sums_n[0].item(), 0.5 * d * d)
    log(f"scalar_nll n={n} mask=None: sum {e0:.2e}; count {sums_n[1].item():.0f}")
    assert e0 <= FTOL and sums_n[1].item() == float(n) and relerr(dp_n, d * scale) < 1e-6
    # an all-zero mask: nothing counts, exactly
    sums_z, dp_z = run("zero mask", torch.zeros(n, device="cuda"))
    assert sums_z.tolist() == [0.0, 0.0] and not bool(dp_z.any())


@pytest.mark.parametrize("n", N_FLAT)
def test_normal_entropy_at_each_grid_regime(ops, n):
    blocks = rr.normal_entropy_blocks(n)
    rs = np.random.RandomState(n + 1)
    sd = rnd(rs, n).abs() + 0.1
    gs = F32(2.0)
    s = dev(sd)
    what = f"normal_entropy n={n} blocks={blocks}"
    (out, dsd), _ = reduction(ops, lambda: ops.normal_entropy(s, gscale=gs, want_grad=True), lambda r: r[0],
                              "normal_entropy_kernel", blocks, 1, what)
    e = sum_err(out.item(), 0.5 + 0.5 * math.log(2 * math.pi) + sd.double().log())
    eg = relerr(dsd, gs / sd.double())
    log(f"{what}: sum {e:.2e}; dstd relerr {eg:.2e}")
    assert e <= FTOL and eg < 1e-6 and l2err(dsd, gs / sd.double()) < GTOL
    (out2, none), _ = reduction(ops, lambda: ops.normal_entropy(s, gscale=gs, want_grad=False), lambda r: r[0],
                                "normal_entropy_kernel", blocks, 1, what + " no grad")
    assert none is None and same_bits(out2, out)


# -------------------------------------------------------------------------------------------------------- lambda_return
@pytest.mark.parametrize("gamma,lam", [(0.99, 0.95), (0.99, 0.0), (0.99, 1.0)])
@pytest.mark.parametrize("Hm,N", [(2, 1), (3, 255), (15, 16384), (15, 16385), (3, 262145)])
def test_lambda_return_at_each_grid_regime(ops, Hm, N, gamma, lam):
    blocks = rr.lambda_return_blocks(N)
    rs = np.random.RandomState(Hm * 7 + N + int(lam * 100))
    r32, v32 = rnd(rs, Hm, N), rnd(rs, Hm, N)
    g, l_ = F32(gamma), F32(lam)
    r, v = r32.double().requires_grad_(True), v32.double().requires_grad_(True)
    ret = ro.lambda_return(r[:-1], v[:-1], torch.full((Hm - 1, N), g, dtype=torch.float64), v[-1], l_)
    gret = F32(-1.0 / ret.numel())
    (gret * ret.sum()).backward()
    rd, vd = dev(r32), dev(v32)
    what = f"lambda_return Hm={Hm} N={N} gamma={gamma} lambda={lam} blocks={blocks}"
    (returns, dr, dv, rsum), _ = reduction(ops, lambda: ops.lambda_return(rd, vd, g, l_, gret), lambda x: x[3],
                                           "lambda_return_kernel", blocks, 1, what)
    e = sum_err(rsum.item(), ret)
    errs = relerr(returns, ret), relerr(dr, r.grad), relerr(dv, v.grad)
    log(f"{what}: sum {e:.2e}; relerr returns {errs[0]:.2e} dr {errs[1]:.2e} dv {errs[2]:.2e}")
    assert e <= FTOL
    assert max(errs) < 1e-5, errs                       # test_rssm_gpu.py::test_losses' figure
    assert l2err(dr, r.grad) < GTOL and l2err(dv, v.grad) < GTOL
    (returns2, dr2, dv2, rsum2), _ = reduction(ops, lambda: ops.lambda_return(rd, vd, g, l_, gret, want_grads=False),
                                               lambda x: x[3], "lambda_return_kernel", blocks, 1, what + " no grads")
    assert dr2 is None and dv2 is None and same_bits(returns2, returns) and same_bits(rsum2, rsum)


# ------------------------------------------------------------------------------------------------ tanh_normal_entropy
def _actor_dist(rs, rows, A):
    """(mean, std) as float32, the way the actor head makes them; rows 0 and 1 saturated (tanh(u) rounds to +-1 for most
    draws: the clamp branch) where there are that many rows."""
    raw = torch.from_numpy(rs.standard_normal((rows, 2 * A)) * 2.0)
    if rows >= 2:
        raw[0, :A], raw[1, :A] = 40.0, -40.0
    mean = 5.0 * torch.tanh(raw[:, :A] / 5.0)
    std = torch.nn.functional.softplus(raw[:, A:]) + 0.1
    return mean.float(), std.float()


@pytest.mark.parametrize("rows,A,NS", [(1, 1, 1), (2730, 6, 10), (2731, 6, 10), (43691, 6, 4)])
def test_tanh_normal_entropy_at_each_grid_regime(ops, rows, A, NS):
    blocks = rr.tanh_normal_entropy_blocks(rows, A)
    rs = np.random.RandomState(rows + A + NS)
    mean, std = _actor_dist(rs, rows, A)
    eps = rnd(rs, NS, rows, A)
    md, sd = mean.double().requires_grad_(True), std.double().requires_grad_(True)
    ent = ro.tanh_normal_entropy(md, sd, eps.double())     # (rows,)
    ent.sum().backward()
    m, s, ep = dev(mean), dev(std), dev(eps)
    what = f"tanh_normal_entropy rows={rows} A={A} samples={NS} blocks={blocks}"
    (out, dm, ds), _ = reduction(ops, lambda: ops.tanh_normal_entropy(m, s, ep, gscale=1.0), lambda r: r[0],
                                 "tanh_normal_entropy_kernel", blocks, 1, what)
    e = sum_err(out.item(), ent)
    gm, gs = l2err(dm, md.grad), l2err(ds, sd.grad)
    log(f"{what}: sum {e:.2e}; l2 dmean {gm:.2e} dstd {gs:.2e}")
    assert e <= FTOL and gm < GTOL and gs < GTOL, (what, e, gm, gs)
    (out2, a, b), _ = reduction(ops, lambda: ops.tanh_normal_entropy(m, s, ep, gscale=1.0, want_grads=False),
                                lambda r: r[0], "tanh_normal_entropy_kernel", blocks, 1, what + " no grads")
    assert a is None and b is None and same_bits(out2, out)


@pytest.mark.parametrize("offset", [0, 1, 2, 3, 2 ** 32 + 5])
@pytest.mark.parametrize("NS", [1, 3, 4, 10])
def test_tanh_normal_entropy_in_kernel_noise_is_the_explicit_tensor(ops, NS, offset):
    """eps=None draws sample s of element e as normal number offset + e * NS + s of the Philox stream, four to a counter
    block: a thread refills at its first sample and wherever the index crosses a multiple of 4, which differ exactly when
    samples % 4 != 0 or offset % 4 != 0.  The same call on the materialised tensor (sample-fastest per element) must
    give the same bits."""
    rows, A, seed = 37, 7, 20240 + NS
    n = rows * A
    blocks = rr.tanh_normal_entropy_blocks(rows, A)
    rs = np.random.RandomState(NS)
    mean, std = _actor_dist(rs, rows, A)
    m, s = dev(mean), dev(std)
    z = ops.philox_normal(n * NS, seed, offset, m.device)
    eps = z.view(n, NS).t().contiguous().view(NS, rows, A)
    what = f"tanh_normal_entropy in-kernel noise samples={NS} offset={offset}"
    (o1, dm1, ds1), _ = reduction(ops, lambda: ops.tanh_normal_entropy(m, s, eps, gscale=0.7), lambda r: r[0],
                                  "tanh_normal_entropy_kernel", blocks, 1, what + " explicit")
    (o2, dm2, ds2), _ = reduction(ops, lambda: ops.tanh_normal_entropy(m, s, None, gscale=0.7, noise=(seed, offset), samples=NS),
                                  lambda r: r[0], "tanh_normal_entropy_kernel", blocks, 1, what + " drawn")
    nd = int((bits(dm1) != bits(dm2)).sum()) + int((bits(ds1) != bits(ds2)).sum())
    log(f"{what}: sums {o1.item():.6f} {o2.item():.6f}; gradient elements with other bits {nd}")
    assert same_bits(o1, o2) and same_bits(dm1, dm2) and same_bits(ds1, ds2), (what, nd)


@pytest.mark.parametrize("A,NS", [(1, 1), (6, 63), (6, 64), (6, 65), (70, 100)])
def test_tanh_normal_mode_sample_counts_around_a_wave(ops, A, NS):
    """SampleDist.mode over one wave per row: fewer samples than lanes, exactly 64, one more (the lane-stride loop), and
    more action columns than lanes.  Judged like test_widths_gpu.py: the float64 argmax's sample is picked, or the picked
    one's log-probability is within 1e-5 of the best, and at most 1 % of the rows differ.  (The 1 % is a cap, not a
    measurement: a float32 torch restatement of the argmax picks the float64 one's sample on all of these 600 rows at every
    (A, samples) here, and on all of 20000 rows (4000 at A = 70) drawn with another seed.)"""
    rows = 600
    rs = np.random.RandomState(A * 1000 + NS)
    mean32, std32 = _actor_dist(rs, rows, A)
    eps32 = rnd(rs, NS, rows, A)
    mode, names = traced(lambda: ops.tanh_normal_mode(dev(mean32), dev(std32), dev(eps32)))
    assert has(names, r"\btanh_normal_mode_kernel\b"), names
    assert bool(torch.isfinite(mode).all())
    mode = mode.double().cpu()
    mean, std, eps = mean32.double(), std32.double(), eps32.double()
    ys = torch.tanh(mean + std * eps).float().double()
    lp = ro.tanh_normal_log_prob(ys, mean, std)
    want = ys[lp.argmax(0), torch.arange(rows)]
    same = (mode - want).abs().max(1).values <= 1e-6
    lp_got = ro.tanh_normal_log_prob(mode[None], mean, std)[0]
    gap = (lp.max(0).values - lp_got).abs() / lp.abs().max(0).values.clamp_min(1.0)
    worst = float(gap[~same].max()) if (~same).any() else 0.0
    log(f"tanh_normal_mode A={A} samples={NS}: {int((~same).sum())} of {rows} rows picked another sample; worst log-prob gap {worst:.2e}")
    assert bool((same | (gap < 1e-5)).all())
    assert float((~same).double().mean()) < 1e-2


# -------------------------------------------------------------------------------------------------------- tia_blend_nll
def _tia_ref(t, d, wb, tgt, scale):
    """tia.py:123-133 and its gradients in closed form (float64): (the 8 sums, sum|terms| of each, dt, dd, recon)."""
    z = wb[6] + sum(wb[c] * t[:, 3 + c] + wb[3 + c] * d[:, 3 + c] for c in range(3))
    m = torch.sigmoid(z)[:, None]
    recon = t[:, :3] * m + d[:, :3] * (1 - m)
    df = recon - tgt
    g = df * scale
    dz = (g * (t[:, :3] - d[:, :3])).sum(1, keepdim=True) * m * (1 - m)
    dt = torch.cat((g * m, dz * wb[:3].view(1, 3, 1, 1)), 1)
    dd = torch.cat((g * (1 - m), dz * wb[3:6].view(1, 3, 1, 1)), 1)
    terms = [0.5 * df * df] + [dz[:, 0] * t[:, 3 + c] for c in range(3)] + [dz[:, 0] * d[:, 3 + c] for c in range(3)] + [dz]
    return [x.sum().item() for x in terms], [x.abs().sum().item() for x in terms], dt, dd, recon


@pytest.mark.parametrize("nimg,H", [(3, 2), (5, 6), (32, 64), (33, 64), (513, 64)])
def test_tia_blend_nll_at_each_grid_regime(ops, nimg, H):
    pixels = H * H
    blocks = rr.tia_blend_blocks(nimg, pixels)
    gen = torch.Generator().manual_seed(nimg * 100 + H)
    t_out = torch.randn(nimg, 6, H, H, generator=gen)
    d_out = torch.randn(nimg, 6, H, H, generator=gen)
    wb = torch.randn(7, generator=gen) * 0.7
    tgt_u8 = torch.randint(0, 256, (nimg, 3, H, H), generator=gen, dtype=torch.uint8)
    tgt = ((tgt_u8.float() / 255.0) * 2.0) - 1.0       # the kernel's (and common/utils.py:79's) float32 expression
    scale = F32(0.37)
    sums64, abs64, dt64, dd64, rc64 = _tia_ref(t_out.double(), d_out.double(), wb.double(), tgt.double(), scale)
    if nimg <= 5:   # the closed form against autograd, where that is cheap
        tr, dr, w = (x.double().requires_grad_(True) for x in (t_out, d_out, wb))
        mm = torch.sigmoid(torch.nn.functional.conv2d(torch.cat((tr[:, 3:], dr[:, 3:]), 1), w[:6].view(1, 6, 1, 1), w[6:]))
        loss = (0.5 * (tr[:, :3] * mm + dr[:, :3] * (1 - mm) - tgt.double()) ** 2).sum()
        (loss * scale).backward()
        assert abs(loss.item() - sums64[0]) < 1e-12 * abs64[0] and l2err(dt64, tr.grad) < 1e-12 and l2err(dd64, dr.grad) < 1e-12
        assert l2err(torch.tensor(sums64[1:], dtype=torch.float64), w.grad) < 1e-12
    td, ddv, wd = dev(t_out), dev(d_out), dev(wb)
    for u8 in (False, True):
        tg = tgt_u8.cuda() if u8 else dev(tgt)
        kern = r"tia_blend_nll_kernel<(?!float)" if u8 else r"tia_blend_nll_kernel<float"
        what = f"tia_blend_nll nimg={nimg} pixels={pixels} {'u8' if u8 else 'float'} blocks={blocks}"
        (sums, dt, dd, rc), _ = reduction(ops, lambda: ops.tia_blend_nll(td, ddv, wd, tg, scale, want_recon=True),
                                          lambda r: r[0], kern, blocks, 8, what)
        errs = [abs(sums[i].item() - sums64[i]) / (abs64[i] + 1e-300) for i in range(8)]
        gt, gd, er = l2err(dt, dt64), l2err(dd, dd64), relerr(rc, rc64)
        log(f"{what}: sums " + " ".join(f"{x:.1e}" for x in errs) + f"; l2 dt {gt:.2e} dd {gd:.2e}; recon relerr {er:.2e}")
        assert max(errs) <= FTOL, (what, errs)
        assert gt < GTOL and gd < GTOL and er < FTOL
        # test_tia_gpu.py's elementwise figures for the same tensors
        np.testing.assert_allclose(rc.cpu().numpy(), rc64.float().numpy(), rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(dt.cpu().numpy(), dt64.float().numpy(), rtol=1e-4, atol=1e-5)
        np.testing.assert_allclose(dd.cpu().numpy(), dd64.float().numpy(), rtol=1e-4, atol=1e-5)
        (s2, a, b, c), _ = reduction(ops, lambda: ops.tia_blend_nll(td, ddv, wd, tg, scale, want_grads=False),
                                     lambda r: r[0], kern, blocks, 8, what + " no grads")
        assert a is None and b is None and c is None and same_bits(s2, sums)
        ta, da = td.clone(), ddv.clone()
        (s3, dt3, dd3, _), _ = reduction(ops, lambda: ops.tia_blend_nll(ta, da, wd, tg, scale, inplace=True),
                                         lambda r: r[0], kern, blocks, 8, what + " in place")
        assert dt3.data_ptr() == ta.data_ptr() and dd3.data_ptr() == da.data_ptr()
        assert same_bits(s3, sums) and same_bits(dt3, dt) and same_bits(dd3, dd)


# ---------------------------------------------------------------------------------------------------------- grad_sqnorm
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 4095, 4097, 4194307])
def test_grad_sqnorm_tails_and_the_capped_grid(ops, n):
    """float4 body with a scalar tail (n % 4 = 1, 2, 3 and n < 4), two blocks, and the 1024-block cap with a 3-element
    tail.  Its two launches leave the workspace header alone."""
    blocks = rr.sqnorm_blocks(n)
    g = rnd(np.random.RandomState(n), n, scale=3.0)
    gd = dev(g)
    what = f"grad_sqnorm n={n} blocks={blocks}"
    out, _ = reduction(ops, lambda: ops.grad_sqnorm(gd), lambda r: r, r"sqnorm_kernel\b", blocks, 1, what,
                       follow_up=(r"\bsqnorm_final_kernel\b", True))
    e = sum_err(out.item(), g.double() ** 2)
    log(f"{what}: {e:.2e}")
    assert e <= FTOL


# ------------------------------------------------------------------------------------------------------------ clip_adam
BETAS = (F32(0.9), F32(0.999))     # the float32 values the kernel receives; the float64 reference takes the same
LR = 1e-2


def _adam64(p0, lr=LR):
    ref = p0.double().clone().requires_grad_(True)
    return ref, torch.optim.Adam([ref], lr=lr, betas=BETAS, eps=1e-8)


def _adam_bound(k, pmax, lr=LR):
    return k * (2.0 ** -24 * pmax + 2.0 ** -18 * lr)


@pytest.mark.parametrize("n", [1, 257, 524547])
def test_clip_adam_against_float64_adam(ops, n):
    """Three steps against torch.optim.Adam + clip_grad_norm_ in float64 (step 2 clipped), one block, two blocks, and more
    than 2048 blocks' worth (the grid-stride loop).

    Bound on |p - p64| after k steps: k * (2^-24 * max|p| + 2^-18 * lr).  Per step the kernel forms
    p <- fl(p - u), u = fl(lr_bc1 * q), q = m' / (sqrt(v') / sqrt(bc2) + eps).  The subtraction rounds once: half an ulp
    of p, at most 2^-24 |p|.  q carries the roundings of its operands -- the clip coefficient (3), m' (3, absolute
    error 3 * 2^-24 * max(b1 |m|, (1 - b1) |g|), which cancellation in m' does not amplify relative to sqrt(v')), v' (3,
    halved by the root), the root, the scaling, the sum, the quotient (1 each), lr_bc1 and the product (1 each): about 14
    roundings of 2^-24 relative to a quantity of magnitude at most 4 (|m_hat / sqrt(v_hat)| < 4 is asserted on the
    reference; Adam's ratio is bounded by (1 - b1) / sqrt(1 - b2) = 3.2 times the bias corrections' ratio), so
    |u - u64| <= 14 * 2^-24 * 4 * lr = 2^-18.2 * lr < 2^-18 * lr.  The moments' own rounding history (k <= 3 steps,
    damped by b1, b2) is inside the slack between 14 and the 16 that 2^-18 = 16 * 2^-24 * 4 leaves, and in practice every
    rounding is far from its worst case.  The errors of successive steps add: k times the sum.  The reference takes
    beta1, beta2 as the float32 values the kernel is given (1 - beta is exact in float32 for both)."""
    assert -(-n // 256) == {1: 1, 257: 2, 524547: 2050}[n] and rr.clip_adam_blocks(n) == min(2048, -(-n // 256))
    rs = np.random.RandomState(n)
    p0 = rnd(rs, n, scale=0.3)
    ref, opt = _adam64(p0)
    p, m, v = dev(p0), torch.zeros(n, device="cuda"), torch.zeros(n, device="cuda")
    max_norm = F32(math.sqrt(n))
    for step in (1, 2, 3):
        g = rnd(rs, n, scale=5.0 if step == 2 else 0.01)
        if n == 1:
            g = g.sign() * (5.0 if step == 2 else 0.01)      # a single draw may not land on its side of max_norm
        ref.grad = g.double().clone()
        total = float(torch.nn.utils.clip_grad_norm_([ref], max_norm))
        assert (total > max_norm) == (step == 2), (step, total, max_norm)
        opt.step()
        st = opt.state[ref]
        bc1, bc2 = 1 - BETAS[0] ** step, 1 - BETAS[1] ** step
        assert float(((st["exp_avg"] / bc1) / (st["exp_avg_sq"] / bc2).sqrt()).abs().max()) < 4.0
        sq = torch.tensor([F32((g.double() ** 2).sum().item())], device="cuda")
        gd = dev(g)
        _, names = traced(lambda: ops.clip_adam(p, gd, m, v, sq, max_norm, LR, step, betas=BETAS))
        assert has(names, r"\bclip_adam_kernel\b"), names
        e = (p.double().cpu() - ref.detach()).abs().max().item()
        bound = _adam_bound(step, ref.detach().abs().max().item())
        em, ev = relerr(m, st["exp_avg"]), relerr(v, st["exp_avg_sq"])
        log(f"clip_adam n={n} step {step}: max |p - p64| {e:.2e} (bound {bound:.2e}); relerr m {em:.2e} v {ev:.2e}")
        assert e <= bound, (n, step, e, bound)
        assert em < FTOL and ev < FTOL


def test_clip_adam_optional_operands(ops):
    """sqnorm == NULL (no clipping), an all-zero gradient, step = 1000 from zero moments, and skip_if_nonzero."""
    n = 257
    rs = np.random.RandomState(9)
    p0, g = rnd(rs, n, scale=0.3), rnd(rs, n, scale=5.0)
    gd = dev(g)
    zeros = lambda: torch.zeros(n, device="cuda")
    # no sqnorm: a gradient far above max_norm is applied unclipped (one step: bound with k = 1)
    for step in (1, 1000):
        ref, opt = _adam64(p0)
        if step > 1:   # zero moments at a late step: the bias corrections are 1 - 0.9^1000 = 1 and 1 - 0.999^1000 = 0.632
            opt.state[ref] = dict(step=torch.tensor(float(step - 1)), exp_avg=torch.zeros_like(ref),
                                  exp_avg_sq=torch.zeros_like(ref))
        ref.grad = g.double().clone()
        opt.step()
        assert float(opt.state[ref]["step"]) == step
        p, m, v = dev(p0), zeros(), zeros()
        ops.clip_adam(p, gd, m, v, None, 1e-3, LR, step, betas=BETAS)
        e = (p.double().cpu() - ref.detach()).abs().max().item()
        bound = _adam_bound(1, ref.detach().abs().max().item())
        moved = (ref.detach() - p0.double()).abs().min().item()
        log(f"clip_adam sqnorm=None step={step}: max |p - p64| {e:.2e} (bound {bound:.2e}); smallest move {moved:.2e}")
        assert e <= bound and moved > 0.5 * LR
        assert relerr(m, opt.state[ref]["exp_avg"]) < FTOL and relerr(v, opt.state[ref]["exp_avg_sq"]) < FTOL
    # all-zero gradient, sqnorm = 0: the coefficient is min(1, max_norm / 1e-6) = 1 and nothing moves
    p, m, v = dev(p0), zeros(), zeros()
    ops.clip_adam(p, zeros(), m, v, torch.zeros(1, device="cuda"), 100.0, LR, 1, betas=BETAS)
    assert same_bits(p, dev(p0)) and not bool(m.any()) and not bool(v.any())
    # skip word zero = no skip word, bit for bit; non-zero = nothing is touched
    sq = ops.grad_sqnorm(gd)
    m0, v0 = dev(rnd(rs, n, scale=0.1)), dev(rnd(rs, n, scale=0.1).abs())
    a = [dev(p0), m0.clone(), v0.clone()]
    b = [dev(p0), m0.clone(), v0.clone()]
    c = [dev(p0), m0.clone(), v0.clone()]
    ops.clip_adam(a[0], gd, a[1], a[2], sq, 1.0, LR, 3, betas=BETAS)
    ops.clip_adam(b[0], gd, b[1], b[2], sq, 1.0, LR, 3, betas=BETAS, skip=torch.zeros(1, dtype=torch.int32, device="cuda"))
    ops.clip_adam(c[0], gd, c[1], c[2], sq, 1.0, LR, 3, betas=BETAS, skip=torch.full((1,), 4, dtype=torch.int32, device="cuda"))
    assert not same_bits(a[0], dev(p0))
    assert all(same_bits(x, y) for x, y in zip(a, b))
    assert same_bits(c[0], dev(p0)) and same_bits(c[1], m0) and same_bits(c[2], v0)


# ------------------------------------------------------------------------------------------------------------ dual_step
def test_dual_step_five_steps_with_carried_moments(ops):
    """Five consecutive steps of the Lagrangian dual variable against float64 Adam on -log_beta * (kl - target), the
    moments carried and the KL on both sides of the target.  log_beta is held to k * (2^-24 |log_beta| + 2^-18 lr), the
    bound of test_clip_adam_against_float64_adam (one parameter, no clipping, |m_hat / sqrt(v_hat)| <= 1 at step 1 and
    < 4 after); the four scalars to FTOL relative."""
    lr, target, rows = 1e-2, F32(3.0), 100
    lb0 = math.log(0.3)
    lbp = torch.tensor([lb0], dtype=torch.float32, device="cuda")
    m, vv = torch.zeros(1, device="cuda"), torch.zeros(1, device="cuda")
    ref = torch.tensor([float(lbp.item())], dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([ref], lr=lr, betas=BETAS, eps=1e-8)
    for step, kl in enumerate((0.2, 4.0, 1.0, 6.5, 2.0), start=1):
        klsum = torch.tensor([kl * rows], dtype=torch.float32, device="cuda")
        kl64 = klsum.double().item() / rows
        before = ref.detach().item()
        opt.zero_grad()
        (-ref * (kl64 - target)).sum().backward()
        opt.step()
        sc, names = traced(lambda: ops.dual_step(lbp, m, vv, klsum, rows, target, lr, step, betas=BETAS))
        assert has(names, r"\bdual_step_kernel\b"), names
        want = [kl64, math.exp(before) * (kl64 - target), -before * (kl64 - target), math.exp(ref.item())]
        errs = [abs(sc[i].item() - want[i]) / abs(want[i]) for i in range(4)]
        e = abs(lbp.double().item() - ref.item())
        bound = step * (2.0 ** -24 * abs(ref.item()) + 2.0 ** -18 * lr)
        log(f"dual_step step {step} kl={kl}: |log_beta - ref| {e:.2e} (bound {bound:.2e}); scalars " + " ".join(f"{x:.1e}" for x in errs))
        assert e <= bound, (step, e, bound)
        assert max(errs) <= FTOL, (step, errs)
        assert abs(ref.item() - before) > 100 * bound   # the reference's own step: an update 1 % off cannot hide in the bound
    assert relerr(m, opt.state[ref]["exp_avg"]) < FTOL and relerr(vv, opt.state[ref]["exp_avg_sq"]) < FTOL
    # apply = 0 and a non-zero skip word: the scalars are written, the variable and its moments are not
    klsum = torch.tensor([5.0 * rows], dtype=torch.float32, device="cuda")
    lb_f = lbp.double().item()
    for kw in (dict(apply=False), dict(skip=torch.full((1,), 2, dtype=torch.int32, device="cuda"))):
        keep = [lbp.clone(), m.clone(), vv.clone()]
        sc = ops.dual_step(lbp, m, vv, klsum, rows, target, lr, 6, betas=BETAS, **kw)
        assert all(same_bits(x, y) for x, y in zip((lbp, m, vv), keep)), kw
        want = [5.0, math.exp(lb_f) * 2.0, -lb_f * 2.0, math.exp(lb_f)]
        errs = [abs(sc[i].item() - want[i]) / abs(want[i]) for i in range(4)]
        log(f"dual_step {sorted(kw)}: scalars " + " ".join(f"{x:.1e}" for x in errs))
        assert bool(torch.isfinite(sc).all()) and max(errs) <= FTOL, (kw, errs)
    # a zero skip word changes nothing against no skip word
    s1 = [lbp.clone(), m.clone(), vv.clone()]
    s2 = [lbp.clone(), m.clone(), vv.clone()]
    o1 = ops.dual_step(*s1, klsum, rows, target, lr, 6, betas=BETAS)
    o2 = ops.dual_step(*s2, klsum, rows, target, lr, 6, betas=BETAS, skip=torch.zeros(1, dtype=torch.int32, device="cuda"))
    assert same_bits(o1, o2) and all(same_bits(x, y) for x, y in zip(s1, s2)) and not same_bits(s1[0], lbp)


# ---------------------------------------------------------------------------------------------------------- channel_sum
@pytest.mark.parametrize("nimg,C,P", [(1, 1, 1), (300, 5, 1), (7, 3, 255), (7, 3, 256), (7, 3, 257), (9, 32, 900),
                                      (1001, 128, 25), (200, 3, 4096)])
def test_channel_sum_plane_sizes_and_splits(ops, nimg, C, P):
    """The flattened (image, pixel) walk's carry (dq = 256 / P, dr = 256 % P) at P = 1, on both sides of the block size
    and at dr = 0; a ragged last split; more splits than lanes in the final kernel; C not a multiple of 4."""
    splits = rr.chansum_splits(nimg, C, P)
    assert ops.lib().repo_channel_sum_workspace_bytes(nimg, C, P) == splits * C * 4     # pins the mirror
    rs = np.random.RandomState(nimg + C + P)
    x = rnd(rs, nimg, C, P)
    xd = dev(x)
    want, wabs = x.double().sum((0, 2)), x.double().abs().sum((0, 2))
    what = f"channel_sum nimg={nimg} C={C} P={P} splits={splits}"
    out, names = traced(lambda: ops.channel_sum(xd))
    assert has(names, r"\bchannel_sum_kernel\b") and has(names, r"\bchannel_sum_final_kernel\b"), names
    assert bool(torch.isfinite(out).all())
    e = ((out.double().cpu() - want).abs() / wabs).max().item()
    assert same_bits(ops.channel_sum(xd), out), what
    pre = rnd(rs, C)
    acc = ops.channel_sum(xd, out=dev(pre), accumulate=True)
    ea = ((acc.double().cpu() - (want + pre.double())).abs() / (wabs + pre.double().abs())).max().item()
    log(f"{what}: {e:.2e}; accumulated {ea:.2e}")
    assert e <= FTOL and ea <= FTOL, (what, e, ea)


# ------------------------------------------------------------------------------------------------------------ relu_mask
SPECIALS = [0.0, -0.0, 1e-40, -1e-40, float("nan"), 1.1754944e-38, -1.1754944e-38]   # zeros, denormals, NaN, smallest normals


@pytest.mark.parametrize("n", [1, 255, 1048589])
def test_relu_mask_zeros_denormals_nan(ops, n):
    """y = h > 0 ? dy : +0: -0.0, NaN and negative denormals are not positive, a positive denormal is.  One block, and more
    than 4096 blocks' worth (the grid-stride loop).  n = 0 is a success that writes nothing."""
    rs = np.random.RandomState(n)
    dy = rnd(rs, n)
    variants = range(len(SPECIALS)) if n == 1 else [0]
    for k in variants:
        h = rnd(rs, n)
        where = np.unique(np.concatenate([np.arange(0, n, max(1, n // 97)), [n - 1]]))
        for j, i in enumerate(where):
            h[i] = SPECIALS[(j + k) % len(SPECIALS)]
        want = torch.where(h > 0, dy, torch.zeros(()))
        if n > 1:
            assert bool((want[where] != 0).any()) and bool((want[where] == 0).any())
        hd, dyd = dev(h), dev(dy)
        assert same_bits(hd.cpu(), h)       # the upload kept the denormals and the sign of zero
        got, names = traced(lambda: ops.relu_mask(dyd, hd))
        assert has(names, r"\brelu_mask_kernel\b"), names
        nd = int((bits(got.cpu()) != bits(want)).sum())
        log(f"relu_mask n={n} variant {k}: {nd} elements with other bits")
        assert nd == 0
    out = torch.full((8,), 7.0, device="cuda")
    assert ops.relu_mask(dev(dy)[:0], dev(dy)[:0], out=out) is out
    torch.cuda.synchronize()
    assert out.tolist() == [7.0] * 8


# ------------------------------------------------------------------------------------------------------------ transpose
SENTINEL = -12345.0


def _transpose_case(rows, cols, lds, ldd, seed=0):
    wide = dev(rnd(np.random.RandomState(rows + cols + seed), rows, lds))
    out = torch.full((cols + 1, ldd), SENTINEL, device="cuda")
    return wide, wide[:, :cols], out


@pytest.mark.parametrize("rows,cols,lds,ldd", [(1, 1, 4, 4), (3, 5, 8, 4), (64, 64, 64, 64), (65, 63, 64, 68),
                                               (65, 63, 64, 128), (130, 1940, 1940, 132), (64, 64, 64, 68),
                                               (128, 70, 72, 188)])
def test_transpose_writes_the_transpose_and_zero_pads(ops, rows, cols, lds, ldd):
    """include/repo_hip.h: dst[c][r] = src[r][c], columns [rows, ldd) of dst zero for every ldd - rows < 64 -- also where
    the pads lie beyond the last 64-row tile of src (the last two cases) -- and nothing beyond dst's `cols` rows."""
    wide, src, out = _transpose_case(rows, cols, lds, ldd)
    view, names = traced(lambda: ops.transpose(src, out=out))
    assert has(names, r"\btranspose_kernel\b"), names
    assert view.shape == (cols + 1, rows) and view.data_ptr() == out.data_ptr()      # out's first `rows` columns
    bad = int((bits(out[:cols, :rows]) != bits(src.t())).sum())
    pad = out[:cols, rows:]
    unwritten, nonzero = int((pad == SENTINEL).sum()), int((pad != 0).sum())
    log(f"transpose rows={rows} cols={cols} lds={lds} ldd={ldd}: {bad} wrong elements; of {pad.numel()} pad elements "
        f"{nonzero} non-zero ({unwritten} never written)")
    assert bad == 0
    assert nonzero == 0, (nonzero, unwritten)
    assert bool((out[cols] == SENTINEL).all())


def test_transpose_refusals_write_nothing(ops):
    from repo_amd._lib import RepoHipError

    rows, cols = 64, 40
    wide, src, out = _transpose_case(rows, cols, 44, rows + 64)
    L, st = ops.lib(), torch.cuda.current_stream().cuda_stream
    E_SHAPE, E_ALIGN = -2, -3       # include/repo_hip.h
    assert L.repo_transpose(rows, cols, src.data_ptr(), 44, out.data_ptr(), rows + 64, st) == E_SHAPE       # ldd - rows = 64
    assert L.repo_transpose(rows, cols, src.data_ptr(), 44, out.data_ptr(), rows - 4, st) == E_SHAPE        # ldd < rows
    assert L.repo_transpose(rows, cols, src.data_ptr(), 42, out.data_ptr(), rows + 4, st) == E_ALIGN        # lds % 4
    assert L.repo_transpose(rows, cols, src.data_ptr(), 44, out.data_ptr(), rows + 2, st) == E_ALIGN        # ldd % 4
    assert L.repo_transpose(rows, cols, src.data_ptr() + 4, 44, out.data_ptr(), rows + 4, st) == E_ALIGN    # src pointer
    assert L.repo_transpose(rows, cols, src.data_ptr(), 44, out.data_ptr() + 4, rows + 4, st) == E_ALIGN    # dst pointer
    with pytest.raises(RepoHipError):
        ops.transpose(src, out=out)          # out's pitch is rows + 64
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


# ------------------------------------------------------------------------------------------------- the ticket, in sequence
def _ticket_calls(ops):
    """Every single-launch reduction of loss.hip as (name, call -> tensors whose bits are compared), each in its ticket regime
    with more than one block, on device inputs made once."""
    rs = np.random.RandomState(77)
    rows, S = 1000, 30
    pm, qm = dev(rnd(rs, rows, S)), dev(rnd(rs, rows, S))
    ps, qs = dev(rnd(rs, rows, S).abs() + 0.1), dev(rnd(rs, rows, S).abs() + 0.1)
    lb = torch.tensor(math.log(0.3), dtype=torch.float32).cuda()
    n = 30000
    pred, tgt, mask = dev(rnd(rs, n)), dev(rnd(rs, n)), dev(torch.from_numpy((rs.uniform(size=n) > 0.3).astype(np.float32)))
    sd = dev(rnd(rs, n).abs() + 0.1)
    mean, std = (dev(t) for t in _actor_dist(rs, 1200, 6))
    eps = dev(rnd(rs, 5, 1200, 6))
    r, v = dev(rnd(rs, 8, 5000)), dev(rnd(rs, 8, 5000))
    gen = torch.Generator().manual_seed(5)
    t_out, d_out = torch.randn(9, 6, 64, 64, generator=gen).cuda(), torch.randn(9, 6, 64, 64, generator=gen).cuda()
    wb = (torch.randn(7, generator=gen) * 0.7).cuda()
    tg8 = torch.randint(0, 256, (9, 3, 64, 64), generator=gen, dtype=torch.uint8).cuda()
    tgf = ((tg8.float() / 255.0) * 2.0) - 1.0
    calls = [
        ("kl mode 0", rr.kl_blocks(rows), lambda: ops.kl_balance(pm, ps, qm, qs, 0, 0.8, lb, 2.0, 1e-3)),
        ("kl mode 1", rr.kl_blocks(rows), lambda: ops.kl_balance(pm, ps, qm, qs, 1, 0.0, None, 2.0, 1e-3)),
        ("scalar_nll", rr.scalar_nll_blocks(n), lambda: ops.scalar_nll(pred, tgt, mask, 0.5)),
        ("normal_entropy", rr.normal_entropy_blocks(n), lambda: ops.normal_entropy(sd, gscale=2.0, want_grad=True)),
        ("tanh_normal_entropy", rr.tanh_normal_entropy_blocks(1200, 6), lambda: ops.tanh_normal_entropy(mean, std, eps, gscale=1.0)),
        ("tanh_normal_entropy drawn", rr.tanh_normal_entropy_blocks(1200, 6),
         lambda: ops.tanh_normal_entropy(mean, std, None, gscale=1.0, noise=(11, 3), samples=5)),
        ("lambda_return", rr.lambda_return_blocks(5000), lambda: ops.lambda_return(r, v, 0.99, 0.95, -1e-4)),
        ("tia float", rr.tia_blend_blocks(9, 4096), lambda: ops.tia_blend_nll(t_out, d_out, wb, tgf, 0.37)),
        ("tia u8", rr.tia_blend_blocks(9, 4096), lambda: ops.tia_blend_nll(t_out, d_out, wb, tg8, 0.37)),
    ]
    for name, blocks, _ in calls:
        assert 1 < blocks <= rr.LAST_BLOCK_MAX_GRID, (name, blocks)
    return [(name, fn) for name, _, fn in calls]


def test_ticket_is_rearmed_between_back_to_back_reductions_and_per_stream(ops):
    """Each launch's last block puts the ticket word back to 0 for the next launch on the stream.  All ticket-regime
    reductions back to back on the default stream with no synchronisation in between, then once more in reverse order:
    every result has the bits of the same call run alone, and the word is 0 at the end.  A side stream has a workspace (and
    a ticket) of its own and gives the same bits."""
    device = torch.device("cuda", torch.cuda.current_device())
    calls = _ticket_calls(ops)
    alone = {}
    for name, fn in calls:
        torch.cuda.synchronize()
        alone[name] = [t.clone() for t in _tensors(fn())]
        torch.cuda.synchronize()
    ws = ops.reduce_ws(device)
    assert header_word(ws) == 0
    (first, second), names = traced(lambda: ([(n, fn()) for n, fn in calls], [(n, fn()) for n, fn in reversed(calls)]))
    assert not has(names, r"\bfinal_sum_kernel\b"), names
    assert header_word(ws) == 0
    for which, results in (("forward", first), ("reverse", second)):
        for name, res in results:
            got = list(_tensors(res))
            assert len(got) == len(alone[name]) and all(same_bits(a, b) for a, b in zip(got, alone[name])), (which, name)
    # the side stream
    name, fn = calls[0]
    side = torch.cuda.Stream(device=device)
    side.wait_stream(torch.cuda.current_stream(device))
    with torch.cuda.stream(side):
        ws_side = ops.reduce_ws(device)
        res = fn()
    side.synchronize()
    assert ws_side.data_ptr() != ws.data_ptr()
    assert all(same_bits(a, b) for a, b in zip(_tensors(res), alone[name])), name
    assert header_word(ws_side) == 0 and header_word(ws) == 0
    torch.cuda.current_stream(device).wait_stream(side)
    log(f"ticket sequence: {len(calls)} reductions forward and reverse on one stream and '{name}' on a side stream: bit-equal to the calls run alone")
