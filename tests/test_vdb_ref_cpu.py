"""tests/vdb_ref.py tied down without a GPU: its reverse formulas against float64 autograd of its forward ones, its forward
against tests/calib_ref.py (which tests/test_calib_cpu.py ties to the reference's own modules), the grid mirrors at the
boundaries of every regime, the finishing sum against a hand-written loop, and the float32 table of
tests/test_vdb_kernels_gpu.py against its own measurement."""
import numpy as np
import pytest
import torch

from tests import calib_ref as cr
from tests import test_calib_gpu as tc
from tests import test_vdb_kernels_gpu as tv
from tests import vdb_ref as vr
from tests.util import l2err

RTOL = 1e-12


def rel(got, want):
    got, want = (float(x.detach()) if torch.is_tensor(x) else float(x) for x in (got, want))
    return abs(got - want) / abs(want)


@pytest.mark.parametrize("mode", tv.MODES, ids=tv.MODE_NAMES)
@pytest.mark.parametrize("N,Z", [(1, 1), (7, 5), (33, 65)])
def test_head_bwd_is_autograd_of_head_fwd_and_loss(N, Z, mode):
    """L = gscale sum f(d) + beta kl_coef sum kl_rows + <extra, logstd>: dL/dz, dL/dfc_w, dL/dfc_b."""
    z32, eps, w32, b32 = tv.head_inputs(N, Z)
    dd_unused, beta, klc, extra, _ = tv.bwd_inputs(N, Z)
    tau = tv.loss_inputs(N)[1]
    gscale = 1.0 / N
    z, w, b = (t.double().requires_grad_(True) for t in (z32, w32, b32))
    lat, d, kl_rows = vr.head_fwd(z, eps, w, b)
    terms, dd = vr.loss(d, mode, tau, gscale)
    L = gscale * terms.sum() + beta.double()[0] * klc * kl_rows.sum() + (extra.double() * z[:, Z:]).sum()
    gz, gw, gb = torch.autograd.grad(L, (z, w, b))
    dz, tw, tb = vr.head_bwd(z32, eps, lat.detach(), w32, dd.detach(), beta, klc, extra)
    assert l2err(dz, gz) < RTOL and l2err(tw.sum(0), gw) < RTOL and rel(tb.sum(), gb) < RTOL
    # the nullable operands: no KL term, no extra
    L0 = gscale * vr.loss(vr.head_fwd(z, eps, w, b)[1], mode, tau, gscale)[0].sum()
    gz0, = torch.autograd.grad(L0, z)
    assert l2err(vr.head_bwd(z32, eps, lat.detach(), w32, dd.detach())[0], gz0) < RTOL


@pytest.mark.parametrize("N,Z", [(1, 1), (7, 5), (33, 65)])
def test_gp_head_is_autograd_of_the_inner_product_with_gp_delta(N, Z):
    """<a5, delta5(fc_w, logstd)> with leaky'(lat) held constant: d/d fc_w = the column sums, d/d logstd = extra."""
    z32, eps, w32, b32 = tv.head_inputs(N, Z)
    a5 = tv.bwd_inputs(N, Z)[4]
    lat = vr.head_fwd(z32, eps, w32, b32, dtype=torch.float32)[0]
    z, w = z32.double().requires_grad_(True), w32.double().requires_grad_(True)
    inner = (a5.double() * vr.gp_delta(z, eps, lat, w)).sum()
    gz, gw = torch.autograd.grad(inner, (z, w))
    extra, tw = vr.gp_head(a5, z32, eps, lat, w32)
    assert float(gz[:, :Z].abs().max()) == 0.0            # delta5 does not depend on the mean half
    assert l2err(extra, gz[:, Z:]) < RTOL and l2err(tw.sum(0), gw) < RTOL


@pytest.mark.parametrize("support", [False, True])
def test_forward_loss_and_penalty_compose_to_calib_ref(support):
    """head_fwd + loss + gp_delta + gp_norm on the encoder's output = calib_ref.disc_forward / disc_losses on a case of
    tests/test_calib_gpu.py."""
    ci = 2
    Nr, Nf, E, Hf, Z = tc.CASES[ci]
    xr, xf, er, ef, tau = (None if v is None else v.double() for v in tc.make_case(ci, support, tc.SEEDS[(ci, support)]))
    p = {k: torch.from_numpy(v).double() for k, v in cr.make_disc_params(E, Hf, Z).items()}
    want = cr.disc_losses(p, xr, xf, er, ef, tc.BETA0, tau=tau)
    xr = xr.clone().requires_grad_(True)
    zr, zf = cr.mlp(p, xr, "leaky", prefix="encoder."), cr.mlp(p, xf, "leaky", prefix="encoder.")
    lat_r, d_r, kl_r = vr.head_fwd(zr, er, p["fc.weight"], p["fc.bias"])
    lat_f, d_f, kl_f = vr.head_fwd(zf, ef, p["fc.weight"], p["fc.bias"])
    d_want, mean, logstd = cr.disc_forward(p, xf, ef)
    assert l2err(d_f, d_want) < RTOL and l2err(d_r, want["d_real"]) < RTOL and l2err(zf, torch.cat((mean, logstd), 1)) < RTOL
    real = vr.loss(d_r, vr.NEG_TAU if support else vr.BCE1, tau)[0].mean()
    fake = vr.loss(d_f, vr.CHI if support else vr.BCE0)[0].mean()
    kl = 0.5 * (kl_r.mean() + kl_f.mean())
    assert rel(real, want["real"]) < RTOL and rel(fake, want["fake"]) < RTOL and rel(kl, want["kl"]) < RTOL
    assert rel(vr.loss(d_f, vr.NEG_CHI if support else vr.BCE1)[0].mean(), cr.generator_loss(d_f, support)) < RTOL
    # the penalty: g = d(sum d)/dx is the chain's reverse pass fed gp_delta; its value is gp_norm's sum / N
    g, = torch.autograd.grad(zr, xr, grad_outputs=vr.gp_delta(zr.detach(), er, lat_r.detach(), p["fc.weight"]))
    terms, scaled = vr.gp_norm(g, 2.0 / Nr)
    assert rel(terms.sum() / Nr, want["gp"]) < RTOL and l2err(scaled, 2.0 * g / Nr) < RTOL
    # beta_step and tau against calib_ref's
    new_beta, klm = vr.beta_step(tc.BETA0, kl_r.sum().item(), Nr, kl_f.sum().item(), Nf, 5e-3, 0.1)
    assert rel(klm, want["kl"]) < RTOL and rel(new_beta, cr.beta_step(tc.BETA0, want["kl"].item())) < RTOL
    lt = torch.log(tau) if support else torch.from_numpy(np.random.RandomState(3).standard_normal(Nr) * 0.5)
    u = torch.tensor([0.3], dtype=torch.float64, requires_grad=True)
    ltg = lt.double().clone().requires_grad_(True)
    tau_loss, u_loss = cr.tau_losses(torch.exp(ltg), d_r.detach(), u)
    t0, t1, tt, dlt = vr.tau(ltg.detach(), d_r.detach(), u.detach())
    assert rel(t0.mean() + u.detach()[0] * t1.mean(), tau_loss) < RTOL and rel(-u.detach()[0] * t1.mean(), u_loss) < RTOL
    assert l2err(dlt, torch.autograd.grad(tau_loss, ltg)[0]) < RTOL and l2err(tt, torch.exp(ltg)) < RTOL


def test_loss_terms_and_derivatives_of_every_mode():
    d = torch.tensor(tv.EDGE_D + [0.3, -2.5], dtype=torch.float64, requires_grad=True)
    tau = torch.linspace(0.5, 2.0, d.numel(), dtype=torch.float64)
    zero = torch.zeros_like(d)
    closed = {vr.BCE0: torch.logaddexp(zero, d), vr.BCE1: torch.logaddexp(zero, -d), vr.NEG_TAU: -tau * d,
              vr.CHI: d + d * d / 4, vr.NEG_CHI: -(d + d * d / 4)}
    for mode, want in closed.items():
        terms, dd = vr.loss(d, mode, tau, 0.25)
        # (atol: torch forms log(1 + exp(-|x|)), not log1p: 6e-16 off at x = -20, and 0 where softplus(-88) = 6e-39)
        assert torch.allclose(terms, want, rtol=1e-12, atol=1e-14), mode
        g, = torch.autograd.grad(terms.sum(), d, retain_graph=True)
        assert l2err(dd, 0.25 * g) < RTOL, mode
    with pytest.raises(ValueError):
        vr.loss(d, 5)


def test_grid_mirrors_at_the_regime_boundaries():
    assert [vr.head_fwd_blocks(n) for n in (1, 4, 5, 256, 257, 2500)] == [1, 1, 2, 64, 64, 64]
    assert [vr.loss_blocks(n) for n in (1, 256, 257, 16384, 16385)] == [1, 1, 2, 64, 64]
    assert [vr.gp_norm_blocks(n) for n in (1, 4096, 4097, 262144, 262145, 2500 * 1024)] == [1, 1, 2, 64, 64, 64]
    assert [vr.colsum_grid(n) for n in (1, 3, 32, 33, 2048, 2049, 2500)] == [(1, 1), (1, 3), (1, 32), (2, 17), (64, 32), (64, 33),
                                                                            (64, 40)]
    assert vr.colsum_rows(33, 1) == 16
    assert vr.colsum_rows(2048, 63) == 32
    assert vr.colsum_rows(2049, 62) == 3 and vr.colsum_rows(2049, 63) == 0          # 62 * 33 = 2046: block 63 is empty
    assert vr.colsum_rows(2500, 61) == 40 and vr.colsum_rows(2500, 62) == 20 and vr.colsum_rows(2500, 63) == 0
    for n in (1, 3, 33, 2049, 2500, 100000):
        G, rpb = vr.colsum_grid(n)
        assert sum(vr.colsum_rows(n, b) for b in range(G)) == n
    assert [vr.gp_delta_blocks(n, z) for n, z in ((1, 1), (37, 5), (4096, 128), (4097, 128), (2500, 64))] == [1, 1, 2048, 2048, 625]
    # the cases of the GPU suite sit where its ids say
    assert tv.HEAD_IDS[3:5] == ["N256-Z64-64blk", "N257-Z64-64blk-strided"]
    assert tv.DELTA_IDS[2:4] == ["N4096-Z128-2048blk", "N4097-Z128-2048blk-strided"]


def test_colsum_finish_is_the_in_order_float32_sum():
    rs = np.random.RandomState(0)
    for G in (1, 2, 64):
        parts = (rs.standard_normal(G) * 10.0 ** rs.uniform(-3, 3, G)).astype(np.float32)
        s = np.float32(0.0)
        for i in range(G):
            s = np.float32(s + parts[i])
        assert vr.colsum_finish(parts).tobytes() == s.tobytes()
        prev = np.float32(rs.standard_normal())
        assert vr.colsum_finish(parts, prev).tobytes() == np.float32(prev + s).tobytes()
    # the order matters: a sum that pairs the partials differently has other bits
    parts = np.array([1.0, 2.0 ** -24, 2.0 ** -24, -1.0], dtype=np.float32)
    assert vr.colsum_finish(parts) == 0.0 and np.float32(np.float32(parts[0] + parts[3]) + np.float32(parts[1] + parts[2])) != 0.0


def test_the_float32_table_of_the_gpu_suite_is_its_own_measurement():
    """F32 of tests/test_vdb_kernels_gpu.py (the elementwise bounds are 8 x these) is measure_f32() to two digits as measured
    where the table was written.  Several figures are decided by a single rounding of a case of one to five rows, so
    another CPU or exp() may measure a little more or less: a figure is at most 1.2 times the measurement made here and at
    least half of it."""
    got = tv.measure_f32()
    assert sorted(got) == sorted(tv.F32)
    for k, v in got.items():
        assert 0.5 * v <= tv.F32[k] <= 1.2 * v, (k, v, tv.F32[k])
        assert tv.bound(k) == 8.0 * tv.F32[k] < tv.GTOL
