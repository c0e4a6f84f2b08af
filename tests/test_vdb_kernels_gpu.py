"""Every entry point of csrc/vdb.hip on its own, against the float64 statement of tests/vdb_ref.py, at each grid regime, latent
width and row pitch, with proof of which kernels ran.

Regimes (tests/vdb_ref.py mirrors each grid; a case's id names the regime it reaches):
 * vdb_head_fwd_kernel: min(64, ceil(N / 4)) blocks, a row per wave -- N = 1, 4 | 5 (one block | two), 256 | 257 (64 blocks
   without | with the row stride 4 * grid), 2500 (the workload: ten strides);
 * vdb_loss_kernel, vdb_tau_kernel: min(64, ceil(N / 256)) -- 1, 256 | 257 (the ticket with one | two blocks), 16384 | 16385
   (64 blocks without | with the stride);
 * vdb_gp_norm_kernel: min(64, ceil(n / 4096)) -- 1, 4096 | 4097, 262144 | 262145;
 * vdb_colsum_kernel<GP>: G = min(64, ceil(N / 32)) blocks of rpb = ceil(N / G) rows -- 1, 3 (fewer rows than waves),
   32 | 33 (G = 1 | 2), 2048 | 2049 (rpb = 32 | 33, block 63 left without rows), 2500 (rpb = 40, block 62 has 20 rows, 63 none);
 * vdb_gp_delta_kernel: min(2048, ceil(N Z / 256)) -- (1, 1), (37, 5), (4096, 128) | (4097, 128) (2048 blocks without | with
   the stride), and strided with a Z that does not divide the stride 2048 * 256: (104858, 5), (8067, 65), (4097, 130).  At
   Z = 128 a thread meets the same column j on every pass, so a kernel that carried j, fc_w[j] or the row across passes
   instead of recomputing them from the element index would show only there.  This kernel leaves no partials: its
   block count is mirrored (vr.gp_delta_blocks) to place the cases, and cannot be pinned by counting.
Z = 1, 5, 63, 64, 65, 130 (one lane, a partial wave, 63 | 64 | 65 around the wave, and three 64-column slabs: the second
pass of the forward's lane loop and the column-sum kernel's later `jb` slabs, where the dfc_b partial is not rewritten)
run at one N below and one above each kernel's cap; Z = 64 everywhere else.  Every pitched operand also runs as a view
into a wider, sentinel-filled buffer (ldz = 2Z + 3, lda5 = 2Z + 1, lddz = 2Z + 5, lddelta = 2Z + 2): the results have the
bits of the contiguous call and the pad columns, of inputs and outputs alike, keep the sentinel.

Checks.  The four ticketed reductions (the forward's KL, loss, gp_norm, tau) go through
tests.test_reductions_gpu.reduction(): exactly nvals x blocks finite partials after a NaN fill (which pins the mirrored
block count), the ticket word back at 0, the output = reduce_ref.fixed_order_sum of its partials bit for bit, every output
finite, no final_sum_kernel.  The two column-sum entry points: exactly (Z + 1) G (Z G for gp_head) finite floats in the
NaN-filled scratch at parts[v][b], dfc_w[j] / dfc_b[0] = vdb_ref.colsum_finish of their row bit for bit (prev + s when
accumulating), the scratch untouched and no finish kernel when no sums are asked for.

Values.  Sums: |got - sum terms| <= FTOL * sum |terms| (FTOL = 1e-5, the project's figure).  Elementwise outputs: l2err <=
min(GTOL, 8 x F32[output]), F32 = the l2 error of tests/vdb_ref.py run in float32 on the CPU against its float64 self on
the same inputs, the largest over the output's cases (`measure_f32()` below recomputes the table; tests/test_vdb_ref_cpu.py
holds the table to it).  The factor 8 covers the device's expf / log1pf being a couple of ulp off the CPU's, and FMA
contraction.  Measured:

    output     cases                                           F32
    lat        HEAD_CASES                                      7.7e-08
    d          HEAD_CASES                                      1.7e-07
    dd         LOSS_NS x the five modes                        9.7e-08
    dd (edge)  EDGE_D x the five modes                         3.1e-08
    dz         COL_CASES                                       1.1e-07
    extra      COL_CASES                                       7.8e-08
    delta5     DELTA_CASES                                     4.8e-08
    g          NORM_NS                                         2.6e-08
    tau_out    LOSS_NS                                         2.6e-08
    dlt        LOSS_NS                                         5.4e-08

(the largest figure of lat, d, dd and dz comes from a case of one to five rows, where a single rounding decides it; the
cases of 2000 rows and more measure 4.0e-08, 8.4e-08, 5.0e-08 and 4.5e-08), so every bound is below 1.4e-6 and GTOL = 1e-4
never binds.  repo_vdb_beta_step: 1e-6 relative (a handful of float32 operations on O(1) values).  Bitwise assertions carry no tolerance."""
import numpy as np
import pytest
import torch

from tests import reduce_ref as rr
from tests import vdb_ref as vr
from tests.test_reductions_gpu import F32 as f32, FTOL, GTOL, _tensors, dev, header_word, reduction, same_bits, sum_err
from tests.util import has, l2err, log, rnd, traced

pytestmark = pytest.mark.gpu

SENT = -12345.0
ZS = [1, 5, 63, 64, 65, 130]
NOT64 = [z for z in ZS if z != 64]
HEAD_CASES = [(n, 64) for n in (1, 4, 5, 256, 257, 2500)] + [(n, z) for n in (5, 257) for z in NOT64]
LOSS_NS = [1, 256, 257, 16384, 16385]
NORM_NS = [1, 4096, 4097, 262144, 262145]
COL_CASES = [(n, 64) for n in (1, 3, 32, 33, 2048, 2049, 2500)] + [(n, z) for n in (3, 2049) for z in NOT64] + [(2500, 130)]
DELTA_CASES = ([(1, 1), (37, 5), (4096, 128), (4097, 128)] + [(37, z) for z in (1, 63, 64, 65, 130)]
               + [(104858, 5), (8067, 65), (4097, 130)])
MODES = [vr.BCE0, vr.BCE1, vr.NEG_TAU, vr.CHI, vr.NEG_CHI]
MODE_NAMES = ["bce0", "bce1", "neg_tau", "chi", "neg_chi"]
EDGE_D = [0.0, 1e-4, -1e-4, 20.0, -20.0, 88.0, -88.0, 100.0, -100.0, 1e4, -1e4]
GSCALE = f32(1.0 / 37)
EDGE_TOL = 8 * 2.0 ** -24      # test_loss_edge_values
NORM_SCALE = f32(2.0 / 37)

# the table of the module docstring: output -> l2 error of the float32 CPU statement against float64 (measure_f32())
F32 = {"lat": 7.7e-08, "d": 1.7e-07, "dd": 9.7e-08, "dd_edge": 3.1e-08, "dz": 1.1e-07, "extra": 7.8e-08, "delta5": 4.8e-08,
       "g": 2.6e-08, "tau_out": 2.6e-08, "dlt": 5.4e-08}


def bound(name):
    return min(GTOL, 8.0 * F32[name])


# --------------------------------------------------------------------------------------------------------------- inputs
def head_inputs(N, Z):
    """mean ~ N(0, 1), logstd ~ 0.5 N(0, 1) with elements at -20 and +5, eps, fc_w ~ N(0, 1), fc_b: float32, seeded."""
    rs = np.random.RandomState(1000 * Z + N)
    mean, ls = rnd(rs, N, Z), rnd(rs, N, Z, scale=0.5)
    flat, n = ls.view(-1), N * Z
    flat[0] = -20.0
    if n > 1:
        flat[n - 1] = 5.0
    if n > 8:
        flat[n // 3], flat[n // 2] = 5.0, -20.0
    return torch.cat((mean, ls), 1).contiguous(), rnd(rs, N, Z), rnd(rs, Z), rnd(rs, 1)


def bwd_inputs(N, Z):
    """The upstreams of the two reverse kernels: dd (N), beta (1), kl_coef, extra (N, Z), a5 (N, 2Z)."""
    rs = np.random.RandomState(7000 * Z + N)
    return rnd(rs, N), torch.tensor([0.37], dtype=torch.float32), f32(0.5 / N), rnd(rs, N, Z), rnd(rs, N, 2 * Z)


def loss_inputs(N):
    """d ~ N(0, 2), tau = exp(0.3 N(0, 1))."""
    rs = np.random.RandomState(N)
    return rnd(rs, N, scale=2.0), torch.exp(0.3 * rnd(rs, N))


def tau_inputs(N):
    rs = np.random.RandomState(N + 5)
    return rnd(rs, N, scale=0.5), rnd(rs, N, scale=2.0), torch.tensor([0.3], dtype=torch.float32)


def norm_inputs(n):
    return rnd(np.random.RandomState(n), n, scale=3.0)


def measure_f32():
    """The table F32, recomputed: tests/vdb_ref.py in float32 on the CPU against its float64 self, per output the largest
    l2 error over the output's cases.  `lat` of the reverse kernels is the float32 forward's, on both sides."""
    out = {k: 0.0 for k in F32}

    def put(name, got, want):
        out[name] = max(out[name], l2err(got, want))

    h = torch.float32
    for N, Z in HEAD_CASES:
        a = head_inputs(N, Z)
        lo, hi = vr.head_fwd(*a, dtype=h), vr.head_fwd(*a)
        put("lat", lo[0], hi[0])
        put("d", lo[1], hi[1])
    for N, Z in COL_CASES:
        z, eps, w, b = head_inputs(N, Z)
        dd, beta, klc, extra, a5 = bwd_inputs(N, Z)
        lat = vr.head_fwd(z, eps, w, b, dtype=h)[0]
        put("dz", vr.head_bwd(z, eps, lat, w, dd, beta, klc, extra, dtype=h)[0], vr.head_bwd(z, eps, lat, w, dd, beta, klc, extra)[0])
        put("extra", vr.gp_head(a5, z, eps, lat, w, dtype=h)[0], vr.gp_head(a5, z, eps, lat, w)[0])
    for N, Z in DELTA_CASES:
        z, eps, w, b = head_inputs(N, Z)
        lat = vr.head_fwd(z, eps, w, b, dtype=h)[0]
        put("delta5", vr.gp_delta(z, eps, lat, w, dtype=h), vr.gp_delta(z, eps, lat, w))
    for N in LOSS_NS:
        d, tau = loss_inputs(N)
        for m in MODES:
            put("dd", vr.loss(d, m, tau, GSCALE, dtype=h)[1], vr.loss(d, m, tau, GSCALE)[1])
        lt, dv, u = tau_inputs(N)
        lo, hi = vr.tau(lt, dv, u, dtype=h), vr.tau(lt, dv, u)
        put("tau_out", lo[2], hi[2])
        put("dlt", lo[3], hi[3])
    d = torch.tensor(EDGE_D, dtype=torch.float32)
    tau = loss_inputs(len(EDGE_D))[1]
    for m in MODES:
        put("dd_edge", vr.loss(d, m, tau, GSCALE, dtype=h)[1], vr.loss(d, m, tau, GSCALE)[1])
    for n in NORM_NS:
        g = norm_inputs(n)
        put("g", vr.gp_norm(g, NORM_SCALE, dtype=h)[1], vr.gp_norm(g, NORM_SCALE)[1])
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


def device():
    return torch.device("cuda", torch.cuda.current_device())


def pitched(t, ld):
    """(the wide sentinel-filled buffer, its view holding t): a (rows, cols) operand with row pitch ld."""
    rows, cols = t.shape
    wide = torch.full((rows, ld), SENT, dtype=torch.float32, device="cuda")
    wide[:, :cols] = t.cuda()
    return wide, wide[:, :cols]


def pads_kept(wide, cols):
    return bool((wide[:, cols:] == SENT).all())


def red_area(ops):
    """The partial area of the current stream's reduction workspace, NaN-filled."""
    ws = ops.reduce_ws(device())
    area = ws[rr.RED_HEADER_BYTES:].view(torch.float32)
    area.fill_(float("nan"))
    return ws, area


def colsum_area(ops, Z):
    """The current stream's scratch as floats, NaN-filled; fetched BEFORE the call so that the call is served from it."""
    ws = ops.workspace(ops.lib().repo_vdb_colsum_workspace_bytes(Z), device())
    area = ws[:ws.numel() // 4 * 4].view(torch.float32)
    area.fill_(float("nan"))
    return area


def colsum_parts(area, nv, G, what):
    """Exactly nv x G finite floats, at parts[v][b] with pitch G: -> the (nv, G) float32 array."""
    finite = torch.isfinite(area)
    k = nv * G
    assert bool(finite[:k].all()) and not bool(finite[k:].any()), (what, "finite partials", int(finite.sum()), "expected", k)
    return area[:k].cpu().view(nv, G).numpy()


def finish_bits(parts, prev=None):
    """vdb_colsum_finish_kernel on every row of `parts` as a float32 tensor."""
    rows = [vr.colsum_finish(parts[v], None if prev is None else prev[v]) for v in range(parts.shape[0])]
    return torch.from_numpy(np.array(rows, dtype=np.float32))


def col_err(got, terms):
    """The largest sum_err over the columns of a (N, Z) block of terms."""
    got = got.detach().cpu().reshape(-1)
    terms = terms.reshape(terms.shape[0], -1)
    return max(sum_err(got[j].item(), terms[:, j]) for j in range(terms.shape[1]))


def all_same(a, b):
    a, b = list(_tensors(a)), list(_tensors(b))
    return len(a) == len(b) and all(same_bits(x, y) for x, y in zip(a, b))


def regime(blocks, work, per_block, cap=vr.LAST_BLOCK_MAX_GRID):
    return f"{blocks}blk" + ("-strided" if work > cap * per_block else "")


def col_id(N, Z):
    G, rpb = vr.colsum_grid(N)
    return f"N{N}-Z{Z}-G{G}-rpb{rpb}-last{vr.colsum_rows(N, G - 1)}rows"


HEAD_IDS = [f"N{n}-Z{z}-{regime(vr.head_fwd_blocks(n), n, 4)}" for n, z in HEAD_CASES]
COL_IDS = [col_id(n, z) for n, z in COL_CASES]
DELTA_IDS = [f"N{n}-Z{z}-{regime(vr.gp_delta_blocks(n, z), n * z, 256, 2048)}" for n, z in DELTA_CASES]


# ------------------------------------------------------------------------------------------------------------- head_fwd
@pytest.mark.parametrize("N,Z", HEAD_CASES, ids=HEAD_IDS)
def test_head_fwd_at_each_grid_regime_and_width(ops, N, Z):
    """lat, d and the KL sum; the row stride 4 * grid above N = 256; the second pass of the lane loop above Z = 64;
    z as a view with ldz = 2Z + 3; want_kl=False leaves the partial area alone."""
    blocks = vr.head_fwd_blocks(N)
    z, eps, w, b = head_inputs(N, Z)
    lat64, d64, kl_rows = vr.head_fwd(z, eps, w, b)
    zd, ed, wd, bd = dev(z), dev(eps), dev(w), dev(b)
    what = f"head_fwd N={N} Z={Z} {regime(blocks, N, 4)}"
    (lat, d, kl), _ = reduction(ops, lambda: ops.vdb_head_fwd(zd, wd, bd, eps=ed), lambda r: r[2], "vdb_head_fwd_kernel", blocks, 1,
                                what)
    e, el, ed_ = sum_err(kl.item(), kl_rows), l2err(lat, lat64), l2err(d, d64)
    log(f"{what}: kl {e:.2e}; l2 lat {el:.2e} (bound {bound('lat'):.1e}) d {ed_:.2e} (bound {bound('d'):.1e})")
    assert e <= FTOL, (what, e)
    assert el <= bound("lat") and ed_ <= bound("d"), (what, el, ed_)
    # ldz = 2Z + 3: the same bits, through the same checks
    wide, zv = pitched(z, 2 * Z + 3)
    assert zv.stride(0) == 2 * Z + 3 or N == 1
    res_p, _ = reduction(ops, lambda: ops.vdb_head_fwd(zv, wd, bd, eps=ed), lambda r: r[2], "vdb_head_fwd_kernel", blocks, 1,
                         what + " ldz=2Z+3")
    assert all_same(res_p, (lat, d, kl)) and pads_kept(wide, 2 * Z), what
    # without the KL: no partial is written, lat and d keep their bits
    ws, area = red_area(ops)
    lat2, d2, none = ops.vdb_head_fwd(zd, wd, bd, eps=ed, want_kl=False)
    torch.cuda.synchronize()
    assert none is None and same_bits(lat2, lat) and same_bits(d2, d), what
    assert bool(torch.isnan(area).all()) and header_word(ws) == 0, what
    assert all_same(ops.vdb_head_fwd(zd, wd, bd, eps=ed), (lat, d, kl)), (what, "two calls differ")


# ----------------------------------------------------------------------------------------------------------------- loss
@pytest.mark.parametrize("mode", MODES, ids=MODE_NAMES)
@pytest.mark.parametrize("N", LOSS_NS, ids=[f"N{n}-{regime(vr.loss_blocks(n), n, 256)}" for n in LOSS_NS])
def test_loss_at_each_grid_regime(ops, N, mode):
    """One block, the ticket with two blocks (257), 64 blocks, and the strided loop (16385), for the five losses."""
    blocks = vr.loss_blocks(N)
    d, tau = loss_inputs(N)
    terms, dd64 = vr.loss(d, mode, tau, GSCALE)
    dd_, td = dev(d), dev(tau) if mode == vr.NEG_TAU else None
    what = f"loss {MODE_NAMES[mode]} N={N} {regime(blocks, N, 256)}"
    (s, dd), _ = reduction(ops, lambda: ops.vdb_loss(dd_, mode, GSCALE, tau=td), lambda r: r[0], "vdb_loss_kernel", blocks, 1, what)
    e, eg = sum_err(s.item(), terms), l2err(dd, dd64)
    log(f"{what}: sum {e:.2e}; l2 dd {eg:.2e} (bound {bound('dd'):.1e})")
    assert e <= FTOL and eg <= bound("dd"), (what, e, eg)
    (s2, none), _ = reduction(ops, lambda: ops.vdb_loss(dd_, mode, GSCALE, tau=td, want_grad=False), lambda r: r[0],
                              "vdb_loss_kernel", blocks, 1, what + " no grad")
    assert none is None and same_bits(s2, s), what
    assert all_same(ops.vdb_loss(dd_, mode, GSCALE, tau=td), (s, dd)), (what, "two calls differ")


@pytest.mark.parametrize("mode", MODES, ids=MODE_NAMES)
def test_loss_edge_values(ops, mode):
    """d = 0, +-1e-4, +-20, +-88, +-100, +-1e4: expf overflows in the sigmoid's denominator at -100 and -1e4, and the
    log1pf(expf(-|x|)) form of softplus must not.  Judged by its own sum, by l2err(dd), and element by element:
    |dd - dd64| <= EDGE_TOL * max(|dd64|, gscale) with EDGE_TOL = 8 * 2^-24.  A rounding is 2^-24 relative.  The sigmoid is
    s = 1 / (1 + e), e = expf(-x) taken within 2 ulp = 4 roundings, whose error reaches s scaled by e / (1 + e) <= 1; the sum
    and the quotient round once each, s - t at most once (s <= 1), the product with gscale once: 8 roundings of a quantity
    of size at most max(|dd|, gscale).  Where expf overflows or underflows s is exactly 0 or 1, and where s - 1 cancels
    (x = 20: -2e-9) the error is an absolute one of the size of s = 1, hence the floor at gscale.  The other three modes
    take three roundings (1 + x / 2, the sign is exact, gscale; -tau gscale one)."""
    d = torch.tensor(EDGE_D, dtype=torch.float32)
    tau = loss_inputs(len(EDGE_D))[1]
    terms, dd64 = vr.loss(d, mode, tau, GSCALE)
    what = f"loss edge values {MODE_NAMES[mode]}"
    (s, dd), _ = reduction(ops, lambda: ops.vdb_loss(dev(d), mode, GSCALE, tau=dev(tau) if mode == vr.NEG_TAU else None),
                           lambda r: r[0], "vdb_loss_kernel", 1, 1, what)
    e, eg = sum_err(s.item(), terms), l2err(dd, dd64)
    each = (dd.double().cpu() - dd64).abs() / dd64.abs().clamp_min(GSCALE)
    log(f"{what}: sum {e:.2e}; l2 dd {eg:.2e} (bound {bound('dd_edge'):.1e}); per element, relative to max(|dd64|, gscale): "
        + " ".join(f"{x:.1e}" for x in each.tolist()) + f" (bound {EDGE_TOL:.1e})")
    assert e <= FTOL and eg <= bound("dd_edge"), (what, e, eg)
    assert bool((each <= EDGE_TOL).all()), (what, each.tolist())


# ------------------------------------------------------------------------------------------------------------------ tau
@pytest.mark.parametrize("N", LOSS_NS, ids=[f"N{n}-{regime(vr.loss_blocks(n), n, 256)}" for n in LOSS_NS])
def test_tau_at_each_grid_regime_and_optional_operands(ops, N):
    blocks = vr.loss_blocks(N)
    lt, dv, u = tau_inputs(N)
    ltd, dvd, ud = dev(lt), dev(dv), dev(u)
    what = f"tau N={N} {regime(blocks, N, 256)}"

    def run(tag, **kw):
        return reduction(ops, lambda: ops.vdb_tau(ltd, **kw), lambda r: r[0], "vdb_tau_kernel", blocks, 2, f"{what} {tag}")[0]

    t0, t1, tau64, dlt64 = vr.tau(lt, dv, u)
    sums, tau, dlt = run("all", d=dvd, u=ud, want_tau=True, want_grad=True)
    e0, e1, et, eg = sum_err(sums[0].item(), t0), sum_err(sums[1].item(), t1), l2err(tau, tau64), l2err(dlt, dlt64)
    log(f"{what}: sums {e0:.2e} {e1:.2e}; l2 tau {et:.2e} (bound {bound('tau_out'):.1e}) dlt {eg:.2e} (bound {bound('dlt'):.1e})")
    assert e0 <= FTOL and e1 <= FTOL and et <= bound("tau_out") and eg <= bound("dlt"), (what, e0, e1, et, eg)
    assert all_same(ops.vdb_tau(ltd, d=dvd, u=ud, want_tau=True, want_grad=True), (sums, tau, dlt)), (what, "two calls differ")
    # each output off: the others keep their bits
    s_a, tau_a, none = run("no grad", d=dvd, u=ud, want_tau=True)
    assert none is None and same_bits(s_a, sums) and same_bits(tau_a, tau)
    s_b, none, dlt_b = run("no tau", d=dvd, u=ud, want_grad=True)
    assert none is None and same_bits(s_b, sums) and same_bits(dlt_b, dlt)
    # u == NULL: dlt = tau d / N
    s_u, _, dlt_u = run("u=None", d=dvd, want_grad=True)
    eu = l2err(dlt_u, vr.tau(lt, dv, None)[3])
    assert same_bits(s_u, sums) and eu <= bound("dlt"), (what, eu)
    # d == NULL: sums[0] = 0 exactly, sums[1] and tau as before, dlt = tau u / N
    s_d, tau_d, dlt_d = run("d=None", u=ud, want_tau=True, want_grad=True)
    ed = l2err(dlt_d, vr.tau(lt, None, u)[3])
    log(f"{what}: u=None l2 dlt {eu:.2e}; d=None l2 dlt {ed:.2e}")
    assert s_d[0].item() == 0.0 and same_bits(s_d[1], sums[1]) and same_bits(tau_d, tau) and ed <= bound("dlt"), (what, ed)


# -------------------------------------------------------------------------------------------------------------- gp_norm
@pytest.mark.parametrize("n", NORM_NS, ids=[f"n{n}-{regime(vr.gp_norm_blocks(n), n, 4096)}" for n in NORM_NS])
def test_gp_norm_at_each_grid_regime(ops, n):
    blocks = vr.gp_norm_blocks(n)
    g = norm_inputs(n)
    terms, scaled = vr.gp_norm(g, NORM_SCALE)
    what = f"gp_norm n={n} {regime(blocks, n, 4096)}"
    bufs = [dev(g), dev(g)]
    (sq, _), _ = reduction(ops, lambda: (ops.vdb_gp_norm(bufs[0], NORM_SCALE), bufs[0]), lambda r: r[0], "vdb_gp_norm_kernel",
                           blocks, 1, what)
    e, eg = sum_err(sq.item(), terms), l2err(bufs[0], scaled)
    log(f"{what}: sum {e:.2e}; l2 scaled g {eg:.2e} (bound {bound('g'):.1e})")
    assert e <= FTOL and eg <= bound("g"), (what, e, eg)
    sq2 = ops.vdb_gp_norm(bufs[1], NORM_SCALE)
    assert same_bits(sq2, sq) and same_bits(bufs[1], bufs[0]), (what, "two calls differ")


# ------------------------------------------------------------------------------------------------------------ head_bwd
def forward_lat(ops, zd, ed, wd, bd):
    """The reverse kernels are given the forward's own lat."""
    return ops.vdb_head_fwd(zd, wd, bd, eps=ed, want_kl=False)[0]


@pytest.mark.parametrize("N,Z", COL_CASES, ids=COL_IDS)
def test_head_bwd_at_each_grid_regime_and_width(ops, N, Z):
    """dz and the column sums dfc_w, dfc_b: fewer rows than waves, G = 1 | 2, rpb = 32 | 33 with an empty last block, the
    workload's N = 2500; the later 64-column slabs above Z = 64; accumulation; a frozen head (no sums); ldz = 2Z + 3 and
    lddz = 2Z + 5."""
    G, rpb = vr.colsum_grid(N)
    z, eps, w, b = head_inputs(N, Z)
    dd, beta, klc, extra, _ = bwd_inputs(N, Z)
    zd, ed, wd, bd, ddd, betad, exd = (dev(t) for t in (z, eps, w, b, dd, beta, extra))
    lat = forward_lat(ops, zd, ed, wd, bd)
    dz64, tw, tb = vr.head_bwd(z, eps, lat.cpu(), w, dd, beta, klc, extra)
    what = f"head_bwd {col_id(N, Z)}"
    area = colsum_area(ops, Z)

    def call(zv=zd, sums=True, prev=None, out=None):
        dw = None if not sums else torch.empty(Z, device="cuda") if prev is None else dev(prev[:Z])
        db = None if not sums else torch.empty(1, device="cuda") if prev is None else dev(prev[Z:])
        dz = ops.vdb_head_bwd(zv, lat, wd, ddd, eps=ed, beta=betad, kl_coef=klc, extra=exd, dfc_w=dw, dfc_b=db,
                              accumulate=prev is not None, out=out)
        return dz, dw, db

    (dz, dw, db), names = traced(call)
    assert has(names, r"vdb_colsum_kernel<false>") and has(names, r"\bvdb_colsum_finish_kernel\b"), (what, names)
    assert not has(names, r"vdb_colsum_kernel<true>"), (what, names)
    parts = colsum_parts(area, Z + 1, G, what)
    want = finish_bits(parts)
    assert torch.equal(dw.cpu(), want[:Z]) and torch.equal(db.cpu(), want[Z:]), (what, "not the in-order sum of its partials")
    assert bool(torch.isfinite(dz).all()), (what, "an element of dz was left unwritten")
    ez, ew, eb = l2err(dz, dz64), col_err(dw, tw), sum_err(db.item(), tb)
    log(f"{what}: l2 dz {ez:.2e} (bound {bound('dz'):.1e}); dfc_w {ew:.2e} dfc_b {eb:.2e}")
    assert ez <= bound("dz") and ew <= FTOL and eb <= FTOL, (what, ez, ew, eb)
    # accumulate: prev + s, from the same partials
    prev = rnd(np.random.RandomState(N + Z), Z + 1)
    area.fill_(float("nan"))
    dz_a, dw_a, db_a = call(prev=prev)
    parts_a = colsum_parts(area, Z + 1, G, what + " accumulate")
    assert np.array_equal(parts_a.view(np.int32), parts.view(np.int32)), what
    want_a = finish_bits(parts, prev.numpy())
    assert torch.equal(dw_a.cpu(), want_a[:Z]) and torch.equal(db_a.cpu(), want_a[Z:]) and same_bits(dz_a, dz), what
    # a frozen head: no sums, the scratch untouched, no finish kernel, dz as before
    area.fill_(float("nan"))
    (dz_f, _, _), names = traced(lambda: call(sums=False))
    assert bool(torch.isnan(area).all()), (what, "the scratch was written without sums")
    assert has(names, r"vdb_colsum_kernel<false>") and not has(names, r"\bvdb_colsum_finish_kernel\b"), (what, names)
    assert same_bits(dz_f, dz), what
    # ldz = 2Z + 3, lddz = 2Z + 5
    zwide, zv = pitched(z, 2 * Z + 3)
    owide = torch.full((N, 2 * Z + 5), SENT, device="cuda")
    dz_p, dw_p, db_p = call(zv=zv, out=owide[:, :2 * Z])
    assert dz_p.data_ptr() == owide.data_ptr() and same_bits(dz_p, dz) and same_bits(dw_p, dw) and same_bits(db_p, db), what
    assert pads_kept(owide, 2 * Z) and pads_kept(zwide, 2 * Z), (what, "pad columns of dz or z were written")


def test_head_bwd_optional_operands(ops):
    """beta == NULL is c = 0 (against the reference with kl_coef = 0, and the bits of beta given with kl_coef = 0);
    extra == NULL is an all-zero extra bit for bit."""
    N, Z = 300, 65
    z, eps, w, b = head_inputs(N, Z)
    dd, beta, klc, extra, _ = bwd_inputs(N, Z)
    zd, ed, wd, bd, ddd, betad, exd = (dev(t) for t in (z, eps, w, b, dd, beta, extra))
    lat = forward_lat(ops, zd, ed, wd, bd)

    def call(**kw):
        dw, db = torch.empty(Z, device="cuda"), torch.empty(1, device="cuda")
        return ops.vdb_head_bwd(zd, lat, wd, ddd, eps=ed, dfc_w=dw, dfc_b=db, **kw), dw, db

    no_beta = call(extra=exd)
    e = l2err(no_beta[0], vr.head_bwd(z, eps, lat.cpu(), w, dd, None, 0.0, extra)[0])
    assert all_same(no_beta, call(beta=betad, kl_coef=0.0, extra=exd))
    no_extra = call(beta=betad, kl_coef=klc)
    e2 = l2err(no_extra[0], vr.head_bwd(z, eps, lat.cpu(), w, dd, beta, klc, None)[0])
    assert all_same(no_extra, call(beta=betad, kl_coef=klc, extra=torch.zeros(N, Z, device="cuda")))
    log(f"head_bwd N={N} Z={Z}: beta=None l2 dz {e:.2e}; extra=None l2 dz {e2:.2e} (bound {bound('dz'):.1e})")
    assert e <= bound("dz") and e2 <= bound("dz"), (e, e2)
    assert not same_bits(no_beta[0], no_extra[0])


# ------------------------------------------------------------------------------------------------------------- gp_head
@pytest.mark.parametrize("N,Z", COL_CASES, ids=COL_IDS)
def test_gp_head_at_each_grid_regime_and_width(ops, N, Z):
    """extra and the column sum dfc_w of the penalty's head end, accumulate = 0 and 1, a5 and z as views (lda5 = 2Z + 1,
    ldz = 2Z + 3)."""
    G, rpb = vr.colsum_grid(N)
    z, eps, w, b = head_inputs(N, Z)
    a5 = bwd_inputs(N, Z)[4]
    zd, ed, wd, bd, ad = (dev(t) for t in (z, eps, w, b, a5))
    lat = forward_lat(ops, zd, ed, wd, bd)
    ex64, tw = vr.gp_head(a5, z, eps, lat.cpu(), w)
    what = f"gp_head {col_id(N, Z)}"
    area = colsum_area(ops, Z)

    def call(av=ad, zv=zd, prev=None):
        dw = torch.empty(Z, device="cuda") if prev is None else dev(prev)
        return ops.vdb_gp_head(av, zv, lat, wd, dw, eps=ed, accumulate=prev is not None), dw

    (ex, dw), names = traced(call)
    assert has(names, r"vdb_colsum_kernel<true>") and has(names, r"\bvdb_colsum_finish_kernel\b"), (what, names)
    assert not has(names, r"vdb_colsum_kernel<false>"), (what, names)
    parts = colsum_parts(area, Z, G, what)
    assert torch.equal(dw.cpu(), finish_bits(parts)), (what, "not the in-order sum of its partials")
    assert bool(torch.isfinite(ex).all()), (what, "an element of extra was left unwritten")
    ee, ew = l2err(ex, ex64), col_err(dw, tw)
    log(f"{what}: l2 extra {ee:.2e} (bound {bound('extra'):.1e}); dfc_w {ew:.2e}")
    assert ee <= bound("extra") and ew <= FTOL, (what, ee, ew)
    prev = rnd(np.random.RandomState(N + Z + 1), Z)
    area.fill_(float("nan"))
    ex_a, dw_a = call(prev=prev)
    parts_a = colsum_parts(area, Z, G, what + " accumulate")
    assert np.array_equal(parts_a.view(np.int32), parts.view(np.int32)), what
    assert torch.equal(dw_a.cpu(), finish_bits(parts, prev.numpy())) and same_bits(ex_a, ex), what
    awide, av = pitched(a5, 2 * Z + 1)
    zwide, zv = pitched(z, 2 * Z + 3)
    assert all_same(call(av=av, zv=zv), (ex, dw)), (what, "pitched operands")
    assert pads_kept(awide, 2 * Z) and pads_kept(zwide, 2 * Z), (what, "pad columns of a5 or z were written")


# ------------------------------------------------------------------------------------------------------------ gp_delta
@pytest.mark.parametrize("N,Z", DELTA_CASES, ids=DELTA_IDS)
def test_gp_delta_at_each_grid_regime_and_width(ops, N, Z):
    """(4096, 128) fills the 2048-block cap, (4097, 128) strides with the same column on every pass of a thread, the last
    three cases stride with another column on each pass; ldz = 2Z + 3, lddelta = 2Z + 2."""
    blocks = vr.gp_delta_blocks(N, Z)
    z, eps, w, b = head_inputs(N, Z)
    zd, ed, wd, bd = dev(z), dev(eps), dev(w), dev(b)
    lat = forward_lat(ops, zd, ed, wd, bd)
    what = f"gp_delta N={N} Z={Z} {regime(blocks, N * Z, 256, 2048)}"
    out, names = traced(lambda: ops.vdb_gp_delta(zd, lat, wd, eps=ed))
    assert has(names, r"\bvdb_gp_delta_kernel\b"), (what, names)
    assert bool(torch.isfinite(out).all()), (what, "an element of delta5 was left unwritten")
    e = l2err(out, vr.gp_delta(z, eps, lat.cpu(), w))
    log(f"{what}: l2 delta5 {e:.2e} (bound {bound('delta5'):.1e})")
    assert e <= bound("delta5"), (what, e)
    zwide, zv = pitched(z, 2 * Z + 3)
    owide = torch.full((N, 2 * Z + 2), SENT, device="cuda")
    out_p = ops.vdb_gp_delta(zv, lat, wd, eps=ed, out=owide[:, :2 * Z])
    assert out_p.data_ptr() == owide.data_ptr() and same_bits(out_p, out), what
    assert pads_kept(owide, 2 * Z) and pads_kept(zwide, 2 * Z), (what, "pad columns of delta5 or z were written")
    assert same_bits(ops.vdb_gp_delta(zd, lat, wd, eps=ed), out), (what, "two calls differ")


# ------------------------------------------------------------------------------------------------------- in-kernel noise
@pytest.mark.parametrize("offset", [0, 1, 2, 3, 2 ** 32 + 5])
@pytest.mark.parametrize("N,Z", [(37, 5), (300, 65), (8067, 65)])
def test_in_kernel_noise_is_the_explicit_tensor(ops, N, Z, offset):
    """eps == NULL draws element n Z + j as normal number offset + n Z + j of the Philox stream: the four lanes of a counter
    block and a carry into the high counter word.  The forward and its three reverse consumers give the bits of the same
    call on the materialised normals.  (8067, 65) is gp_delta's strided regime."""
    seed = 20250 + Z
    z, _, w, b = head_inputs(N, Z)
    dd, beta, klc, extra, a5 = bwd_inputs(N, Z)
    zd, wd, bd, ddd, betad, exd, ad = (dev(t) for t in (z, w, b, dd, beta, extra, a5))
    eps = ops.philox_normal(N * Z, seed, offset, "cuda").view(N, Z)
    how = [dict(eps=eps), dict(eps=None, noise=(seed, offset))]
    fwd = [ops.vdb_head_fwd(zd, wd, bd, **kw) for kw in how]
    assert all_same(fwd[0], fwd[1]), "head_fwd"
    lat = fwd[0][0]

    def bwd(kw):
        dw, db = torch.empty(Z, device="cuda"), torch.empty(1, device="cuda")
        return ops.vdb_head_bwd(zd, lat, wd, ddd, beta=betad, kl_coef=klc, extra=exd, dfc_w=dw, dfc_b=db, **kw), dw, db

    def gph(kw):
        dw = torch.empty(Z, device="cuda")
        return ops.vdb_gp_head(ad, zd, lat, wd, dw, **kw), dw

    assert all_same(bwd(how[0]), bwd(how[1])), "head_bwd"
    assert all_same(ops.vdb_gp_delta(zd, lat, wd, **how[0]), ops.vdb_gp_delta(zd, lat, wd, **how[1])), "gp_delta"
    assert all_same(gph(how[0]), gph(how[1])), "gp_head"
    # the noise matters: another offset gives other bits
    assert not same_bits(ops.vdb_head_fwd(zd, wd, bd, noise=(seed, offset + 1))[0], lat)
    log(f"in-kernel noise N={N} Z={Z} offset={offset}: head_fwd, head_bwd, gp_delta, gp_head bit-equal to the explicit tensor")


# ------------------------------------------------------------------------------------------------------------ beta_step
@pytest.mark.parametrize("beta0,klr,klf,lr", [(0.1, 40.0, 25.0, 5e-3), (0.1, 1.5, 0.75, 5e-3), (0.001, 1.5, 0.75, 0.5)],
                         ids=["kl-above-target", "kl-below-target", "clamped-at-0"])
def test_beta_step(ops, beta0, klr, klf, lr):
    n_real, n_fake, target = 37, 41, 0.1
    lr32, target32 = f32(lr), f32(target)
    kr, kf = torch.tensor([klr], device="cuda"), torch.tensor([klf], device="cuda")
    want, kl = vr.beta_step(f32(beta0), kr.item(), n_real, kf.item(), n_fake, lr32, target32)
    assert (kl > target) == (klr == 40.0) and (want == 0.0) == (lr == 0.5)
    got = []
    for with_kl in (True, False, True):
        beta = torch.tensor([beta0], dtype=torch.float32, device="cuda")
        kl_out = torch.empty(1, device="cuda") if with_kl else None
        _, names = traced(lambda: ops.vdb_beta_step(beta, kr, n_real, kf, n_fake, lr32, target32, kl_out=kl_out))
        assert has(names, r"\bvdb_beta_step_kernel\b"), names
        got.append((beta, kl_out))
    (b1, k1), (b2, _), (b3, k3) = got
    assert same_bits(b1, b2) and same_bits(b1, b3) and same_bits(k1, k3)
    eb = abs(b1.item() - want) / abs(want) if want else abs(b1.item())
    ek = abs(k1.item() - kl) / abs(kl)
    log(f"beta_step beta0={beta0} lr={lr}: beta {b1.item():.7g} want {want:.7g} rel {eb:.2e}; kl rel {ek:.2e}")
    assert eb <= 1e-6 and ek <= 1e-6, (eb, ek)


# ------------------------------------------------------------------------------------------------- the ticket, in sequence
def test_ticket_is_rearmed_between_vdb_reductions_and_per_stream(ops):
    """The four ticketed reductions of vdb.hip back to back on one stream, forward and in reverse order, with no
    synchronisation in between, then once more on a second stream with its own workspace: every result has the bits of
    the same call run alone, and both ticket words are 0 at the end."""
    z, eps, w, b = (dev(t) for t in head_inputs(300, 65))
    d, tau = (dev(t) for t in loss_inputs(1000))
    lt, dv, u = (dev(t) for t in tau_inputs(1000))
    g = dev(norm_inputs(20000))

    def norm():
        buf = g.clone()
        return ops.vdb_gp_norm(buf, NORM_SCALE), buf

    calls = [("head_fwd", vr.head_fwd_blocks(300), lambda: ops.vdb_head_fwd(z, w, b, eps=eps)),
             ("loss", vr.loss_blocks(1000), lambda: ops.vdb_loss(d, vr.NEG_TAU, GSCALE, tau=tau)),
             ("gp_norm", vr.gp_norm_blocks(20000), norm),
             ("tau", vr.loss_blocks(1000), lambda: ops.vdb_tau(lt, d=dv, u=u, want_tau=True, want_grad=True))]
    assert all(1 < blocks <= vr.LAST_BLOCK_MAX_GRID for _, blocks, _ in calls)
    alone = {}
    for name, _, fn in calls:
        torch.cuda.synchronize()
        alone[name] = [t.clone() for t in _tensors(fn())]
        torch.cuda.synchronize()
    ws = ops.reduce_ws(device())
    assert header_word(ws) == 0
    (first, second), names = traced(lambda: ([(n, fn()) for n, _, fn in calls], [(n, fn()) for n, _, fn in reversed(calls)]))
    assert not has(names, r"\bfinal_sum_kernel\b"), names
    assert header_word(ws) == 0
    for which, results in (("forward", first), ("reverse", second)):
        for name, res in results:
            assert all_same(res, alone[name]), (which, name)
    side = torch.cuda.Stream(device=device())
    side.wait_stream(torch.cuda.current_stream(device()))
    with torch.cuda.stream(side):
        ws_side = ops.reduce_ws(device())
        third = [(n, fn()) for n, _, fn in calls]
    side.synchronize()
    assert ws_side.data_ptr() != ws.data_ptr()
    for name, res in third:
        assert all_same(res, alone[name]), ("side stream", name)
    assert header_word(ws_side) == 0 and header_word(ws) == 0
    torch.cuda.current_stream(device()).wait_stream(side)
    log(f"vdb ticket sequence: {len(calls)} reductions forward and reverse on one stream and on a side stream: bit-equal to the calls run alone")


# ------------------------------------------------------------------------------------------------------------- refusals
def test_refusals_write_nothing(ops):
    E_BADARG, E_SHAPE, E_WS = -1, -2, -4       # include/repo_hip.h
    N, Z = 9, 5
    L, st = ops.lib(), torch.cuda.current_stream().cuda_stream
    z, eps, w, b = (dev(t) for t in head_inputs(N, Z))
    filled = lambda *s: torch.full(s, SENT, device="cuda")  # noqa: E731
    lat, d, kl, dz, dw, db, dd, s1, s2, delta, extra, tau_o, dlt = (filled(*s) for s in (
        (N, Z), (N,), (1,), (N, 2 * Z), (Z,), (1,), (N,), (1,), (2,), (N, 2 * Z), (N, Z), (N,), (N,)))
    outs = (lat, d, kl, dz, dw, db, dd, s1, s2, delta, extra, tau_o, dlt)
    src = dev(rnd(np.random.RandomState(1), N))          # a valid d / lt / dd operand
    g = filled(N)
    lat_in = dev(rnd(np.random.RandomState(2), N, Z))
    rws = ops.reduce_ws(device())
    red_min = rr.RED_HEADER_BYTES + 2 * rr.LAST_BLOCK_MAX_GRID * 4
    cws = ops.workspace(L.repo_vdb_colsum_workspace_bytes(Z), device())
    col_min = L.repo_vdb_colsum_workspace_bytes(Z)
    assert col_min == (Z + 1) * vr.LAST_BLOCK_MAX_GRID * 4
    p = lambda t: t.data_ptr()  # noqa: E731

    def fwd(ldz, ws_bytes):
        return L.repo_vdb_head_fwd(N, Z, p(z), ldz, p(eps), 0, 0, p(w), p(b), p(lat), p(d), p(kl), p(rws), ws_bytes, st)

    def bwd(ldz, lddz, pdw, pdb, ws_bytes):
        return L.repo_vdb_head_bwd(N, Z, p(z), ldz, p(eps), 0, 0, p(lat_in), p(w), p(src), None, 0.0, None, p(dz), lddz, pdw,
                                   pdb, 0, p(cws), ws_bytes, st)

    def loss(mode, ptau, ws_bytes):
        return L.repo_vdb_loss(N, p(src), mode, ptau, 1.0, p(dd), p(s1), p(rws), ws_bytes, st)

    a5 = dev(rnd(np.random.RandomState(3), N, 2 * Z))
    big = rws.numel()
    assert fwd(2 * Z - 1, big) == E_SHAPE
    assert bwd(2 * Z - 1, 2 * Z, p(dw), p(db), col_min) == E_SHAPE
    assert bwd(2 * Z, 2 * Z - 1, p(dw), p(db), col_min) == E_SHAPE
    assert L.repo_vdb_gp_delta(N, Z, p(z), 2 * Z, p(eps), 0, 0, p(lat_in), p(w), p(delta), 2 * Z - 1, st) == E_SHAPE
    assert L.repo_vdb_gp_delta(N, Z, p(z), 2 * Z - 1, p(eps), 0, 0, p(lat_in), p(w), p(delta), 2 * Z, st) == E_SHAPE
    assert L.repo_vdb_gp_head(N, Z, p(a5), 2 * Z - 1, p(z), 2 * Z, p(eps), 0, 0, p(lat_in), p(w), p(extra), p(dw), 0, p(cws),
                              col_min, st) == E_SHAPE
    assert bwd(2 * Z, 2 * Z, p(dw), None, col_min) == E_BADARG            # dfc_w without dfc_b
    assert bwd(2 * Z, 2 * Z, None, p(db), col_min) == E_BADARG
    assert loss(vr.NEG_TAU, None, big) == E_BADARG                       # REPO_VDB_NEG_TAU without tau
    assert loss(5, p(src), big) == E_BADARG and loss(-1, p(src), big) == E_BADARG
    # a reduction workspace one byte short
    assert fwd(2 * Z, red_min - 1) == E_WS
    assert loss(vr.CHI, None, red_min - 1) == E_WS
    assert L.repo_vdb_gp_norm(N, p(g), 2.0, p(s1), p(rws), red_min - 1, st) == E_WS
    assert L.repo_vdb_tau(N, p(src), p(src), None, p(tau_o), p(dlt), p(s2), p(rws), red_min - 1, st) == E_WS
    # a column-sum workspace one byte short
    assert bwd(2 * Z, 2 * Z, p(dw), p(db), col_min - 1) == E_WS
    assert L.repo_vdb_gp_head(N, Z, p(a5), 2 * Z, p(z), 2 * Z, p(eps), 0, 0, p(lat_in), p(w), p(extra), p(dw), 0, p(cws),
                              col_min - 1, st) == E_WS
    torch.cuda.synchronize()
    for t in outs + (g,):
        assert bool((t == SENT).all()), "a refused call wrote an output"
    assert header_word(rws) == 0
    # and the smallest workspaces are taken
    assert loss(vr.CHI, None, red_min) == 0 and bwd(2 * Z, 2 * Z, p(dw), p(db), col_min) == 0
    torch.cuda.synchronize()
    assert not bool((dd == SENT).any()) and not bool((dz == SENT).any()) and not bool((dw == SENT).any())
