"""Plain-torch statement of every entry point of csrc/vdb.hip, written from the contracts of include/repo_hip.h ("VDB
discriminator (ABI v12)"), and the grids of its launches restated in Python.

The functions take the float32 tensors a kernel is given and compute at `dtype` (float64 unless a test measures the
float32 rounding of the same formulas).  Every function that needs leaky'(lat) takes `lat` as an input, as the kernels
do: the sign decision is then made on the same float32 values on both sides and needs no margin.  Sums are returned as
their TERMS, so that a test can judge a float32 sum against sum |terms|.  tests/test_vdb_ref_cpu.py ties the formulas to
autograd and to tests/calib_ref.py.

The grid mirrors follow the launches of vdb.hip; tests/test_vdb_kernels_gpu.py pins them by counting the partials a
launch wrote.  `colsum_finish` is the order of vdb_colsum_finish_kernel: a left-to-right float32 sum of the G partials
of a column, then prev + s when accumulating.  There is no multiply to contract into an FMA, so numpy's float32
arithmetic reproduces the device's bits (the argument of tests/reduce_ref.py)."""
import numpy as np
import torch
import torch.nn.functional as F

SLOPE = 0.01                 # kLeakySlope: nn.LeakyReLU()'s default
LAST_BLOCK_MAX_GRID = 64     # kLastBlockMaxGrid: the cap of every small grid of vdb.hip
BCE0, BCE1, NEG_TAU, CHI, NEG_CHI = range(5)     # REPO_VDB_*


def _up(dtype, *ts):
    return [None if t is None else torch.as_tensor(t).to(dtype) for t in ts]


def leaky(x):
    return torch.where(x > 0, x, SLOPE * x)


def leaky_grad(x):
    return torch.where(x > 0, torch.ones_like(x), torch.full_like(x, SLOPE))


def _halves(z):
    Z = z.shape[1] // 2
    return z[:, :Z], z[:, Z:2 * Z]


def head_fwd(z, eps, fc_w, fc_b, dtype=torch.float64):
    """z (N, 2Z) = [mean | logstd] -> (lat (N, Z), d (N,), kl_rows (N,)); *kl_sum of the kernel is kl_rows.sum()."""
    z, eps, fc_w, fc_b = _up(dtype, z, eps, fc_w, fc_b)
    mean, ls = _halves(z)
    lat = mean + eps * torch.exp(ls)
    d = (leaky(lat) * fc_w.reshape(1, -1)).sum(1) + fc_b.reshape(-1)[0]
    kl_rows = (-ls + 0.5 * (torch.exp(2 * ls) + mean ** 2)).sum(1) - 0.5 * mean.shape[1]
    return lat, d, kl_rows


def loss(d, mode, tau=None, gscale=1.0, dtype=torch.float64):
    """-> (terms (N,) = f(d[n]), dd (N,) = gscale * f'(d[n])) for the five REPO_VDB_* modes."""
    d, tau = _up(dtype, d, tau)
    if mode in (BCE0, BCE1):
        t = torch.full_like(d, 1.0 if mode == BCE1 else 0.0)
        terms = F.binary_cross_entropy_with_logits(d, t, reduction="none")
        g = torch.sigmoid(d) - t
    elif mode == NEG_TAU:
        terms, g = -tau * d, -tau
    elif mode in (CHI, NEG_CHI):
        terms, g = d + 0.25 * d * d, 1.0 + 0.5 * d
        if mode == NEG_CHI:
            terms, g = -terms, -g
    else:
        raise ValueError(mode)
    return terms, g * gscale


def head_bwd(z, eps, lat, fc_w, dd, beta=None, kl_coef=0.0, extra=None, dtype=torch.float64):
    """-> (dz (N, 2Z), dfc_w_terms (N, Z), dfc_b_terms (N,)): the sums of the kernel are the terms' column sums.
    beta None = no KL term (c = 0); extra None = no further upstream on the logstd half."""
    z, eps, lat, fc_w, dd, beta, extra = _up(dtype, z, eps, lat, fc_w, dd, beta, extra)
    mean, ls = _halves(z)
    sd = torch.exp(ls)
    c = 0.0 if beta is None else beta.reshape(-1)[0] * kl_coef
    dlat = dd[:, None] * fc_w.reshape(1, -1) * leaky_grad(lat)
    dls = dlat * eps * sd + c * (torch.exp(2 * ls) - 1.0)
    if extra is not None:
        dls = dls + extra
    return torch.cat((dlat + c * mean, dls), 1), dd[:, None] * leaky(lat), dd


def gp_delta(z, eps, lat, fc_w, dtype=torch.float64):
    """-> delta5 (N, 2Z) = [r | r eps exp(logstd)], r = fc_w leaky'(lat)."""
    z, eps, lat, fc_w = _up(dtype, z, eps, lat, fc_w)
    r = fc_w.reshape(1, -1) * leaky_grad(lat)
    return torch.cat((r, r * eps * torch.exp(_halves(z)[1])), 1)


def gp_norm(g, scale, dtype=torch.float64):
    """-> (terms = g^2, g * scale)."""
    g, = _up(dtype, g)
    return g * g, g * scale


def gp_head(a5, z, eps, lat, fc_w, dtype=torch.float64):
    """-> (extra (N, Z), dfc_w_terms (N, Z)) from a5 = dP/d delta5 (N, 2Z)."""
    a5, z, eps, lat, fc_w = _up(dtype, a5, z, eps, lat, fc_w)
    am, as_ = _halves(a5)
    es = eps * torch.exp(_halves(z)[1])
    gl = leaky_grad(lat)
    return as_ * fc_w.reshape(1, -1) * gl * es, (am + as_ * es) * gl


def tau(lt, d=None, u=None, dtype=torch.float64):
    """-> (terms0 = tau d, terms1 = tau - 1, tau = exp(lt), dlt = tau (d + u) / N); d None = zeros, u None = 0."""
    lt, d, u = _up(dtype, lt, d, u)
    t = torch.exp(lt)
    dv = torch.zeros_like(t) if d is None else d
    uv = 0.0 if u is None else u.reshape(-1)[0]
    return t * dv, t - 1.0, t, t * (dv + uv) / lt.numel()


def beta_step(beta, kl_real_sum, n_real, kl_fake_sum, n_fake, beta_lr, target_kl):
    """-> (the new beta, the mean KL) as Python floats (float64)."""
    kl = 0.5 * (float(kl_real_sum) / n_real + float(kl_fake_sum) / n_fake)
    return max(float(beta) + beta_lr * (kl - target_kl), 0.0), kl


# ------------------------------------------------------------------------------------------------------------ the grids
def _small_grid(work, per_block):
    return max(1, min(LAST_BLOCK_MAX_GRID, -(-work // per_block)))


def head_fwd_blocks(N):        # vdb_head_fwd_kernel: one row per wave, 4 per block; rows stride by 4 * grid above N = 256
    return _small_grid(N, 4)


def loss_blocks(N):            # vdb_loss_kernel and vdb_tau_kernel: one element per thread; strided above N = 16384
    return _small_grid(N, 256)


def gp_norm_blocks(n):         # vdb_gp_norm_kernel: 4096 elements per block; strided above n = 262144
    return _small_grid(n, 4096)


def colsum_grid(N):
    """vdb_colsum_kernel: (G blocks, rows per block); block b owns rows [b * rpb, min(N, (b + 1) * rpb))."""
    G = _small_grid(N, 32)
    return G, -(-N // G)


def colsum_rows(N, b):
    """Rows of block b (0 for a block past the end: N = 2049 leaves block 63 empty)."""
    G, rpb = colsum_grid(N)
    return max(0, min(N, (b + 1) * rpb) - b * rpb)


def gp_delta_blocks(N, Z):     # vdb_gp_delta_kernel: one element per thread; strided above N * Z = 524288
    return min(2048, -(-(N * Z) // 256))


def colsum_finish(parts_row, prev=None):
    """vdb_colsum_finish_kernel on one column's G partials: s = 0, s += parts[i] in order; prev + s when accumulating."""
    s = np.float32(0.0)
    for p in np.asarray(parts_row, dtype=np.float32).ravel():
        s = np.float32(s + p)
    return s if prev is None else np.float32(np.float32(prev) + s)
