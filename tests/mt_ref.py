"""Plain-torch statement of every entry point of csrc/multitask.hip, written from the contracts of include/repo_hip.h
("multitask (task-conditioned) agents"), and the grids of its launches restated in Python.

The functions take the float32 (or uint8) tensors a kernel is given and compute at `dtype` (float64 unless a test
measures the float32 rounding of the same formulas).  Sums come with the sum of their terms' magnitudes, or as their
terms, so that a test can judge a float32 sum against sum |terms|.  tests/test_mt_ref_cpu.py ties the formulas to autograd
and to torch.optim.Adam; tests/test_mt_kernels_gpu.py holds the kernels to them.

`film_tables` is the one float32 statement: 1 + gamma is a single float32 addition, so numpy reproduces the device's bits.
Where a float32 run of a statement sets a bound, its sums are taken term by term in a fixed order (`film_layer_y_seq`,
`seq_sum`): the figure is then the same on every host.

The grid mirrors follow the launches of multitask.hip.  A FiLM kernel walks (image, channel) planes: film_fwd and film_bwd
with one WAVE per plane (four per block, stride 4 * grid once the cap binds), film_fwd below 64 pixels per plane with one
lane per element, film_exact with one BLOCK per plane; `passes(work, per_pass)` is how often the busiest unit loops."""
import numpy as np
import torch
import torch.nn.functional as F

FILM_FWD_CAP, FILM_BWD_CAP, FILM_EXACT_CAP, FILM_TABLES_CAP, KL_TASKS_CAP = 8192, 16384, 4096, 4096, 512
FILM_EXACT_BELOW = 1e-3      # kFilmExactBelow: |1 + gamma| below this recomputes y (compared in float32, on fl(1 + gamma))
MAX_TASKS = 13               # kMtMaxTasks
CONV_DOWN, CONV_UP, DENSE = 1, 2, 3


def _up(dtype, *ts):
    return [None if t is None else torch.as_tensor(t).to(dtype) for t in ts]


def _planes(film, off, C, ndim, dtype):
    """film[:, off : off + C] shaped to broadcast over (n, C, ...)."""
    blk = torch.as_tensor(film)[:, off:off + C].to(dtype)
    return blk.reshape(blk.shape + (1,) * (ndim - 2))


# ----------------------------------------------------------------------------------------------------------------- FiLM
def film_fwd(y, film, goff, boff, dtype=torch.float64):
    """-> (h = relu((1 + gamma) y + beta), mag = |(1 + gamma) y| + |beta|) for y (n, C, ...), film (n, ld)."""
    y, = _up(dtype, y)
    C = y.shape[1]
    g, b = 1 + _planes(film, goff, C, y.dim(), dtype), _planes(film, boff, C, y.dim(), dtype)
    return torch.relu(g * y + b), (g * y).abs() + b.abs()


def film_bwd(dh, y, film, goff, boff, dtype=torch.float64):
    """dh = the gradient at the ReLU's input.  -> (dy, dgamma (n, C), dbeta (n, C), sum_p |dh y| (n, C), sum_p |dh| (n, C))."""
    dh, y = _up(dtype, dh, y)
    n, C = y.shape[:2]
    g = 1 + _planes(film, goff, C, y.dim(), dtype)
    t = (dh * y).reshape(n, C, -1)
    d = dh.reshape(n, C, -1)
    return dh * g, t.sum(2), d.sum(2), t.abs().sum(2), d.abs().sum(2)


def film_tables(film, channels):
    """-> (the flat float32 buffer [layer][n][2][C_l], its per-layer (n, 2, C_l) views): [1 + gamma | beta] in float32;
    gammas of all layers first in a film row, then the betas."""
    f = np.asarray(film, dtype=np.float32)
    n, total = f.shape[0], int(sum(channels))
    out, off = [], 0
    for C in channels:
        t = np.empty((n, 2, C), dtype=np.float32)
        t[:, 0] = np.float32(1.0) + f[:, off:off + C]
        t[:, 1] = f[:, total + off:total + off + C]
        out.append(t)
        off += C
    flat = np.concatenate([t.ravel() for t in out])
    return torch.from_numpy(flat), [torch.from_numpy(t) for t in out]


def film_layer_y(kind, geo, x, w, bias, dtype=torch.float64):
    """The pre-FiLM output y of the layer a repo_film_bwd_h call describes.
    kind 1, geo (CB, CS, HB, KS): the stride-2 convolution of x (n, CB, HB, HB) (uint8: x / 255 * 2 - 1) -> (n, CS, HS, HS);
    kind 2, same geo: its transpose on x (n, CS, HS, HS) -> (n, CB, HB, HB), HB = 2 (HS - 1) + KS; w (CS, CB, KS, KS) in both;
    kind 3, geo (K, per_element_bias): x (n, K) @ w (K, N) -> (n, N), bias (N) if per_element_bias, else per channel
    (C = bias.numel(), N / C pixels each).  bias may be None."""
    x = torch.as_tensor(x)
    xs = (x.to(dtype) / 255) * 2 - 1 if x.dtype == torch.uint8 else x.to(dtype)
    w, bias = _up(dtype, w, bias)
    if kind == CONV_DOWN:
        return F.conv2d(xs, w, bias, stride=2)
    if kind == CONV_UP:
        return F.conv_transpose2d(xs, w, bias, stride=2)
    assert kind == DENSE
    y = xs @ w
    if bias is None:
        return y
    if geo[1]:
        return y + bias.reshape(1, -1)
    C = bias.numel()
    return (y.reshape(y.shape[0], C, -1) + bias.reshape(1, C, 1)).reshape(y.shape)


def film_layer_y_seq(kind, geo, x, w, bias, dtype=torch.float32):
    """film_layer_y accumulated one term at a time in a fixed order (outer index, then tap row, then tap column), every step
    an elementwise multiply and an elementwise add: the same bits on every host, which a library convolution or matrix
    product does not promise.  The float32 statement the GPU suite's bounds are measured with."""
    x = torch.as_tensor(x)
    xs = (x.to(dtype) / 255) * 2 - 1 if x.dtype == torch.uint8 else x.to(dtype)
    w, bias = _up(dtype, w, bias)
    n = xs.shape[0]
    if kind == DENSE:
        y = torch.zeros(n, w.shape[1], dtype=dtype)
        for k in range(w.shape[0]):
            y = y + xs[:, k, None] * w[k][None]
        if bias is None:
            return y
        if geo[1]:
            return y + bias.reshape(1, -1)
        C = bias.numel()
        return (y.reshape(n, C, -1) + bias.reshape(1, C, 1)).reshape(y.shape)
    CB, CS, HB, KS = geo
    HS = (HB - KS) // 2 + 1
    if kind == CONV_DOWN:
        y = torch.zeros(n, CS, HS, HS, dtype=dtype)
        for cb in range(CB):
            for a in range(KS):
                for b in range(KS):
                    y = y + xs[:, cb, None, a:a + 2 * HS - 1:2, b:b + 2 * HS - 1:2] * w[None, :, cb, a, b, None, None]
    else:
        assert kind == CONV_UP and HB == 2 * (HS - 1) + KS
        y = torch.zeros(n, CB, HB, HB, dtype=dtype)
        for cs in range(CS):
            for a in range(KS):
                for b in range(KS):
                    y[:, :, a:a + 2 * HS - 1:2, b:b + 2 * HS - 1:2] += xs[:, cs, None] * w[None, cs, :, a, b, None, None]
    return y if bias is None else y + bias.reshape(1, -1, 1, 1)


def seq_sum(t, dim=-1):
    """The sum along `dim` added left to right at t's dtype (numpy's accumulate is strictly sequential): reproducible bits."""
    a = np.add.accumulate(torch.as_tensor(t).movedim(dim, -1).contiguous().numpy(), axis=-1)
    return torch.from_numpy(np.ascontiguousarray(a[..., -1]))


# --------------------------------------------------------------------------------------------------- KL and the dual step
def kl_tasks(pm, ps, qm, qs, alpha, log_beta, tasks, target, scale, dtype=torch.float64):
    """-> (terms (rows, 3 + C): the per-row terms of the kernel's sums [KL_row, beta_row viol_row, lb_row viol_row,
    tasks[row][i] viol_row], (dpm, dps, dqm, dqs)): lb_row = tasks[row] . log_beta (any real task rows), beta_row =
    exp(lb_row), viol_row = KL_row - target, KL_row = sum_s KL(N(qm, qs) || N(pm, ps)); the gradients are those of
    scale * sum_rows beta_row * (alpha KL(sg q || p) + (1 - alpha) KL(q || sg p)), beta_row held constant."""
    pm, ps, qm, qs, log_beta, tasks = _up(dtype, pm, ps, qm, qs, log_beta, tasks)
    S = pm.shape[-1]
    pm, ps, qm, qs = (t.reshape(-1, S) for t in (pm, ps, qm, qs))
    tasks = tasks.reshape(pm.shape[0], -1)
    vr, dm = (qs / ps) ** 2, qm - pm
    kl = seq_sum(0.5 * (vr + (dm / ps) ** 2 - 1 - torch.log(vr)), 1)      # (left to right: the same bits on every host)
    lb = seq_sum(tasks * log_beta.reshape(1, -1), 1)
    beta, viol = torch.exp(lb), kl - target
    terms = torch.cat((kl[:, None], (beta * viol)[:, None], (lb * viol)[:, None], tasks * viol[:, None]), 1)
    wp, wq = (beta * alpha * scale)[:, None], (beta * (1 - alpha) * scale)[:, None]
    gqm = dm / ps ** 2
    gqs = -1 / qs + qs / ps ** 2
    gps = 1 / ps - (qs ** 2 + dm ** 2) / ps ** 3
    return terms, (-gqm * wp, gps * wp, gqm * wq, gqs * wq)


def dual_step_tasks(log_beta, m, v, sums, rows, lr, b1, b2, eps, step, apply=True, dtype=torch.float64):
    """One Adam step on the C-vector with grad[i] = -sums[3 + i] / rows.  -> (log_beta, m, v after the step (the inputs'
    values when not apply), scalars [sums[0] / rows, sums[1] / rows, -sums[2] / rows, exp(log_beta after)])."""
    lb, m, v, sums = _up(dtype, log_beta, m, v, sums)
    C = lb.numel()
    g = -sums[3:3 + C] / rows
    if apply:
        m = b1 * m + (1 - b1) * g
        v = b2 * v + (1 - b2) * g * g
        bc1, bc2 = 1 - b1 ** step, 1 - b2 ** step
        lb = lb - (lr / bc1) * m / (torch.sqrt(v) / bc2 ** 0.5 + eps)
    scalars = torch.cat((torch.stack((sums[0] / rows, sums[1] / rows, -sums[2] / rows)), torch.exp(lb)))
    return lb, m, v, scalars


# ------------------------------------------------------------------------------------------------------------ the grids
def _cdiv(a, b):
    return -(-a // b)


def film_fwd_blocks(planes, P):
    """repo_film_fwd: a wave per plane from 64 pixels (4 per block), else a lane per element; cap 8192."""
    return min(FILM_FWD_CAP, _cdiv(planes, 4) if P >= 64 else _cdiv(planes * P, 256))


def film_bwd_blocks(planes):
    """repo_film_bwd / repo_film_bwd_h's streaming pass: a wave per plane, cap 16384."""
    return min(FILM_BWD_CAP, _cdiv(planes, 4))


def film_exact_blocks(planes):
    """film_exact_kernel: a block per plane, cap 4096."""
    return min(FILM_EXACT_CAP, planes)


def film_exact_slices(P, outer):
    """film_exact_kernel's k-slices per pixel: the largest power of two S with S * P <= 256, clamped to the outer
    reduction length (CB, CS or K); a batch is 256 // S pixels."""
    S = 1
    while 2 * S * P <= 256:
        S *= 2
    return min(S, outer)


def film_tables_blocks(nimg, total):
    """repo_film_tables: a thread per table element, cap 4096."""
    return min(FILM_TABLES_CAP, _cdiv(nimg * 2 * total, 256))


def kl_tasks_blocks(rows):
    """repo_kl_balance_tasks: a wave per row, 4 per block, cap 512 (= partials per value)."""
    return min(KL_TASKS_CAP, _cdiv(rows, 4))


def passes(work, per_pass):
    """Loop trips of the busiest unit when `work` items are dealt `per_pass` at a time."""
    return _cdiv(work, per_pass)


def film_fwd_passes(planes, P):
    b = film_fwd_blocks(planes, P)
    return passes(planes, 4 * b) if P >= 64 else passes(planes * P, 256 * b)


def film_bwd_passes(planes):
    return passes(planes, 4 * film_bwd_blocks(planes))


def film_exact_passes(planes):
    return passes(planes, film_exact_blocks(planes))


def film_tables_passes(nimg, total):
    return passes(nimg * 2 * total, 256 * film_tables_blocks(nimg, total))


def kl_tasks_passes(rows):
    return passes(rows, 4 * kl_tasks_blocks(rows))


def film_exact_loops(kind, geo, P):
    """(S, batches of pixels, main-loop trips of slice 0, tail trips of slice 0, threads idle because sl >= S)."""
    outer = geo[0] if kind != CONV_UP else geo[1]
    S = film_exact_slices(P, outer)
    main = 0
    o = 0
    while o + 3 * S < outer:
        o += 4 * S
        main += 1
    tail = len(range(o, outer, S))
    per = 256 // S
    return S, _cdiv(P, per), main, tail, 256 - per * S
