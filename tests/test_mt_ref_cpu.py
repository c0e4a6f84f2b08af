"""tests/mt_ref.py against autograd, torch.optim.Adam and the definitions written out as loops; its grid mirrors at their
boundaries; and the cases and adversarial inputs of tests/test_mt_kernels_gpu.py: each case sits in the regime its id names,
each input set has the property it is there for.  Runs without a GPU."""
import numpy as np
import pytest
import torch

from oracle import repo_oracle as ro
from tests import mt_ref as mr
from tests import test_mt_kernels_gpu as tm
from tests.util import relerr


# ------------------------------------------------------------------------------------------- the statements and autograd
def _conv_down_loops(x, w, bias):
    n, CB, HB, _ = x.shape
    CS, _, KS, _ = w.shape
    HS = (HB - KS) // 2 + 1
    y = torch.zeros(n, CS, HS, HS, dtype=torch.float64)
    for oy in range(HS):
        for ox in range(HS):
            patch = x[:, :, 2 * oy:2 * oy + KS, 2 * ox:2 * ox + KS]
            y[:, :, oy, ox] = torch.einsum("ncuv,scuv->ns", patch, w) + bias
    return y


def _conv_up_loops(x, w, bias):
    n, CS, HS, _ = x.shape
    _, CB, KS, _ = w.shape
    HB = 2 * (HS - 1) + KS
    y = bias.reshape(1, CB, 1, 1).repeat(n, 1, HB, HB)
    for iy in range(HS):
        for ix in range(HS):
            y[:, :, 2 * iy:2 * iy + KS, 2 * ix:2 * ix + KS] += torch.einsum("ns,sbuv->nbuv", x[:, :, iy, ix], w)
    return y


@pytest.mark.parametrize("case", [(mr.CONV_DOWN, (2, 5, 3, 9, 3), False, "channel"), (mr.CONV_DOWN, (3, 3, 5, 10, 4), True, "channel"),
                                  (mr.CONV_UP, (2, 6, 5, 4, 5), False, "channel"), (mr.CONV_UP, (3, 7, 4, 1, 4), False, "channel"),
                                  (mr.DENSE, (3, 7, 5, 4), False, "channel"), (mr.DENSE, (3, 7, 5, 4), False, "element"),
                                  (mr.DENSE, (3, 7, 5, 4), False, "none")])
def test_film_statements_are_autograd_of_relu_film_of_the_layer(case):
    """relu((1 + g) y + b) through a convolution (float and uint8 frames), its transpose and a dense layer: film_layer_y is the
    layer written as loops, film_fwd the formula, film_bwd its autograd."""
    kind, dims, u8, bias_mode = case
    c = tm.exact_case(kind, dims, u8, bias_mode, "std")
    n, C, P, goff, boff = c["n"], c["C"], c["P"], c["goff"], c["boff"]
    x = c["x"]
    xs = (x.double() / 255) * 2 - 1 if u8 else x.double()
    w, bias = c["w"].double(), None if c["bias"] is None else c["bias"].double()
    if kind == mr.CONV_DOWN:
        y = _conv_down_loops(xs, w, bias)
    elif kind == mr.CONV_UP:
        y = _conv_up_loops(xs, w, bias)
    else:
        y = (xs @ w).view(n, C, P)
        if bias_mode == "channel":
            y = y + bias.view(1, C, 1)
        elif bias_mode == "element":
            y = y + bias.view(1, C, P)
    y = y.reshape(n, C, P)
    assert relerr(c["y64"], y) < 1e-14
    # the term-by-term form that the float32 figures are measured with is the same layer
    assert relerr(mr.film_layer_y_seq(kind, c["geo"], x, c["w"], c["bias"], dtype=torch.float64).reshape(n, C, P), y) < 1e-14
    film = c["film"].double()
    gam = film[:, goff:goff + C].clone().requires_grad_(True)
    bet = film[:, boff:boff + C].clone().requires_grad_(True)
    yv = y.clone().requires_grad_(True)
    hh = torch.relu((1 + gam[..., None]) * yv + bet[..., None])
    cot = torch.from_numpy(np.random.RandomState(3).standard_normal(tuple(hh.shape)))
    (hh * cot).sum().backward()
    h, mag = mr.film_fwd(c["y64"], c["film"], goff, boff)
    assert relerr(h, hh) < 1e-14 and bool((mag >= h.abs() - 1e-12).all())
    dy, dg, db, sg, sb = mr.film_bwd(cot * (hh.detach() > 0), c["y64"], c["film"], goff, boff)
    assert relerr(dy, yv.grad) < 1e-13 and relerr(dg, gam.grad) < 1e-13 and relerr(db, bet.grad) < 1e-13
    assert bool((sg >= dg.abs() - 1e-12).all()) and bool((sb >= db.abs() - 1e-12).all())


def test_film_tables_is_the_chunk_and_split_of_the_film_row():
    from repo_amd.algorithms.repo.models.conditional import DEC_CHANNELS, ENC_CHANNELS, film_offsets

    assert list(ENC_CHANNELS) == tm.ENC_CHANNELS and list(DEC_CHANNELS) == tm.DEC_CHANNELS
    for ch in ([1], [5, 3], tm.ENC_CHANNELS, tm.DEC_CHANNELS):
        film = tm.rnd(np.random.RandomState(1), 3, 2 * sum(ch))
        flat, views = mr.film_tables(film, ch)
        gam, bet = film.chunk(2, dim=1)
        o = 0
        for l, ((g, b), C) in enumerate(zip(film_offsets(ch), ch)):
            assert torch.equal(views[l][:, 0], 1 + film[:, g:g + C]) and torch.equal(views[l][:, 1], film[:, b:b + C])
            assert torch.equal(views[l][:, 0], 1 + gam.split(list(ch), dim=1)[l]) and torch.equal(views[l][:, 1], bet.split(list(ch), dim=1)[l])
            assert torch.equal(flat[o:o + 3 * 2 * C].view(3, 2, C), views[l])      # [layer][n][2][C_l]
            o += 3 * 2 * C
        assert o == flat.numel()


@pytest.mark.parametrize("case", [(37, 30, 3, False), (5, 1, 3, False), (9, 64, 13, True)])
def test_kl_tasks_is_autograd_of_the_balanced_kl(case):
    """As tests/test_mt_gpu.py::test_kl_balance_tasks_and_dual_step_match_torch writes repo_mt.py:75-99."""
    rows, S, C, real = case
    pm, ps, qm, qs, alpha, lb0, tasks, target, scale = tm.kl_inputs(*case)
    P = [t.double().requires_grad_(True) for t in (pm, ps, qm, qs)]
    lb = lb0.double().requires_grad_(True)
    kl_prior = ro.normal_kl(P[2].detach(), P[3].detach(), P[0], P[1]).sum(1)
    kl_post = ro.normal_kl(P[2], P[3], P[0].detach(), P[1].detach()).sum(1)
    kl_div = alpha * kl_prior + (1 - alpha) * kl_post
    viol = kl_div - target
    lbr = tasks.double() @ lb
    (scale * (lbr.exp().detach() * viol).sum()).backward()
    beta_loss = -(lbr * viol.detach()).mean()
    lb_grad, = torch.autograd.grad(beta_loss, lb)
    terms, grads = mr.kl_tasks(pm, ps, qm, qs, alpha, lb0, tasks, target, scale)
    for got, want in zip(grads, P):
        assert relerr(got, want.grad) < 1e-12
    sums = terms.sum(0)
    assert terms.shape == (rows, 3 + C)
    assert abs(sums[0] - kl_div.sum().item()) < 1e-10 * abs(kl_div.sum().item())
    assert abs(sums[1] - (lbr.exp() * viol).sum().item()) < 1e-10 * (lbr.exp() * viol).abs().sum().item()
    assert abs(sums[2] + rows * beta_loss.item()) < 1e-10 * (lbr * viol).abs().sum().item()
    assert relerr(-sums[3:] / rows, lb_grad) < 1e-12       # the gradient repo_dual_step_tasks takes from the sums


@pytest.mark.parametrize("C", tm.DUAL_CS)
def test_dual_step_tasks_is_adam_over_five_steps(C):
    lb0, sums = tm.dual_inputs(C)
    ref = lb0.double().clone().requires_grad_(True)
    opt = torch.optim.Adam([ref], lr=tm.DUAL_LR, betas=tm.BETAS, eps=1e-8)
    run = tm.dual_run(C, torch.float64)
    before = lb0.double()
    for k in range(tm.DUAL_STEPS):
        ref.grad = -sums[k, 3:].double() / tm.DUAL_ROWS
        opt.step()
        lb, m, v, sc = run[k]
        st = opt.state[ref]
        assert relerr(lb, ref.detach()) < 1e-13 and relerr(m, st["exp_avg"]) < 1e-13 and relerr(v, st["exp_avg_sq"]) < 1e-13
        want = torch.cat((sums[k, :2].double() / tm.DUAL_ROWS, -sums[k, 2:3].double() / tm.DUAL_ROWS, ref.detach().exp()))
        assert relerr(sc, want) < 1e-13
        # the guards of the GPU test: Adam's ratio stays below 4 (the bound's premise), and every entry that moves at all moves
        # by more than 100 times the bound it is held to
        bc1, bc2 = 1 - tm.BETAS[0] ** (k + 1), 1 - tm.BETAS[1] ** (k + 1)
        assert float(((st["exp_avg"] / bc1) / ((st["exp_avg_sq"] / bc2).sqrt() + 1e-8)).abs().max()) < 4.0
        bnd = (k + 1) * (tm.U * lb.abs() + 2.0 ** -18 * tm.DUAL_LR)
        step = (lb - before).abs()
        moving = torch.ones(C, dtype=torch.bool)
        if C > 1:
            moving[1] = False
            assert step[1].item() == 0.0 and float(sums[:, 4].abs().max()) == 0.0
        assert bool((step[moving] > 100 * bnd[moving]).all()), (C, k, step.tolist(), bnd.tolist())
        before = lb
    g = -sums[:, 3:]
    if C > 1:
        assert bool((g[:, 0] > 0).any()) and bool((g[:, 0] < 0).any())        # task 0 on both sides of the target
        assert bool((g[0] > 0).any()) and bool((g[0] < 0).any())              # per-task sums of both signs within a step
    lbn, mn, vn, scn = mr.dual_step_tasks(lb0, torch.ones(C), torch.ones(C), sums[0], tm.DUAL_ROWS, tm.DUAL_LR, *tm.BETAS, 1e-8, 3, apply=False)
    assert torch.equal(lbn, lb0.double()) and torch.equal(mn, torch.ones(C, dtype=torch.float64)) and relerr(scn[3:], lb0.double().exp()) < 1e-15


# ------------------------------------------------------------------------------------------------------ the grid mirrors
def test_grid_mirrors_at_the_regime_boundaries():
    assert [mr.film_fwd_blocks(p, 64) for p in (1, 4, 5, 32768, 32769, 80000)] == [1, 1, 2, 8192, 8192, 8192]
    assert [mr.film_fwd_blocks(p, 63) for p in (1, 4, 5)] == [1, 1, 2]                  # 63, 252, 315 elements
    assert [mr.film_fwd_blocks(*a) for a in ((1, 1), (1024, 4), (83886, 25), (83887, 25), (83888, 25))] == [1, 16, 8192, 8192, 8192]
    assert [mr.film_fwd_passes(*a) for a in ((32768, 64), (32769, 64), (65536, 64), (65537, 64), (83886, 25), (83887, 25))] == [1, 2, 2, 3, 1, 2]
    assert [mr.film_bwd_blocks(p) for p in (1, 4, 5, 65533, 65536, 65537, 80000)] == [1, 1, 2, 16384, 16384, 16384, 16384]
    assert [mr.film_bwd_passes(p) for p in (65536, 65537, 131072, 131073)] == [1, 2, 2, 3]
    assert [mr.film_exact_blocks(p) for p in (1, 4095, 4096, 4097, 80000)] == [1, 4095, 4096, 4096, 4096]
    assert [mr.film_exact_passes(p) for p in (4096, 4097, 65792, 80000)] == [1, 2, 17, 20]
    assert [mr.film_exact_slices(P, 10 ** 6) for P in (1, 2, 3, 4, 16, 25, 32, 33, 64, 121, 128, 129, 256, 257, 900)] == \
        [256, 128, 64, 64, 16, 8, 8, 4, 4, 2, 2, 1, 1, 1, 1]
    assert [mr.film_exact_slices(4, o) for o in (1, 7, 63, 64, 65)] == [1, 7, 63, 64, 64]
    assert [mr.film_tables_blocks(n, 480) for n in (1, 1092, 1093, 2500)] == [4, 4095, 4096, 4096]
    assert mr.film_tables_blocks(1, 1) == 1 and 1092 * 960 <= 4096 * 256 < 1093 * 960
    assert [mr.film_tables_passes(n, 480) for n in (1092, 1093, 2500)] == [1, 2, 3]
    assert [mr.kl_tasks_blocks(r) for r in (1, 4, 5, 2048, 2049, 2450)] == [1, 1, 2, 512, 512, 512]
    assert [mr.kl_tasks_passes(r) for r in (2048, 2049, 4096, 4097, 6144, 6145)] == [1, 2, 2, 3, 3, 4]
    # the loops of film_exact_part for slice 0: (S, pixel batches, main trips, tail trips, idle threads)
    assert mr.film_exact_loops(mr.DENSE, (7, 0, 0, 0), 4) == (7, 1, 0, 1, 4)
    assert mr.film_exact_loops(mr.DENSE, (70, 0, 0, 0), 25) == (8, 1, 2, 1, 0)
    assert mr.film_exact_loops(mr.DENSE, (1024, 0, 0, 0), 25) == (8, 1, 32, 0, 0)


def test_every_gpu_case_sits_in_the_regime_it_is_named_for():
    ids = {c: tm.fwd_id(*c) for c in tm.FWD_CASES}
    assert ids[(1, 1, 64)].endswith("wave-1blk-1pass") and ids[(3, 5, 65)].endswith("wave-4blk-1pass")
    assert ids[(128, 256, 64)].endswith("wave-8192blk-1pass") and 128 * 256 == 4 * 8192
    assert ids[(3, 10923, 64)].endswith("wave-8192blk-2pass") and 3 * 10923 == 4 * 8192 + 1
    assert ids[(5, 13108, 64)].endswith("wave-8192blk-3pass") and 5 * 13108 == 2 * 4 * 8192 + 4
    assert ids[(1, 1, 1)].endswith("elem-1blk-1pass") and ids[(2, 3, 63)].endswith("elem-2blk-1pass")
    assert ids[(4, 256, 4)].endswith("elem-16blk-1pass")
    assert ids[(7, 11984, 25)].endswith("elem-8192blk-2pass") and 0 < 7 * 11984 * 25 - 8192 * 256 <= 64
    assert sorted(P for _, _, P in tm.FWD_CASES if P < 64) == [1, 4, 25, 63] and {64, 65} <= {P for _, _, P in tm.FWD_CASES}
    ids = {c: tm.bwd_id(*c) for c in tm.BWD_CASES}
    assert all(ids[c].endswith("-1pass") for c in tm.BWD_SMALL) and [c[2] for c in tm.BWD_SMALL] == [1, 63, 64, 65, 961]
    assert ids[(256, 256, 4)].endswith("16384blk-1pass") and 256 * 256 == 65536
    assert ids[(257, 255, 4)].endswith("16384blk-1pass") and 257 * 255 == 65535
    assert ids[(1, 65537, 4)].endswith("16384blk-2pass") and ids[(3, 43691, 4)].endswith("16384blk-3pass") and 3 * 43691 == 131073
    # the descriptions: slices, batches, loops
    loops = {}
    for case in tm.EXACT_CASES:
        kind, dims, u8, b, gate = case
        n, C, P, geo, outer = tm.exact_geometry(kind, dims)
        loops[(kind, dims)] = (P,) + mr.film_exact_loops(kind, geo, P) + (mr.film_exact_passes(n * C), mr.film_bwd_passes(n * C))
    D, DN, UPC = mr.DENSE, mr.CONV_DOWN, mr.CONV_UP
    assert loops[(D, (3, 7, 5, 4))] == (4, 7, 1, 0, 1, 4, 1, 1)          # S clamps to 7: 36 pixels a batch, 4 threads with sl = 7
    assert loops[(D, (3, 1, 5, 25))] == (25, 1, 1, 0, 1, 0, 1, 1)
    assert loops[(D, (2, 70, 3, 25))] == (25, 8, 1, 2, 1, 0, 1, 1)       # main loop twice, then the tail
    assert loops[(D, (2, 1024, 4, 25))] == (25, 8, 1, 32, 0, 0, 1, 1)
    assert loops[(D, tm.DENSE_BIG)] == (4, 7, 1, 0, 1, 4, 17, 2) and 257 * 256 == 65792
    assert loops[(DN, (3, 3, 5, 10, 4))] == (16, 3, 1, 0, 1, 1, 1, 1)    # S clamps to 3: 85 pixels a batch, thread 255 has sl = 3
    assert loops[(DN, (2, 21, 4, 10, 4))] == (16, 16, 1, 0, 2, 0, 1, 1)  # the tail alone
    assert loops[(DN, (2, 70, 4, 10, 4))] == (16, 16, 1, 1, 1, 0, 1, 1)  # main loop, then the tail
    assert loops[(DN, (2, 5, 3, 9, 3))] == (16, 5, 1, 0, 1, 1, 1, 1)
    assert loops[(DN, (2, 4, 3, 36, 4))] == (289, 1, 2, 1, 0, 0, 1, 1)   # two pixel batches, S = 1
    assert loops[(UPC, (2, 6, 5, 4, 5))][:3] == (121, 2, 1) and loops[(UPC, (2, 6, 5, 4, 6))][:3] == (144, 1, 1)
    assert loops[(UPC, (3, 7, 4, 1, 4))][:3] == (16, 7, 1) and loops[(UPC, (2, 9, 3, 8, 6))][:3] == (400, 1, 2)
    assert {(d, u8) for k, d, u8, _, _ in tm.EXACT_CASES if u8} == {((3, 3, 5, 10, 4), True), ((2, 4, 3, 36, 4), True)}
    assert all({(D, d, False, b, "std") for b in tm.BIASES} <= set(tm.EXACT_CASES) for d in tm.DENSE_SMALL + [tm.DENSE_BIG])
    # tables and the KL
    ids = [tm.table_id(c) for c in tm.TABLE_CASES]
    assert ids[-2].endswith("4096blk-2pass") and ids[-1].endswith("4096blk-3pass") and all(i.endswith("-1pass") for i in ids[:-2])
    assert [tm.kl_id(c).split("-", 4)[4] for c in tm.KL_CASES] == ["1blk-1pass", "512blk-1pass", "512blk-2pass", "512blk-2pass",
                                                                   "512blk-4pass", "512blk-2pass"]
    assert {c[1] for c in tm.KL_CASES} == {1, 30, 64} and {c[2] for c in tm.KL_CASES} == {1, 3, 13}


# -------------------------------------------------------------------------------------------------- the adversarial inputs
def test_film_inputs_have_the_properties_they_are_there_for():
    seen_below = False
    for n, C, P in tm.FWD_CASES + tm.BWD_CASES:
        marked = (n, C, P) in tm.BWD_CAP
        y, film, goff, boff, up = tm.film_inputs(n, C, P, marked)
        ld = film.shape[1]
        assert ld > 2 * C and min(goff, boff) > 0 and max(goff, boff) + C < ld            # both blocks in the middle of the row
        assert goff + C <= boff or boff + C <= goff
        seen_below |= boff < goff
        g1 = 1 + tm.plane_block(film, goff, C)
        assert float(g1.abs().min()) >= 0.0999
        if n * C * P >= 100:
            dead = float((mr.film_fwd(y, film, goff, boff)[0] == 0).double().mean())
            assert 0.1 < dead < 0.9, (n, C, P, dead)                                        # the ReLU is live
        if marked:
            g1, bet = g1.reshape(-1), tm.plane_block(film, boff, C).reshape(-1)
            two = sorted(int(i) for i in (g1 == 2).nonzero().reshape(-1))
            assert two == sorted({p % (n * C) for p in tm.MARKED if p < n * C}) and bool((bet[two] == 0).all())
            assert bool((g1[[i for i in range(n * C) if i not in two][:1000]] == 0.5).all()) and int((g1 == 0.5).sum()) == n * C - len(two)
    assert seen_below
    # the planes a capped grid reaches on a later pass are among the marked ones
    assert mr.film_bwd_passes(65537) == 2 and 65536 in tm.MARKED and mr.film_bwd_passes(131073) == 3


@pytest.mark.parametrize("case", tm.EXACT_CASES, ids=[tm.exact_id(c) for c in tm.EXACT_CASES])
def test_exact_cases_have_gated_off_planes_that_matter(case):
    kind, dims, u8, b, gate = case
    c = tm.exact_case(*case)
    n, C, P = c["n"], c["C"], c["P"]
    g1 = (1 + tm.plane_block(c["film"], c["goff"], C)).reshape(-1)
    gated = torch.from_numpy(tm.is_gated(c["film"], c["goff"], C)).reshape(-1)
    want = {p for p, v in c["special"].items() if v in tm.GATED}
    assert {int(i) for i in gated.nonzero().reshape(-1)} == want and want
    if gate == "std":
        assert bool((g1 == 0).any()) and bool(((g1 - 1e-4).abs() < 1e-7).any()) and bool(((g1 + 1e-4).abs() < 1e-7).any())
        assert bool(((g1 - 0.05).abs() < 1e-6).any()) and bool(((g1 + 0.05).abs() < 1e-6).any())
    assert float(g1[~gated].abs().min()) > 0.049
    assert float(tm.plane_block(c["film"], c["boff"], C).min()) >= 0.2           # beta > 0: a gated-off plane is active
    h, dh = c["h"].reshape(n * C, P), c["dh"].reshape(n * C, P)
    assert bool((h[gated] > 0).all()) and bool((dh[gated] != 0).all())
    plain = torch.tensor([p not in c["special"] for p in range(n * C)])
    dead = float((h[plain] == 0).double().mean())
    assert 0.05 < dead < 0.9, dead                                               # the ReLU is live on the ordinary planes
    dg = mr.film_bwd(c["dh"], c["y64"], c["film"], c["goff"], c["boff"])[1].reshape(-1)
    assert float(dg[gated].abs().max()) > 1e-2 * float(dg.abs().max())           # what film_exact writes matters
    if n * C > 60000:
        fb, fe = 4 * mr.film_bwd_blocks(n * C), mr.film_exact_blocks(n * C)
        if gate == "std":
            assert want == {0, 4095, 4096, 65536, n * C - 1}
            assert {p // fe for p in want} == {0, 1, 16} and {p // fb for p in want} == {0, 1}     # on first and later passes
        else:
            assert want == {n * C - 1} and (n * C - 1) // fb == 1 and (n * C - 1) // fe == 16    # met on strided passes alone
    none = tm.exact_case(kind, dims, u8, b, "none")
    assert not tm.is_gated(none["film"], none["goff"], C).any() and torch.equal(none["w"], c["w"]) and set(none["special"]) >= want


def test_kl_and_table_inputs():
    for case in tm.KL_CASES:
        rows, S, C, real = case
        pm, ps, qm, qs, alpha, lb, tasks, target, scale = tm.kl_inputs(*case)
        assert tasks.shape == (rows, C) and float(ps.min()) >= 0.2 and float(qs.min()) >= 0.2
        if real:
            assert not bool(((tasks == 0) | (tasks == 1)).all())
        else:
            assert bool((tasks.sum(1) == 1).all()) and bool(((tasks == 0) | (tasks == 1)).all())
            assert C == 1 or (float(tasks[:, C - 1].sum()) == 0 and (rows < C or bool((tasks[:, :C - 1].sum(0) > 0).all())))
        assert alpha == float(np.float32(alpha)) and 1 - alpha == float(np.float32(1) - np.float32(alpha))
    assert sum(1 for c in tm.KL_CASES if c[3]) == 1
    lists = [tuple(ch) for _, ch, _ in tm.TABLE_CASES]
    assert {len(ch) for ch in lists} == {1, 2, 3, 4} and {n for n, _, _ in tm.TABLE_CASES} == {1, 9, 1093, 2500}
    assert {w for _, _, w in tm.TABLE_CASES} == {False, True}


def test_seq_sum_adds_left_to_right():
    rs = np.random.RandomState(0)
    t = torch.from_numpy((rs.standard_normal((3, 5, 37)) * 10.0 ** rs.uniform(-3, 3, (3, 5, 37))).astype(np.float32))
    for dim in (0, 1, 2):
        want = torch.zeros_like(t.select(dim, 0))
        for i in range(t.shape[dim]):
            want = want + t.select(dim, i)
        assert torch.equal(mr.seq_sum(t, dim), want)
    # the order matters: pairing the terms differently gives other bits
    t = torch.tensor([1.0, 2.0 ** -24, 2.0 ** -24, -1.0])
    assert mr.seq_sum(t).item() == 0.0 and ((t[0] + t[3]) + (t[1] + t[2])).item() != 0.0


def test_the_float32_table_of_the_gpu_suite_is_its_own_measurement():
    """F32 of tests/test_mt_kernels_gpu.py is measure_f32() to two digits.  The float32 statement adds term by term in a fixed
    order with elementwise operations (mt_ref.film_layer_y_seq, seq_sum, reduce_ref.fixed_order_sum), so the figure does not
    depend on a host's convolution, matrix product, vectorised sum or thread count; what may still differ between hosts is
    the last bit of a vectorised exp or log.  A figure is at most 1.2 times the measurement made here and at least half of
    it (tests/test_vdb_ref_cpu.py's window).  Every bound is the 8 x figure, far below the figure of the older test."""
    got = tm.measure_f32()
    assert sorted(got) == sorted(tm.F32)
    for k, v in got.items():
        assert 0.5 * v <= tm.F32[k] <= 1.2 * v, (k, v, tm.F32[k])
        assert tm.bound(k) == 8.0 * tm.F32[k] < tm.FIGURE[k]
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        assert tm.measure_f32() == got        # the same bits with one thread
    finally:
        torch.set_num_threads(threads)
