"""tests/mlp_tiles.py against the tile loops it restates, and the proof that tests/test_mlp_persistent_gpu.py would notice a
wrong kernel: its per-row measure passes a float32 chain against the float64 one, and fails after one row of a
workgroup's SECOND tile is scaled by 1 + 2e-5, after one cell of a guard row is written, and after one guard column cell is."""
import numpy as np
import pytest
import torch

from oracle import fixtures as fx
from tests import mlp_tiles as mt
from tests.test_mlp32_gpu import FTOL, GTOL, HEADS, HID, IN, LDX, chain64, guarded, untouched
from tests.util import rnd

CUS = [256, 304, 64]


@pytest.mark.parametrize("cus", CUS)
def test_row_counts_reach_their_regimes(cus):
    S = mt.slots(cus)
    assert S == 2 * cus
    rows = mt.regime_rows(cus)   # (asserts the right-hand column of the table per count)
    assert len(rows) == 7
    if cus == 256:
        assert sorted(rows.values()) == [8193, 16370, 16385, 16385, 24590, 32745, 32769]
    assert rows[(mt.R16, mt.SHARED)] == rows[(mt.R32, mt.SHARED)]
    for (R, name), n in rows.items():
        assert mt.grid(n, R, cus) == S and mt.grid(n, R, cus) == min(mt.blocks(n, R), S)
        # one count less reaches less: the counts are the smallest of their regime
        if name.endswith("+1"):
            with pytest.raises(AssertionError):
                mt.confirm(R, name, n - 1, cus)


@pytest.mark.parametrize("cus", CUS)
def test_every_row_is_owned_once(cus):
    for (R, name), rows in mt.regime_rows(cus).items():
        seen = np.zeros(rows, dtype=np.int32)
        nxt = 0
        for b in range(mt.grid(rows, R, cus)):
            first, count = mt.owned(rows, R, cus, b)
            assert first == nxt and count >= 1   # contiguous runs, in workgroup order, none empty
            nxt = first + count
            ts = mt.tiles(rows, R, cus, b)
            assert sum(rb for _, _, rb in ts) == count
            assert all(rb == 2 for _, _, rb in ts[:-1]) or R == mt.R32   # pairs, then at most one single
            for r0, nr, rb in ts:
                assert r0 % R == 0 and 0 < nr <= rb * R and (rb == 1 or nr > R)   # a pair's second block is never empty
                seen[r0:r0 + nr] += 1
        assert nxt == mt.blocks(rows, R) and (seen == 1).all(), (R, name)


@pytest.mark.parametrize("cus", CUS + [3])
def test_locate_and_weight_rows_agree_with_the_tiles(cus):
    for (R, name), rows in mt.regime_rows(cus).items():
        for b, i, r0, nr, rb in mt.all_tiles(rows, R, cus)[:: max(1, cus // 8)]:
            for row in (r0, r0 + nr - 1):
                assert mt.locate(rows, R, cus, row)[:4] == (b, i, len(mt.tiles(rows, R, cus, b)), rb)
        w = mt.weight_rows(rows, R, cus)
        b, i, n, rb, k = mt.locate(rows, R, cus, w)
        r0 = mt.tiles(rows, R, cus, b)[i][0]
        assert w % 32 != 0 and r0 < w < rows
        if mt.later_tiles(rows, R, cus):
            assert i > 0
        else:   # one tile per workgroup (the 16-row engine at 16 S + 1 and 32 S - 14): the second block of a pair
            assert R == mt.R16 and name in ("16S+1", "32S-14") and rb == 2 and k == 1
    rows = mt.regime_rows(cus)[(mt.R32, mt.SHARED)]
    assert mt.weight_rows(rows, mt.R16, cus) == mt.weight_rows(rows, mt.R32, cus)


def test_below_the_slots_every_workgroup_has_one_block():
    for R in (mt.R16, mt.R32):
        for rows in (1, R, R + 1, 2081, R * 512):
            g = mt.grid(rows, R, 256)
            assert g == mt.blocks(rows, R)
            assert all(mt.tiles(rows, R, 256, b) == [(b * R, min(R, rows - b * R), 1)] for b in range(g))


# ------------------------------------------------------------------------------------------------- planted errors
CUS_SMALL = 4   # 8 workgroups: 32 S + 1 = 257 rows, workgroup 0 has a second tile on either engine


def f32_chain(p, L, x, up):
    """The head in float32 torch (ELU): (out, hiddens, dx, d pre-activations)."""
    W = [p[f"fc{i}.weight"] for i in range(1, L + 1)]
    b = [p[f"fc{i}.bias"] for i in range(1, L + 1)]
    h, hs = x, []
    for l in range(L - 1):
        h = torch.nn.functional.elu(h @ W[l].T + b[l])
        hs.append(h)
    out = h @ W[L - 1].T + b[L - 1]
    g, dz = up, [None] * (L - 1)
    for l in range(L - 1, 0, -1):
        g = (g @ W[l]) * torch.where(hs[l - 1] > 0, torch.ones_like(hs[l - 1]), hs[l - 1] + 1)
        dz[l - 1] = g
    return out, hs, g @ W[0], dz


@pytest.fixture(scope="module", params=list(HEADS))
def planted(request):
    mod, L = HEADS[request.param]
    rows = mt.regime_rows(CUS_SMALL)[(mt.R32, mt.SHARED)]
    rs = np.random.RandomState(5 + L)
    p = {k: torch.tensor(v) for k, v in fx.make_params(6, 7)[mod].items()}
    x, up = rnd(rs, rows, IN), rnd(rs, rows, p[f"fc{L}.weight"].shape[0])
    out, hs, _, dz, dx = chain64(p, L, "elu", x, up)
    gout, ghs, gdx, gdz = f32_chain(p, L, x, up)
    want = {"out": (out, FTOL, None), "hidden": (hs[-1], FTOL, None), "dx": (dx, GTOL, LDX), "d pre-activation": (dz[0], GTOL, None)}
    got = {"out": gout, "hidden": ghs[-1], "dx": gdx, "d pre-activation": gdz[0]}
    return rows, want, got


def passes(buf, view, want, tol):
    return mt.worst_row(view, want)[0] < tol and untouched(buf, *want.shape)


def second_tile_row(rows, R, want):
    """The row of largest norm (by the float64 side alone) in the second tile of workgroup 0."""
    ts = mt.tiles(rows, R, CUS_SMALL, 0)
    assert len(ts) >= 2
    r0, nr, _ = ts[1]
    r = r0 + int(want[r0:r0 + nr].norm(dim=1).argmax())
    assert mt.locate(rows, R, CUS_SMALL, r)[:2] == (0, 1)
    return r


@pytest.mark.parametrize("what", ["out", "hidden", "dx", "d pre-activation"])
def test_the_measure_notices_planted_errors(planted, what):
    rows, wants, gots = planted
    want, tol, ld = wants[what]
    cols = want.shape[1]

    def fresh():
        buf, view = guarded(rows, cols, ld, device="cpu")
        view.copy_(gots[what])
        return buf, view

    buf, view = fresh()
    e = mt.worst_row(view, want)[0]
    assert passes(buf, view, want, tol) and e < 0.2 * tol, e   # float32 arithmetic leaves 5 x and more
    for R in (mt.R16, mt.R32):   # (a) one row of a second tile, off by twice the bound (forward: by 2e-5 as well)
        buf, view = fresh()
        r = second_tile_row(rows, R, want)
        view[r] *= 1 + 2 * tol
        assert not passes(buf, view, want, tol)
        assert mt.worst_row(view, want)[1] == r
        if tol == FTOL:
            buf, view = fresh()
            view[r] *= 1 + 2e-5
            assert not passes(buf, view, want, tol)
    buf, view = fresh()   # (b) one cell of the guard row
    buf[rows, cols // 2] = 0.0
    assert not passes(buf, view, want, tol)
    if ld:   # (c) one guard column cell beside a view
        buf, view = fresh()
        buf[rows // 2, cols] = 0.0
        assert not passes(buf, view, want, tol)
    buf, view = fresh()   # a NaN is the worst there is
    view[rows - 1, 0] = float("nan")
    assert not passes(buf, view, want, tol)


def test_one_wrong_row_hides_in_a_whole_tensor_norm():
    """What the update-sized cases of tests/test_rssm_gpu.py cannot see: one row of 8193 off by 1e-3 moves the
    whole-tensor l2 error by about 1e-3 / sqrt(8193) = 1.1e-5 of FTOL's scale -- and the per-row measure by 1e-3."""
    from tests.util import l2err

    rs = np.random.RandomState(1)
    want = rnd(rs, 8193, HID).double()
    got = want.float()
    got[4321] *= 1 + 1e-3
    assert l2err(got, want) < 2e-5
    e, r = mt.worst_row(got, want)
    assert r == 4321 and 0.9e-3 < e < 1.1e-3
