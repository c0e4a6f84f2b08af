"""The fused head chains where a workgroup walks SEVERAL row tiles: past 2 x CUs blocks both engines (csrc/mlp16.hip,
16-row fp32 blocks; csrc/mlp32.hip, 32-row bf16x6 tiles) keep their grid at 2 x CUs workgroups and each workgroup takes a
contiguous run of tiles.  Everything carried from one tile to the next lives in that loop: the next tile's input rows
issued during the current tile's last layer (mlp16: into the buffer that layer does not read, and Ta / Tb swapped per tile
for odd L only -- the 5-layer actor and the 4-layer value head take different paths; mlp32: XLoad32 registers), the first
weight window of the next tile opened before the current one ends (mopen32), blocks taken in pairs then at most one single
(mlp16), column-tile ownership rotating per tile, and a ragged `nr` on a tile that is not the workgroup's first.

tests/mlp_tiles.py restates which rows a workgroup takes; its seven row counts (a function of the device's CU count) are
the smallest that reach each transition -- 8193 .. 32 769 rows at 256 CUs -- and tests/test_mlp_persistent_cpu.py holds
them against the mirror and shows that the measure below notices one wrong row and one written guard cell.

Per case -- engine (forced by REPO_MLP32_MIN_ROWS, proven from the device trace by the helpers of tests/test_mlp32_gpu.py)
x its row counts x the value head (230 -> 200^3 -> 1, L = 4) and the actor head (230 -> 200^4 -> 12, L = 5) x ELU
(ReLU at 32 S + 1, inputs scaled by 16) -- one forward (out and every saved hidden) or one reverse in the modes dx / dsave /
both / acc / dual (dx and every saved pre-activation gradient, read out of the patterned workspace), with x and dx
row-slice views of pitch 237, a guard row behind every written buffer, guard columns beside views and the workspace's
bytes up to the next 256-byte boundary.  The scalar head's second upstream ends (rows_w) inside a tile that is not its
workgroup's first, and on no multiple of 32.

Measure, per row r of each tensor against the float64 restatement (chain64, on the device):
|got_r - want_r|_2 / max(|want_r|_2, rms over rows of |want_r|_2) < FTOL (forward) / GTOL (gradients) -- one wrong row of
30 000 shows as it is, where a whole-tensor norm dilutes it by sqrt(rows).  A float32 torch restatement of these chains
stays at or below 1.9e-6 per row, so the bounds leave 5 x and more to fp32 arithmetic.  The worst row of every tensor is
logged with the workgroup and the tile of that workgroup it belongs to.  ReLU: rows with a float64 pre-activation within
act_ref.PRE_MARGIN of zero leave the float64 GRADIENT comparisons (chosen by the restatement alone; at least 9 of 10 stay).

At 32 S + 1, the count both engines take, the two are compared on the same operands with every row kept, under the 25 %
rule of tests/test_mlp32_gpu.py (both_engines, pooled_rule).

Left out: the heads' parameter gradients at these counts (tests/test_dense_wgrad_gpu.py's kernels), widths other than
230 / 200."""
import functools

import numpy as np
import pytest
import torch

from oracle import fixtures as fx
from tests import act_ref as ar
from tests import mlp_tiles as mt
from tests.test_mlp32_gpu import (FTOL, GTOL, HEADS, IN, _poison_lds, both_engines, chain64, forward, ops,  # noqa: F401
                                  pooled_rule, reverse)
from tests.util import log, rnd

pytestmark = pytest.mark.gpu

MODES = ("dx", "dsave", "both", "acc", "dual")   # dual (two upstream gradients through one chain): scalar heads only


def steps(head):
    return ("fwd",) + tuple(m for m in MODES if m != "dual" or head == "value")


# (head, act, regime, R, step), sorted so that the cases sharing a float64 reference -- (head, act, rows): at 32 S + 1
# both engines -- are adjacent
CASES = sorted(((h, a, name, R, s) for R, name, _ in mt.REGIMES for h in HEADS for a in ("elu", "relu")
                if a == "elu" or name == mt.SHARED for s in steps(h)),
               key=lambda c: (c[0], c[1], c[2], c[3]))
VERSUS = [(h, a, s) for h in HEADS for a in ("elu", "relu") for s in ("fwd", "both", "dual") if s != "dual" or h == "value"]


@functools.lru_cache(maxsize=None)
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


@functools.lru_cache(maxsize=None)
def rows_of(R, name):
    return mt.regime_rows(cus())[(R, name)]


@functools.lru_cache(maxsize=2)   # (one case at 32 769 rows holds about 0.3 GB of float64, on the device)
def case(head, act, rows, rows_w):
    """Operands (seeds and scale of tests/test_mlp32_gpu.py's case()) and the float64 restatement, on the device."""
    mod, L = HEADS[head]
    rs = np.random.RandomState(9000 + 7 * rows + L)
    p = {k: torch.tensor(v).cuda() for k, v in fx.make_params(6, 7)[mod].items()}
    O = p[f"fc{L}.weight"].shape[0]
    x, up = rnd(rs, rows, IN, scale=16.0 if act == "relu" else 1.0).cuda(), rnd(rs, rows, O).cuda()
    up_w = torch.zeros(rows, 1, device="cuda")
    up_w[:rows_w] = rnd(rs, rows_w, 1, scale=0.1).cuda()
    out, hs, zs, dz, dx = chain64(p, L, act, x, up)
    good = None
    if act == "relu":
        good = torch.ones(rows, dtype=torch.bool, device="cuda")
        for z in zs:
            good &= z.abs().min(dim=1).values >= ar.PRE_MARGIN
        kept = int(good.sum())
        log(f"mlp persistent {head} relu rows={rows}: {kept} rows ({100.0 * kept / rows:.1f} %) clear the margin")
        assert 10 * kept >= 9 * rows, (head, rows, kept)
    del zs
    c = dict(head=head, act=act, rows=rows, L=L, O=O, p=p, x=x, up=up, rows_w=rows_w, up_w=up_w, out=out, hs=hs, dz=dz, dx=dx,
             good=good)
    if O == 1:   # two upstreams through one chain: dx from `up`, the saved gradients from up_w (zero past rows_w)
        c["dz_w"] = chain64(p, L, act, x, up_w)[3]
    return c


def shared_case(head, act):
    """The case at 32 S + 1: one rows_w serves both engines (inside the second tile of workgroup 0 on either)."""
    rows = rows_of(mt.R32, mt.SHARED)
    assert rows == rows_of(mt.R16, mt.SHARED)
    w = mt.weight_rows(rows, mt.R32, cus())
    assert w == mt.weight_rows(rows, mt.R16, cus())
    return case(head, act, rows, w)


def case_of(head, act, name, R):
    if name == mt.SHARED:
        return shared_case(head, act)
    rows = rows_of(R, name)
    return case(head, act, rows, mt.weight_rows(rows, R, cus()))


def check(c, R, what, got, want, tol, keep=None):
    """The per-row measure of one tensor, logged with where its worst row ran; `keep`: the rows that are compared."""
    assert got.shape == want.shape, (what, got.shape, want.shape)
    idx = torch.arange(c["rows"], device=got.device)
    if keep is not None:
        got, want, idx = got[keep], want[keep], idx[keep]
    e, i = mt.worst_row(got, want)
    log(f"mlp persistent R={R} {what}: worst row {e:.2e}  {mt.where(c['rows'], R, cus(), int(idx[i]))}")
    assert e < tol, (what, e, int(idx[i]))


_hid = {}   # the saved hiddens of the last (case, engine), shared by its reverse variants and left unchanged


def hiddens(ops, monkeypatch, c, R):
    key = (c["head"], c["act"], c["rows"], R)
    if key not in _hid:
        _hid.clear()
        _hid[key] = forward(ops, monkeypatch, c, R == mt.R32)
    return _hid[key]


def dual_lies_in_a_later_tile(c, R):
    b, i, n, rb, k = mt.locate(c["rows"], R, cus(), c["rows_w"])
    r0 = mt.tiles(c["rows"], R, cus(), b)[i][0]
    assert c["rows_w"] % 32 != 0 and c["rows_w"] > r0, (c["rows_w"], r0)   # ends inside the tile, not on its edge
    # a tile that is not its workgroup's first; 16 S + 1 and 32 S - 14 on the 16-row engine have none (one tile per
    # workgroup): there it is the second block of a pair
    assert i > 0 or (not mt.later_tiles(c["rows"], R, cus()) and rb == 2 and k == 1), (b, i, n, rb, k)


@pytest.mark.parametrize("head,act,name,R,step", CASES, ids=lambda v: str(v))
def test_chain_over_several_tiles(ops, monkeypatch, head, act, name, R, step):
    c = case_of(head, act, name, R)
    what = f"{head} {act} rows={c['rows']} ({name}) {step}"
    if step == "fwd":
        _hid.clear()
        out, hid = hiddens(ops, monkeypatch, c, R)
        check(c, R, f"{what} out", out, c["out"], FTOL)
        for l, (h, w) in enumerate(zip(hid, c["hs"])):
            check(c, R, f"{what} hidden {l}", h, w, FTOL)
        return
    if step == "dual":
        dual_lies_in_a_later_tile(c, R)
    dx, ds = reverse(ops, monkeypatch, c, hiddens(ops, monkeypatch, c, R)[1], step, R == mt.R32)
    assert (dx is None) == (step == "dsave") and (ds is None) == (step == "dx")
    if dx is not None:
        check(c, R, f"{what} dx", dx, c["dx"] + (3.0 if step == "acc" else 0.0), GTOL, c["good"])
    if ds is not None:
        for l, w in enumerate(c["dz_w"] if step == "dual" else c["dz"]):
            check(c, R, f"{what} d pre-activation {l}", ds[l], w, GTOL, c["good"])


def worst(got, want):
    return mt.worst_row(got, want)[0]


@pytest.mark.parametrize("head,act,step", VERSUS, ids=lambda v: str(v))
def test_engine_against_engine_where_both_walk_tiles(ops, monkeypatch, head, act, step):
    """32 S + 1 rows: workgroup 0 runs pair then single on the 16-row engine and two tiles on the 32-row one."""
    c = shared_case(head, act)
    what, pool = f"persistent {head} {act} rows={c['rows']} {step}", []
    out32, hid32 = forward(ops, monkeypatch, c, True)
    if step == "fwd":
        out16, hid16 = forward(ops, monkeypatch, c, False)
        both_engines(pool, f"{what} out", out32, out16, c["out"], worst, FTOL)
        for l, (h32, h16, w) in enumerate(zip(hid32, hid16, c["hs"])):
            both_engines(pool, f"{what} hidden {l}", h32, h16, w, worst, FTOL)
    else:   # both engines from the same saved hiddens: every row is kept between them
        dx32, ds32 = reverse(ops, monkeypatch, c, hid32, step, True)
        dx16, ds16 = reverse(ops, monkeypatch, c, hid32, step, False)
        both_engines(pool, f"{what} dx", dx32, dx16, c["dx"], worst, GTOL, c["good"])
        for l, w in enumerate(c["dz_w"] if step == "dual" else c["dz"]):
            both_engines(pool, f"{what} d pre-activation {l}", ds32[l], ds16[l], w, worst, GTOL, c["good"])
    pooled_rule(pool, what)
