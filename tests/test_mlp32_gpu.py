"""The fused dense heads on 32-row tiles and the bf16 matrix pipe (csrc/mlp32.hip), forced at every row count by
REPO_MLP32_MIN_ROWS=0 and proven from the device trace (the engine's instantiations carry a fifth template argument, 32).

Per case -- rows in {1, 31, 32, 33, 77, 2081} (one lane of a tile, one row short of / exactly / one past a tile, three
tiles with a ragged last, 66 tiles: more than one tile per workgroup is reached only past 2 x CUs tiles, where
tests/test_mlp_persistent_gpu.py takes both engines through every transition of their tile loops with the helpers of this
module) x the value head (230 -> 200^3 -> 1) and the actor head
(230 -> 200^4 -> 12) x ELU / ReLU -- outputs, saved hiddens, dx and every saved pre-activation gradient are compared

  * with a float64 restatement of the chain, at the FTOL / GTOL of tests/test_rssm_gpu.py;
  * with the 16-row fp32 engine (REPO_MLP32_MIN_ROWS beyond any row count) on the same operands, at the same bounds;
  * and the new engine's float64 error may exceed the fp32 engine's by at most 25 % (+ 1e-8: the rule of
    test_head_weight_gradients_on_the_bf16_pipe_match_fp64_and_the_fp32_engine for the six-product split), in the l2
    norm.  Both errors are rounding noise, and the ratio of two l2 norms of n noise samples scatters by about 1 / sqrt(n):
    the rule is applied to a tensor alone where it has at least 1000 elements (3 % scatter: 25 % is eight of them), and
    in every case to all of its tensors pooled (the one output of a 1-row scalar head alone is ONE sample: a few ulps
    either way).

ReLU has no agreed derivative within rounding of zero: rows with a float64 pre-activation closer to zero than
act_ref.PRE_MARGIN are left out of the float64 GRADIENT comparisons (chosen by the restatement alone, never by a kernel's
result); the engine-against-engine comparison, whose two sides share the saved activations, keeps every row.

The input is a row-slice view with ldx = 237 > in_dim, dx one with lddx = 237; every buffer a kernel writes has a guard
row behind it (and guard columns beside it where it is a view) that must come back untouched; the pre-activation
gradients live in the call's workspace, where the bytes up to the next 256-byte boundary are the guard."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import fixtures as fx
from tests import act_ref as ar
from tests.util import has, l2err, log, relerr, rnd, traced

pytestmark = pytest.mark.gpu

FTOL = 1e-5   # tests/test_rssm_gpu.py FTOL
GTOL = 1e-4   # tests/test_rssm_gpu.py GTOL
K32 = r"\bmlp_%s_kernel<[^>]*,\s*32>"
IN, HID, LDX = 230, 200, 237
HEADS = {"value": ("value_model", 4), "actor": ("actor_model", 5)}
ROWS = [1, 31, 32, 33, 77, 2081]
ACTS = ["elu", "relu"]
S = -777.25   # sentinel of the guard rows / columns
SB = 0x5A     # ... and of the workspace bytes
FAR = str(10 ** 9)
SEED_BUMP = {("actor", 1): 300}   # (found on the restatement alone: the one row's ReLU pre-activations clear the margin)


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


def chain64(p, L, act, x, up):
    """float64: (out, hiddens, pre-activations, d pre-activations, dx) of the head for the upstream gradient `up`."""
    W = [p[f"fc{i}.weight"].double() for i in range(1, L + 1)]
    b = [p[f"fc{i}.bias"].double() for i in range(1, L + 1)]
    h, hs, zs = x.double(), [], []
    for l in range(L - 1):
        z = h @ W[l].T + b[l]
        h = F.elu(z) if act == "elu" else F.relu(z)
        zs.append(z)
        hs.append(h)
    out = h @ W[L - 1].T + b[L - 1]
    g, dz = up.double(), [None] * (L - 1)
    for l in range(L - 1, 0, -1):
        hh = hs[l - 1]
        d = (hh > 0).double() if act == "relu" else torch.where(hh > 0, torch.ones_like(hh), hh + 1)
        g = (g @ W[l]) * d
        dz[l - 1] = g
    return out, hs, zs, dz, g @ W[0]


@functools.lru_cache(maxsize=None)
def case(head, act, rows):
    mod, L = HEADS[head]
    rs = np.random.RandomState(9000 + 7 * rows + L + SEED_BUMP.get((head, rows), 0))
    p = {k: torch.tensor(v) for k, v in fx.make_params(6, 7)[mod].items()}
    O = p[f"fc{L}.weight"].shape[0]
    # ReLU: wider inputs, hence wider pre-activations, put fewer of them inside the margin (tests/act_cases.py MLP_SCALE);
    # not at one row, whose few hundred pre-activations clear it as they are: the one output of a scalar head is the
    # tensor's largest entry whatever it is, and 16 x wider terms cancelling into it are 16 x its rounding error
    x, up = rnd(rs, rows, IN, scale=16.0 if act == "relu" and rows > 1 else 1.0), rnd(rs, rows, O)
    rows_w = max(1, rows // 2)       # 15, 16, 16, 38, 1040: below rows, none a multiple of 32
    up_w = torch.zeros(rows, 1)
    up_w[:rows_w] = rnd(rs, rows_w, 1, scale=0.1)
    out, hs, zs, dz, dx = chain64(p, L, act, x, up)
    good = torch.ones(rows, dtype=torch.bool)
    if act == "relu":
        for z in zs:
            good &= z.abs().min(dim=1).values >= ar.PRE_MARGIN
    # the margin rule leaves most rows of every case (the only row of a 1-row case) in the float64 gradient comparison
    assert int(good.sum()) >= max(1, (3 * rows) // 4), (head, act, rows, int(good.sum()))
    c = dict(head=head, act=act, rows=rows, L=L, O=O, p=p, x=x, up=up, rows_w=rows_w, up_w=up_w, out=out, hs=hs, dz=dz, dx=dx,
             good=good)
    if O == 1:   # two upstreams through one chain: dx from `up`, the saved gradients from up_w (zero past rows_w)
        c["dz_w"] = chain64(p, L, act, x, up_w)[3]
    return c


def guarded(rows, cols, ld=None, fill=S, device="cuda"):
    """-> (buffer of rows + 1 rows of ld columns, all sentinel; its [rows, cols] view)."""
    buf = torch.full((rows + 1, ld or cols), fill, dtype=torch.float32, device=device)
    return buf, buf[:rows, :cols]


def untouched(buf, rows, cols):
    return bool((buf[rows:] == S).all()) and bool((buf[:rows, cols:] == S).all())


def device_x(c):
    buf = torch.full((c["rows"] + 1, LDX), 1e30, dtype=torch.float32, device="cuda")   # (a value that would show in a sum)
    buf[:c["rows"], :IN] = c["x"].cuda()
    return buf[:c["rows"], :IN]


def params(c):
    return [v.cuda().contiguous() for v in c["p"].values()]


def forward(ops, monkeypatch, c, engine32):
    monkeypatch.setenv("REPO_MLP32_MIN_ROWS", "0" if engine32 else FAR)
    rows, L, O = c["rows"], c["L"], c["O"]
    ob, out = guarded(rows, O)
    hb = [guarded(rows, HID) for _ in range(L - 1)]
    a = ops.DENSE_ACTIVATIONS[c["act"]]
    _, names = traced(lambda: ops.mlp_fwd(params(c), device_x(c), out=out, hid=[h for _, h in hb], act=a))
    assert has(names, r"\bmlp_fwd_kernel") and has(names, K32 % "fwd") == engine32, names
    assert untouched(ob, rows, O) and all(untouched(b, rows, HID) for b, _ in hb)
    return out, [h for _, h in hb]


def reverse(ops, monkeypatch, c, hid, mode, engine32):
    """mode: dx | dsave | both | acc (accumulate_dx onto 3.0) | dual (dout_w).  -> (dx or None, dsave (L-1, rows, 200) or None)."""
    from repo_amd._lib import lib

    monkeypatch.setenv("REPO_MLP32_MIN_ROWS", "0" if engine32 else FAR)
    rows, L, O = c["rows"], c["L"], c["O"]
    a = ops.DENSE_ACTIVATIONS[c["act"]]
    want_dx, want_w = mode != "dsave", mode != "dx"
    db = dx = None
    if want_dx:
        db, dx = guarded(rows, IN, LDX)
        if mode == "acc":
            dx.fill_(3.0)
    dparams = [torch.zeros_like(v) for v in params(c)] if want_w else None
    nb = lib().repo_mlp_bwd_workspace_bytes(rows, IN, HID, O, L)
    ws = torch.full((max(nb, 1 << 20),), SB, dtype=torch.uint8, device="cuda")
    idx = torch.cuda.current_device()
    kw = dict(dout_w=c["up_w"][:c["rows_w"]].cuda().contiguous()) if mode == "dual" else {}

    def run():
        with ops.scratch_scope({(idx, ops._raw_stream(idx)): ws}):
            ops.mlp_bwd(params(c), device_x(c), hid, c["up"].cuda(), dparams=dparams, dx=dx, accumulate_dx=mode == "acc",
                        act=a, **kw)

    _, names = traced(run)
    assert has(names, r"\bmlp_bwd_kernel") and has(names, K32 % "bwd") == engine32, names
    if want_dx:
        assert untouched(db, rows, IN), mode
    nd = (L - 1) * rows * HID * 4
    pad = ws[nd:(nd + 255) // 256 * 256]
    assert bool((pad == SB).all()), mode
    if not want_w:
        assert bool((ws[:nd] == SB).all()), mode   # nothing kept: nothing written
        return dx, None
    return dx, ws[:nd].view(torch.float32).view(L - 1, rows, HID).clone()


MIN_SAMPLE = 1000


def sq(a, b):
    return float((a.detach().double().cpu() - b.detach().double().cpu()).pow(2).sum())


def both_engines(pool, what, got32, got16, want, measure, tol, rows=None):
    """The comparisons of one tensor; `rows`: the rows that enter the float64 comparison.  The tensor joins `pool`."""
    sel = (lambda t: t[rows.to(t.device)]) if rows is not None else (lambda t: t)
    e32, e16, ee = measure(sel(got32), sel(want)), measure(sel(got16), sel(want)), measure(got32, got16)
    n32, n16, n = l2err(sel(got32), sel(want)), l2err(sel(got16), sel(want)), sel(want).numel()
    log(f"mlp32 {what}: fp64 error bf16x6 {e32:.2e}  fp32 {e16:.2e}  |  between the engines {ee:.2e}  |  l2 {n32:.2e}  {n16:.2e}  n={n}")
    assert e32 < tol and e16 < tol and ee < tol, (what, e32, e16, ee)
    if n >= MIN_SAMPLE:
        assert n32 <= 1.25 * n16 + 1e-8, (what, n32, n16)
    w2 = float(sel(want).double().pow(2).sum()) + 1e-300
    pool.append((sq(sel(got32), sel(want)) / w2, sq(sel(got16), sel(want)) / w2, n))


def pooled_rule(pool, what):
    """The 25 % rule over all of a case's tensors: each tensor's squared l2 error, weighted by its element count."""
    n = sum(k for _, _, k in pool)
    p32, p16 = (sum(e[0] * e[2] for e in pool) / n) ** 0.5, (sum(e[1] * e[2] for e in pool) / n) ** 0.5
    log(f"mlp32 {what}: pooled fp64 l2 error bf16x6 {p32:.2e}  fp32 {p16:.2e}  n={n}")
    assert p32 <= 1.25 * p16 + 1e-8, (what, p32, p16)


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("head", list(HEADS))
@pytest.mark.parametrize("rows", ROWS)
def test_forward_chain(ops, monkeypatch, rows, head, act):
    c = case(head, act, rows)
    out32, hid32 = forward(ops, monkeypatch, c, True)
    out16, hid16 = forward(ops, monkeypatch, c, False)
    what, pool = f"{head} {act} rows={rows}", []
    both_engines(pool, f"{what} out", out32, out16, c["out"], relerr, FTOL)
    for l, (h32, h16, w) in enumerate(zip(hid32, hid16, c["hs"])):
        both_engines(pool, f"{what} hidden {l}", h32, h16, w, relerr, FTOL)
    pooled_rule(pool, what)


_hid = {}   # the saved hiddens of a case (the bf16 engine's), shared by its reverse variants and left unchanged


# two upstream gradients through one chain ("dual"): scalar heads only (repo_mlp_bwd)
REVERSE = [(r, h, a, m) for r in ROWS for h in HEADS for a in ACTS for m in ("dx", "dsave", "both", "acc", "dual")
           if m != "dual" or h == "value"]


@pytest.mark.parametrize("rows,head,act,mode", REVERSE, ids=lambda v: str(v))
def test_reverse_chain(ops, monkeypatch, rows, head, act, mode):
    c = case(head, act, rows)
    if (head, act, rows) not in _hid:
        _hid[(head, act, rows)] = forward(ops, monkeypatch, c, True)[1]
    hid = _hid[(head, act, rows)]
    dx32, ds32 = reverse(ops, monkeypatch, c, hid, mode, True)
    dx16, ds16 = reverse(ops, monkeypatch, c, hid, mode, False)
    what, pool = f"{head} {act} rows={rows} {mode}", []
    if dx32 is not None:
        both_engines(pool, f"{what} dx", dx32, dx16, c["dx"] + (3.0 if mode == "acc" else 0.0), l2err, GTOL, c["good"])
    if ds32 is not None:
        for l, w in enumerate(c["dz_w"] if mode == "dual" else c["dz"]):
            both_engines(pool, f"{what} d pre-activation {l}", ds32[l], ds16[l], w, l2err, GTOL, c["good"])
    pooled_rule(pool, what)
