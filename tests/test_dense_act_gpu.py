"""dense_activation_function in {"elu", "relu"} at the op level: every dense kernel that carries the activation, per
tensor, against the float64 restatement of tests/act_ref.py (tied to the pinned oracle by tests/test_dense_act_cpu.py),
on the inputs of tests/act_cases.py (seeds committed there: no ReLU pre-activation within 1e-4 of zero).

Bounds: the ones the ELU tests of tests/test_rssm_gpu.py apply to the same quantities (test_observe_fwd_bwd,
test_imagine_fwd_bwd, test_mlp_fwd_bwd): forward values 1e-5 of the tensor's largest entry, gradients 1e-4 in the l2 norm."""
import re

import pytest
import torch

from tests import act_cases as ac
from tests import act_ref as ar
from tests.util import has, l2err, log, relerr, traced

pytestmark = pytest.mark.gpu

FTOL = 1e-5   # tests/test_rssm_gpu.py FTOL
GTOL = 1e-4   # tests/test_rssm_gpu.py GTOL
ACTS = ["elu", "relu"]


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


def devs(p):
    return [dev(v) for v in p.values()]


def margin_ok(pre, what):
    m = ar.min_abs_pre(pre)
    log(f"{what}: smallest |relu pre-activation| {m:.3e} over {sum(z.numel() for z in pre)}")
    assert m >= ar.PRE_MARGIN, what


def act_id(ops, act):
    return ops.DENSE_ACTIVATIONS[act]


# ----------------------------------------------------------------------------- MLP heads
@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("case", ac.MLP_CASES, ids=lambda c: f"{c.mod}-{c.rows}")
def test_mlp_fwd_bwd_act(ops, case, act):
    """230 -> 200^3 -> 1 and 230 -> 200^4 -> 12 at 1 row, one row past a 16-row tile, and several tiles with a ragged
    tail: output, dx, every dW / db; the fused mlp16 kernel ran."""
    p, x, up = ac.mlp_inputs(case)
    pre = []
    want = ar.mlp_head(p, x, case.layers, act, pre)
    margin_ok(pre, f"mlp {case} {act}")
    (want * up).sum().backward()
    a = act_id(ops, act)
    (out, hid), names = traced(lambda: ops.mlp_fwd(devs(p), dev(x), act=a))
    assert has(names, r"\bmlp_fwd_kernel")
    e = relerr(out, want)
    log(f"mlp {case} {act} out: {e:.2e}")
    assert e < FTOL
    dparams = [torch.full_like(dev(v), 7.0) for v in p.values()]
    dx = torch.ones_like(dev(x))
    _, names = traced(lambda: ops.mlp_bwd(devs(p), dev(x), hid, dev(up), dparams=dparams, dx=dx, accumulate_dx=True, act=a))
    assert has(names, r"\bmlp_bwd_kernel")
    for (k, v), g in zip(p.items(), dparams):
        e = l2err(g, v.grad)
        log(f"mlp {case} {act} d{k}: {e:.2e}")
        assert e < GTOL, k
    e = l2err(dx, x.grad + 1)
    log(f"mlp {case} {act} dx: {e:.2e}")
    assert e < GTOL


# ----------------------------------------------------------------------------- observe scan
OBS_NAMES = ["beliefs", "prior_states", "prior_means", "prior_stds", "post_states", "post_means", "post_stds"]


def _observe_ref(case, act):
    p, x, ups = ac.obs_inputs(case)
    pre = []
    outs = ar.observe(p, x["b0"], x["s0"], x["actions"], x["embeds"], x["nonterms"], x["eps_prior"], x["eps_post"], act, pre)
    margin_ok(pre, f"observe {case.width.id} B={case.B} {act}")
    sum((o * u).sum() for o, u in zip(outs, ups)).backward()
    return p, x, ups, outs


def _observe_gpu(ops, p, x, ups, act, prior_stream=None):
    """-> (the seven outputs, the fourteen parameter gradients, dembeds, kernel names of forward + reverse)."""
    D = x["b0"].shape[1]

    def run():
        sv = ops.rssm_observe_fwd(devs(p), dev(x["b0"]), dev(x["s0"]), dev(x["actions"]), dev(x["nonterms"]),
                                  dev(x["embeds"]), dev(x["eps_prior"]), dev(x["eps_post"]), prior_stream=prior_stream,
                                  act=act)
        if sv.prior_ready is not None:
            torch.cuda.current_stream().wait_stream(sv.prior_ready)
        dparams = [torch.zeros_like(dev(v)) for v in p.values()]
        dembeds = torch.empty_like(dev(x["embeds"]))
        ops.rssm_observe_bwd(devs(p), sv, dparams, dfeat=torch.cat([dev(ups[0]), dev(ups[4])], dim=2).contiguous(),
                             dprior_state=dev(ups[1]), dpm=dev(ups[2]), dps=dev(ups[3]), dqm=dev(ups[5]), dqs=dev(ups[6]),
                             dembeds=dembeds)
        return sv, dparams, dembeds

    (sv, dparams, dembeds), names = traced(run)
    got = [sv.featx[1:, :, :D], sv.prior_state, sv.prior_mean, sv.prior_std, sv.featx[1:, :, D:], sv.post_mean, sv.post_std]
    return got, dparams, dembeds, names


def _observe_check(what, p, x, outs, got, dparams, dembeds):
    for n, g, w in zip(OBS_NAMES, got, outs):
        e = relerr(g, w)
        log(f"{what} {n}: {e:.2e}")
        assert e < FTOL, n
    for (k, v), g in zip(p.items(), dparams):
        e = l2err(g, v.grad)
        log(f"{what} d{k}: {e:.2e}")
        assert e < GTOL, k
    e = l2err(dembeds, x["embeds"].grad)
    log(f"{what} dembeds: {e:.2e}")
    assert e < GTOL


def _row_kernels(names, relu):
    """The row scan ran, in the instantiation of the activation (csrc/rssm.hip: observe_*_kernel / observe_*_relu_kernel)."""
    mine, other = (r"\bobserve_(fwd|bwd)_relu_kernel", r"\bobserve_(fwd|bwd)_kernel") if relu else \
                  (r"\bobserve_(fwd|bwd)_kernel", r"\bobserve_(fwd|bwd)_relu_kernel")
    assert has(names, mine) and not has(names, other) and not has(names, r"observe_cs_"), names


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("hoisted", [False, True], ids=["prior-in-scan", "prior-hoisted"])
@pytest.mark.parametrize("case", ac.OBS_CASES, ids=lambda c: f"{c.width.id}-B{c.B}")
def test_row_scan_fwd_bwd_act(ops, monkeypatch, case, hoisted, act):
    """The row scan with the prior head inside it (prior_only = 0) and hoisted out of it (prior_only = 2: the prior
    hidden layer and its backward are GEMM epilogues): seven outputs, fourteen parameter gradients, dembeds."""
    monkeypatch.setenv("REPO_SCAN_CS", "0")
    p, x, ups, outs = _observe_ref(case, act)
    side = torch.cuda.Stream() if hoisted else None
    got, dparams, dembeds, names = _observe_gpu(ops, p, x, ups, act_id(ops, act), prior_stream=side)
    _row_kernels(names, act == "relu")
    _observe_check(f"row scan {case.width.id} B={case.B} hoisted={hoisted} {act}", p, x, outs, got, dparams, dembeds)


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("case", [c for c in ac.OBS_CASES if c.B in (5, 17)], ids=lambda c: f"{c.width.id}-B{c.B}")
def test_column_split_scan_fwd_bwd_act(ops, monkeypatch, case, act):
    """prior_only = 3 forward, accumulate bit 1 reverse: against the restatement, against the row scan on the same inputs,
    and the status word stays zero."""
    p, x, ups, outs = _observe_ref(case, act)
    a = act_id(ops, act)
    monkeypatch.setenv("REPO_SCAN_CS", "1")
    got, dparams, dembeds, names = _observe_gpu(ops, p, x, ups, a)
    assert has(names, r"observe_cs_fwd_kernel") and has(names, r"observe_cs_bwd_kernel"), names
    assert not has(names, r"\bobserve_(fwd|bwd)(_relu)?_kernel"), names
    assert int(ops.scan_status(torch.device("cuda", torch.cuda.current_device())).item()) == 0
    what = f"column-split scan {case.width.id} B={case.B} {act}"
    _observe_check(what, p, x, outs, got, dparams, dembeds)
    monkeypatch.setenv("REPO_SCAN_CS", "0")
    rgot, rdparams, rdembeds, rnames = _observe_gpu(ops, p, x, ups, a)
    _row_kernels(rnames, act == "relu")
    for n, g, w in zip(OBS_NAMES, got, rgot):
        e = relerr(g, w)
        log(f"{what} vs row scan {n}: {e:.2e}")
        assert e < FTOL, n
    for k, g, w in zip(p, dparams, rdparams):
        e = l2err(g, w)
        log(f"{what} vs row scan d{k}: {e:.2e}")
        assert e < GTOL, k
    assert l2err(dembeds, rdembeds) < GTOL


# ----------------------------------------------------------------------------- rollout
@pytest.fixture(params=[1, 0], ids=["rowtile32", "rowtile16"])
def rollout_engine(request):
    """Both persistent rollout engines (the switch tests/test_rssm_gpu.py uses)."""
    from repo_amd._lib import lib

    prev = lib().repo_debug_rowtile32(request.param)
    yield request.param
    lib().repo_debug_rowtile32(prev)


@pytest.mark.parametrize("act", ACTS)
@pytest.mark.parametrize("case", ac.IMG_CASES, ids=lambda c: f"N{c.N}")
def test_imagine_fwd_bwd_act(ops, rollout_engine, case, act):
    """The RSSM part of a rollout step runs `act`; the ACTOR TRUNK runs ELU whatever `act` is (the reference's agents never
    hand ActorModel the config's activation).  The restatement is built exactly that way: under act = "relu" a kernel that
    applied relu to the actor's layers would miss the saved raw actor outputs, the rollout and every gradient."""
    rp, ap, x, ups = ac.img_inputs(case)
    pre = []
    Hm, N = case.Hm, case.N
    D = x["b0"].shape[1]
    ib, istate, im, isd, raw = ar.imagine(rp, ap, x["b0"], x["s0"], Hm + 1, x["eps_act"], x["eps_prior"], act, "elu", pre)
    margin_ok(pre, f"imagine N={N} {act}")
    sum((o * u).sum() for o, u in zip((ib, istate, im, isd), ups)).backward()
    a = act_id(ops, act)
    sv, names = traced(lambda: ops.rssm_imagine_fwd(devs(rp), devs(ap), dev(x["b0"]), dev(x["s0"]), dev(x["eps_act"]),
                                                    dev(x["eps_prior"]), act=a))
    k32, k16 = has(names, r"imagine32_fwd_kernel"), has(names, r"\bimagine_fwd_kernel")
    assert (k32, k16) == (rollout_engine == 1, rollout_engine == 0), names
    what = f"imagine N={N} engine={'32' if rollout_engine else '16'} {act}"
    for n, g, w in [("beliefs", sv.featx[1:, :, :D], ib), ("states", sv.featx[1:, :, D:], istate),
                    ("means", sv.prior_mean, im), ("stds", sv.prior_std, isd),
                    ("actor raw", sv.a_raw[:Hm * N].view(Hm, N, -1), raw)]:
        e = relerr(g, w)
        log(f"{what} {n}: {e:.2e}")
        assert e < FTOL, n
    dfeat = torch.cat([dev(ups[0]), dev(ups[1])], dim=2).contiguous()
    (d_araw, dfeat0), names = traced(lambda: ops.rssm_imagine_bwd(devs(rp), sv, dfeat, dprior_mean=dev(ups[2]),
                                                                  dprior_std=dev(ups[3]), want_dfeat0=True))
    k32, k16 = has(names, r"imagine32_bwd_kernel"), has(names, r"\bimagine_bwd_kernel")
    assert (k32, k16) == (rollout_engine == 1, rollout_engine == 0), names
    e1, e2 = l2err(dfeat0[:, :D], x["b0"].grad), l2err(dfeat0[:, D:], x["s0"].grad)
    log(f"{what} dbelief0 {e1:.2e} dstate0 {e2:.2e}")
    assert e1 < GTOL and e2 < GTOL
    dap = [torch.zeros_like(dev(v)) for v in ap.values()]
    xs = sv.featx[:Hm].reshape(Hm * N, -1)
    hid = [sv.a_hidden[l] for l in range(sv.a_hidden.shape[0])]
    ops.mlp_bwd(devs(ap), xs, hid, d_araw, dparams=dap, dx=None, act=ops.ACT_ELU)   # the actor trunk: ELU
    for (k, v), g in zip(ap.items(), dap):
        e = l2err(g, v.grad)
        log(f"{what} actor d{k}: {e:.2e}")
        assert e < GTOL, k


def test_backward_refuses_the_other_activation(ops):
    """The saved state remembers the activation of its forward."""
    case = ac.OBS_CASES[0]
    p, x, ups = ac.obs_inputs(case)
    sv = ops.rssm_observe_fwd(devs(p), dev(x["b0"]), dev(x["s0"]), dev(x["actions"]), dev(x["nonterms"]),
                              dev(x["embeds"]), dev(x["eps_prior"]), dev(x["eps_post"]), act=ops.ACT_RELU)
    assert sv.act == ops.ACT_RELU
    with pytest.raises(ValueError):
        ops.rssm_observe_bwd(devs(p), sv, [torch.zeros_like(dev(v)) for v in p.values()], act=ops.ACT_ELU)


# ----------------------------------------------------------------------------- ELU unchanged, unknown ids
def test_act_entry_points_with_elu_are_bit_identical_to_the_legacy_entry_points(ops):
    """One head case and one scan case through the C ABI: repo_mlp_fwd_act / repo_rssm_observe_fwd_act with REPO_ACT_ELU
    against repo_mlp_fwd / repo_rssm_observe_fwd, bit for bit; an unknown activation id is REPO_E_BADARG."""
    from repo_amd._lib import lib

    L_ = lib()
    st = torch.cuda.current_stream().cuda_stream
    ptr = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
    # head
    case = ac.MLP_CASES[1]
    p, x, _ = ac.mlp_inputs(case)
    P, X = devs(p), dev(x)
    rows, in_dim = X.shape
    nb = L_.repo_mlp_fwd_workspace_bytes(rows, in_dim, 200, 1, 4)
    pa = ops.ptr_array(P)
    res = []
    for fn, extra in ((L_.repo_mlp_fwd, ()), (L_.repo_mlp_fwd_act, (ops.ACT_ELU,))):
        hid = [torch.empty(rows, 200, device="cuda") for _ in range(3)]
        out = torch.empty(rows, 1, device="cuda")
        ws = torch.empty(max(nb, 16), dtype=torch.uint8, device="cuda")
        assert fn(rows, in_dim, 200, 1, 4, ptr(X), in_dim, pa, ops.ptr_array(hid), ptr(out), 1, ptr(ws), nb, st, *extra) == 0
        res.append([out] + hid)
    for a, b in zip(*res):
        assert torch.equal(a, b)
    hid = [torch.empty(rows, 200, device="cuda") for _ in range(3)]
    out = torch.empty(rows, 1, device="cuda")
    ws = torch.empty(max(nb, 16), dtype=torch.uint8, device="cuda")
    assert L_.repo_mlp_fwd_act(rows, in_dim, 200, 1, 4, ptr(X), in_dim, pa, ops.ptr_array(hid), ptr(out), 1, ptr(ws), nb, st,
                               2) == -1   # REPO_E_BADARG
    # scan (the row scan, prior head inside)
    c = ac.OBS_CASES[1]
    p, x, _ = ac.obs_inputs(c)
    w, T, B = c.width, c.T, c.B
    P = devs(p)
    pa = ops.ptr_array(P)
    ins = [dev(x[k]) for k in ("b0", "s0", "actions", "nonterms", "embeds", "eps_prior", "eps_post")]
    nb = L_.repo_rssm_observe_fwd_workspace_bytes(T, B, w.A, w.D, w.Hd, w.S, ac.E)
    res = []
    for fn, extra in ((L_.repo_rssm_observe_fwd, ()), (L_.repo_rssm_observe_fwd_act, (ops.ACT_ELU,))):
        f = lambda *s: torch.empty(*s, device="cuda")   # noqa: E731
        outs = [f(T + 1, B, w.D + w.S)] + [f(T, B, w.S) for _ in range(5)] + \
               [f(T, B, w.S + w.A), f(T, B, w.D), f(T, B, 4 * w.D), f(T, B, w.Hd), f(T, B, w.Hd), f(T, B, w.Hd)]
        ws = torch.empty(nb, dtype=torch.uint8, device="cuda")
        rc = fn(T, B, w.A, w.D, w.Hd, w.S, ac.E, pa, *[ptr(t) for t in ins], 0, 0, 0.1, *[ptr(t) for t in outs], 0, None,
                ptr(ws), nb, st, *extra)
        assert rc == 0
        res.append(outs[:-1])   # (eemb is scratch)
    torch.cuda.synchronize()
    for a, b in zip(*res):
        assert torch.equal(a, b)
