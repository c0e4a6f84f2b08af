"""The RSSM scan, the imagination rollout, the dense heads and the elementwise losses at every width their engines take.

The agent's widths come from its config (belief_size, state_size, hidden_size) and its task (the action width: 1 for
cartpole, 6 for walker, 12 for quadruped, 21 for humanoid).  The kernel layer picks an engine for each of them by
counting 16-wide blocks (csrc/scan_cs.hip scan_cs_ok, csrc/rssm.hip, csrc/imagine32.hip imagine32_ok,
csrc/imagine16.hip imagine_fused_ok, csrc/mlp16.hip mlp_fused_ok).  One width table drives every test here; each row
names the engines it is expected to select, every case checks from a device trace that exactly that engine ran, and
compares every tensor on its own with float64 autograd of the oracle on the same parameters.

Tolerances are test_rssm_gpu.py's: forward values FTOL relative to the largest element, gradients GTOL normwise.
"""
import math
import re
from collections import namedtuple

import numpy as np
import pytest
import torch

from oracle import fixtures as fx
from oracle import repo_oracle as ro
from tests.util import has, l2err, log, relerr, traced

FTOL = 1e-5
GTOL = 1e-4
E = 1024

W = namedtuple("W", "id D Hd S A scan roll32 roll16 value_fused actor_fused")
# scan: the observe engine at B <= 64 ("cs" column-split, "row" row scan); roll32 / roll16: the rollout engine with
# repo_debug_rowtile32 on / off; *_fused: the head runs as one mlp16 kernel (else layer by layer on the GEMM engine)
WIDTHS = [
    W("default", 200, 200, 30, 6, "cs", "imagine32", "imagine16", True, True),
    W("full-blocks", 208, 208, 32, 16, "cs", "imagine32", "per-step", True, False),
    W("full-blocks-a8", 208, 208, 32, 8, "cs", "imagine32", "imagine16", True, True),
    W("widest-pad", 196, 196, 30, 3, "cs", "imagine32", "imagine16", True, True),
    W("hidden-ne-belief", 200, 208, 30, 6, "cs", "imagine16", "imagine16", True, True),
    W("odd-state", 200, 200, 31, 6, "cs", "imagine16", "imagine16", True, True),
    W("cartpole", 200, 200, 30, 1, "row", "per-step", "per-step", True, True),
    W("quadruped", 200, 200, 30, 12, "cs", "imagine32", "per-step", True, False),
    W("humanoid", 200, 200, 30, 21, "row", "per-step", "per-step", True, False),
    W("belief-not-quad", 202, 200, 30, 6, "row", "per-step", "per-step", True, True),
    W("max-width", 256, 256, 32, 6, "row", "per-step", "per-step", False, False),
    W("wide-state", 200, 200, 58, 6, "row", "per-step", "per-step", False, False),
]
WIDTH_IDS = [w.id for w in WIDTHS]
BY_ID = {w.id: w for w in WIDTHS}


# ----------------------------------------------------------------------------- the selection predicates, in Python
def _blk(k):
    return (k + 15) // 16


def cs_ok(D, Hd, S, A):
    return _blk(D) == 13 and _blk(Hd) == 13 and _blk(S + A) == 3 and 2 * S <= 64 and S <= 32 and D % 4 == 0


def imagine32_ok(D, Hd, S, A, C=0):
    return (D % 4 == 0 and Hd % 4 == 0 and D == Hd and _blk(D) == 13 and _blk(D + S) == 15 and _blk(D + S + C) == 15
            and _blk(S + A) == 3 and _blk(S + A + C) == 3 and 2 * S <= 64 and S % 2 == 0 and 2 * A <= 32)


def imagine16_ok(D, Hd, S, A, C=0):
    return (D % 4 == 0 and Hd % 4 == 0 and _blk(D) == 13 and _blk(Hd) == 13 and _blk(D + S) == 15
            and _blk(D + S + C) == 15 and _blk(S + A) == 3 and _blk(S + A + C) == 3 and _blk(2 * S) == 4 and 2 * A <= 16)


def mlp_fused_ok(in_dim, hidden, out_dim):
    return _blk(in_dim) == 15 and _blk(hidden) == 13 and hidden % 4 == 0 and out_dim <= 16


def rollout_engine(w, rowtile32, C=0):
    if rowtile32 and imagine32_ok(w.D, w.Hd, w.S, w.A, C):
        return "imagine32"
    return "imagine16" if imagine16_ok(w.D, w.Hd, w.S, w.A, C) else "per-step"


def row_scan_tile(B, S=None):
    """The row scan's <rows per workgroup, k-split> instantiation at B rows (csrc/rssm.hip): the forward's (S=None), or
    the reverse's at state width S -- its output-delta role needs R x 2S <= 256 x KQ threads, so S > 32 takes <2, 2>
    from B = 512 up."""
    if B >= 512 and (S is None or 8 * S <= 256):
        return (4, 1)
    return (2, 2) if B >= 128 else (2, 4) if B >= 32 else (1, 4)


def test_width_table_matches_the_selection_predicates():
    """CPU-side: the table's expected engines are what the kernels' predicates (mirrored above) select."""
    for w in WIDTHS:
        assert ("cs" if cs_ok(w.D, w.Hd, w.S, w.A) else "row") == w.scan, w.id
        assert rollout_engine(w, 1) == w.roll32 and rollout_engine(w, 0) == w.roll16, w.id
        assert mlp_fused_ok(w.D + w.S, w.Hd, 1) == w.value_fused, w.id
        assert mlp_fused_ok(w.D + w.S, w.Hd, 2 * w.A) == w.actor_fused, w.id
    assert not imagine32_ok(208, 208, 32, 8, 3) and not imagine16_ok(208, 208, 32, 8, 3)   # D + S + C = 243


# ----------------------------------------------------------------------------- GPU fixtures and helpers
@pytest.fixture(autouse=True)
def _poison_lds(request):
    """Start every GPU test from NaN-filled LDS on all CUs: reads of never-written LDS cannot hide."""
    if "gpu" in request.keywords:
        from repo_amd._lib import lib

        assert lib().repo_debug_poison_lds(torch.cuda.current_stream().cuda_stream) == 0
    yield


@pytest.fixture(scope="module")
def ops():
    assert torch.cuda.is_available()
    from repo_amd import ops as o

    return o


@pytest.fixture
def rowtile32():
    """Set repo_debug_rowtile32 for the test; restored after it."""
    from repo_amd._lib import lib

    prev = lib().repo_debug_rowtile32(1)
    lib().repo_debug_rowtile32(prev)
    yield lambda on: lib().repo_debug_rowtile32(int(on))
    lib().repo_debug_rowtile32(prev)


def params64(w, mod, C=0):
    """One module's parameters at the row's widths: float64 leaves for the reference, float32 device copies."""
    p = fx.make_params(w.A, 7, cond=C, belief=w.D, state=w.S, hidden=w.Hd)[mod]
    p64 = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in p.items()}
    return p64, [torch.from_numpy(v).cuda() for v in p.values()]


def g64(rs, *shape, scale=1.0):
    return torch.from_numpy(rs.standard_normal(shape) * scale).float().double()


def dev(t):
    return t.detach().float().cuda().contiguous()


def row_tiles(names, direction):
    """The <R, KQ> instantiations of the row scan's `direction` ("fwd" / "bwd") kernel in a trace."""
    return {tuple(int(x) for x in m.groups()) for n in names
            for m in [re.search(rf"\bobserve_{direction}_kernel<(\d+), (\d+)>", n)] if m}


def assert_engine(names, kind, engine, what):
    """The kernels that ran are exactly those of `engine`."""
    if kind == "observe":
        cs = r"observe_cs_(fwd|bwd)_kernel"
        if engine == "cs":
            assert has(names, cs) and not has(names, r"\bobserve_(fwd|bwd)_kernel"), (what, names)
        else:   # {"fwd": (R, KQ), "bwd": (R, KQ) or None}: each direction's instantiation on its own
            assert row_tiles(names, "fwd") == {engine["fwd"]}, (what, engine, names)
            assert row_tiles(names, "bwd") == ({engine["bwd"]} if engine["bwd"] else set()), (what, engine, names)
            assert not has(names, cs), (what, names)
    elif kind == "rollout":
        k32, k16 = has(names, r"imagine32_(fwd|bwd)_kernel"), has(names, r"\bimagine_(fwd|bwd)_kernel")
        step = has(names, r"\bgru_(fwd|bwd)_kernel")
        assert (k32, k16, step) == (engine == "imagine32", engine == "imagine16", engine == "per-step"), (what, engine, names)
    elif kind == "mlp":
        assert has(names, r"\bmlp_(fwd|bwd)_kernel") == engine, (what, engine, names)
    log(f"{what}: engine {engine} ran")


def report(what, errs):
    log(f"{what}: " + " ".join(f"{k} {v:.2e}" for k, v in errs.items()))


# ----------------------------------------------------------------------------- observe scan, forward and reverse
OBS_T = {5: 5, 33: 4, 130: 3, 515: 3}


def observe_ref(p, b0, s0, act, emb, non, e1, e2):
    outs = ro.observe(p, b0, s0, act, emb, non, e1, e2)
    bel = outs[0]
    T, B, D = bel.shape
    prev_post = torch.cat([s0[None], outs[4][:-1]], 0)
    xsa = torch.cat([prev_post * non, act], 2)
    e = torch.nn.functional.elu(torch.nn.functional.linear(xsa, p["fc_embed_state_action.weight"], p["fc_embed_state_action.bias"]))
    hp = torch.nn.functional.elu(torch.nn.functional.linear(bel, p["fc_embed_belief_prior.weight"], p["fc_embed_belief_prior.bias"]))
    hq = torch.nn.functional.elu(torch.nn.functional.linear(torch.cat([bel, emb], 2), p["fc_embed_belief_posterior.weight"],
                                                            p["fc_embed_belief_posterior.bias"]))
    return outs, dict(xsa=xsa, e=e, hp=hp, hq=hq)


@pytest.mark.gpu
@pytest.mark.parametrize("B", [5, 33, 130, 515])
@pytest.mark.parametrize("wid", WIDTH_IDS)
def test_observe_scan_at_width(ops, monkeypatch, wid, B):
    """Both scans (where the column-split one is eligible) at the four row-scan instantiations (B = 5, 33, 130, 515: each
    with a ragged last row group), noise as tensors and drawn in the kernels from Philox (the float64 reference takes
    ops.philox_normal of the same ranges: the posterior's stream starts T x B x S after the prior's); every output, the
    saved activations and every gradient of the reverse scan -- dparams, dembeds, dprev_belief, dprev_state."""
    w = BY_ID[wid]
    T, D, Hd, S, A = OBS_T[B], w.D, w.Hd, w.S, w.A
    rs = np.random.RandomState(B * 7 + len(wid))
    p64, p = params64(w, "transition_model")
    act = torch.from_numpy(rs.uniform(-1, 1, (T, B, A))).float().double()
    non = torch.from_numpy((rs.uniform(size=(T, B, 1)) > 0.2).astype(np.float64))
    emb = g64(rs, T, B, E).clamp_min(0).requires_grad_(True)
    b0, s0 = g64(rs, B, D, scale=0.3).requires_grad_(True), g64(rs, B, S).requires_grad_(True)
    seed, off = 4242 + B, 1000 + 3 * B
    e1 = ops.philox_normal(T * B * S, seed, off, torch.device("cuda")).view(T, B, S)
    e2 = ops.philox_normal(T * B * S, seed, off + T * B * S, torch.device("cuda")).view(T, B, S)
    outs, saved = observe_ref(p64, b0, s0, act, emb, non, e1.double().cpu(), e2.double().cpu())
    ups = [g64(rs, *o.shape, scale=0.1) for o in outs]
    sum((o * u).sum() for o, u in zip(outs, ups)).backward()
    names = ["beliefs", "prior_states", "prior_means", "prior_stds", "post_states", "post_means", "post_stds"]
    up = dict(dfeat=dev(torch.cat([ups[0], ups[4]], 2)), dprior_state=dev(ups[1]), dpm=dev(ups[2]), dps=dev(ups[3]),
              dqm=dev(ups[5]), dqs=dev(ups[6]))
    engines = [("0", {"fwd": row_scan_tile(B), "bwd": row_scan_tile(B, S)})]
    if w.scan == "cs" and B <= 130:
        engines.append(("1", "cs"))
    for mode, engine in engines:
        monkeypatch.setenv("REPO_SCAN_CS", mode)
        for noise in ("tensors", "philox"):
            eps = (e1, e2) if noise == "tensors" else (None, None)
            what = f"observe {wid} B={B} T={T} {'cs' if engine == 'cs' else 'row fwd%s bwd%s' % (engine['fwd'], engine['bwd'])} {noise}"
            dp = [torch.zeros_like(t) for t in p]
            demb, dpb, dps_ = torch.empty(T, B, E).cuda(), torch.empty(B, D).cuda(), torch.empty(B, S).cuda()

            def run():
                sv = ops.rssm_observe_fwd(p, dev(b0), dev(s0), dev(act), dev(non), dev(emb), eps[0], eps[1], 0.1,
                                          noise=(seed, off))
                ops.rssm_observe_bwd(p, sv, dp, dembeds=demb, dprev_belief=dpb, dprev_state=dps_, **up)
                return sv

            sv, kern = traced(run)
            assert_engine(kern, "observe", engine, what)
            assert sv.cs == (engine == "cs")
            got = [sv.featx[1:, :, :D], sv.prior_state, sv.prior_mean, sv.prior_std, sv.featx[1:, :, D:], sv.post_mean,
                   sv.post_std]
            errs = {n: relerr(g, o) for n, g, o in zip(names, got, outs)}
            errs.update({n: relerr(getattr(sv, n), t) for n, t in saved.items()})
            report(what + " fwd", errs)
            for n, e in errs.items():
                assert e < FTOL, (what, n, e)
            gerr = {f"d{k}": l2err(g, v.grad) for (k, v), g in zip(p64.items(), dp)}
            gerr.update(dembeds=l2err(demb, emb.grad), dprev_belief=l2err(dpb, b0.grad), dprev_state=l2err(dps_, s0.grad))
            report(what + " bwd", gerr)
            for n, e in gerr.items():
                assert e < GTOL, (what, n, e)
    if w.scan == "row" or B > 64:
        _observe_hoisted_and_prior_only(ops, monkeypatch, w, B, T, p, p64, act, non, emb, b0, s0, e1, e2, seed, off, outs)


def _observe_hoisted_and_prior_only(ops, monkeypatch, w, B, T, p, p64, act, non, emb, b0, s0, e1, e2, seed, off, outs):
    """Where the row scan runs: the prior head hoisted onto a side stream, and prior_only (the open-loop rollout that
    feeds the prior sample forward), Philox noise."""
    monkeypatch.setenv("REPO_SCAN_CS", "0")
    D = w.D
    side = torch.cuda.Stream()
    what = f"observe {w.id} B={B} prior_stream"
    sv, kern = traced(lambda: ops.rssm_observe_fwd(p, dev(b0), dev(s0), dev(act), dev(non), dev(emb), None, None, 0.1,
                                                   noise=(seed, off), prior_stream=side))
    torch.cuda.current_stream().wait_stream(side)
    assert_engine(kern, "observe", {"fwd": row_scan_tile(B), "bwd": None}, what)
    errs = {n: relerr(g, o) for n, g, o in zip(("beliefs", "prior_states", "prior_means", "prior_stds", "post_states"),
                                              (sv.featx[1:, :, :D], sv.prior_state, sv.prior_mean, sv.prior_std,
                                               sv.featx[1:, :, D:]), outs)}
    report(what, errs)
    for n, e in errs.items():
        assert e < FTOL, (what, n, e)
    # prior_only: beliefs, prior samples, means, stds of the open loop
    pr = {k: v.detach() for k, v in p64.items()}
    eps = e1.double().cpu()
    with torch.no_grad():
        bel, st, want = b0.detach(), s0.detach(), [[], [], [], []]
        for t in range(T):
            bel = ro.compute_belief(pr, bel, st * non[t], act[t])
            st, mean, std = ro.gaussian_head(pr, "fc_embed_belief_prior", "fc_state_prior", bel, eps[t])
            for lst, v in zip(want, (bel, st, mean, std)):
                lst.append(v)
    what = f"observe {w.id} B={B} prior_only"
    sv, kern = traced(lambda: ops.rssm_observe_fwd(p, dev(b0), dev(s0), dev(act), dev(non), dev(emb), None, None, 0.1,
                                                   noise=(seed, off), prior_only=True))
    assert_engine(kern, "observe", {"fwd": row_scan_tile(B), "bwd": None}, what)
    errs = {n: relerr(g, torch.stack(o)) for n, g, o in zip(("beliefs", "prior_states", "prior_means", "prior_stds"),
                                                           (sv.featx[1:, :, :D], sv.prior_state, sv.prior_mean,
                                                            sv.prior_std), want)}
    report(what, errs)
    for n, e in errs.items():
        assert e < FTOL, (what, n, e)


# ----------------------------------------------------------------------------- imagination rollout
def _rollout_case(ops, set_rowtile32, w, N, Hm=5, C=0):
    D, S, A = w.D, w.S, w.A
    rs = np.random.RandomState(N + 31 * len(w.id) + C)
    rp64, rp = params64(w, "transition_model", C)
    ap64, ap = params64(w, "actor_model", C)
    for v in rp64.values():
        v.requires_grad_(False)
    b0, s0 = g64(rs, N, D, scale=0.3).requires_grad_(True), g64(rs, N, S).requires_grad_(True)
    cond = None
    if C:
        cond = torch.zeros(N, C, dtype=torch.float64)
        cond[torch.arange(N), torch.from_numpy(rs.randint(0, C, size=N))] = 1.0
    seed, off = 99 + N, 5000 + N
    ea = ops.philox_normal(Hm * N * A, seed, off, torch.device("cuda")).view(Hm, N, A)
    ep = ops.philox_normal(Hm * N * S, seed, off + Hm * N * A, torch.device("cuda")).view(Hm, N, S)
    ea64, ep64 = ea.double().cpu(), ep.double().cpu()
    if C:
        ib, ist, im, isd = ro.cond_imagine(rp64, ap64, b0, s0, cond, Hm + 1, ea64, ep64)
    else:
        ib, ist, im, isd = ro.imagine(rp64, ap64, b0, s0, Hm + 1, ea64, ep64)
    with torch.no_grad():
        fb = torch.cat([b0[None], ib[:-1]], 0).reshape(Hm * N, D)
        fs = torch.cat([s0[None], ist[:-1]], 0).reshape(Hm * N, S)
        if C:
            fs = torch.cat([fs, cond.repeat(Hm, 1)], 1)
        apd = {k: v.detach() for k, v in ap64.items()}
        raw_want = ro.mlp_head(apd, fb, fs, 5)
        am_want, as_want = ro.actor_fwd(apd, fb, fs)
        # the saved intermediates the reverse reads: xsa = [state | action | cond], e, the GRU's [r | z | n | gh_n], hp
        lin = torch.nn.functional.linear
        act = torch.tanh(am_want + as_want * ea64.reshape(Hm * N, A))
        xsa_want = torch.cat([fs[:, :S], act] + ([fs[:, S:]] if C else []), 1)
        e_want = torch.nn.functional.elu(lin(xsa_want, rp64["fc_embed_state_action.weight"], rp64["fc_embed_state_action.bias"]))
        gi = lin(e_want, rp64["rnn.weight_ih"], rp64["rnn.bias_ih"])
        gh = lin(fb, rp64["rnn.weight_hh"], rp64["rnn.bias_hh"])
        r_ = torch.sigmoid(gi[:, :D] + gh[:, :D])
        z_ = torch.sigmoid(gi[:, D:2 * D] + gh[:, D:2 * D])
        n_ = torch.tanh(gi[:, 2 * D:] + r_ * gh[:, 2 * D:])
        gates_want = torch.cat([r_, z_, n_, gh[:, 2 * D:]], 1)
        hp_want = torch.nn.functional.elu(lin(ib.detach().reshape(Hm * N, D), rp64["fc_embed_belief_prior.weight"],
                                              rp64["fc_embed_belief_prior.bias"]))
    ub, us, um, usd = (g64(rs, *x.shape, scale=0.1) for x in (ib, ist, im, isd))
    ((ib * ub).sum() + (ist * us).sum() + (im * um).sum() + (isd * usd).sum()).backward()
    dfeat = dev(torch.cat([ub, us], 2))
    results = {}
    for r32 in (1, 0):
        engine = rollout_engine(w, r32, C)
        for noise in ("tensors", "philox"):
            what = f"rollout {w.id} N={N} Hm={Hm} C={C} rowtile32={r32} {noise}"
            set_rowtile32(r32)
            eps = (ea, ep) if noise == "tensors" else (None, None)

            def run():
                sv = ops.rssm_imagine_fwd(rp, ap, dev(b0), dev(s0), eps[0], eps[1], noise=(seed, off), horizon=Hm,
                                          cond=dev(cond) if C else None)
                d_araw, dfeat0 = ops.rssm_imagine_bwd(rp, sv, dfeat, dprior_mean=dev(um), dprior_std=dev(usd),
                                                      want_dfeat0=True)
                return sv, d_araw, dfeat0

            (sv, d_araw, dfeat0), kern = traced(run)
            assert_engine(kern, "rollout", engine, what)
            errs = {"beliefs": relerr(sv.featx[1:, :, :D], ib), "states": relerr(sv.featx[1:, :, D:], ist),
                    "prior_mean": relerr(sv.prior_mean, im), "prior_std": relerr(sv.prior_std, isd),
                    "a_raw": relerr(sv.a_raw[:Hm * N], raw_want), "a_mean": relerr(sv.a_mean[:Hm * N], am_want),
                    "a_std": relerr(sv.a_std[:Hm * N], as_want), "xsa": relerr(sv.xsa, xsa_want),
                    "e": relerr(sv.e, e_want), "hp": relerr(sv.hp, hp_want)}
            for k, name in enumerate(("gates r", "gates z", "gates n", "gates gh_n")):   # each D-wide block on its own
                errs[name] = relerr(sv.gates[:, k * D:(k + 1) * D], gates_want[:, k * D:(k + 1) * D])
            report(what + " fwd", errs)
            for n, e in errs.items():
                assert e < FTOL, (what, n, e)
            # the deferred actor backward over all steps (mlp_bwd on the saved activations)
            dap = [torch.zeros_like(v) for v in ap]
            x = sv.featx[:Hm].reshape(Hm * N, D + S)
            if C:
                x = torch.cat([x, dev(cond).repeat(Hm, 1)], 1)
            ops.mlp_bwd(ap, x, [sv.a_hidden[l] for l in range(sv.a_hidden.shape[0])], d_araw, dparams=dap, dx=None)
            gerr = {"dbelief0": l2err(dfeat0[:, :D], b0.grad), "dstate0": l2err(dfeat0[:, D:], s0.grad)}
            gerr.update({f"actor d{k}": l2err(g, v.grad) for (k, v), g in zip(ap64.items(), dap)})
            report(what + " bwd", gerr)
            for n, e in gerr.items():
                assert e < GTOL, (what, n, e)
            results[(engine, noise)] = max(gerr.values())
    return results


@pytest.mark.gpu
@pytest.mark.parametrize("N", [28, 300])
@pytest.mark.parametrize("wid", WIDTH_IDS)
def test_rollout_at_width(ops, rowtile32, wid, N):
    """The rollout (Hm = 5 steps; N = 28 and 300 leave both persistent engines a ragged last tile) with rowtile32 on and
    off, noise as tensors and from Philox: every output of the forward, the actor's saved raw outputs / mean / std,
    d feat0 and the deferred actor backward.  Where the 32-row bf16x6 engine and another one both take the shape, its
    worst gradient error may not exceed the 16-row fp32-MFMA engine's by more than 25 % (against the per-step engine's
    GEMMs it is logged only)."""
    w = BY_ID[wid]
    res = _rollout_case(ops, rowtile32, w, N)
    for noise in ("tensors", "philox"):
        if ("imagine32", noise) in res and ("imagine16", noise) in res:
            e32, e16 = res[("imagine32", noise)], res[("imagine16", noise)]
            log(f"rollout {wid} N={N} {noise}: worst gradient error bf16x6 {e32:.2e} fp32 MFMA {e16:.2e}")
            assert e32 <= 1.25 * e16 + 1e-8, (wid, N, noise, res)
        elif ("imagine32", noise) in res and ("per-step", noise) in res:
            log(f"rollout {wid} N={N} {noise}: worst gradient error bf16x6 {res[('imagine32', noise)]:.2e} "
                f"per-step {res[('per-step', noise)]:.2e}")


@pytest.mark.gpu
def test_conditioned_rollout_beyond_the_padding_takes_the_per_step_engine(ops, rowtile32):
    """full-blocks-a8 with a 3-column condition: D + S + C = 243 is past the 15 blocks of either persistent engine, so the
    rollout falls back to the per-step engine -- and is still right."""
    _rollout_case(ops, rowtile32, BY_ID["full-blocks-a8"], 28, C=3)


# ----------------------------------------------------------------------------- heads
def _head_cases():
    seen, out = set(), []
    for w in WIDTHS:
        for mod, L, od in (("reward_model", 4, 1), ("value_model", 4, 1), ("actor_model", 5, 2 * w.A)):
            key = (mod, w.D + w.S, w.Hd, od)
            if key not in seen:
                seen.add(key)
                out.append(pytest.param(w.id, mod, L, id=f"{w.id}-{mod.split('_')[0]}"))
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("rows", [333, 16400])
@pytest.mark.parametrize("wid,mod,L", _head_cases())
def test_head_at_width(ops, wid, mod, L, rows):
    """mlp_fwd / mlp_bwd of each distinct head shape of the table (rows = 16400: the 32-row tiles with a ragged last
    one): output, every hidden activation, every parameter gradient and d x against float64; the value head's two-loss
    chain (dout_w over the first rows_w < rows rows) too."""
    w = BY_ID[wid]
    F_ = w.D + w.S
    rs = np.random.RandomState(rows + len(wid))
    p64, p = params64(w, mod)
    x = g64(rs, rows, F_).requires_grad_(True)
    hs, h = [], x
    for i in range(1, L):
        h = torch.nn.functional.elu(torch.nn.functional.linear(h, p64[f"fc{i}.weight"], p64[f"fc{i}.bias"]))
        hs.append(h)
    want = torch.nn.functional.linear(h, p64[f"fc{L}.weight"], p64[f"fc{L}.bias"])
    fused = mlp_fused_ok(F_, w.Hd, want.shape[1])
    up = g64(rs, *want.shape)
    (want * up).sum().backward(retain_graph=True)
    what = f"head {wid} {mod} rows={rows}"
    dp = [torch.full_like(v, 7.0) for v in p]
    dx = torch.empty(rows, F_).cuda()

    def run():
        out, hid = ops.mlp_fwd(p, dev(x))
        ops.mlp_bwd(p, dev(x), hid, dev(up), dparams=dp, dx=dx)
        return out, hid

    (out, hid), kern = traced(run)
    assert_engine(kern, "mlp", fused, what)
    errs = {"out": relerr(out, want)}
    errs.update({f"hidden{i + 1}": relerr(g, t) for i, (g, t) in enumerate(zip(hid, hs))})
    report(what + " fwd", errs)
    for n, e in errs.items():
        assert e < FTOL, (what, n, e)
    gerr = {f"d{k}": l2err(g, v.grad) for (k, v), g in zip(p64.items(), dp)}
    gerr["dx"] = l2err(dx, x.grad)
    report(what + " bwd", gerr)
    for n, e in gerr.items():
        assert e < GTOL, (what, n, e)
    if mod == "value_model" and rows == 16400:
        rows_w = 16001
        up_x, up_w = g64(rs, rows, 1, scale=1e-3), g64(rs, rows_w, 1, scale=1e-4)
        up_x[::7] = 0.0
        gx, = torch.autograd.grad((want * up_x).sum(), x, retain_graph=True)
        gw = torch.autograd.grad((want[:rows_w] * up_w).sum(), list(p64.values()))
        dp2 = [torch.full_like(v, 7.0) for v in p]
        dx2 = torch.full((rows, F_), 3.0).cuda()
        ops.mlp_bwd(p, dev(x), hid, dev(up_x), dparams=dp2, dx=dx2, dout_w=dev(up_w))
        gerr = {f"d{k}": l2err(g, t) for k, g, t in zip(p64, dp2, gw)}
        gerr["dx"] = l2err(dx2, gx)
        report(what + f" two losses rows_w={rows_w}", gerr)
        for n, e in gerr.items():
            assert e < GTOL, (what, "two losses", n, e)


# ----------------------------------------------------------------------------- elementwise and reduction kernels
ROWS = [2450, 2450 * 15]


@pytest.mark.gpu
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("A", [1, 3, 12, 21])
def test_actor_head_entropy_and_mode_at_action_width(ops, A, rows):
    """actor_head_fwd / _bwd (distribution path and the sampled-action path with eps / state / d action),
    tanh_normal_entropy and tanh_normal_mode against float64, saturated rows included."""
    rs = np.random.RandomState(A * 1000 + rows)
    S, NS = 30, (100 if rows <= 2450 else 10)
    raw = g64(rs, rows, 2 * A, scale=2.0)
    raw[0, :A], raw[1, :A] = 40.0, -40.0          # saturated: tanh(u) rounds to +-1 in fp32
    rawt = raw.clone().requires_grad_(True)
    mean = 5.0 * torch.tanh(rawt[:, :A] / 5.0)
    std = torch.nn.functional.softplus(rawt[:, A:]) + 0.1
    eps_a, state = g64(rs, rows, A), g64(rs, rows, S)
    action = torch.tanh(mean + std * eps_a)
    m, s, xsa = ops.actor_head_fwd(dev(raw), eps=dev(eps_a), state=dev(state))
    errs = {"mean": relerr(m, mean), "std": relerr(s, std), "xsa state": relerr(xsa[:, :S], state),
            "xsa action": relerr(xsa[:, S:], action)}
    # distribution path, then the sampled-action path
    dm_up, ds_up, da_up = g64(rs, rows, A), g64(rs, rows, A), g64(rs, rows, A)
    gd, = torch.autograd.grad((mean * dm_up).sum() + (std * ds_up).sum(), rawt, retain_graph=True)
    ga, = torch.autograd.grad((action * da_up).sum(), rawt, retain_graph=True)
    d1 = ops.actor_head_bwd(m, s, dmean=dev(dm_up), dstd=dev(ds_up))
    d2 = ops.actor_head_bwd(m, s, daction=dev(da_up), action=xsa[:, S:], eps=dev(eps_a))
    gerr = {"draw (mean, std)": l2err(d1, gd), "draw (action)": l2err(d2, ga)}
    # entropy
    eps = g64(rs, NS, rows, A)
    md, sd = mean.detach().requires_grad_(True), std.detach().requires_grad_(True)
    ent = ro.tanh_normal_entropy(md, sd, eps).sum()
    ent.backward()
    out, dmg, dsg = ops.tanh_normal_entropy(m, s, dev(eps), gscale=1.0)
    errs["entropy sum"] = abs(out.item() - ent.item()) / abs(ent.item())
    gerr.update({"entropy dmean": l2err(dmg, md.grad), "entropy dstd": l2err(dsg, sd.grad)})
    what = f"actor head A={A} rows={rows} samples={NS}"
    report(what + " fwd", errs)
    report(what + " bwd", gerr)
    for n, e in errs.items():
        assert e < FTOL, (what, n, e)
    for n, e in gerr.items():
        assert e < GTOL, (what, n, e)
    # mode: the sample of highest log-probability (a near-tie may pick the other one: then their log-probs agree)
    mode = ops.tanh_normal_mode(m, s, dev(eps)).double().cpu()
    with torch.no_grad():
        ys = torch.tanh(mean + std * eps).float().double()
        lp = ro.tanh_normal_log_prob(ys, mean, std)
        best = lp.argmax(0)
        want = ys[best, torch.arange(rows)]
        same = (mode - want).abs().max(1).values <= 1e-6
        lp_got = ro.tanh_normal_log_prob(mode[None], mean, std)[0]
        gap = (lp.max(0).values - lp_got).abs() / lp.abs().max(0).values.clamp_min(1.0)
    log(f"{what} mode: {int((~same).sum())} rows picked another sample; worst log-prob gap {float(gap[~same].max()) if (~same).any() else 0:.2e}")
    assert bool((same | (gap < 1e-5)).all())
    assert float((~same).double().mean()) < 1e-2


@pytest.mark.gpu
@pytest.mark.parametrize("rows", ROWS)
@pytest.mark.parametrize("S", [1, 30, 31, 32, 58, 64])
def test_kl_balance_and_normal_entropy_at_state_width(ops, S, rows):
    """kl_balance in both modes (RePo's balanced KL; Dreamer's free nats, with rows exactly at the threshold: there
    torch.max hands each side half the gradient) and normal_entropy, against float64."""
    rs = np.random.RandomState(S * 100 + rows)
    pm, qm = g64(rs, rows, S), g64(rs, rows, S)
    ps, qs = g64(rs, rows, S).abs() + 0.1, g64(rs, rows, S).abs() + 0.1
    lb, alpha, scale = math.log(0.3), 5 / 6, 1.0 / rows
    P = [t.clone().requires_grad_(True) for t in (pm, ps, qm, qs)]
    klp = ro.normal_kl(P[2].detach(), P[3].detach(), P[0], P[1]).sum(1)
    klq = ro.normal_kl(P[2], P[3], P[0].detach(), P[1].detach()).sum(1)
    (math.exp(lb) * (alpha * klp + (1 - alpha) * klq) * scale).sum().backward()
    out, g = ops.kl_balance(dev(pm), dev(ps), dev(qm), dev(qs), 0, alpha, torch.tensor(lb).float().cuda(), 3.0, scale)
    errs = {"balanced sum": abs(out.item() - klp.sum().item()) / abs(klp.sum().item())}
    gerr = {f"balanced d{n}": l2err(gg, t.grad) for n, gg, t in zip(("pm", "ps", "qm", "qs"), g, P)}
    # free nats: a third of the rows under the threshold, and some exactly at it -- one element of KL exactly 2
    # ((qm - pm) / ps = 2, qs = ps = 1: fp32 and fp64 both give 2), every other element of those rows exactly 0
    qm2, qs2, pm2, ps2 = qm.clone(), qs.clone(), pm.clone(), ps.clone()
    qm2[::3], qs2[::3] = pm2[::3], ps2[::3]
    ties = torch.arange(1, rows, 11)
    pm2[ties], ps2[ties], qm2[ties], qs2[ties] = 0.0, 1.0, 0.0, 1.0
    qm2[ties, 0] = 2.0
    fn = 2.0
    P = [t.clone().requires_grad_(True) for t in (pm2, ps2, qm2, qs2)]
    kl = ro.normal_kl(P[2], P[3], P[0], P[1]).sum(1)
    assert bool((kl[ties] == fn).all())
    tot = torch.max(kl, torch.full((1,), fn, dtype=torch.float64))
    (tot * scale).sum().backward()
    out, g = ops.kl_balance(dev(pm2), dev(ps2), dev(qm2), dev(qs2), 1, 0.0, None, fn, scale)
    errs["free-nats sum"] = abs(out.item() - tot.sum().item()) / abs(tot.sum().item())
    gerr.update({f"free-nats d{n}": l2err(gg, t.grad) for n, gg, t in zip(("pm", "ps", "qm", "qs"), g, P)})
    tie_err = (g[2][ties.cuda()].double().cpu() - P[2].grad[ties]).abs().max().item()
    # normal entropy
    sd = (g64(rs, rows, S).abs() + 0.1).requires_grad_(True)
    ne = (0.5 + 0.5 * math.log(2 * math.pi) + sd.log()).sum()
    (2.0 * ne).backward()
    out, dsd = ops.normal_entropy(dev(sd), gscale=2.0, want_grad=True)
    errs["normal entropy"] = abs(out.item() - ne.item()) / abs(ne.item())
    gerr["normal entropy dstd"] = l2err(dsd, sd.grad)
    what = f"kl / entropy S={S} rows={rows}"
    report(what, {**errs, **gerr, "free-nats tie rows |d qm| err": tie_err})
    for n, e in errs.items():
        assert e < FTOL, (what, n, e)
    for n, e in gerr.items():
        assert e < GTOL, (what, n, e)
    assert tie_err < 1e-6 * (2.0 * scale) + 1e-12, tie_err
