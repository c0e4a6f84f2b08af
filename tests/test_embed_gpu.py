"""config.embedding_size != 1024 on the GPU: the encoder's `fc` 1024 -> E and the E-wide decoder head per tensor, the
observe scans at embedding widths other than 1024 (the hoisted embedding product and its weight gradient into the column
block [D, D + E) of a (D + E)-pitch matrix: at E = 250 that pitch is 450 floats and rows are 8-byte aligned only), the
discriminator at input_dim 250, every pixel agent against goldens the REFERENCE produced at E = 250 / 64
(tests/golden/gen_golden_embed.py), the acting path, checkpoints and the data-parallel update.

Bounds are the project's own:
 * TOL = 1e-5 normwise (tests/util.relerr) for op-level values and per-tensor gradients: tests/test_ops_gpu.py;
 * FTOL = 1e-5 / GTOL = 1e-4 for the scan: tests/test_rssm_gpu.py;
 * goldens as tests/test_inv_dyn_gpu.py: scalars 1e-3 relative, gradient norms 2e-3, latents rtol 1e-3, parameter
   checksums 1e-3 |abs-sum| + 1e-6.  The RePo / Dreamer, TIA and multitask golden tests ARE the existing ones
   (tests/test_update_gpu.py, test_tia_gpu.py, test_mt_gpu.py), run with tests/embed_ref.py:FixturesAt(E) in the place of
   the `fx` those modules build their agents from: same loop, same bounds, uint8 and float frames alternating.

On the parent commit everything that builds a module or an agent at E != 1024 fails with the NotImplementedError this
width used to raise; the scan and discriminator tests (which only ever took E as a run-time argument) pass there."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import fixtures as fx
from oracle import repo_oracle as orc
from tests import act_ref as ar
from tests import calib_pair_ref as cp
from tests import calib_ref as cr
from tests import embed_ref as er
from tests import inv_dyn_ref as ir
from tests import test_calib_gpu as tcg
from tests import test_calib_pair_gpu as tpg
from tests import test_host_gpu as thg
from tests import test_mt_gpu as tmg
from tests import test_ops_gpu as tog
from tests import test_tia_gpu as ttg
from tests import test_update_gpu as tu
from tests.util import l2err, log, relerr, rnd

pytestmark = pytest.mark.gpu

TOL = 1e-5    # tests/test_ops_gpu.py
FTOL = 1e-5   # tests/test_rssm_gpu.py
GTOL = 1e-4   # tests/test_rssm_gpu.py
A = 6


@pytest.fixture(autouse=True)
def _poison_lds():
    from repo_amd._lib import lib

    assert lib().repo_debug_poison_lds(torch.cuda.current_stream().cuda_stream) == 0
    yield


def dev(t):
    return t.cuda().contiguous()


def at(monkeypatch, E):
    """Every agent factory of the existing GPU tests reads its configuration and parameters through its module's `fx`."""
    fa = er.FixturesAt(E)
    for mod in (tu, ttg, tmg):
        monkeypatch.setattr(mod, "fx", fa)
    return fa


# ----------------------------------------------------------------------------- 1. the encoder, per tensor
def _frames(rs, n, image, u8):
    raw = rs.randint(0, 256, size=(n, 3, image, image)).astype(np.uint8)
    f32 = torch.from_numpy(fx.preprocess_u8(raw))
    return (torch.from_numpy(raw) if u8 else f32), f32.double()


def _cot(rs, n, E):
    """The upstream gradient of an encoder test: zero-mean noise on a per-column offset of +-(1 .. 2), over n.  A bias
    gradient is ONE sum per channel over frames and positions, and a sum of zero-mean terms cancels to a few roots of its sum
    of squares, which no fp32 summation is bounded relative to (tests/test_conv_engines_gpu.py, class Data, says the same
    and offsets its operands for the same reason; with a zero-mean upstream d conv1.bias over 513 x 961 terms came out at
    1.15e-5 of |want| on an MI355X in one of four cases, 3e-7 .. 4e-6 in the others).  With the offset every frame pushes a
    given activation the same way and the sums do not cancel across frames: in float64, at E = 250 and 513 frames, sum |terms|
    over |sum of terms| of d conv1.bias (largest channel) falls from 244 to 13, of d conv2.bias from 111 to 10.  All ten
    gradients are judged against |want|."""
    off = (rs.randint(0, 2, size=E) * 2 - 1) * (1 + rs.uniform(size=E))
    return torch.from_numpy(((off[None, :] + rs.standard_normal((n, E))) / n).astype(np.float32))


def _check_backward(tag, names, wants, bwd, rs):
    """bwd(g=None, **kw) -> the gradients in `names` order.  Each within TOL; accumulate=True adds to pre-filled gradients; a
    side stream gives the serial run's bits."""
    got = bwd()
    torch.cuda.synchronize()
    errs = {k: relerr(a, w) for k, a, w in zip(names, got, wants)}
    log(f"{tag}: " + " ".join(f"d {k} {e:.2e}" for k, e in errs.items()))
    bad = {k: e for k, e in errs.items() if e >= TOL}
    assert not bad, (tag, bad)
    pre = [dev(rnd(rs, *w.shape, scale=0.5 * float(w.abs().max()))) for w in wants]
    for k, a, w, b in zip(names, bwd(g=[t.clone() for t in pre], accumulate=True), wants, pre):
        e = relerr(a, w + b.double().cpu())
        assert e < TOL, (tag, "accumulate", k, e)
    assert all(torch.equal(a, b) for a, b in zip(bwd(side=torch.cuda.Stream()), got)), (tag, "side stream")


def _encoder_case(monkeypatch, E, n, u8, image):
    import repo_amd.functional as Fn

    rs = np.random.RandomState(1000 * image + 10 * E + n + int(u8))
    P = er.make_params(A, E, seed=E + n, image=image)["encoder"]
    assert list(P)[8:] == ["fc.weight", "fc.bias"] and P["fc.weight"].shape == (E, 1024 if image == 64 else 9216)
    p = [dev(torch.from_numpy(v)) for v in P.values()]
    obs, obs64 = _frames(rs, n, image, u8)
    embeds, saved = Fn.encoder_fwd(p, dev(obs))
    assert tuple(embeds.shape) == (n, E)
    if image == 64:
        assert len(saved) == 7 and saved[5] is not None and saved[6] is not None   # the channel-quad masks are kept
    P64 = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in P.items()}
    with torch.no_grad():
        want = orc.encoder_fwd(P64, obs64)
    e = relerr(embeds, want)
    log(f"encoder {image} E={E} n={n} u8={u8}: embeds {e:.2e}")
    assert e < TOL, e
    # the ReLU decisions of the GPU's own activations (as the decoder test of tests/test_ops_gpu.py takes them)
    gates = [(h > 0).double().cpu() for h in saved[:4]]
    monkeypatch.setattr(orc, "RELU_TIE_BREAK", lambda i, pre, h: pre * gates[i - 1])
    cot = _cot(rs, n, E)
    (orc.encoder_fwd(P64, obs64) * cot.double()).sum().backward()
    monkeypatch.setattr(orc, "RELU_TIE_BREAK", None)
    wants = [P64[k].grad for k in P]
    dcot = dev(cot)

    def bwd(g=None, **kw):
        g = [torch.empty_like(t) for t in p] if g is None else g
        Fn.encoder_bwd(p, dev(obs), saved, dcot, g, **kw)
        return g

    _check_backward(f"encoder {image} E={E} n={n} u8={u8}", list(P), wants, bwd, rs)


@pytest.mark.parametrize("u8", [True, False], ids=["u8", "f32"])
@pytest.mark.parametrize("n", [12, 513])
@pytest.mark.parametrize("E", [64, 250, 1536])
def test_encoder_with_fc_matches_fp64_per_tensor(monkeypatch, E, n, u8):
    """Fn.encoder_fwd / encoder_bwd on the 64 x 64 stack with the reference's fc 1024 -> E: embeds and all ten gradients
    against float64 autograd of oracle encoder_fwd; 513 frames: more than one row tile, and past the 512 rows from which
    the bf16x6 engine may take the fc's products at E >= 512."""
    _encoder_case(monkeypatch, E, n, u8, 64)


def test_encoder_with_fc_at_an_odd_width(monkeypatch):
    """E = 251: K % 2 != 0 sends the fc's data gradient to the gather engine, and the rows of d embeds are 4-byte aligned."""
    _encoder_case(monkeypatch, 251, 12, True, 64)


def test_encoder_128_stack_at_250(monkeypatch):
    _encoder_case(monkeypatch, 250, 12, True, 128)


def _cond_enc64(P, obs, cond, gates=None):
    """oracle cond_encoder_fwd (its lines, with the gates of _encoder_case) followed by the reference's fc."""
    gs, bs = orc._film(P, cond, (32, 64, 128, 256))
    h = obs
    for i in range(4):
        pre = orc._mod(F.conv2d(h, P[f"conv{i + 1}.weight"], P[f"conv{i + 1}.bias"], stride=2), gs[i], bs[i])
        h = F.relu(pre) if gates is None else pre * gates[i]
    flat = h.reshape(h.shape[0], -1)
    return flat, F.linear(flat, P["fc.weight"], P["fc.bias"])


def test_film_encoder_with_fc_matches_fp64_per_tensor():
    import repo_amd.functional_mt as Fm

    E, C, n = 250, 3, 12
    rs = np.random.RandomState(77)
    P = er.make_params(A, E, seed=5, cond=C)["encoder"]
    assert list(P)[8:] == ["fc.weight", "fc.bias", "film.weight", "film.bias"]
    p = [dev(torch.from_numpy(v)) for v in P.values()]
    obs, obs64 = _frames(rs, n, 64, True)
    cond = torch.from_numpy(np.eye(C, dtype=np.float32)[rs.randint(0, C, size=n)])
    embeds, saved = Fm.cond_encoder_fwd(p, dev(obs), dev(cond))
    assert tuple(embeds.shape) == (n, E)
    P64 = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in P.items()}
    with torch.no_grad():
        flat, want = _cond_enc64(P64, obs64, cond.double())
        assert torch.equal(flat, orc.cond_encoder_fwd(P64, obs64, cond.double()))   # the restatement IS the oracle's stack
    e = relerr(embeds, want)
    log(f"film encoder E={E}: embeds {e:.2e}")
    assert e < TOL, e
    gates = [(h > 0).double().cpu() for h in saved[2]]
    cot = _cot(rs, n, E)
    (_cond_enc64(P64, obs64, cond.double(), gates)[1] * cot.double()).sum().backward()
    wants = [P64[k].grad for k in P]
    dcot = dev(cot)

    def bwd(g=None, **kw):
        g = [torch.empty_like(t) for t in p] if g is None else g
        Fm.cond_encoder_bwd(p, dev(obs), dev(cond), saved, dcot, g, **kw)
        return g

    _check_backward(f"film encoder E={E}", list(P), wants, bwd, rs)


# ----------------------------------------------------------------------------- 2. the decoder, per tensor
def _compose_rule(rows, F_, E, compose):
    return rows >= 512 and compose == "1" and E * (F_ + 3200) > F_ * 3200


DEC_CASES = [(512, 230, 250, "64"), (512, 230, 1536, "64"), (511, 230, 250, "64"), (512, 230, 64, "64"), (512, 231, 250, "64"),
             (512, 230, 250, "tia"), (512, 230, 250, "128")]


@pytest.mark.parametrize("compose", ["1", "0"])
@pytest.mark.parametrize("rows,F_,E,stack", DEC_CASES)
def test_decoder_at_other_embedding_widths_matches_fp64_per_tensor(monkeypatch, rows, F_, E, stack, compose):
    """tests/test_ops_gpu.py's decoder test with fc1 (E, F) and conv1 (E, 128, 5, 5): every activation, the output, the NLL
    and its gradient, each parameter gradient and d feat against float64 autograd of the two-layer form; the composed head
    engages exactly when the multiplication count says (functional._dec_compose) -- not at E = 64."""
    import repo_amd.functional as Fn

    monkeypatch.setenv("REPO_DEC_COMPOSE", compose)
    image, tia = (128 if stack == "128" else 64), stack == "tia"
    rs = np.random.RandomState(rows + 7 * F_ + E + len(stack))
    P = er.make_params(A, E, seed=rows + F_, image=image, tia=tia, belief=F_ - 30, state=30)["obs_model"]
    assert P["fc1.weight"].shape == (E, F_) and P["conv1.weight"].shape[0] == E
    p = [dev(torch.from_numpy(v)) for v in P.values()]
    feat = rnd(rs, rows, F_, scale=0.7)
    u8, tgt = tog._dec_frames(rs, rows, image)
    gs = 1.0 / rows
    if tia:
        out, saved = Fn.decoder_fwd(p, dev(feat))
        cot = rnd(rs, *out.shape, scale=gs)
        saved = (*saved, dev(cot))
    else:
        loss, saved = Fn.decoder_fwd_nll(p, dev(feat), dev(u8), gs)
        out, _ = Fn.decoder_fwd(p, dev(feat))
    composed = isinstance(saved[0], Fn.DecHead)
    assert composed == _compose_rule(rows, F_, E, compose), (rows, F_, E, compose, type(saved[0]))
    nrelu = 4 if image == 128 else 3
    hs_gpu = saved[1 : 1 + nrelu]
    P64 = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in P.items()}
    feat64 = feat.double().requires_grad_(True)
    errs = {}
    with torch.no_grad():
        h0w, hsw, outw = tog._dec64(P64, feat64)
    if not composed:
        errs["h0"] = relerr(saved[0], h0w)
    for i, (hg, hw) in enumerate(zip(hs_gpu, hsw), 1):
        errs[f"h{i}"] = relerr(hg, hw)
    errs["out"] = relerr(out, outw)
    if not tia:
        d = outw - tgt
        want_loss = (0.5 * d * d).sum().item()
        errs["nll"] = abs(loss.item() - want_loss) / want_loss
        errs["dpre"] = relerr(saved[4] if image == 64 else saved[5], d * gs)
    del h0w, hsw, outw
    gates = [(h > 0).double().cpu() for h in hs_gpu]
    _, _, out64 = tog._dec64(P64, feat64, gates=gates)
    if tia:
        (out64 * cot.double()).sum().backward()
    else:
        (0.5 * gs * (out64 - tgt).pow(2)).sum().backward()
    del out64, gates
    names = list(P) + ["dfeat"]
    wants = [P64[k].grad for k in P] + [feat64.grad]
    tag = f"decoder {stack} rows={rows} F={F_} E={E} compose={compose} (composed {composed})"
    log(f"{tag}: " + " ".join(f"{k} {e:.2e}" for k, e in errs.items()))
    bad = {k: e for k, e in errs.items() if e >= TOL}
    assert not bad, bad

    def bwd(g=None, accumulate=False, **kw):
        g = [torch.empty_like(t) for t in p] + [torch.empty(rows, F_, device="cuda")] if g is None else g
        Fn.decoder_bwd(p, dev(feat), saved, g[:-1], dfeat=g[-1], accumulate=accumulate, accumulate_dfeat=accumulate, **kw)
        return g

    _check_backward(tag, names, wants, bwd, rs)


@pytest.mark.parametrize("compose", ["1", "0"])
def test_cond_decoder_at_250_matches_fp64_per_tensor(monkeypatch, compose):
    """The multitask decoder (FiLM on conv1..conv3) at (rows, F, E) = (512, 230, 250), composed and two-layer."""
    import repo_amd.functional as Fn
    import repo_amd.functional_mt as Fm

    monkeypatch.setenv("REPO_DEC_COMPOSE", compose)
    rows, F_, E, C = 512, 230, 250, 3
    rs = np.random.RandomState(E + 31)
    P = er.make_params(A, E, seed=7, cond=C)["obs_model"]
    p = [dev(torch.from_numpy(v)) for v in P.values()]
    feat = rnd(rs, rows, F_, scale=0.7)
    cond = torch.from_numpy(np.eye(C, dtype=np.float32)[rs.randint(0, C, size=rows)])
    u8, tgt = tog._dec_frames(rs, rows, 64)
    gs = 1.0 / rows
    loss, saved = Fm.cond_decoder_fwd_nll(p, dev(feat), dev(cond), dev(u8), gs)
    out, _ = Fm.cond_decoder_fwd(p, dev(feat), dev(cond))
    composed = isinstance(saved[1], Fn.DecHead)
    assert composed == _compose_rule(rows, F_, E, compose), (compose, type(saved[1]))
    hs_gpu = saved[3]
    P64 = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in P.items()}
    feat64 = feat.double().requires_grad_(True)
    film = lambda: orc._film(P64, cond.double(), (128, 64, 32))  # noqa: E731
    errs = {}
    with torch.no_grad():
        _, hsw, outw = tog._dec64(P64, feat64, film=film())
    for i, (hg, hw) in enumerate(zip(hs_gpu, hsw), 1):
        errs[f"h{i}"] = relerr(hg, hw)
    errs["out"] = relerr(out, outw)
    d = outw - tgt
    want_loss = (0.5 * d * d).sum().item()
    errs["nll"] = abs(loss.item() - want_loss) / want_loss
    errs["dpre"] = relerr(saved[4], d * gs)
    del hsw, outw, d
    gates = [(h > 0).double().cpu() for h in hs_gpu]
    _, _, out64 = tog._dec64(P64, feat64, gates=gates, film=film())
    (0.5 * gs * (out64 - tgt).pow(2)).sum().backward()
    del out64, gates
    tag = f"cond decoder rows={rows} F={F_} E={E} compose={compose} (composed {composed})"
    log(f"{tag}: " + " ".join(f"{k} {e:.2e}" for k, e in errs.items()))
    bad = {k: e for k, e in errs.items() if e >= TOL}
    assert not bad, bad
    wants = [P64[k].grad for k in P] + [feat64.grad]

    def bwd(g=None, accumulate=False, **kw):
        g = [torch.empty_like(t) for t in p] + [torch.empty(rows, F_, device="cuda")] if g is None else g
        Fm.cond_decoder_bwd(p, dev(feat), dev(cond), saved, g[:-1], dfeat=g[-1], accumulate=accumulate,
                            accumulate_dfeat=accumulate, **kw)
        return g

    _check_backward(tag, list(P) + ["dfeat"], wants, bwd, rs)


# ----------------------------------------------------------------------------- 3. the observe scans at E != 1024
# relu: the first seed >= 0 at which every ReLU pre-activation of the float64 restatement keeps act_ref.PRE_MARGIN from zero
# at (T, B) = (4, 3) (7200 of them), searched on the CPU with tests/act_ref.py alone as tests/act_cases.py's were; the
# embeddings carry that file's EMB_SCALE, which widens the posterior layer's pre-activations
SCAN_RELU_SEEDS = {64: 21, 250: 18, 251: 2, 1536: 27}
EMB_SCALE = 4.0


def _scan_inputs(T, B, E, act, D=200, S=30):
    P = er.make_params(A, E)["transition_model"]
    assert P["fc_embed_belief_posterior.weight"].shape == (200, D + E)
    seed = SCAN_RELU_SEEDS[E] if act == "relu" else 0
    rs = np.random.RandomState(100 * T + B + E + 1000 * seed)
    x = dict(actions=rnd(rs, T, B, A), nonterms=torch.from_numpy((rs.uniform(size=(T, B, 1)) > 0.2).astype(np.float32)),
             embeds=F.relu(rnd(rs, T, B, E, scale=EMB_SCALE)), e1=rnd(rs, T, B, S), e2=rnd(rs, T, B, S),
             b0=rnd(rs, B, D, scale=0.3), s0=rnd(rs, B, S))
    x["ups"] = [rnd(rs, T, B, w, scale=0.1) for w in (D, S, S, S, S, S, S)]
    return P, x


def _scan_case(monkeypatch, T, B, E, act, cs):
    from repo_amd import ops

    D, S = 200, 30
    monkeypatch.setenv("REPO_SCAN_CS", cs)
    P, x = _scan_inputs(T, B, E, act)
    p64 = {k: torch.from_numpy(v).double().requires_grad_(True) for k, v in P.items()}
    emb64 = x["embeds"].double().requires_grad_(True)
    args = (x["b0"].double(), x["s0"].double(), x["actions"].double(), emb64, x["nonterms"].double(), x["e1"].double(),
            x["e2"].double())
    pre = []
    outs = ar.observe(p64, *args, act, pre)
    if act == "relu":
        assert (T, B) == (4, 3) and ar.min_abs_pre(pre) >= ar.PRE_MARGIN, ar.min_abs_pre(pre)
    if act == "elu":   # tests/act_ref.py's ELU form is the oracle's (tests/test_dense_act_cpu.py); here once more, directly
        with torch.no_grad():
            for a, b in zip(outs, orc.observe(p64, *args)):
                assert float((a - b).abs().max()) <= 1e-12
    sum((o * u.double()).sum() for o, u in zip(outs, x["ups"])).backward()
    p = [dev(torch.from_numpy(v)) for v in P.values()]
    sv = ops.rssm_observe_fwd(p, dev(x["b0"]), dev(x["s0"]), dev(x["actions"]), dev(x["nonterms"]), dev(x["embeds"]),
                              dev(x["e1"]), dev(x["e2"]), act=ops.DENSE_ACTIVATIONS[act])
    assert sv.cs == (cs == "1")
    got = [sv.featx[1:, :, :D], sv.prior_state, sv.prior_mean, sv.prior_std, sv.featx[1:, :, D:], sv.post_mean, sv.post_std]
    tag = f"observe E={E} T={T} B={B} {act} cs={cs}"
    for n, g, w in zip(("beliefs", "prior_states", "prior_means", "prior_stds", "post_states", "post_means", "post_stds"),
                       got, outs):
        e = relerr(g, w)
        log(f"{tag} {n}: {e:.2e}")
        assert e < FTOL, (n, e)
    ups = x["ups"]
    dfeat = dev(torch.cat([ups[0], ups[4]], dim=2))
    kw = dict(dfeat=dfeat, dprior_state=dev(ups[1]), dpm=dev(ups[2]), dps=dev(ups[3]), dqm=dev(ups[5]), dqs=dev(ups[6]))
    dparams = [torch.zeros_like(t) for t in p]
    dembeds = torch.full((T, B, E), 7.0, device="cuda")
    ops.rssm_observe_bwd(p, sv, dparams, dembeds=dembeds, **kw)
    for (k, v), g in zip(p64.items(), dparams):
        e = l2err(g, v.grad)
        log(f"{tag} d{k}: {e:.2e}")
        assert e < GTOL, (k, e)
    # fc_embed_belief_posterior.weight, all D + E columns: the belief's block and the embedding's, each on its own
    gq, wq = dparams[10], p64["fc_embed_belief_posterior.weight"].grad
    assert tuple(gq.shape) == (200, D + E)
    for name, sl in (("belief block", slice(0, D)), ("embedding block", slice(D, D + E))):
        e = l2err(gq[:, sl], wq[:, sl])
        log(f"{tag} d W_bq {name}: {e:.2e}")
        assert e < GTOL, (name, e)
    e = l2err(dembeds, emb64.grad)
    log(f"{tag} dembeds: {e:.2e}")
    assert e < GTOL, e
    return p, sv, kw, dembeds


@pytest.mark.parametrize("cs", ["0", "1"], ids=["rowscan", "colsplit"])
@pytest.mark.parametrize("act", ["elu", "relu"])
@pytest.mark.parametrize("E", [64, 250, 251, 1536])   # 251: odd K of the embedding product (gather engine), pitch 451
def test_observe_scan_at_other_embedding_widths(monkeypatch, E, act, cs):
    from repo_amd import ops

    T, B = 4, 3
    p, sv, kw, dembeds = _scan_case(monkeypatch, T, B, E, act, cs)
    if E == 250:   # the frozen reverse scan (no weight-gradient product) gives the full one's d embeds, bit for bit
        frozen = torch.full((T, B, E), 7.0, device="cuda")
        ops.rssm_observe_bwd(p, sv, None, dembeds=frozen, **kw)
        assert torch.equal(frozen, dembeds)


def test_observe_scan_where_the_embedding_gradient_takes_the_bf16_engine_and_where_not(monkeypatch):
    """d embeds = d hq @ W_bq[:, D:] is the (T B, E, Hd) product of the reverse scan -- the one product of the scan whose
    engine depends on E (the embedding product and its weight gradient have Hd = 200 output columns or rows: never the
    bf16x6 engine's).  The library is asked which shapes it sends to that engine; one of each kind runs."""
    from repo_amd._lib import lib

    found = {}
    for T, B, E in ((4, 3, 250), (13, 130, 1536), (16, 130, 1536), (13, 130, 250), (26, 130, 1024)):
        pays = int(lib().repo_gemm_nt_pays(T * B, E, 200))
        found.setdefault(pays, (T, B, E))
    assert sorted(found) == [0, 1], found
    assert found[1][2] != 1024, found   # a width other than 1024 reaches the engine
    for pays in (1, 0):
        T, B, E = found[pays]
        log(f"observe E={E} T={T} B={B}: repo_gemm_nt_pays({T * B}, {E}, 200) = {pays}")
        _scan_case(monkeypatch, T, B, E, "elu", "0")


# ----------------------------------------------------------------------------- 4. the discriminator at input_dim = 250
DISC_250 = (32, 32, 250, 32, 8)   # (N_real, N_fake, E, Hf, Z) of tests/test_calib_gpu.py
DISC_250_SEED = 12                # the first of 0..63 with min |pre| >= PRE_MARGIN, both modes (picked on the CPU)


@pytest.mark.parametrize("support", [False, True], ids=["js", "support"])
def test_discriminator_at_250_train_step_and_input_gradient(monkeypatch, support):
    """tests/test_calib_gpu.py's forward / generator-side and train-step tests (their bounds) at one more case."""
    monkeypatch.setattr(tcg, "CASES", tcg.CASES + [DISC_250])
    ci = len(tcg.CASES) - 1
    monkeypatch.setitem(tcg.SEEDS, (ci, support), DISC_250_SEED)
    tcg.reference.cache_clear()
    try:
        tcg.test_forward_and_generator_side_match_the_restatement(ci, support)
        tcg.test_train_steps_parameters_and_beta_and_repeats_bit_for_bit(ci, support)
    finally:
        tcg.reference.cache_clear()


# ----------------------------------------------------------------------------- 5. the agents against the goldens
@pytest.mark.parametrize("fname,algo,E", [("repo_embed250_tiny.npz", "repo", 250), ("dreamer_embed64_tiny.npz", "dreamer", 64)])
def test_update_matches_reference_goldens(monkeypatch, golden_dir, fname, algo, E):
    at(monkeypatch, E)
    tu.test_update_matches_reference_goldens(golden_dir, fname, algo)


def test_tia_update_matches_reference_golden(monkeypatch, golden_dir):
    at(monkeypatch, 250)
    tu_names = np.load(os.path.join(golden_dir, "tia_embed250_tiny.npz"))["param_names"]
    assert "encoder.fc.weight" in [str(n) for n in tu_names]
    ttg.test_tia_update_matches_reference_goldens(golden_dir, "tia_embed250_tiny.npz")


def test_mt_repo_update_matches_reference_golden(monkeypatch, golden_dir):
    at(monkeypatch, 250)
    tmg.test_mt_update_matches_reference_goldens(golden_dir, "mt_repo_embed250_tiny.npz", "repo_multitask")


def _check_golden_scalars(fname, g, u, scal):
    keys = [str(k) for k in g["scalar_keys"]]
    for k, w in zip(keys, g[f"u{u}/scalars"]):
        r = abs(scal[k] - w) / (abs(w) + 1e-12)
        log(f"[{fname}] update {u} {k}: got {scal[k]:.7g} ref {w:.7g} rel {r:.2e}")
        assert r < 1e-3, (fname, u, k, scal[k], w)


def _check_golden_checksums(g, agent, modules):
    have = {}
    for m in modules:
        for k, v in getattr(agent, m).state_dict().items():
            have[f"{m}.{k}"] = (float(v.double().sum()), float(v.double().abs().sum()))
    names = [str(n) for n in g["param_names"]]
    assert sorted(names) == sorted(have)
    assert "encoder.fc.weight" in names and "encoder.fc.bias" in names
    for n, s_, a_ in zip(names, g["param_sums"], g["param_abssums"]):
        assert abs(have[n][1] - a_) <= 1e-3 * abs(a_) + 1e-6, (n, have[n][1], a_)
        assert abs(have[n][0] - s_) <= 1e-3 * abs(a_) + 1e-6, (n, have[n][0], s_)


def test_finetuned_repo_matches_reference_golden(monkeypatch, golden_dir):
    """FinetunedRePo.train_encoder at E = 250 (the golden half of tests/test_tia_gpu.py's test): the encoder optimiser is a
    view of the model optimiser over TEN tensors; the frozen modules do not move."""
    at(monkeypatch, 250)
    fname = "finetune_embed250_tiny.npz"
    g = np.load(os.path.join(golden_dir, fname))
    L, B, H, A_, n_updates = (int(x) for x in g["meta"])
    init_beta, target_kl = (float(x) for x in g["cfg"])
    agent, cfg = ttg.make_finetuned(L, B, H, A_, init_beta=init_beta, target_kl=target_kl)
    assert len(agent.encoder_optimizer.params) == 10
    # (offsets in the flat buffer are 16-byte aligned: the 250-float fc.bias is followed by two padding floats)
    assert agent.encoder_optimizer.numel == agent.model_optimizer.offsets[10]
    assert 0 <= agent.encoder_optimizer.numel - sum(t.numel() for t in agent.encoder.parameters()) < 4 * 10
    frozen0 = {m: torch.cat([q.detach().reshape(-1).clone() for q in getattr(agent, m).parameters()])
               for m in ("transition_model", "reward_model", "obs_model", "actor_model", "value_model")}
    for u in range(n_updates):
        batch, _ = tu.dev_batch(L, B, A_, 11 + u, u8=(u % 2 == 0))
        agent.noise_source = {k: torch.from_numpy(v).cuda() for k, v in fx.make_noise(L, B, H, A_, seed=101 + u).items()}
        agent.train_encoder(batch[0], batch[1], batch[2], 1.0 - batch[3])
        _check_golden_scalars(fname, g, u, agent.last_scalars)
        tn = float(g[f"u{u}/total_norms"][0])
        assert abs(agent.last_grad_norms["encoder"] - tn) / tn < 2e-3
        assert abs(float(agent.log_beta) - float(g[f"u{u}/log_beta"])) < 1e-5
    _check_golden_checksums(g, agent, fx.MODULES)
    for m, before in frozen0.items():
        assert torch.equal(before, torch.cat([q.detach().reshape(-1) for q in getattr(agent, m).parameters()])), m


def make_calib_agent_at(E, mode, L=8, B=4, H=5, **over):
    """tests/test_calib_gpu.py:make_calib_agent with the seeded parameters of tests/embed_ref.py at width E."""
    from repo_amd.algorithms.repo import CalibratedRePo
    from repo_amd.common.utils import set_gpu_mode

    set_gpu_mode(True)
    cfg = fx.default_config(algo="repo_calibrate", batch_size=B, chunk_size=L, horizon=H, alignment_mode=mode, embedding_size=E,
                            **{**cr.CALIB_CFG, **over})
    agent = CalibratedRePo(cfg, tu.Env(A), tu.Env(A), tcg.PairedEnv(A), tu.Logger())
    params = er.make_params(A, E, 7)
    for mod in fx.MODULES:
        agent._load_module(getattr(agent, mod), {k: torch.from_numpy(v) for k, v in params[mod].items()})
    agent._load_module(agent.src_encoder, {k: torch.from_numpy(v) for k, v in params["encoder"].items()})
    agent._load_module(agent.encoder, {k: torch.from_numpy(v) for k, v in er.make_params(A, E, 9)["encoder"].items()})
    for mod, p in ((agent.disc, cr.make_disc_params(E, cfg.f_hidden_size, cfg.f_latent_size)),
                   (agent.log_tau, cr.make_tau_params(E, cfg.f_hidden_size))):
        assert list(mod.state_dict().keys()) == list(p.keys())
        agent._load_module(mod, {k: torch.from_numpy(v) for k, v in p.items()})
    return agent, cfg


def test_calibration_steps_match_the_reference_golden(golden_dir):
    """CalibratedRePo, simple_pair, alignment_mode="js" at E = 250: the loop and bounds of tests/test_calib_gpu.py."""
    fname = "calib_js_embed250_tiny.npz"
    g = np.load(os.path.join(golden_dir, fname))
    L, B, H, A_, n_updates = (int(x) for x in g["meta"])
    agent, cfg = make_calib_agent_at(250, "js", L, B, H)
    assert len(agent.src_encoder.plist()) == 10 and len(agent.encoder_optimizer.params) == 10
    keys = [str(k) for k in g["scalar_keys"]]
    modules = [str(m) for m in g["grad_norm_modules"]]
    for u in range(n_updates):
        scal = tcg.calib_step(agent, cfg, u)
        assert sorted(scal.keys()) == keys
        _check_golden_scalars(fname, g, u, scal)
        for name, got, w in (("disc beta", float(agent.disc.beta), float(g[f"u{u}/disc_beta"])),
                             ("u", float(agent.u.detach()), float(g[f"u{u}/u"]))):
            assert abs(got - w) <= 1e-3 * abs(w), (name, got, w)
        for name, w in zip(modules, g[f"u{u}/grad_norms"]):
            r = abs(agent.last_grad_norms[name] - w) / w
            log(f"[{fname}] step {u} grad-norm {name}: got {agent.last_grad_norms[name]:.6g} ref {w:.6g} rel {r:.2e}")
            assert r < 2e-3, (name, agent.last_grad_norms[name], w)
    _check_golden_checksums(g, agent, ("encoder", "disc", "log_tau", "src_encoder"))


# ----------------------------------------------------------------------------- 6. calibration_mode="pair" at E = 250
@pytest.mark.parametrize("mode", ["js", "support"])
def test_pair_latent_losses_reach_250_wide_embeddings_as_float64_autograd_does(mode):
    """tests/calib_pair_ref.py takes the embeddings as they come (any width): tests/test_calib_pair_gpu.py's comparison of
    CalibratedRePo._latent_losses with float64 autograd through it, at E = 250, in both alignment modes (the mode decides
    the discriminator's loss, not this half; both agents must build and run it)."""
    T, B, E = 4, 3, 250
    L = T + 1
    coefs = dict(dyn_coef=1.3, calib_coef=0.7)
    agent, cfg = make_calib_agent_at(E, mode, L=L, B=B, calibration_mode="pair", dense_activation_function="elu", **coefs)
    D, S = cfg.belief_size, cfg.state_size
    inv_np = ir.make_inv_params(D, S, A, cfg.inv_dynamics_hidden_size)
    agent._load_module(agent.inv_dynamics, {k: torch.from_numpy(v) for k, v in inv_np.items()})
    rs = np.random.RandomState(43)
    f32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32))  # noqa: E731
    embeds = [f32(np.abs(rs.standard_normal((L, B, E)))) for _ in range(3)]                  # cal_src, cal_tgt, aln_tgt
    acts = [f32(rs.uniform(-1, 1, (L, B, A))) for _ in range(2)]
    nons = [f32(rs.uniform(size=(L, B)) > 0.3) for _ in range(2)]
    for m in nons:
        assert 0 < int(m[1:-1].sum()) < (T - 1) * B
    eps = [f32(rs.standard_normal((T, 3 * B, S))) for _ in range(2)]
    rssm = {k: torch.from_numpy(v).double() for k, v in er.make_params(A, E, 7)["transition_model"].items()}
    inv = {k: torch.from_numpy(v).double() for k, v in inv_np.items()}
    leaves = [e.double().requires_grad_(True) for e in embeds]
    dyn, calib = cp.latent_losses(rssm, inv, "elu", *leaves, acts[0].double(), nons[0].double().unsqueeze(2),
                                  acts[1].double(), nons[1].double().unsqueeze(2), eps[0].double(), eps[1].double())
    _, g_ct, g_at = torch.autograd.grad(coefs["dyn_coef"] * dyn + coefs["calib_coef"] * calib, leaves)
    agent.noise_source = {"cal_prior": eps[0].cuda(), "cal_post": eps[1].cuda()}
    out = agent._latent_losses(*(e.cuda() for e in embeds), acts[0].cuda(), nons[0].cuda(), acts[1].cuda(), nons[1].cuda())
    torch.cuda.synchronize()
    for name, sums, want, m in (("dyn", out["dyn_sums"], dyn, nons[1]), ("calib", out["cal_sums"], calib, nons[0])):
        s, n = sums.tolist()
        assert n == float(m[1:-1].sum())
        r = abs(s / n - float(want.detach())) / abs(float(want.detach()))
        log(f"[pair latent E={E} {mode}] {name}_loss: got {s / n:.7g} ref {float(want.detach()):.7g} rel {r:.2e}")
        assert r < 1e-3, (name, s / n, float(want.detach()))
    d_ct, d_at = out["d_cal_tgt"], out["d_aln_tgt"]
    assert tuple(d_ct.shape) == (L, B, E) and tuple(d_at.shape) == (T, B, E)
    assert float(d_ct[0].abs().max()) == 0.0
    for name, got, want in (("cal_tgt", d_ct[1:], g_ct[1:]), ("aln_tgt", d_at, g_at[1:])):
        e = l2err(got, want)
        log(f"[pair latent E={E} {mode}] d embeds {name}: l2err {e:.2e}")
        assert e < GTOL, (name, e)


@pytest.mark.parametrize("mode", ["js", "support"])
def test_pair_steps_match_the_reference_goldens(golden_dir, mode):
    """The whole calibration_mode="pair" step at E = 250 in both alignment modes against the reference's own class
    (calib_pair_{js,support}_embed250_tiny.npz): four encoder passes on ten tensors, the two scans, the alignment gradient
    viewed (L, B, 250) and added to the scan's, two accumulating encoder backward passes, the encoder's step; in support mode
    log_tau's MLP(250, ...) and the u step.  The loop and bounds of tests/test_calib_pair_gpu.py."""
    fname = f"calib_pair_{mode}_embed250_tiny.npz"
    g = np.load(os.path.join(golden_dir, fname))
    L, B, H, A_, n_updates = (int(x) for x in g["meta"])
    agent, cfg = make_calib_agent_at(250, mode, L, B, H, calibration_mode="pair")
    inv = ir.make_inv_params(cfg.belief_size, cfg.state_size, A, cfg.inv_dynamics_hidden_size)
    assert list(agent.inv_dynamics.state_dict().keys()) == list(inv.keys())
    agent._load_module(agent.inv_dynamics, {k: torch.from_numpy(v) for k, v in inv.items()})
    keys = [str(k) for k in g["scalar_keys"]]
    modules = [str(m) for m in g["grad_norm_modules"]]
    assert "train/dyn_loss" in keys and ("train/tau_loss" in keys) == (mode == "support")
    for u in range(n_updates):
        scal = tpg.pair_step(agent, cfg, u)
        assert sorted(scal.keys()) == keys
        _check_golden_scalars(fname, g, u, scal)
        for name, got, w in (("disc beta", float(agent.disc.beta), float(g[f"u{u}/disc_beta"])),
                             ("u", float(agent.u.detach()), float(g[f"u{u}/u"]))):
            assert abs(got - w) <= 1e-3 * abs(w), (name, got, w)
        for name, w in zip(modules, g[f"u{u}/grad_norms"]):
            r = abs(agent.last_grad_norms[name] - w) / w
            log(f"[{fname}] step {u} grad-norm {name}: got {agent.last_grad_norms[name]:.6g} ref {w:.6g} rel {r:.2e}")
            assert r < 2e-3, (name, agent.last_grad_norms[name], w)
    _check_golden_checksums(g, agent, ("encoder", "disc", "log_tau", "src_encoder", "inv_dynamics"))


# ----------------------------------------------------------------------------- 7. the acting path at E = 250
def test_acting_path_at_250_graph_equals_eager_and_eager_matches_fp64(monkeypatch):
    E, D, S = 250, 200, 30
    at(monkeypatch, E)
    agent, cfg = tu.make_agent("repo", 8, 4, 5, A)
    P = er.make_params(A, E, 7)
    p64 = {m: {k: torch.from_numpy(v).double() for k, v in P[m].items()} for m in ("encoder", "transition_model", "actor_model")}
    rs = np.random.RandomState(5)
    obs = torch.from_numpy(fx.preprocess_u8(rs.randint(0, 256, (1, 3, 64, 64)).astype(np.uint8)))
    belief, state = rnd(rs, 1, D, scale=0.3), rnd(rs, 1, S)
    action = torch.from_numpy(rs.uniform(-1, 1, (1, A)).astype(np.float32))
    e1, e2, ea = rnd(rs, 1, 1, S), rnd(rs, 1, 1, S), rnd(rs, 1, A)
    # eager, explicit noise, against the float64 composition of the oracle's modules
    with torch.no_grad():
        emb = orc.encoder_fwd(p64["encoder"], obs.double())
        assert tuple(emb.shape) == (1, E)
        outs = orc.observe(p64["transition_model"], belief.double(), state.double(), action.double()[None], emb[None],
                           torch.ones(1, 1, 1, dtype=torch.float64), e1.double(), e2.double())
        mean, std = orc.actor_fwd(p64["actor_model"], outs[0][0], outs[4][0])
        want_a = torch.tanh(mean + std * ea.double())
        emb_g = agent.encoder(obs.cuda())
        outs_g = agent.transition_model.observe(belief.cuda(), state.cuda(), action.cuda()[None], emb_g[None],
                                                noise=(e1.cuda(), e2.cuda()))
        a_g = agent.actor_model.get_action(outs_g[0][0], outs_g[4][0], det=False, eps=ea.cuda())
    for name, got, want in (("embed", emb_g, emb), ("belief", outs_g[0][0], outs[0][0]), ("state", outs_g[4][0], outs[4][0]),
                            ("action", a_g, want_a)):
        e = relerr(got, want)
        log(f"[acting E={E}] eager {name}: {e:.2e}")
        assert e < FTOL, (name, e)
    # the captured graph against the eager step, three chained steps; torch's generator is reseeded in front of each so
    # that both draw the same normals
    lat = (belief.cuda(), state.cuda(), action.cuda())
    frames = [torch.from_numpy(fx.preprocess_u8(rs.randint(0, 256, (1, 3, 64, 64)).astype(np.uint8))).cuda() for _ in range(3)]
    assert agent._act_graph_enabled
    agent.update_latent_and_select_action(*lat, frames[0], explore=True)   # captures (its warm-up runs draw normals too)
    for i, frame in enumerate(frames):
        torch.manual_seed(100 + i)
        replayed = agent.update_latent_and_select_action(*lat, frame, explore=True)
        torch.cuda.synchronize()
        torch.manual_seed(100 + i)
        with torch.no_grad():
            eager = agent._act_eager(*lat, frame, True)
        assert (True, 1, torch.float32) in agent._act_graphs
        for name, a, b in zip(("belief", "state", "action"), replayed, eager):
            assert torch.equal(a, b), (i, name, float((a - b).abs().max()))
        lat = replayed


# ----------------------------------------------------------------------------- 8. checkpoints
def test_checkpoints_carry_the_fc_and_a_1024_checkpoint_still_loads(monkeypatch):
    E = 250
    L, B, H = 8, 4, 5
    at(monkeypatch, E)
    a, _ = tu.make_agent("repo", L, B, H, A)
    for u in range(2):
        batch, _ = tu.dev_batch(L, B, A, 11 + u)
        a.noise_source, _ = tu.dev_noise(L, B, H, A, 101 + u)
        a.update(batch)
    ck = a.get_param_dict()
    shapes = er.param_shapes(A, E)
    assert list(ck["encoder"].keys())[6:] == ["conv4.weight", "conv4.bias", "fc.weight", "fc.bias"]
    for mod in fx.MODULES:
        assert [(k, tuple(v.shape)) for k, v in ck[mod].items()] == [(k, tuple(s)) for k, s in shapes[mod].items()], mod
    n_model = sum(len(shapes[m]) for m in fx.MODEL_MODULES)
    assert sorted(ck["model_optimizer"]["state"].keys()) == list(range(n_model))       # ten encoder tensors lead
    ps = [torch.nn.Parameter(torch.zeros(tuple(s))) for m in fx.MODEL_MODULES for s in shapes[m].values()]
    torch.optim.Adam(ps, lr=1.0).load_state_dict(ck["model_optimizer"])
    for i, s in enumerate(shapes["encoder"].values()):
        assert tuple(ck["model_optimizer"]["state"][i]["exp_avg"].shape) == tuple(s)
        assert float(ck["model_optimizer"]["state"][i]["exp_avg"].abs().max()) > 0.0    # the fc's moments are live
    # a reference-layout state dict built from the seeded parameters loads key for key
    b, _ = tu.make_agent("repo", L, B, H, A, seed=8)
    assert not torch.equal(b.model_optimizer.flat, a.model_optimizer.flat)
    ref_layout = {m: {k: torch.from_numpy(v) for k, v in er.make_params(A, E, 7)[m].items()} for m in fx.MODULES}
    for m in fx.MODULES:
        b._load_module(getattr(b, m), ref_layout[m])
        for k, v in getattr(b, m).state_dict().items():
            assert torch.equal(v.cpu(), ref_layout[m][k]), (m, k)
    # round trip: parameters and the moments of all ten encoder tensors (and of everything behind them)
    b.load_param_dict(ck)
    n_enc = sum(t.numel() for t in a.encoder.parameters())
    assert n_enc == sum(int(np.prod(s)) for s in shapes["encoder"].values())
    for name in ("flat", "exp_avg", "exp_avg_sq"):
        x, y = getattr(a.model_optimizer, name), getattr(b.model_optimizer, name)
        assert torch.equal(x[:n_enc], y[:n_enc]) and torch.equal(x, y), name
    assert b.model_optimizer.step_count == a.model_optimizer.step_count == 2
    # a checkpoint written at E = 1024 (eight encoder tensors) loads into an agent of that width
    monkeypatch.setattr(tu, "fx", fx)
    c, _ = tu.make_agent("repo", L, B, H, A)
    ck1024 = c.get_param_dict()
    assert list(ck1024["encoder"].keys()) == list(fx.param_shapes(A)["encoder"].keys()) and len(ck1024["encoder"]) == 8
    d, _ = tu.make_agent("repo", L, B, H, A, seed=8)
    d.load_param_dict(ck1024)
    assert torch.equal(d.model_optimizer.flat, c.model_optimizer.flat)
    with pytest.raises(AssertionError):
        b.load_param_dict(ck1024)   # and not into the 250-wide one: the keys differ


# ----------------------------------------------------------------------------- 9. data parallel
def test_data_parallel_two_shards_equal_full_batch_at_250(monkeypatch):
    """tests/test_host_gpu.py's two-shard test (its ThreadDP stand-in and its bounds) for RePo at E = 250, B = 4 = 2 + 2: the
    bucket cut behind the decoder and reward head sits two tensors further into the flat buffer."""
    at(monkeypatch, 250)
    L, B, H = 8, 4, 5
    batch, _ = tu.dev_batch(L, B, A, 21)
    nz, _ = tu.dev_noise(L, B, H, A, 22)
    full, _ = tu.make_agent("repo", L, B, H, A)
    assert len(list(full.encoder.parameters())) == 10
    full.noise_source = nz
    full.update(batch)
    s_full, n_full = dict(full.last_scalars), dict(full.last_grad_norms)
    agents, scal = thg._run_sharded("repo", L, B, H, A, 2, batch, nz)
    for k, w in s_full.items():
        assert abs(scal[0][k] - w) <= 2e-4 * abs(w) + 1e-7, (k, scal[0][k], w)
    assert scal[0] == scal[1]
    for r in range(2):
        for k, w in n_full.items():
            got = agents[r].last_grad_norms[k]
            log(f"[dp 2 shards E=250] rank {r} grad-norm {k}: got {got:.7g} full {w:.7g}")
            assert abs(got - w) <= 2e-4 * abs(w) + 1e-7, (r, k, got, w)
        e = ((agents[r].model_optimizer.flat - full.model_optimizer.flat).abs().max()).item()
        ea = ((agents[r].actor_optimizer.flat - full.actor_optimizer.flat).abs().max()).item()
        log(f"[dp 2 shards E=250] rank {r}: max |param diff| vs full batch after one update: model {e:.2e} actor {ea:.2e}")
        assert e < 2e-5 and ea < 2e-5
    assert torch.equal(agents[0].model_optimizer.flat, agents[1].model_optimizer.flat)
    assert abs(float(agents[0].log_beta) - float(full.log_beta)) < 1e-6
    assert agents[0].dp_buckets_seen[0] == agents[0].dp_buckets_seen[1]
