"""CalibratedRePo's calibration_mode="pair" on the GPU: the pack across two column blocks and its adjoint
(csrc/invdyn.hip), the reverse scan for frozen weights (repo_rssm_observe_bwd_frozen) against the full one, the two latent
losses' gradient into the embeddings against float64 autograd through tests/calib_pair_ref.py (tied to the reference's own
pair_calibration by tests/test_calib_pair_cpu.py), and the agent against the REFERENCE's goldens
(tests/golden/calib_pair_{js,support}_tiny.npz, written by gen_golden_calib_pair.py).

Bounds:
 * pack: bit for bit (a copy);
 * unpack: per element 4e-7 (|a| + |b|), a and b the two terms in float64 -- each an fp32 product (2^-24 relative), their
   sum one fp32 add (2^-24 of at most |a| + |b| + the products' errors): under 1.8e-7 (|a| + |b|).  With `accumulate` the
   old value is a third operand of one more rounded add, so it joins the magnitude: 4e-7 (|a| + |b| + |old|);
 * frozen reverse scan: torch.equal to the full one (the same kernels on the same inputs);
 * d embeds of the latent losses: GTOL = 1e-4 in the l2 norm per block (tests/test_rssm_gpu.py's bound for dembeds); the
   two losses themselves 1e-3 relative (the goldens' scalar bound);
 * goldens: those of tests/test_calib_gpu.py -- scalars 1e-3 relative, gradient norms 2e-3, checksums 1e-3 |a| + 1e-6."""
import math
import os

import numpy as np
import pytest
import torch

from oracle import fixtures as fx
from tests import calib_pair_ref as cp
from tests import calib_ref as cr
from tests import inv_dyn_ref as ir
from tests.test_calib_gpu import _fill_rings, make_calib_agent
from tests.util import l2err, log

pytestmark = pytest.mark.gpu

GTOL = 1e-4   # tests/test_rssm_gpu.py GTOL (dembeds)
# (T, B, D, S): float2 (D + S = 230), float4, scalar with N = B
PACK_CASES = [(3, 2, 200, 30), (4, 3, 8, 4), (2, 1, 5, 3)]


@pytest.fixture(autouse=True)
def _poison_lds():
    from repo_amd._lib import lib

    assert lib().repo_debug_poison_lds(torch.cuda.current_stream().cuda_stream) == 0
    yield


def _blocks(rs, T, B, F, layout):
    """(cur, nxt) as (T, B, F) device views: one contiguous tensor, or column blocks of a (T+1, 3B, F) tensor whose
    storage starts `layout` floats into its allocation (1, 2: the column offset then breaks the 16- / 8-byte alignment)."""
    if layout == "contiguous":
        t = torch.from_numpy(rs.standard_normal((T, B, F)).astype(np.float32)).cuda()
        return t, t
    flat = torch.from_numpy(rs.standard_normal((T + 1) * 3 * B * F + 4).astype(np.float32)).cuda()
    wide = flat[layout : layout + (T + 1) * 3 * B * F].view(T + 1, 3 * B, F)
    return wide[1:, :B], wide[1:, B : 2 * B]


@pytest.mark.parametrize("layout", ["contiguous", 0, 1, 2])
@pytest.mark.parametrize("T,B,D,S", PACK_CASES)
def test_pack_pair_is_torch_indexing_bit_for_bit(T, B, D, S, layout):
    from repo_amd import ops

    F, N = D + S, (T - 1) * B
    rs = np.random.RandomState(T * 100 + B)
    cur, nxt = _blocks(rs, T, B, F, layout)
    want = torch.cat((cur[:-1], nxt[1:, :, :D]), dim=2).reshape(N, F + D)
    assert torch.equal(ops.inv_dyn_pack_pair(cur, nxt, D), want)
    # x = the second half of a (2N, W) buffer; the first half stays as it was
    buf = torch.full((2 * N, F + D), float("nan"), device="cuda")
    ops.inv_dyn_pack_pair(cur, nxt, D, out=buf[N:])
    assert torch.equal(buf[N:], want) and bool(torch.isnan(buf[:N]).all())
    if layout == "contiguous":   # one block in both roles is repo_inv_dyn_pack
        assert torch.equal(ops.inv_dyn_pack_pair(nxt, nxt, D), ops.inv_dyn_pack(nxt, D))


@pytest.mark.parametrize("T,B,D,S,pad,want_v", [(3, 1, 6, 4, 0, 2), (3, 2, 8, 4, 0, 4), (3, 1, 8, 4, 2, 2),
                                                (3, 1, 8, 4, 1, 1)])
def test_pack_pair_from_column_offsets_and_pitches_that_break_the_wider_alignment(T, B, D, S, pad, want_v):
    """An ALIGNED allocation; what limits the access width is the column offset itself or the row pitch:
    F = 10 -- the second block starts 10 floats in, 8- but not 16-byte aligned (float2);  F = 12 unpadded (float4, the
    control);  F = 12 in rows of 14 floats (float2) and of 13 (scalar).  want_v restates the rule of the entry point."""
    from repo_amd import ops

    F, N, ld = D + S, (T - 1) * B, D + S + pad
    rs = np.random.RandomState(T * 10 + pad)
    wide = torch.from_numpy(rs.standard_normal((T + 1, 3 * B, ld)).astype(np.float32)).cuda()
    cur, nxt = wide[1:, B : 2 * B, :F], wide[1:, 2 * B :, :F]
    v = next(v for v in (4, 2, 1) if all(n % v == 0 for n in (F, D, ld, 3 * B * ld))
             and cur.data_ptr() % (4 * v) == 0 and nxt.data_ptr() % (4 * v) == 0)
    assert v == want_v and wide.data_ptr() % 16 == 0
    want = torch.cat((cur[:-1], nxt[1:, :, :D]), dim=2).reshape(N, F + D)
    assert torch.equal(ops.inv_dyn_pack_pair(cur, nxt, D), want)
    # and the adjoint writes such a block, its padding left alone
    dx = torch.from_numpy(rs.standard_normal((N, F + D)).astype(np.float32)).cuda()
    back = torch.full((T, 3 * B, ld), float("nan"), device="cuda")
    ops.inv_dyn_unpack_pair(dx, dx, D, back[:, B : 2 * B, :F])
    ref = torch.zeros(T, B, F, device="cuda")
    ref[:-1] = dx.view(T - 1, B, F + D)[:, :, :F]
    ref[1:, :, :D] += dx.view(T - 1, B, F + D)[:, :, F:]
    assert torch.equal(back[:, B : 2 * B, :F], ref)
    assert bool(torch.isnan(back[:, :B]).all()) and bool(torch.isnan(back[:, 2 * B :]).all())
    assert bool(torch.isnan(back[:, :, F:]).all())


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("scales", [(1.0, 1.0), (0.7, 1.3)])
@pytest.mark.parametrize("with_cur", [True, False])
@pytest.mark.parametrize("T,B,D,S", PACK_CASES)
def test_unpack_pair_matches_the_float64_adjoint(T, B, D, S, with_cur, scales, accumulate):
    from repo_amd import ops

    F, N, W = D + S, (T - 1) * B, 2 * D + S
    rs = np.random.RandomState(T * 100 + B + 7)
    dx = torch.from_numpy(rs.standard_normal((2 * N, W)).astype(np.float32)).cuda()
    dx_cur, dx_next = (dx[:N] if with_cur else None), dx[N:]
    old = torch.from_numpy(rs.standard_normal((T, 2 * B, F)).astype(np.float32)).cuda()
    sc, sn = (np.float32(v) for v in scales)
    a = torch.zeros(T, B, F, dtype=torch.float64)
    b = torch.zeros(T, B, F, dtype=torch.float64)
    if with_cur:
        a[:-1] = float(sc) * dx[:N].double().cpu().view(T - 1, B, W)[:, :, :F]
    b[1:, :, :D] = float(sn) * dx[N:].double().cpu().view(T - 1, B, W)[:, :, F:]
    runs = []
    for _ in range(2):
        wide = old.clone() if accumulate else torch.full((T, 2 * B, F), float("nan"), device="cuda")
        dfeat = wide[:, B:]   # a column block: row pitch F, time pitch 2 B F
        ops.inv_dyn_unpack_pair(dx_cur, dx_next, D, dfeat, float(sc), float(sn), accumulate=accumulate)
        runs.append(wide)
    assert torch.equal(runs[0][:, B:], runs[1][:, B:])                       # two calls: identical bits
    assert torch.equal(runs[0][:, :B], old[:, :B]) if accumulate else bool(torch.isnan(runs[0][:, :B]).all())
    got = runs[0][:, B:].double().cpu()
    o = old[:, B:].double().cpu() if accumulate else torch.zeros_like(a)
    bound = 4e-7 * (a.abs() + b.abs() + o.abs())
    err = (got - (a + b + o)).abs()
    assert bool((err <= bound).all()), float((err - bound).max())
    if accumulate:   # sharper: one rounded add of the non-accumulating call's value onto the old one, bit for bit
        fresh = torch.full((T, 2 * B, F), float("nan"), device="cuda")
        ops.inv_dyn_unpack_pair(dx_cur, dx_next, D, fresh[:, B:], float(sc), float(sn))
        assert torch.equal(runs[0][:, B:], old[:, B:] + fresh[:, B:])
    if not accumulate:
        zeros = (a == 0) & (b == 0)
        assert bool(zeros.any()) and bool((got[zeros] == 0).all())            # written, not skipped
    log(f"[unpack_pair {(T, B, D, S)} cur={with_cur} scales={scales} acc={accumulate}] max err / bound "
        f"{float((err / (bound + 1e-300)).max()):.2f}")


# ----------------------------------------------------------------------------- the frozen reverse scan
def _cu(d):
    return [torch.from_numpy(v).cuda().contiguous() for v in d.values()]


@pytest.mark.parametrize("act", ["elu", "relu"])
@pytest.mark.parametrize("T,B,cs_env,want_cs", [(3, 9, "1", True), (3, 9, "0", False), (2, 100, "auto", False),
                                                (2, 150, "auto", False)])
def test_frozen_reverse_scan_equals_the_full_one(monkeypatch, T, B, cs_env, want_cs, act):
    """(2, 100) and (2, 150): the two row-scan launch shapes 2 B and 3 B columns reach at B = 50."""
    from repo_amd import ops
    from repo_amd._lib import lib

    A, D, S, E = 6, 200, 30, 1024
    rs = np.random.RandomState(3000 * T + B)
    p = _cu(fx.make_params(A, 7)["transition_model"])
    dev = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32)).cuda()  # noqa: E731
    b0, s0 = dev(rs.standard_normal((B, D)) * 0.3), dev(rs.standard_normal((B, S)))
    actions, non = dev(rs.uniform(-1, 1, (T, B, A))), dev(rs.uniform(size=(T, B)) > 0.15)
    emb = dev(np.maximum(rs.standard_normal((T, B, E)), 0))
    eps = dev(rs.standard_normal((T, B, S))), dev(rs.standard_normal((T, B, S)))
    ups = {k: dev(rs.standard_normal(shp) * 0.1) for k, shp in
           (("dfeat", (T, B, D + S)), ("dqm", (T, B, S)), ("dqs", (T, B, S)))}
    monkeypatch.setenv("REPO_SCAN_CS", cs_env)
    a_id = ops.ACT_RELU if act == "relu" else ops.ACT_ELU
    sv = ops.rssm_observe_fwd(p, b0, s0, actions, non, emb, eps[0], eps[1], 0.1, act=a_id)
    assert sv.cs == want_cs
    out = {}
    for frozen in (False, True):
        dembeds, dpb, dps_ = torch.empty(T, B, E).cuda(), torch.empty(B, D).cuda(), torch.empty(B, S).cuda()
        g = None if frozen else [torch.zeros_like(t) for t in p]
        ops.rssm_observe_bwd(p, sv, g, dembeds=dembeds, dprev_belief=dpb, dprev_state=dps_, **ups)
        out[frozen] = (dembeds, dpb, dps_)
    torch.cuda.synchronize()
    for name, full, frz in zip(("dembeds", "dprev_belief", "dprev_state"), out[False], out[True]):
        assert bool(torch.isfinite(full).all()) and float(full.abs().max()) > 0, name
        assert torch.equal(full, frz), (name, float((full - frz).abs().max()))
    dims = (T, B, A, D, sv.Hd, S, E)
    assert lib().repo_rssm_observe_bwd_frozen_workspace_bytes(*dims) <= lib().repo_rssm_observe_bwd_workspace_bytes(*dims)
    with pytest.raises(AssertionError):
        ops.rssm_observe_bwd(p, sv, None, accumulate=True, **ups)


# ----------------------------------------------------------------------------- the agent
def make_pair_agent(mode, L=8, B=4, H=5, A=6, **over):
    """tests/test_calib_gpu.py's agent in "pair" mode, its inverse-dynamics model seeded as the goldens' is."""
    agent, cfg = make_calib_agent(mode, L, B, H, A, **{"calibration_mode": "pair", **over})
    inv = ir.make_inv_params(cfg.belief_size, cfg.state_size, A, cfg.inv_dynamics_hidden_size)
    assert list(agent.inv_dynamics.state_dict().keys()) == list(inv.keys())
    agent._load_module(agent.inv_dynamics, {k: torch.from_numpy(v) for k, v in inv.items()})
    return agent, cfg


def pair_step(agent, cfg, u, inject=True, cal_nonterms=None):
    L, B = cfg.chunk_size, cfg.batch_size
    frames, noise = cr.make_calib_inputs(L, B, 6, cfg.f_latent_size, u)
    pair, scan_noise = cp.make_pair_inputs(L, B, 6, cfg.state_size, u)
    agent.noise_source = {k: torch.from_numpy(v).cuda() for k, v in {**noise, **scan_noise}.items()} if inject else None
    f = {k: torch.from_numpy(v).cuda() for k, v in {**frames, **pair}.items()}
    cal_non = 1.0 - f["cal_dones"] if cal_nonterms is None else cal_nonterms
    agent.pair_calibration_step(f["aln_src"], f["aln_tgt"], f["aln_actions"], 1.0 - f["aln_dones"], f["cal_src"],
                                f["cal_tgt"], f["cal_actions"], cal_non)
    return agent.last_scalars


@pytest.mark.parametrize("cs_env", ["1", "0"])
def test_latent_losses_reach_the_embeddings_as_float64_autograd_does(monkeypatch, cs_env):
    T, B, A, E = 4, 3, 6, 1024
    L = T + 1
    coefs = dict(dyn_coef=1.3, calib_coef=0.7)
    monkeypatch.setenv("REPO_SCAN_CS", cs_env)
    agent, cfg = make_pair_agent("js", L=L, B=B, dense_activation_function="elu", **coefs)
    D, S = cfg.belief_size, cfg.state_size
    rs = np.random.RandomState(41)
    f32 = lambda a: torch.from_numpy(np.asarray(a, dtype=np.float32))  # noqa: E731
    embeds = [f32(np.abs(rs.standard_normal((L, B, E)))) for _ in range(3)]                  # cal_src, cal_tgt, aln_tgt
    acts = [f32(rs.uniform(-1, 1, (L, B, A))) for _ in range(2)]                             # cal, aln
    nons = [f32(rs.uniform(size=(L, B)) > 0.3) for _ in range(2)]
    for m in nons:
        assert 0 < int(m[1:-1].sum()) < (T - 1) * B                                          # both values present
    eps = [f32(rs.standard_normal((T, 3 * B, S))) for _ in range(2)]
    # float64 autograd through oracle.repo_oracle.observe and the restatement
    rssm = {k: torch.from_numpy(v).double() for k, v in fx.make_params(A, 7)["transition_model"].items()}
    inv = {k: torch.from_numpy(v).double() for k, v in
           ir.make_inv_params(D, S, A, cfg.inv_dynamics_hidden_size).items()}
    leaves = [e.double().requires_grad_(True) for e in embeds]
    dyn, calib = cp.latent_losses(rssm, inv, "elu", *leaves, acts[0].double(), nons[0].double().unsqueeze(2),
                                  acts[1].double(), nons[1].double().unsqueeze(2), eps[0].double(), eps[1].double())
    g_cs, g_ct, g_at = torch.autograd.grad(coefs["dyn_coef"] * dyn + coefs["calib_coef"] * calib, leaves)
    assert float(g_ct[0].abs().max()) == 0.0 and float(g_at[0].abs().max()) == 0.0           # frame 0 is not in the scan
    # the device
    agent.noise_source = {"cal_prior": eps[0].cuda(), "cal_post": eps[1].cuda()}
    before = agent._noise_counter
    out = agent._latent_losses(*(e.cuda() for e in embeds), acts[0].cuda(), nons[0].cuda(), acts[1].cuda(), nons[1].cuda())
    torch.cuda.synchronize()
    assert agent._noise_counter == before
    assert sorted(out) == ["cal_sums", "d_aln_tgt", "d_cal_tgt", "dyn_sums"]                 # cal_src: no gradient path
    for name, sums, want, m in (("dyn", out["dyn_sums"], dyn, nons[1]), ("calib", out["cal_sums"], calib, nons[0])):
        s, n = sums.tolist()
        assert n == float(m[1:-1].sum())
        r = abs(s / n - float(want.detach())) / abs(float(want.detach()))
        log(f"[pair latent cs={cs_env}] {name}_loss: got {s / n:.7g} ref {float(want.detach()):.7g} rel {r:.2e}")
        assert r < 1e-3, (name, s / n, float(want.detach()))
    d_ct, d_at = out["d_cal_tgt"], out["d_aln_tgt"]
    assert tuple(d_ct.shape) == (L, B, E) and tuple(d_at.shape) == (T, B, E)
    assert float(d_ct[0].abs().max()) == 0.0                                                  # exact zeros, written
    for name, got, want in (("cal_tgt", d_ct[1:], g_ct[1:]), ("aln_tgt", d_at, g_at[1:])):
        e = l2err(got, want)
        log(f"[pair latent cs={cs_env}] d embeds {name}: l2err {e:.2e}")
        assert e < GTOL, (name, e)


@pytest.mark.parametrize("mode", ["js", "support"])
def test_pair_steps_match_the_reference_goldens(golden_dir, mode):
    fname = f"calib_pair_{mode}_tiny.npz"
    g = np.load(os.path.join(golden_dir, fname))
    L, B, H, A, n_updates = (int(x) for x in g["meta"])
    agent, cfg = make_pair_agent(mode, L, B, H, A)
    keys = [str(k) for k in g["scalar_keys"]]
    modules = [str(m) for m in g["grad_norm_modules"]]
    assert "train/dyn_loss" in keys
    for u in range(n_updates):
        scal = pair_step(agent, cfg, u)
        assert sorted(scal.keys()) == keys
        for k, w in zip(keys, g[f"u{u}/scalars"]):
            r = abs(scal[k] - w) / (abs(w) + 1e-12)
            log(f"[{fname}] step {u} {k}: got {scal[k]:.7g} ref {w:.7g} rel {r:.2e}")
            assert r < 1e-3, (fname, u, k, scal[k], w)
        for name, got, w in (("disc beta", float(agent.disc.beta), float(g[f"u{u}/disc_beta"])),
                             ("u", float(agent.u), float(g[f"u{u}/u"]))):
            assert abs(got - w) <= 1e-3 * abs(w), (name, got, w)
        for name, w in zip(modules, g[f"u{u}/grad_norms"]):
            r = abs(agent.last_grad_norms[name] - w) / w
            log(f"[{fname}] step {u} grad-norm {name}: got {agent.last_grad_norms[name]:.6g} ref {w:.6g} rel {r:.2e}")
            assert r < 2e-3, (name, agent.last_grad_norms[name], w)
    have = {}
    for m in ("encoder", "disc", "log_tau", "src_encoder", "inv_dynamics"):
        for k, v in getattr(agent, m).state_dict().items():
            have[f"{m}.{k}"] = (float(v.double().sum()), float(v.double().abs().sum()))
    names = [str(n) for n in g["param_names"]]
    assert sorted(names) == sorted(have)
    for n, s_, a_ in zip(names, g["param_sums"], g["param_abssums"]):
        assert abs(have[n][1] - a_) <= 1e-3 * abs(a_) + 1e-6, (n, have[n][1], a_)
        assert abs(have[n][0] - s_) <= 1e-3 * abs(a_) + 1e-6, (n, have[n][0], s_)


def test_train_agent_in_pair_mode_moves_the_target_encoder_and_nothing_else():
    agent, cfg = make_pair_agent("support", train_steps=2)
    _fill_rings(agent)
    frozen = [m for m in fx.MODULES if m != "encoder"] + ["src_encoder", "inv_dynamics"]
    before = {m: {k: v.clone() for k, v in getattr(agent, m).state_dict().items()} for m in frozen + ["encoder"]}
    log_beta = agent.log_beta.clone()
    io = agent.inv_dynamics_optimizer
    inv_state = [t.clone() for t in (io.flat, io.exp_avg, io.exp_avg_sq)]
    np.random.seed(3)
    agent.train_agent()
    torch.cuda.synchronize()
    for m in frozen:
        for k, v in getattr(agent, m).state_dict().items():
            assert torch.equal(v, before[m][k]), (m, k)
    assert torch.equal(agent.log_beta, log_beta)
    for t, w in zip((io.flat, io.exp_avg, io.exp_avg_sq), inv_state):
        assert torch.equal(t, w)
    assert io.step_count == 0
    assert any(not torch.equal(v, before["encoder"][k]) for k, v in agent.encoder.state_dict().items())
    assert agent.encoder_optimizer.step_count == agent.disc.optimizer.step_count == agent.tau_optimizer.step_count == 2
    assert agent.u_optimizer.step_count == 2 and agent.model_optimizer.step_count == 0
    scal = agent.last_scalars
    assert "train/dyn_loss" in scal and all(np.isfinite(v) for v in scal.values()), scal
    agent.c.calibration_mode = "triple"
    with pytest.raises(ValueError):
        agent.train_agent()


@pytest.mark.parametrize("mode", ["js", "support"])
def test_a_pair_step_with_in_kernel_noise_and_the_noise_accounting(mode):
    from repo_amd.algorithms.repo import RePo

    agent, cfg = make_pair_agent(mode)
    before = agent._noise_counter
    scal = pair_step(agent, cfg, 0, inject=False)
    assert scal and all(np.isfinite(v) for v in scal.values()), scal
    L, B, Z, S = cfg.chunk_size, cfg.batch_size, cfg.f_latent_size, cfg.state_size
    want = 2 * (L - 1) * 3 * B * S + (4 if mode == "support" else 3) * L * B * Z
    assert agent._noise_counter - before == want <= agent._noise_stride()
    # simple_pair keeps the stride it had: an update's + 4 L B Z, rounded up to a power of two
    simple, _ = make_calib_agent(mode)
    per_update = RePo._noise_stride(simple) + 4 * L * B * Z
    assert simple._noise_stride() == 1 << max(int(per_update) - 1, 1).bit_length()


def test_no_selected_calibration_row_logs_nan_and_leaves_the_encoder_finite():
    agent, cfg = make_pair_agent("js")
    L, B = cfg.chunk_size, cfg.batch_size
    non = torch.ones(L, B, 1, device="cuda")
    non[1:-1] = 0.0
    steps = agent.encoder_optimizer.step_count
    scal = pair_step(agent, cfg, 0, cal_nonterms=non)
    assert math.isnan(scal["train/calib_loss"]) and math.isnan(scal["train/encoder_loss"])
    assert np.isfinite(scal["train/dyn_loss"]) and np.isfinite(scal["train/aln_loss"])
    assert all(bool(torch.isfinite(v).all()) for v in agent.encoder.state_dict().values())
    assert agent.encoder_optimizer.step_count == steps + 1
