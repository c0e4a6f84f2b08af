"""config.pixel_obs = False on the GPU: the fused output head of csrc/symbolic.hip (repo_linear_unit_nll) against float64,
the encoder's and decoder's chains against the restatement of tests/symbolic_ref.py (tied to the reference's modules and
loss line by tests/test_symbolic_cpu.py), whole updates of RePo and Dreamer against the REFERENCE's goldens
(tests/golden/gen_golden_symbolic.py), the acting path, checkpoints, and the configurations that keep refusing.

Bounds, all taken from the tests of the neighbouring quantities:
 * NLL sums 1e-5, gradient 1e-6 (normwise, tests.util.relerr): tests/test_rssm_gpu.py::test_losses on scalar_nll; the
   reconstruction 1e-5 (tests/test_dense_act_gpu.py FTOL on a dense forward);
 * per-tensor gradients of the chains 1e-4 in the l2 norm: tests/test_dense_act_gpu.py (GTOL) on mlp_bwd; the loss 1e-5;
 * agents: tests/test_update_gpu.py::test_update_matches_reference_goldens (scalars 1e-3, clip totals 2e-3, checksums
   1e-3 of the absolute sum, latents 1e-4 / 2e-3)."""
import os

import numpy as np
import pytest
import torch

from oracle import fixtures as fx
from tests import symbolic_ref as sr
from tests import test_update_gpu as tu
from tests.util import has, l2err, log, relerr, traced

pytestmark = pytest.mark.gpu

GTOL = 1e-4   # tests/test_dense_act_gpu.py GTOL
OBS = 17


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


# ----------------------------------------------------------------------------- the fused head
ROWS = [1, 63, 64, 65, 257]      # one row; around the 32-row tile and the 64-lane wave; nine row tiles
OUTS = [1, 3, 17, 64, 67]        # odd widths; one full 64-output tile; one output past it (a second column tile)
KS = [8, 30, 1024]               # one ragged K slice; K % 4 != 0: the composition; the modules' embedding width


def _head_case(rows, O, K, seed):
    rs = np.random.RandomState(seed)
    h = torch.from_numpy(rs.standard_normal((rows, K)).astype(np.float32))
    w = torch.from_numpy((rs.standard_normal((O, K)) / np.sqrt(K)).astype(np.float32))
    b = torch.from_numpy(rs.standard_normal(O).astype(np.float32))
    t = torch.from_numpy(rs.standard_normal((rows, O)).astype(np.float32))
    return h, w, b, t


def _check_head(ops, h, w, b, t, scale, hd, td, dpre_view, tag):
    """h, w, b, t: host tensors; hd / td: the device operands (possibly views); dpre_view: None or a NaN-filled view."""
    pred = torch.nn.functional.linear(h.double(), w.double(), b.double())
    want_sum = float(sr.nll_sum(pred, t.double()))
    want_d = (pred - t.double()) * scale
    wd, bd = w.cuda(), b.cuda()
    sums, dpre, recon = ops.linear_unit_nll(hd, wd, bd, td, scale, want_recon=True, dpre=dpre_view)
    sums2, dpre2, recon2 = ops.linear_unit_nll(hd, wd, bd, td, scale, want_recon=True)
    assert torch.equal(sums, sums2) and torch.equal(dpre, dpre2) and torch.equal(recon, recon2), "two runs differ"
    sums3, dpre3, none = ops.linear_unit_nll(hd, wd, bd, td, scale, want_recon=False)
    assert none is None and torch.equal(sums3, sums) and torch.equal(dpre3, dpre), "want_recon changes the other outputs"
    for name, x in (("sums", sums), ("dpre", dpre), ("recon", recon), ("dpre (no recon)", dpre3)):
        assert not torch.isnan(x).any(), f"{tag}: NaN left in {name}"   # fresh allocations are NaN-poisoned (conftest)
    e_s = abs(float(sums[0]) - want_sum) / abs(want_sum)
    e_g, e_r = relerr(dpre, want_d), relerr(recon, pred)
    log(f"linear_unit_nll {tag}: sum {e_s:.2e} dpre {e_g:.2e} recon {e_r:.2e}")
    assert e_s < 1e-5
    assert e_g < 1e-6
    assert e_r < 1e-5


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("rows", ROWS)
def test_linear_unit_nll_against_float64(ops, rows, K):
    for O in OUTS:
        h, w, b, t = _head_case(rows, O, K, 10000 * K + 100 * rows + O)
        _check_head(ops, h, w, b, t, 1.0 / rows, h.cuda(), t.cuda(), None, f"rows={rows} O={O} K={K}")


@pytest.mark.parametrize("K", [8, 30])
def test_linear_unit_nll_on_column_slices_of_wider_buffers(ops, K):
    """h, target and dpre as column views (row pitches above the widths); the columns beside dpre's stay untouched."""
    rows, O = 65, 17
    h, w, b, t = _head_case(rows, O, K, 77 + K)
    hw = torch.full((rows, K + 12), float("nan"), device="cuda")
    hw[:, 4:4 + K] = h.cuda()            # a 16-byte aligned view with pitch K + 12 (K = 8: multiple of 4 -> fused)
    tw = torch.full((rows, O + 5), float("nan"), device="cuda")
    tw[:, 2:2 + O] = t.cuda()
    dw = torch.full((rows, O + 7), float("nan"), device="cuda")
    dv = dw[:, 3:3 + O]
    _check_head(ops, h, w, b, t, 0.25, hw[:, 4:4 + K], tw[:, 2:2 + O], dv, f"slices K={K}")
    assert not torch.isnan(dv).any()
    assert torch.isnan(dw[:, :3]).all() and torch.isnan(dw[:, 3 + O:]).all(), "the kernel wrote beside its block"


def test_linear_unit_nll_dispatch_runs_the_kernel_it_names(ops):
    """K = 1024 takes the fused kernel (the tile engine with the NLL operator), K = 30 the composition; the debug
    switch forces the composition on a fused shape, with the same results to rounding."""
    from repo_amd._lib import lib

    h, w, b, t = _head_case(257, 17, 1024, 5)
    args = (h.cuda(), w.cuda(), b.cuda(), t.cuda(), 0.5)
    (s_f, d_f, _), names = traced(lambda: ops.linear_unit_nll(*args))
    assert has(names, r"vgemm_kernel<[^,]*LinearNllOp") and not has(names, r"unit_nll_rows_kernel"), names
    prev = lib().repo_debug_linear_nll(2)
    try:
        (s_c, d_c, _), names = traced(lambda: ops.linear_unit_nll(*args))
    finally:
        lib().repo_debug_linear_nll(prev)
    assert has(names, r"unit_nll_rows_kernel") and not has(names, r"LinearNllOp"), names
    assert abs(float(s_f) - float(s_c)) <= 1e-5 * abs(float(s_c)) and relerr(d_f, d_c) < 1e-6
    h, w, b, t = _head_case(65, 17, 30, 6)
    _, names = traced(lambda: ops.linear_unit_nll(h.cuda(), w.cuda(), b.cuda(), t.cuda(), 0.5))
    assert has(names, r"unit_nll_rows_kernel") and not has(names, r"LinearNllOp"), names


def test_linear_unit_nll_refuses_what_the_header_rules_out(ops):
    from repo_amd._lib import RepoHipError

    h, w, b, t = _head_case(4, 1025, 8, 1)
    with pytest.raises(RepoHipError):
        ops.linear_unit_nll(h.cuda(), w.cuda(), b.cuda(), t.cuda(), 1.0)


# ----------------------------------------------------------------------------- the modules' chains
# 3 x 4 rows.  For relu the inputs are drawn N(0, scale^2) and fc3's weight is divided by scale (a power of two: exact), so
# that the output keeps its size while every ReLU pre-activation grows with scale: at E = 1024 a chain forms 24576 of
# them, about 4 of which would fall within PRE_MARGIN of zero at scale 1.  ELU needs no margin and runs at scale 1.
CHAIN_ROWS = 12
RELU_SCALE = 4096.0


def chain_inputs(obs, E, act, seed=0):
    D, S = 200, 30
    scale = RELU_SCALE if act == "relu" else 1.0
    rs = np.random.RandomState(9000 + 10 * obs + seed)
    p = sr.make_symbolic_params(obs, D, S, E, seed=60 + seed)
    p64 = {m: {k: torch.from_numpy(v).double() for k, v in d.items()} for m, d in p.items()}
    for m in p64:
        p64[m]["fc3.weight"] = p64[m]["fc3.weight"] / scale
    x = torch.from_numpy((rs.standard_normal((CHAIN_ROWS, obs)) * scale).astype(np.float32))
    feat = torch.from_numpy((rs.standard_normal((CHAIN_ROWS, D + S)) * scale).astype(np.float32))
    dembeds = torch.from_numpy(rs.standard_normal((CHAIN_ROWS, E)).astype(np.float32))
    target = torch.from_numpy(rs.standard_normal((CHAIN_ROWS, obs)).astype(np.float32))
    return p64, x, feat, dembeds, target


@pytest.mark.parametrize("act", ["elu", "relu"])
@pytest.mark.parametrize("E", [64, 1024])
@pytest.mark.parametrize("obs", [17, 24])
def test_chains_match_the_restatement(ops, obs, E, act):
    from repo_amd import functional as Fn

    p64, x, feat, dembeds, target = chain_inputs(obs, E, act)
    for d in p64.values():
        for v in d.values():
            v.requires_grad_(True)
    pre = []
    f64 = feat.double().requires_grad_(True)
    emb = sr.encoder(p64["encoder"], x.double(), act, pre)
    recon = sr.decoder(p64["obs_model"], f64[:, :200], f64[:, 200:], act, pre)
    want_sum = sr.nll_sum(recon, target.double())
    gscale = 1.0 / CHAIN_ROWS
    ((emb * dembeds.double()).sum() + want_sum * gscale).backward()
    if act == "relu":
        m = sr.min_abs_pre(pre)
        log(f"symbolic chains obs={obs} E={E}: smallest |relu pre-activation| {m:.3e} over {sum(z.numel() for z in pre)}")
        assert m >= sr.PRE_MARGIN
    a = ops.DENSE_ACTIVATIONS[act]
    pe = [v.detach().float().cuda().contiguous() for v in p64["encoder"].values()]
    pd = [v.detach().float().cuda().contiguous() for v in p64["obs_model"].values()]
    # encoder
    got_emb, saved = Fn.symbolic_encoder_fwd(pe, x.cuda(), a)
    ge = [torch.full_like(t, 7.0) for t in pe]
    Fn.symbolic_encoder_bwd(pe, x.cuda(), saved, dembeds.cuda(), ge, a)
    e = relerr(got_emb, emb)
    log(f"symbolic encoder obs={obs} E={E} {act} embeds: {e:.2e}")
    assert e < 1e-5
    for (k, v), g in zip(p64["encoder"].items(), ge):
        e = l2err(g, v.grad)
        log(f"symbolic encoder obs={obs} E={E} {act} d{k}: {e:.2e}")
        assert e < GTOL, k
    # decoder, attached: the input gradient accumulates onto what is already there
    nll, dsaved = Fn.symbolic_decoder_fwd_nll(pd, feat.cuda(), target.cuda(), gscale, a)
    gd = [torch.full_like(t, 7.0) for t in pd]
    base = torch.from_numpy(np.random.RandomState(1).standard_normal(tuple(feat.shape)).astype(np.float32)).cuda()
    base = base * float(f64.grad.abs().max())
    dfeat = base.clone()
    Fn.symbolic_decoder_bwd(pd, feat.cuda(), dsaved, gd, a, dfeat=dfeat, accumulate_dfeat=True)
    e = abs(float(nll) - float(want_sum.detach())) / abs(float(want_sum.detach()))
    log(f"symbolic decoder obs={obs} E={E} {act} loss: {e:.2e}")
    assert e < 1e-5
    for (k, v), g in zip(p64["obs_model"].items(), gd):
        e = l2err(g, v.grad)
        log(f"symbolic decoder obs={obs} E={E} {act} d{k}: {e:.2e}")
        assert e < GTOL, k
    e = l2err(dfeat - base, f64.grad)
    log(f"symbolic decoder obs={obs} E={E} {act} dfeat: {e:.2e}")
    assert e < GTOL


# ----------------------------------------------------------------------------- agents
class VecEnv:
    def __init__(self, A, obs):
        self.observation_space = tu.Space((obs,))
        self.action_space = tu.Space((A,))


def make_sym_agent(algo, L, B, H, A, obs=OBS, load=True, **over):
    from repo_amd.algorithms.repo import Dreamer, RePo
    from repo_amd.common.utils import set_gpu_mode

    set_gpu_mode(True)
    cfg = fx.default_config(algo=algo, batch_size=B, chunk_size=L, horizon=H, pixel_obs=False, **over)
    agent = (RePo if algo == "repo" else Dreamer)(cfg, VecEnv(A, obs), VecEnv(A, obs), tu.Logger())
    if load:
        params = fx.make_params(A, 7)
        params.update(sr.make_symbolic_params(obs, cfg.belief_size, cfg.state_size, cfg.embedding_size))
        for mod in fx.MODULES:
            agent._load_module(getattr(agent, mod), {k: torch.from_numpy(v) for k, v in params[mod].items()})
    return agent, cfg


def sym_batch(L, B, A, seed, obs=OBS):
    batch, _ = tu.dev_batch(L, B, A, seed)
    return (torch.from_numpy(sr.make_obs(L, B, obs, seed)).cuda(),) + tuple(batch[1:])


def run_updates(agent, L, B, H, A, n, first=0):
    for u in range(first, first + n):
        agent.noise_source, _ = tu.dev_noise(L, B, H, A, 101 + u)
        agent.update(sym_batch(L, B, A, 11 + u))
    return agent.last_scalars


@pytest.mark.parametrize("fname,algo,over", [("repo_symbolic_tiny.npz", "repo", {}),
                                             ("dreamer_symbolic_tiny.npz", "dreamer", {"cnn_activation_function": "elu"})])
def test_symbolic_update_matches_reference_goldens(golden_dir, fname, algo, over):
    g = np.load(os.path.join(golden_dir, fname))
    L, B, H, A, n_updates = (int(x) for x in g["meta"])
    obs = int(g["obs_size"])
    agent, cfg = make_sym_agent(algo, L, B, H, A, obs, **over)
    assert agent._npix == obs
    keys = [str(k) for k in g["scalar_keys"]]
    for u in range(n_updates):
        batch = sym_batch(L, B, A, 11 + u, obs)
        agent.noise_source, _ = tu.dev_noise(L, B, H, A, 101 + u)
        beliefs, post = agent.train_dynamics(batch[0], batch[1], batch[2], 1.0 - batch[3])
        agent.train_actor_critic(beliefs.flatten(0, 1), post.flatten(0, 1))
        scal = agent.last_scalars
        atol = 1e-4 if u == 0 else 2e-3
        np.testing.assert_allclose(beliefs.cpu().numpy(), g[f"u{u}/beliefs"], rtol=1e-3, atol=atol)
        np.testing.assert_allclose(post.cpu().numpy(), g[f"u{u}/posterior_states"], rtol=1e-3, atol=atol)
        for k, w in zip(keys, g[f"u{u}/scalars"]):
            r = abs(scal[k] - w) / (abs(w) + 1e-12)
            log(f"[{fname}] update {u} {k}: got {scal[k]:.7g} ref {w:.7g} rel {r:.2e}")
            assert r < 1e-3, (fname, u, k, scal[k], w)
        if algo == "repo":
            assert abs(float(agent.log_beta) - float(g[f"u{u}/log_beta"])) < 1e-5
        for name, w in zip(("model", "actor", "value"), g[f"u{u}/total_norms"]):
            r = abs(agent.last_grad_norms[name] - w) / w
            log(f"[{fname}] update {u} grad-norm {name}: got {agent.last_grad_norms[name]:.6g} ref {w:.6g} rel {r:.2e}")
            assert r < 2e-3
    have = {}
    for m in fx.MODULES:
        for k, v in getattr(agent, m).state_dict().items():
            have[f"{m}.{k}"] = (float(v.double().sum()), float(v.double().abs().sum()))
    names = [str(n) for n in g["param_names"]]
    assert sorted(names) == sorted(have)
    for n, s_, a_ in zip(names, g["param_sums"], g["param_abssums"]):
        assert abs(have[n][1] - a_) <= 1e-3 * abs(a_) + 1e-6, (n, have[n][1], a_)
        assert abs(have[n][0] - s_) <= 1e-3 * abs(a_) + 1e-6, (n, have[n][0], s_)
    # one more update runs and stays finite
    scal = run_updates(agent, L, B, H, A, 1, first=n_updates)
    assert all(np.isfinite(v) for v in scal.values()), scal
    assert not agent.logger.nonfinite


@pytest.mark.parametrize("algo", ["repo", "dreamer"])
def test_inverse_dynamics_combines_with_state_vectors(algo):
    agent, _ = make_sym_agent(algo, 8, 4, 5, 6, inv_dynamics=True, inv_dynamics_lr=3e-4, inv_dynamics_hidden_size=64)
    scal = run_updates(agent, 8, 4, 5, 6, 1)
    assert "train/inv_dyn_loss" in scal and all(np.isfinite(v) for v in scal.values()), scal


# ----------------------------------------------------------------------------- acting
def test_acting_graph_equals_eager_bit_for_bit(monkeypatch):
    """B = 1 through the captured HIP graph against the eager launches, three steps.  The path draws its noise with
    torch.randn (posterior sample, the policy's mode search); zeros stand in for it here, so that every output -- belief,
    posterior state, action -- is a function of the inputs alone and the symbolic encoder's embedding is compared through
    the posterior state."""
    agent, cfg = make_sym_agent("repo", 8, 4, 5, 6)
    monkeypatch.setattr(torch, "randn", lambda *s, **k: torch.zeros(*s, **k))
    rs = np.random.RandomState(4)
    lat = agent.init_latent_and_action()
    assert agent._act_graph_enabled
    states = []
    for step in range(3):
        frame = torch.from_numpy(rs.standard_normal((1, OBS)).astype(np.float32)).cuda()
        with torch.no_grad():
            eager = agent._act_eager(*lat, frame, False)
        graph = agent.update_latent_and_select_action(*lat, frame, False)
        torch.cuda.synchronize()
        assert agent._act_graphs, "the acting path did not capture a graph"
        for name, a, b in zip(("belief", "posterior state", "action"), graph, eager):
            assert torch.equal(a, b), (step, name)
            assert bool(torch.isfinite(a).all()), (step, name)
        states.append(graph[1].clone())
        lat = graph
    assert not torch.equal(states[0], states[1])   # the observation reaches the posterior state


def test_episode_driver_feeds_float32_vectors():
    from repo_amd.algorithms.repo.rollout import EpisodeDriver

    agent, _ = make_sym_agent("repo", 8, 4, 5, 6)

    class Env(VecEnv):
        def reset(self):
            return np.linspace(-1, 1, OBS)            # float64, as an environment hands it over

        def step(self, action):
            return np.linspace(1, -1, OBS), 1.0, False, {}

    d = EpisodeDriver(agent, Env(6, OBS), explore=False)
    d.begin()
    tr = d.advance()
    assert tr.obs.shape == (OBS,) and np.isfinite(tr.action).all()
    agent.buffer.push(tr.obs, tr.action, tr.reward, tr.done)
    assert agent.buffer.observations.dtype == np.float32 and agent.buffer.observations.shape[1:] == (OBS,)


# ----------------------------------------------------------------------------- checkpoints
SYM_KEYS = [f"fc{i}.{w}" for i in (1, 2, 3) for w in ("weight", "bias")]


def test_checkpoint_round_trip_gives_an_identical_next_update():
    L, B, H, A = 8, 4, 5, 6
    a, _ = make_sym_agent("repo", L, B, H, A)
    run_updates(a, L, B, H, A, 1)
    ck = a.get_param_dict()
    assert list(ck["encoder"].keys()) == SYM_KEYS and list(ck["obs_model"].keys()) == SYM_KEYS
    assert tuple(ck["encoder"]["fc1.weight"].shape) == (1024, OBS) and tuple(ck["obs_model"]["fc3.weight"].shape) == (OBS, 1024)
    b, _ = make_sym_agent("repo", L, B, H, A, load=False)
    b.load_param_dict(ck)
    sa = run_updates(a, L, B, H, A, 1, first=1)
    sb = run_updates(b, L, B, H, A, 1, first=1)
    assert sa == sb, (sa, sb)
    for m in fx.MODULES:
        for (k, va), vb in zip(getattr(a, m).state_dict().items(), getattr(b, m).state_dict().values()):
            assert torch.equal(va, vb), (m, k)


# ----------------------------------------------------------------------------- refusals
def test_refusals():
    from repo_amd.algorithms.repo import TIA, FinetunedRePo, MultitaskRePo
    from repo_amd.common.utils import set_gpu_mode

    set_gpu_mode(True)
    cfg = fx.default_config(algo="tia", batch_size=4, chunk_size=8, horizon=5, pixel_obs=False)
    with pytest.raises(NotImplementedError, match="pixel_obs"):
        TIA(cfg, VecEnv(6, OBS), VecEnv(6, OBS), tu.Logger())
    cfg = fx.default_config(algo="repo", batch_size=4, chunk_size=8, horizon=5, pixel_obs=False)
    with pytest.raises(NotImplementedError, match="pixel_obs"):
        FinetunedRePo(cfg, VecEnv(6, OBS), VecEnv(6, OBS), tu.Logger())
    cfg = fx.default_config(algo="repo_multitask", batch_size=4, chunk_size=8, horizon=5, share_repr=False, pixel_obs=False)
    env = VecEnv(6, OBS)
    env.num_tasks = 3
    with pytest.raises(NotImplementedError, match="pixel_obs"):
        MultitaskRePo(cfg, env, env, tu.Logger())
    with pytest.raises(NotImplementedError, match="observation_size"):
        make_sym_agent("repo", 8, 4, 5, 6, obs=1025, load=False)
    with pytest.raises(NotImplementedError, match="disag_model"):
        make_sym_agent("repo", 8, 4, 5, 6, load=False, disag_model=True)
    with pytest.raises(NotImplementedError):
        make_sym_agent("repo", 8, 4, 5, 6, load=False, cnn_activation_function="tanh")
