"""config.reward_dist = "twohot", config.obs_symlog and config.kl_dyn_scale / kl_rep_scale on the GPU:
repo_symlog against float64 at every regime of its launch and every access path; kl_kernel's mode 2 against mode 1 in bits;
the two-hot loss where the reward path calls it (0 / 1 weights); whole updates of RePo and Dreamer against
tests/wm_losses_ref.py's oracle classes (tied to their parents and to autograd by tests/test_wm_losses_cpu.py); the ties that
need no oracle; the zero initialisation; the configuration in which the keys must change nothing; checkpoints, the families
that refuse, determinism and the device trace.

Bounds.  repo_symlog: units of 2^-24 |y|, at most 8 times what a plain float32 torch evaluation on the CPU gives on the
LARGEST input set of this file (computed once, here; every smaller size draws from the same recipe, and a per-size figure
would be 0 at n = 1) -- room for a device log1pf of about 4 ulp.  Mode 2 and the ties: bits.  Updates: the project's own --
scalars 1e-3, flat gradients 1e-3, per-tensor gradients 5e-3."""
import math

import numpy as np
import pytest
import torch

from oracle import fixtures as fx
from tests import pcont_ref as pr
from tests import test_actor_grad_gpu as tag
from tests import test_symbolic_gpu as tsym
from tests import test_update_gpu as tu
from tests import twohot_ref as th
from tests import wm_losses_ref as wl
from tests.util import has, l2err, log

pytestmark = pytest.mark.gpu

E_BADARG, E_SHAPE = -1, -2   # include/repo_hip.h
UNIT = 2.0 ** -24
GUARD, SENT = 64, -777.0
OBS = tsym.OBS
TWOHOT_KERNELS = ("twohot_decode_kernel", "twohot_decode_bwd_kernel", "twohot_nll_kernel")
WORST = {}


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


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _note(name, ratio):
    WORST[name] = max(WORST.get(name, 0.0), float(ratio))
    return float(ratio)


# ----------------------------------------------------------------------------- 1. repo_symlog
def _ratio(got, x64):
    """max |got - symlog(x)| / (2^-24 |symlog(x)|) over the elements with a non-zero result."""
    ref = wl.symlog(x64)
    nz = ref != 0
    if not bool(nz.any()):
        return 0.0
    return float(((got.double() - ref).abs()[nz] / (UNIT * ref.abs()[nz])).max())


@pytest.fixture(scope="module")
def symlog_limit(ops):
    threads, vec, cap = ops.symlog_geometry()
    x = torch.from_numpy(wl.symlog_inputs(max(wl.symlog_sizes(threads, vec, cap)), 4242))
    cpu = _ratio(torch.sign(x) * torch.log1p(x.abs()), x.double())
    log(f"[symlog] float32 torch on the CPU: {cpu:.3f} units of 2^-24 |y| over {x.numel()} inputs; limit {8 * cpu:.3f}")
    assert 0.5 < cpu < 4.0
    return 8.0 * cpu


def _band(n, shift, fill):
    """n floats at offset GUARD + shift of a buffer filled with `fill` -> (buffer, view)."""
    buf = torch.full((GUARD + shift + n + GUARD,), fill, dtype=torch.float32, device="cuda")
    return buf, buf[GUARD + shift : GUARD + shift + n]


def _intact(buf, n, shift, fill):
    out = torch.cat([buf[: GUARD + shift], buf[GUARD + shift + n :]])
    return bool(torch.isnan(out).all()) if fill != fill else bool((out == fill).all())


@pytest.mark.parametrize("mode", ["aligned", "x+1", "y+1", "both+1", "inplace", "inplace+1"])
def test_symlog_against_float64(ops, symlog_limit, mode):
    threads, vec, cap = ops.symlog_geometry()
    assert (threads, vec, cap) == (256, 4, 1024)
    sx = 1 if mode in ("x+1", "both+1", "inplace+1") else 0
    sy = 1 if mode in ("y+1", "both+1", "inplace+1") else 0
    for n in wl.symlog_sizes(threads, vec, cap):
        x = torch.from_numpy(wl.symlog_inputs(n, 7 * n + 1))
        if mode.startswith("inplace"):
            buf, view = _band(n, sx, SENT)
            view.copy_(x)
            out = ops.symlog(view, out=view)
            assert out.data_ptr() == view.data_ptr() and _intact(buf, n, sx, SENT), (mode, n)
        else:
            xbuf, xin = _band(n, sx, float("nan"))     # a read outside the n elements would poison an output
            xin.copy_(x)
            ybuf, view = _band(n, sy, SENT)
            ops.symlog(xin, out=view)
            assert _intact(ybuf, n, sy, SENT) and _intact(xbuf, n, sx, float("nan")), (mode, n)
            assert torch.equal(_bits(xin), _bits(x)), "the input was written"
        assert view.data_ptr() % 16 == (4 * sy if not mode.startswith("inplace") else 4 * sx)
        got = view.cpu()
        assert not torch.isnan(got).any(), (mode, n)
        r = _note(f"symlog {mode}", _ratio(got, x.double()))
        assert r <= symlog_limit, (mode, n, r, symlog_limit)
        # odd in bits
        neg = ops.symlog((-x).cuda()).cpu()
        assert torch.equal(_bits(neg), _bits(-got)), (mode, n)
    log(f"[symlog {mode}] worst {WORST[f'symlog {mode}']:.3f} units (limit {symlog_limit:.3f})")


def test_symlog_specials_and_error_codes(ops):
    from repo_amd._lib import lib

    den = float(np.float32(1e-41))
    xs = [0.0, -0.0, float("inf"), -float("inf"), float("nan"), den, -den, 1e30, -1e30, 2.0 ** -24, 2.0 ** -25, 1.0, -1.0]
    for shift in (0, 1):     # the vector path (13 elements: three vectors and a tail) and the dword path
        buf, x = _band(len(xs), shift, SENT)
        x.copy_(torch.tensor(xs))
        y = ops.symlog(x).cpu()
        want = wl.symlog(torch.tensor(xs, dtype=torch.float64)).float()
        assert math.copysign(1.0, float(y[0])) == 1.0 and float(y[0]) == 0.0
        assert math.copysign(1.0, float(y[1])) == -1.0 and float(y[1]) == 0.0
        assert float(y[2]) == float("inf") and float(y[3]) == -float("inf") and math.isnan(float(y[4]))
        assert torch.equal(_bits(y[5:7]), _bits(x[5:7])), "a denormal's symlog is the denormal itself"
        assert torch.equal(_bits(y[9:11]), _bits(want[9:11]))
        for i in (7, 8, 11, 12):
            assert abs(float(y[i]) - float(want[i])) <= 8 * UNIT * abs(float(want[i])), (i, float(y[i]), float(want[i]))
        assert torch.equal(_bits(y[8]), _bits(-y[7])) and torch.equal(_bits(y[12]), _bits(-y[11]))
    L_ = lib()
    st = torch.cuda.current_stream().cuda_stream
    ybuf, y = _band(8, 0, SENT)
    x = torch.ones(8, device="cuda")
    assert L_.repo_symlog(8, None, y.data_ptr(), st) == E_BADARG
    assert L_.repo_symlog(8, x.data_ptr(), None, st) == E_BADARG
    assert L_.repo_symlog(0, None, None, st) == E_BADARG
    assert L_.repo_symlog(-1, x.data_ptr(), y.data_ptr(), st) == E_SHAPE
    assert L_.repo_symlog(0, x.data_ptr(), y.data_ptr(), st) == 0
    torch.cuda.synchronize()
    assert bool((ybuf == SENT).all()), "n == 0 wrote something"
    assert L_.repo_symlog_geometry(None, None, None) == E_BADARG
    assert ops.symlog(torch.empty(0, 17, device="cuda")).shape == (0, 17)


# ----------------------------------------------------------------------------- 2. kl_kernel mode 2
def _kl_case(rows, S, seed):
    rs = np.random.RandomState(seed)
    pm, qm = (torch.from_numpy(rs.standard_normal((rows, S)).astype(np.float32)) for _ in range(2))
    ps, qs = (torch.from_numpy(rs.uniform(0.3, 2.0, (rows, S)).astype(np.float32)) for _ in range(2))
    klrow = wl._kl_terms(*(t.double() for t in (pm, ps, qm, qs)))[0]
    free = wl.free_between(klrow)      # about half the rows clipped, none of them near the threshold
    return [t.cuda() for t in (pm, ps, qm, qs)], free, klrow


@pytest.mark.parametrize("S", [1, 30, 64])
@pytest.mark.parametrize("rows", wl.kl_sizes())
def test_kl_mode2_is_mode1_per_side_in_bits(ops, rows, S):
    d, free, klrow = _kl_case(rows, S, 31 * rows + S)
    scale = 1.0 / rows
    if rows > 4:
        frac = float((klrow <= free).double().mean())
        assert 0.3 < frac < 0.7, frac
    for dyn, rep in ((0.5, 0.1), (1.0, 1.0), (0.0, 2.5)):
        out2, g2 = ops.kl_balance(*d, 2, dyn, None, free, scale, rep=rep)
        sp = float(np.float32(dyn) * np.float32(scale))       # ONE float32 product each, as the entry point forms them
        sq = float(np.float32(rep) * np.float32(scale))
        outp, gp = ops.kl_balance(*d, 1, 0.0, None, free, sp)
        outq, gq = ops.kl_balance(*d, 1, 0.0, None, free, sq)
        tagc = f"rows={rows} S={S} dyn={dyn} rep={rep}"
        assert torch.equal(_bits(g2[0]), _bits(gp[0])) and torch.equal(_bits(g2[1]), _bits(gp[1])), tagc
        assert torch.equal(_bits(g2[2]), _bits(gq[2])) and torch.equal(_bits(g2[3]), _bits(gq[3])), tagc
        assert torch.equal(_bits(out2), _bits(outp)) and torch.equal(_bits(out2), _bits(outq)), tagc
        if dyn == rep == 1.0:      # every output is mode 1's
            out1, g1 = ops.kl_balance(*d, 1, 0.0, None, free, scale)
            assert torch.equal(_bits(out2), _bits(out1)), tagc
            for a, b in zip(g2, g1):
                assert torch.equal(_bits(a), _bits(b)), tagc
        elif dyn == 0.5:           # ... and against float64 at mode 1's own bounds (tests/test_rssm_gpu.py::test_losses)
            tot, *gref = wl.kl_mode2(*(t.double().cpu() for t in d), dyn, rep, free, scale)
            assert abs(float(out2) - float(tot)) <= 1e-5 * abs(float(tot)), tagc
            for a, b in zip(g2, gref):
                assert l2err(a, b) < 1e-5, tagc
            assert float(g2[0].abs().max()) > 0 and float(g2[2].abs().max()) > 0
    # nullable gradient outputs: the ones asked for are the full run's
    full, gf = ops.kl_balance(*d, 2, 0.5, None, free, scale, rep=0.1)
    for want in ((True, False, False, True), (False, True, True, False), (False, False, False, False)):
        out, g = ops.kl_balance(*d, 2, 0.5, None, free, scale, want_grads=want, rep=0.1)
        assert torch.equal(_bits(out), _bits(full))
        for w, a, b in zip(want, g, gf):
            assert (a is None) if not w else torch.equal(_bits(a), _bits(b))


def test_kl_mode2_refuses_bad_scales(ops):
    from repo_amd._lib import RepoHipError

    d, free, _ = _kl_case(5, 30, 1)
    for dyn, rep in ((-0.1, 0.1), (0.5, float("nan")), (float("inf"), 0.1)):
        with pytest.raises(RepoHipError):
            ops.kl_balance(*d, 2, dyn, None, free, 0.2, rep=rep)


# ----------------------------------------------------------------------------- 3. the two-hot loss under a 0 / 1 mask
@pytest.mark.parametrize("K", [31, 255])
@pytest.mark.parametrize("rows", [5, 257])
def test_twohot_nll_under_the_nonterminal_mask(ops, rows, K):
    """What the reward path relies on (no new code runs here): rows of weight 0 take exactly zero gradient, sums2[1] is
    the exact count, and the other rows are, in bits, what they are when the masked rows' weights are 1."""
    rs = np.random.RandomState(rows + K)
    z = ops.twohot_rows(rows, K, "cuda")
    z.copy_(torch.from_numpy(rs.standard_normal((rows, K)).astype(np.float32)))
    r = torch.from_numpy((rs.standard_normal(rows) * 3.0).astype(np.float32)).cuda()
    mask = torch.from_numpy((rs.uniform(size=rows) < 0.6).astype(np.float32))
    mask[0], mask[-1] = 0.0, 1.0
    sums, dz = ops.twohot_nll(z, r, mask.cuda(), -5.0, 5.0, 1.0 / rows)
    ones, dz1 = ops.twohot_nll(z, r, torch.ones(rows, device="cuda"), -5.0, 5.0, 1.0 / rows)
    off = mask == 0
    assert float(sums[1]) == float(mask.sum()) and float(ones[1]) == rows
    assert not dz.cpu()[off].any(), "a masked row has a gradient"
    assert torch.equal(_bits(dz.cpu()[~off]), _bits(dz1.cpu()[~off]))
    ref = th.nll(z.cpu().double(), r.cpu().double(), mask.double(), -5.0, 5.0, 1.0 / rows)
    assert abs(float(sums[0]) - float(ref["sums"][0])) <= 1e-5 * abs(float(ref["sums"][0]))


# ----------------------------------------------------------------------------- 4. whole updates against the oracle
LBHA = (10, 5, 6, 6)


def _load(agent, params, mods=fx.MODULES):
    from tests import test_slow_value_gpu as tsv

    for m in mods:
        agent._load_module(getattr(agent, m), tsv.torch_sd(params[m]))


def _pixel_agent(algo, reward_K=None, **over):
    L, B, H, A = LBHA
    agent, cfg = tu.make_agent(algo, L, B, H, A, **over)
    params = wl.wm_params(A, cfg, reward_K=reward_K, value_K=cfg.value_bins if getattr(cfg, "value_dist", "") == "twohot" else None)
    _load(agent, params)
    return agent, cfg, params


def _sym_agent(algo, reward_K=None, **over):
    L, B, H, A = LBHA
    over = dict(dict(cnn_activation_function="elu"), **over)
    agent, cfg = tsym.make_sym_agent(algo, L, B, H, A, **over)
    params = wl.wm_params(A, cfg, reward_K=reward_K, value_K=cfg.value_bins if getattr(cfg, "value_dist", "") == "twohot" else None,
                          obs=OBS)
    _load(agent, params)
    return agent, cfg, params


def _sym_batch(seed):
    L, B, H, A = LBHA
    batch, host = tu.dev_batch(L, B, A, seed)
    obs = wl.scaled_obs(L, B, OBS, seed)
    return (torch.from_numpy(obs).cuda(),) + tuple(batch[1:]), (obs,) + tuple(host[1:])


def _sync_oracle(agent, oracle, algo):
    torch.cuda.synchronize()
    with torch.no_grad():   # the oracle takes the agent's parameters: the second update is compared at the same point
        for m in oracle.p:
            for k, v in getattr(agent, m).state_dict().items():
                oracle.p[m][k].copy_(v.cpu())
        if algo == "repo":
            oracle.log_beta.copy_(agent.log_beta.cpu().reshape(oracle.log_beta.shape))


def _two_updates(agent, oracle, algo, symbolic, tagc, per_update=None):
    L, B, H, A = LBHA
    for u in range(2):
        if symbolic:
            batch, host = _sym_batch(60 + u)
        else:
            batch, host = tu.dev_batch(L, B, A, 60 + u, u8=(u == 0))
        agent.noise_source, nz = tu.dev_noise(L, B, H, A, 160 + u)
        with tu.grad_snapshots(agent) as snap:
            beliefs, post = agent.train_dynamics(batch[0], batch[1], batch[2], 1.0 - batch[3])
            agent.train_actor_critic(beliefs.flatten(0, 1), post.flatten(0, 1))
        _, _, oscal = oracle.update(*host, nz)
        tag.check_against_oracle(agent, oracle, oscal, snap, ("model", "actor", "value"), f"{tagc} update {u}")
        assert not agent.logger.nonfinite
        if per_update is not None:
            per_update(u, oscal)
        _sync_oracle(agent, oracle, algo)


@pytest.mark.parametrize("algo,K,low,high", [("repo", 31, -5.0, 5.0), ("dreamer", 31, -5.0, 5.0), ("repo", 255, -20.0, 20.0)])
def test_twohot_reward_update_matches_oracle(algo, K, low, high):
    agent, cfg, params = _pixel_agent(algo, reward_K=K, reward_dist="twohot", reward_bins=K, reward_bin_low=low,
                                      reward_bin_high=high)
    assert agent._rew_twohot and tuple(agent.reward_model.fc4.weight.shape) == (K, cfg.hidden_size)
    oracle = wl.OracleWm(cfg, LBHA[3], params=params)
    assert oracle.wm["rd_on"] and (oracle.wm["rd_K"], oracle.wm["rd_low"], oracle.wm["rd_high"]) == (K, low, high)

    def imagined(u, oscal):
        r = oracle.last["returns"]
        assert float(r.abs().max()) > 0.05, "a head whose decoded rewards are not all ~0"

    _two_updates(agent, oracle, algo, False, f"[wm twohot reward {algo} K={K}]", imagined)


def test_kl_scales_update_matches_oracle():
    agent, cfg, params = _pixel_agent("dreamer", kl_dyn_scale=0.5, kl_rep_scale=0.1, free_nats=wl.KL_FREE_NATS)
    assert agent._kl_scaled and (agent._kl_dyn, agent._kl_rep) == (0.5, 0.1)
    oracle = wl.OracleWm(cfg, LBHA[3], params=params)

    def clipped(u, oscal):
        _, _, pm, ps, _, qm, qs = oracle.last["observe"]
        frac = float((wl._kl_terms(pm, ps, qm, qs)[0] <= wl.KL_FREE_NATS).float().mean())
        log(f"[wm kl scales] update {u}: {frac:.2f} of the rows clipped")
        assert 0.1 < frac < 0.9

    _two_updates(agent, oracle, "dreamer", False, "[wm kl scales dreamer]", clipped)


@pytest.mark.parametrize("algo", ["repo", "dreamer"])
def test_obs_symlog_update_matches_oracle(algo):
    agent, cfg, params = _sym_agent(algo, obs_symlog=True)
    assert agent._obs_symlog and agent._symbolic
    oracle = wl.OracleWm(cfg, LBHA[3], params=params)
    assert oracle.wm["symlog_on"] and oracle.symbolic
    _two_updates(agent, oracle, algo, True, f"[wm obs_symlog {algo}]")


def test_all_three_keys_with_twohot_value_pcont_return_norm_and_both():
    """State-vector Dreamer with the three keys, value_dist = "twohot", pcont, return_norm and actor_grad = "both" -- and
    slow_value_target, which the oracle class that carries pcont (OracleTwoHotSlowPcont) is built on."""
    from tests import test_slow_value_gpu as tsv

    K = 31
    over = dict(reward_dist="twohot", reward_bins=K, reward_bin_low=-5.0, reward_bin_high=5.0, obs_symlog=True,
                kl_dyn_scale=0.5, kl_rep_scale=0.1, free_nats=wl.KL_FREE_NATS, value_dist="twohot", value_bins=K,
                value_bin_low=-5.0, value_bin_high=5.0, pcont=True, return_norm=True, return_norm_decay=0.5,
                return_norm_limit=1e-3, actor_grad="both", actor_grad_mix=0.1, slow_value_target=True, slow_value_update=2,
                slow_value_fraction=0.5)
    agent, cfg, params = _sym_agent("dreamer", reward_K=K, **over)
    head = pr.make_pcont_params(cfg.belief_size, cfg.state_size, cfg.hidden_size)
    agent._load_module(agent.pcont_model, tsv.torch_sd(head))
    slow = th.make_twohot_value_params(K, seed=th.TWOHOT_SLOW_SEED)
    tsv.load_target(agent, slow)
    oracle = wl.OracleWmSlowPcont(cfg, LBHA[3], params=params, pcont_params=head, slow_params=slow)
    assert oracle.wm["rd_on"] and oracle.wm["symlog_on"] and oracle.wm["kl_on"] and oracle.th_on and oracle.rn_on
    L, B, H, A = LBHA
    for u in range(2):
        batch, host = _sym_batch(60 + u)
        agent.noise_source, nz = tu.dev_noise(L, B, H, A, 160 + u)
        with tu.grad_snapshots(agent) as snap:
            beliefs, post = agent.train_dynamics(batch[0], batch[1], batch[2], 1.0 - batch[3])
            agent.train_actor_critic(beliefs.flatten(0, 1), post.flatten(0, 1))
        _, _, oscal = oracle.update(*host, nz)
        tag.check_against_oracle(agent, oracle, oscal, snap, ("model", "actor", "value"), f"[wm combined] update {u}")
        assert all(np.isfinite(v) for v in agent.last_scalars.values()) and not agent.logger.nonfinite
        _sync_oracle(agent, oracle, "dreamer")


# ----------------------------------------------------------------------------- 5. ties that need no oracle
def _opt_bits(agent):
    out = []
    for name in ("model", "actor", "value"):
        o = getattr(agent, f"{name}_optimizer")
        out += [_bits(o.flat), _bits(o.exp_avg), _bits(o.exp_avg_sq)]
    return out


@pytest.mark.parametrize("algo", ["repo", "dreamer"])
def test_symlog_agent_equals_a_plain_agent_on_symlog_frames(ops, algo):
    L, B, H, A = 8, 4, 5, 6
    keyed, _ = tsym.make_sym_agent(algo, L, B, H, A, obs_symlog=True)
    plain, _ = tsym.make_sym_agent(algo, L, B, H, A)
    for u in range(2):
        batch = tsym.sym_batch(L, B, A, 11 + u)
        x = batch[0] * 50.0
        noise, _ = tu.dev_noise(L, B, H, A, 101 + u)
        keyed.noise_source = plain.noise_source = noise
        keyed.update((x,) + tuple(batch[1:]))
        plain.update((ops.symlog(x),) + tuple(batch[1:]))
    torch.cuda.synchronize()
    for a, b in zip(_opt_bits(keyed), _opt_bits(plain)):
        assert torch.equal(a, b)
    assert keyed.last_scalars == plain.last_scalars


def test_symlog_acting_step_graph_and_eager(ops, monkeypatch):
    keyed, _ = tsym.make_sym_agent("repo", 8, 4, 5, 6, obs_symlog=True)
    plain, _ = tsym.make_sym_agent("repo", 8, 4, 5, 6)
    monkeypatch.setattr(torch, "randn", lambda *s, **k: torch.zeros(*s, **k))
    frame = torch.from_numpy((np.random.RandomState(4).standard_normal((1, OBS)) * 50.0).astype(np.float32)).cuda()
    lat = keyed.init_latent_and_action()
    with torch.no_grad():
        eager_k = keyed._act_eager(*lat, frame, False)
        eager_p = plain._act_eager(*lat, ops.symlog(frame), False)
        raw_p = plain._act_eager(*lat, frame, False)
    graph_k = keyed.update_latent_and_select_action(*lat, frame, False)     # (the launch sits inside the captured region)
    graph_p = plain.update_latent_and_select_action(*lat, ops.symlog(frame), False)
    torch.cuda.synchronize()
    assert keyed._act_graphs and plain._act_graphs
    for a, b, c, d in zip(eager_k, eager_p, graph_k, graph_p):
        assert torch.equal(_bits(a), _bits(b)) and torch.equal(_bits(c), _bits(d)) and torch.equal(_bits(a), _bits(c))
    assert not torch.equal(eager_k[1], raw_p[1]), "the transform reaches the posterior state"


# ----------------------------------------------------------------------------- 6. zero init, 7. the default path
def _fresh(algo, A, seed, **over):
    from repo_amd.algorithms.repo import Dreamer, RePo
    from repo_amd.common.utils import set_gpu_mode

    set_gpu_mode(True)
    cfg = fx.default_config(algo=algo, batch_size=4, chunk_size=8, horizon=5, **over)
    torch.manual_seed(seed)
    return (RePo if algo == "repo" else Dreamer)(cfg, tu.Env(A), tu.Env(A), tu.Logger()), cfg


def test_fresh_twohot_reward_head_decodes_to_zero(ops):
    L, B, H, A = 8, 4, 5, 6
    two, cfg = _fresh("repo", A, 11, reward_dist="twohot")
    plain, _ = _fresh("repo", A, 11)
    assert two._reward_bins == 255 and (two._reward_low, two._reward_high) == (-20.0, 20.0)
    for mod in fx.MODULES:     # the modules constructed BEHIND the reward head (actor, critic) included
        for (k, a), (_, b) in zip(getattr(two, mod).state_dict().items(), getattr(plain, mod).state_dict().items()):
            if mod == "reward_model" and k.startswith("fc4"):
                assert not a.any() and tuple(a.shape)[0] == 255 and b.any()
            else:
                assert torch.equal(_bits(a), _bits(b)), (mod, k)
    pw = [q.detach() for q in two.reward_model.plist()]
    x = torch.randn(300, cfg.belief_size + cfg.state_size, device="cuda")
    z = ops.twohot_rows(300, 255, x.device)
    ops.mlp_fwd(pw, x, out=z, act=two.reward_model.act)
    v = ops.twohot_decode(z, -20.0, 20.0)
    assert not z.any() and torch.equal(_bits(v), torch.zeros(300, 1, dtype=torch.int32))
    batch, _ = tu.dev_batch(L, B, A, 11)
    two.noise_source, _ = tu.dev_noise(L, B, H, A, 101)
    two.update(batch)
    torch.cuda.synchronize()
    sc = two.last_scalars
    assert all(np.isfinite(s) for s in sc.values()) and not two.logger.nonfinite
    nonterm = float((1.0 - batch[3][:-1]).mean())
    assert abs(sc["train/reward_loss"] - nonterm * math.log(255)) < 1e-3 * math.log(255)   # uniform p: CE = log K per kept row
    assert two.reward_model.fc4.weight.any() and two.reward_model.fc4.bias.any()


def _run_updates(agent, L, B, H, A, n, sym=False):
    for u in range(n):
        batch = tsym.sym_batch(L, B, A, 11 + u) if sym else tu.dev_batch(L, B, A, 11 + u)[0]
        agent.noise_source, _ = tu.dev_noise(L, B, H, A, 101 + u)
        agent.update(batch)
    return agent.last_scalars


@pytest.mark.parametrize("sym", [False, True])
def test_default_path_is_untouched(sym):
    from tests import test_slow_value_gpu as tsv

    L, B, H, A = 8, 4, 5, 6
    make = (lambda **o: tsym.make_sym_agent("repo", L, B, H, A, **o)) if sym else (lambda **o: tu.make_agent("repo", L, B, H, A, **o))
    plain, cfg = make()
    assert not any(hasattr(cfg, k) for k in ("reward_dist", "obs_symlog", "kl_dyn_scale", "kl_rep_scale"))
    named, _ = make(reward_dist="normal", reward_bins=31, reward_bin_low=-1.0, reward_bin_high=1.0, obs_symlog=False)
    for agent in (plain, named):
        assert not agent._rew_twohot and not agent._obs_symlog and not agent._kl_scaled and agent.reward_model.bins is None
        _run_updates(agent, L, B, H, A, 2, sym)
    torch.cuda.synchronize()
    for a, b in zip(_opt_bits(named), _opt_bits(plain)):
        assert torch.equal(a, b)
    assert named.last_scalars == plain.last_scalars
    # the device trace: no symlog kernel, no two-hot kernel, the scalar loss twice (reward head, critic)
    batch = tsym.sym_batch(L, B, A, 13) if sym else tu.dev_batch(L, B, A, 13)[0]
    noise, _ = tu.dev_noise(L, B, H, A, 103)
    plain.noise_source = noise
    _, counts = tsv.counted(lambda: [plain.update(batch) for _ in range(3)])
    assert has(counts, "scalar_nll_kernel") and has(counts, "kl_kernel")
    for k in TWOHOT_KERNELS + ("symlog_kernel",):
        assert not has(counts, k), (k, counts)


def test_device_trace_of_the_twohot_reward_path():
    """"twohot" reward: the three two-hot kernels appear (no critic two-hot here: every one of them is the reward path's);
    under "reinforce" nothing flows through the returns and the reward's reverse decode is not launched."""
    from tests import test_slow_value_gpu as tsv

    L, B, H, A = 8, 4, 5, 6
    batch, _ = tu.dev_batch(L, B, A, 13)
    noise, _ = tu.dev_noise(L, B, H, A, 103)
    counts = {}
    for name in ("dynamics", "reinforce"):
        agent, _ = tu.make_agent("repo", L, B, H, A, reward_dist="twohot", reward_bins=31, actor_grad=name)
        _load(agent, {"reward_model": wl.make_twohot_reward_params(31)}, mods=("reward_model",))
        agent.noise_source = noise
        _, counts[name] = tsv.counted(lambda: [agent.update(batch) for _ in range(3)])
        assert all(np.isfinite(v) for v in agent.last_scalars.values())
        assert has(counts[name], "twohot_decode_kernel") and has(counts[name], "twohot_nll_kernel"), counts[name]
        assert has(counts[name], "scalar_nll_kernel")      # the critic's
    assert has(counts["dynamics"], "twohot_decode_bwd_kernel") and not has(counts["reinforce"], "twohot_decode_bwd_kernel")
    sym, _ = tsym.make_sym_agent("dreamer", L, B, H, A, obs_symlog=True, kl_dyn_scale=0.5)
    sym.noise_source = noise
    sbatch = tsym.sym_batch(L, B, A, 13)
    _, c = tsv.counted(lambda: [sym.update(sbatch) for _ in range(3)])
    assert tsv.n_launches(c, "symlog_kernel") == 3 and has(c, "kl_kernel"), c      # one launch per batch


# ----------------------------------------------------------------------------- 8. checkpoints, refusals, determinism
def test_checkpoint_round_trip_and_cross_shape_loads():
    L, B, H, A, K = 8, 4, 5, 6, 31
    over = dict(reward_dist="twohot", reward_bins=K, reward_bin_low=-5.0, reward_bin_high=5.0, kl_dyn_scale=0.5)
    agent, _ = tu.make_agent("dreamer", L, B, H, A, **over)
    _load(agent, {"reward_model": wl.make_twohot_reward_params(K)}, mods=("reward_model",))
    _run_updates(agent, L, B, H, A, 1)
    torch.cuda.synchronize()
    ck = agent.get_param_dict()
    assert tuple(ck["reward_model"]["fc4.weight"].shape) == (K, 200)
    plain_keys = set(tu.make_agent("dreamer", L, B, H, A)[0].get_param_dict())
    assert set(ck) == plain_keys, "no new checkpoint keys"
    fresh, _ = tu.make_agent("dreamer", L, B, H, A, seed=8, **over)
    fresh.load_param_dict(ck)
    for a in (agent, fresh):
        a.noise_source = None
        a.seed_noise(5)
        a._noise_counter = 0
    b2, _ = tu.dev_batch(L, B, A, 12)
    for a in (agent, fresh):
        a.update(b2)
    torch.cuda.synchronize()
    for x, y in zip(_opt_bits(agent), _opt_bits(fresh)):
        assert torch.equal(x, y)
    assert agent.last_scalars == fresh.last_scalars
    scalar, _ = tu.make_agent("dreamer", L, B, H, A)
    before = scalar.reward_model.fc4.weight.detach().clone()
    with pytest.raises(ValueError, match="reward_dist"):
        scalar.load_param_dict(ck)
    assert torch.equal(scalar.reward_model.fc4.weight.detach(), before) and scalar.step == 0
    with pytest.raises(ValueError, match="reward_dist"):
        fresh.load_param_dict(scalar.get_param_dict())
    other, _ = tu.make_agent("dreamer", L, B, H, A, reward_dist="twohot", reward_bins=63)
    with pytest.raises(ValueError, match="reward_dist"):
        other.load_param_dict(ck)


@pytest.mark.parametrize("family", ["FinetunedRePo", "CalibratedRePo", "TIA", "MultitaskDreamer", "MultitaskRePo"])
def test_other_families_refuse(family):
    from tests import test_pcont_gpu as tp

    build = tp._family_builders()[family]
    with pytest.raises(NotImplementedError, match="reward_dist"):
        build(reward_dist="twohot")
    with pytest.raises(NotImplementedError, match="kl_dyn_scale"):
        build(kl_dyn_scale=0.5)
    with pytest.raises(NotImplementedError, match="kl_rep_scale"):
        build(kl_rep_scale=0.1)
    with pytest.raises(NotImplementedError, match="obs_symlog"):
        build(obs_symlog=True)        # (refused as the family's before it is refused as a pixel agent's)
    agent = build(reward_dist="normal", obs_symlog=False)
    assert type(agent).__name__ == family and not agent._rew_twohot and not agent._obs_symlog and not agent._kl_scaled


def test_repo_refuses_the_kl_scales_and_pixels_refuse_symlog():
    with pytest.raises(NotImplementedError, match="kl_dyn_scale"):
        tu.make_agent("repo", 8, 4, 5, 6, kl_dyn_scale=0.5)
    with pytest.raises(NotImplementedError, match="kl_rep_scale"):
        tu.make_agent("repo", 8, 4, 5, 6, kl_rep_scale=0.1)
    for algo in ("repo", "dreamer"):
        with pytest.raises(ValueError, match="obs_symlog"):
            tu.make_agent(algo, 8, 4, 5, 6, obs_symlog=True)
        with pytest.raises(ValueError, match="obs_symlog"):
            tsym.make_sym_agent(algo, 8, 4, 5, 6, load=False, obs_symlog=1)
        with pytest.raises(ValueError, match="reward_bins"):
            tu.make_agent(algo, 8, 4, 5, 6, reward_bins=1)
    with pytest.raises(ValueError, match="kl_rep_scale"):
        tu.make_agent("dreamer", 8, 4, 5, 6, kl_rep_scale=-1.0)


def test_two_seeded_agents_are_bit_equal():
    L, B, H, A = 8, 4, 5, 6
    batches = [tsym.sym_batch(L, B, A, 300 + i) for i in range(3)]
    finals = []
    for _ in range(2):
        agent, _cfg = tsym.make_sym_agent("dreamer", L, B, H, A, reward_dist="twohot", obs_symlog=True, kl_dyn_scale=0.5,
                                          kl_rep_scale=0.1, actor_grad="both")
        _load(agent, {"reward_model": wl.make_twohot_reward_params(255)}, mods=("reward_model",))
        agent.seed_noise(99)
        for b in batches:
            agent.update(b, join=False)
        agent.synchronize()
        torch.cuda.synchronize()
        assert all(np.isfinite(v) for v in agent.last_scalars.values())
        finals.append(_opt_bits(agent) + [torch.tensor([agent.last_scalars[k] for k in ("train/reward_loss", "train/obs_loss")])])
    for a, b in zip(*finals):
        assert torch.equal(a, b)
