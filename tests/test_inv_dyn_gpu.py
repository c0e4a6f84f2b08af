"""config.inv_dynamics on the GPU: the two kernels of csrc/invdyn.hip, the module's chain (pack -> mlp_fwd -> NLL ->
mlp_bwd) against the float64 restatement of tests/inv_dyn_ref.py (tied to the reference's module and loss lines by
tests/test_inv_dyn_cpu.py), whole updates of RePo and Dreamer against the REFERENCE's goldens
(tests/golden/gen_golden_inv_dyn.py), checkpoints, and the configurations that keep refusing.

Bounds, all taken from the tests of the neighbouring quantities:
 * NLL sums 1e-5, gradient 1e-6 (normwise, tests.util.relerr): tests/test_rssm_gpu.py::test_losses on scalar_nll;
 * per-tensor gradients of the chain 1e-4 in the l2 norm: tests/test_dense_act_gpu.py (GTOL) on mlp_bwd; the loss 1e-5;
 * agents: tests/test_update_gpu.py::test_update_matches_reference_goldens (scalars 1e-3, clip totals 2e-3, checksums
   1e-3 of the absolute sum, latents 1e-4 / 2e-3)."""
import math
import os

import numpy as np
import pytest
import torch

from oracle import fixtures as fx
from tests import inv_dyn_ref as ir
from tests import test_update_gpu as tu
from tests.util import l2err, log, relerr

pytestmark = pytest.mark.gpu

GTOL = 1e-4   # tests/test_dense_act_gpu.py GTOL
INV_CFG = dict(inv_dynamics=True, inv_dynamics_lr=3e-4)


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


# ----------------------------------------------------------------------------- pack
# (T, B, D, S, columns of the buffer left of / right of the rows).  The first four are the issue's; the last two take the
# 16-byte path (every width a multiple of 4), plain and as an aligned view of a wider buffer.
PACK_CASES = [(2, 1, 8, 3, 0, 0), (5, 3, 200, 30, 0, 0), (4, 5, 7, 5, 0, 0), (3, 2, 200, 30, 3, 5), (3, 2, 8, 4, 0, 0),
              (4, 3, 16, 12, 4, 8)]


@pytest.mark.parametrize("T,B,D,S,left,right", PACK_CASES)
def test_pack_is_bit_exact_and_writes_every_element(ops, T, B, D, S, left, right):
    rs = np.random.RandomState(T * 100 + D)
    F = D + S
    wide = torch.from_numpy(rs.standard_normal((T, B, left + F + right)).astype(np.float32)).cuda()
    featx = wide[:, :, left:left + F]
    want = ir.pack(featx[:, :, :D].cpu(), featx[:, :, D:].cpu())
    out = torch.full(((T - 1) * B, 2 * D + S), float("nan"), device="cuda")
    got = ops.inv_dyn_pack(featx, D, out=out)
    assert got.shape == want.shape and torch.equal(got.cpu(), want)
    assert torch.equal(ops.inv_dyn_pack(featx, D).cpu(), want)   # into a (poisoned) buffer of its own


# ----------------------------------------------------------------------------- masked Normal NLL
def _masks(rs, N):
    one = np.zeros(N, dtype=np.float32)
    one[N // 2] = 1.0
    return {"ones": np.ones(N, dtype=np.float32), "one-row": one,
            "p0.3": (rs.uniform(size=N) < 0.3).astype(np.float32), "zeros": np.zeros(N, dtype=np.float32)}


@pytest.mark.parametrize("A", [1, 6, 7])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 257])
def test_normal_nll_rows(ops, N, A):
    _normal_nll_rows_case(ops, N, A, ("ones", "one-row", "p0.3", "zeros"), counted=False)


@pytest.mark.parametrize("N,A", [(9362, 7), (9363, 7)], ids=["64-blocks", "64-blocks-capped"])
def test_normal_nll_rows_at_the_grid_cap(ops, N, A):
    """The grid is min(64, ceil(N A / 1024)): N A = 65534 is the last size with a block per 1024 elements, 65541 the
    first that asks for 65 and is capped, so that the element loop's stride no longer covers everything in four passes.
    The assertions of test_normal_nll_rows, and tests.test_reductions_gpu.reduction()'s on the partials and the ticket."""
    assert -(-N * A // 1024) == {9362: 64, 9363: 65}[N]
    _normal_nll_rows_case(ops, N, A, ("p0.3", "ones"), counted=True)


def _normal_nll_rows_case(ops, N, A, mask_names, counted):
    """counted: the first call also goes through reduction() -- 2 x blocks finite partials after a NaN fill, the ticket word
    0 again, sums = the fixed-order sum of the partials, no follow-up kernel."""
    from tests.reduce_ref import LAST_BLOCK_MAX_GRID
    from tests.test_reductions_gpu import reduction

    blocks = min(LAST_BLOCK_MAX_GRID, -(-N * A // 1024))      # csrc/invdyn.hip, repo_normal_nll_rows
    rs = np.random.RandomState(1000 * A + N)
    buf = torch.from_numpy(rs.standard_normal((N, 2 * A + 3)).astype(np.float32))
    buf[:, A:2 * A] *= 3.0
    flat = buf[:, A:2 * A].reshape(-1).clone()
    flat[0] = 25.0                      # above softplus's threshold: std = raw + min_std
    if flat.numel() > 1:
        flat[-1] = -35.0                # exp(raw) below one ulp of 1: std = min_std to rounding
    if flat.numel() > 2:
        flat[flat.numel() // 2] = 20.5
    buf[:, A:2 * A] = flat.view(N, A)
    target = torch.from_numpy(rs.standard_normal((N, A)).astype(np.float32))
    raw_d = buf.cuda()[:, :2 * A]       # ldraw = 2A + 3
    assert raw_d.stride(0) == 2 * A + 3
    for name, mk in _masks(rs, N).items():
        if name not in mask_names:
            continue
        mask = torch.from_numpy(mk)
        r64 = buf[:, :2 * A].double().requires_grad_(True)
        total, count = ir.masked_nll(r64, target.double(), mask)
        if counted:
            (sums, draw), _ = reduction(ops, lambda: ops.normal_nll_rows(raw_d, target.cuda(), mask.cuda()), lambda r: r[0],
                                        "normal_nll_rows_kernel", blocks, 2, f"normal_nll_rows N={N} A={A} {name} blocks={blocks}")
        else:
            sums, draw = ops.normal_nll_rows(raw_d, target.cuda(), mask.cuda())
        sums2, draw2 = ops.normal_nll_rows(raw_d, target.cuda(), mask.cuda())
        assert torch.equal(sums, sums2) and torch.equal(draw, draw2), "two runs differ"
        assert not torch.isnan(sums).any() and not torch.isnan(draw).any()
        assert float(sums[1]) == count, (name, float(sums[1]), count)
        unsel = mask.cuda() != 1
        assert (draw[unsel] == 0).all(), "an unselected row's gradient is not exactly zero"
        if count == 0:
            assert torch.equal(sums.cpu(), torch.zeros(2)) and (draw == 0).all()
            continue
        (total / count).backward()
        e_s = relerr(sums, torch.stack([total.detach(), torch.tensor(float(count), dtype=torch.float64)]))
        e_0 = abs(float(sums[0]) - float(total)) / abs(float(total))
        e_g = relerr(draw, r64.grad)
        log(f"normal_nll_rows N={N} A={A} {name}: sums {e_s:.2e} (nll alone {e_0:.2e}) draw {e_g:.2e}")
        assert e_s < 1e-5 and e_0 < 1e-5
        assert e_g < 1e-6
        # the caller's count: twice the own count halves the gradient, to 1 ulp
        twice = (sums[1:2] * 2).contiguous()
        _, half = ops.normal_nll_rows(raw_d, target.cuda(), mask.cuda(), count_in=twice)
        ulp = torch.abs(torch.nextafter(draw * 0.5, torch.full_like(draw, float("inf"))) - draw * 0.5)
        assert (torch.abs(half - draw * 0.5) <= ulp).all()
        # sums only
        sums3, none = ops.normal_nll_rows(raw_d, target.cuda(), mask.cuda(), want_grad=False)
        assert none is None and torch.equal(sums3, sums)


# ----------------------------------------------------------------------------- the module's chain
# (T, B, hidden, relu scale, seed).  For relu the latents are drawn N(0, scale^2) and fc4's weight is divided by scale
# (powers of two: exact), so that the head's output keeps its usual size while every ReLU pre-activation grows with scale
# -- (49, 50, 512) forms 3.7 M of them, about 1600 / scale of which fall within PRE_MARGIN of zero; the seeds are the first
# for which none does.  ELU needs no margin and runs at scale 1, N(0, 1) latents: its pre-activations then lie in the
# curved region, where its derivative is neither 0 nor 1.  (49, 50, 512): N = 2400 rows, the workload's, so the dense
# plans route as in training.
CHAIN_CASES = [(4, 5, 100, 16.0, 0), (49, 50, 512, 8192.0, 0)]
CHAIN_D, CHAIN_S, CHAIN_A = 200, 30, 6


def chain_inputs(T, B, hidden, scale, seed):
    rs = np.random.RandomState(7000 + seed)
    D, S, A = CHAIN_D, CHAIN_S, CHAIN_A
    p = {k: torch.from_numpy(v).double() for k, v in ir.make_inv_params(D, S, A, hidden, seed=50 + seed).items()}
    p["fc4.weight"] = p["fc4.weight"] / scale
    featx = torch.from_numpy((rs.standard_normal((T, B, D + S)) * scale).astype(np.float32))
    actions = torch.from_numpy(rs.uniform(-1, 1, (T + 1, B, A)).astype(np.float32))
    nonterms = torch.from_numpy((rs.uniform(size=(T + 1, B, 1)) > 0.2).astype(np.float32))
    return p, featx, actions, nonterms


@pytest.mark.parametrize("act", ["elu", "relu"])
@pytest.mark.parametrize("T,B,hidden,scale,seed", CHAIN_CASES, ids=lambda v: str(v))
def test_module_chain_matches_the_restatement(ops, T, B, hidden, scale, seed, act):
    D, S, A = CHAIN_D, CHAIN_S, CHAIN_A
    p, featx, actions, nonterms = chain_inputs(T, B, hidden, scale if act == "relu" else 1.0, seed)
    for v in p.values():
        v.requires_grad_(True)
    pre = []
    want = ir.loss(p, featx[:, :, :D].double(), featx[:, :, D:].double(), actions.double(), nonterms.double(), act, pre)
    if act == "relu":
        m = ir.min_abs_pre(pre)
        log(f"inv-dyn chain {(T, B, hidden)}: smallest |relu pre-activation| {m:.3e} over {sum(z.numel() for z in pre)}")
        assert m >= ir.PRE_MARGIN
    want.backward()
    N = (T - 1) * B
    selected = int((nonterms[1:-1] == 1).sum())
    assert 0 < selected < N
    a = ops.DENSE_ACTIVATIONS[act]
    params = [v.detach().float().cuda().contiguous() for v in p.values()]
    x = ops.inv_dyn_pack(featx.cuda(), D)
    raw, hid = ops.mlp_fwd(params, x, act=a)
    sums, draw = ops.normal_nll_rows(raw, actions.cuda()[1:-1].reshape(N, A), nonterms.cuda()[1:-1].reshape(N))
    dparams = [torch.full_like(t, 7.0) for t in params]
    ops.mlp_bwd(params, x, hid, draw, dparams=dparams, dx=None, act=a)
    assert float(sums[1]) == selected
    e = abs(float(sums[0]) / float(sums[1]) - float(want)) / abs(float(want))
    log(f"inv-dyn chain {(T, B, hidden)} {act} loss: {e:.2e}")
    assert e < 1e-5
    for (k, v), g in zip(p.items(), dparams):
        e = l2err(g, v.grad)
        log(f"inv-dyn chain {(T, B, hidden)} {act} d{k}: {e:.2e}")
        assert e < GTOL, k


def test_module_forward_and_construction(ops):
    from repo_amd.algorithms.repo import InverseDynamicsModel

    D, S, A, hidden = 24, 5, 3, 40
    assert InverseDynamicsModel(D, S, A, hidden).act == ops.ACT_RELU       # the reference's default argument
    with pytest.raises(NotImplementedError, match="'elu' or 'relu'"):
        InverseDynamicsModel(D, S, A, hidden, "tanh")
    m = InverseDynamicsModel(D, S, A, hidden, "elu").cuda()
    inv = ir.make_inv_params(D, S, A, hidden)
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == [(k, v.shape) for k, v in inv.items()]
    m.load_state_dict({k: torch.from_numpy(v) for k, v in inv.items()})
    rs = np.random.RandomState(3)
    b, s, nb = (torch.from_numpy(rs.standard_normal((9, n)).astype(np.float32)) for n in (D, S, D))
    mean, std = m(b.cuda(), s.cuda(), nb.cuda())
    p64 = {k: torch.from_numpy(v).double() for k, v in inv.items()}
    wm, ws, _ = ir.model(p64, torch.cat((b, s, nb), 1).double(), "elu")
    assert relerr(mean, wm) < 1e-5 and relerr(std, ws) < 1e-5   # tests/test_dense_act_gpu.py FTOL


# ----------------------------------------------------------------------------- agents
def make_inv_agent(algo, L, B, H, A, hidden, **over):
    agent, cfg = tu.make_agent(algo, L, B, H, A, inv_dynamics_hidden_size=hidden, **INV_CFG, **over)
    inv = ir.make_inv_params(cfg.belief_size, cfg.state_size, A, hidden)
    agent._load_module(agent.inv_dynamics, {k: torch.from_numpy(v) for k, v in inv.items()})
    return agent, cfg


def run_updates(agent, L, B, H, A, n):
    for u in range(n):
        batch, _ = tu.dev_batch(L, B, A, 11 + u)
        agent.noise_source, _ = tu.dev_noise(L, B, H, A, 101 + u)
        agent.update(batch)
    return agent.last_scalars


@pytest.mark.parametrize("fname,algo,over", [("repo_invdyn_tiny.npz", "repo", {}),
                                             ("dreamer_invdyn_tiny.npz", "dreamer", {"dense_activation_function": "relu"})])
def test_inv_dyn_update_matches_reference_goldens(golden_dir, fname, algo, over):
    g = np.load(os.path.join(golden_dir, fname))
    L, B, H, A, n_updates = (int(x) for x in g["meta"])
    agent, cfg = make_inv_agent(algo, L, B, H, A, int(g["inv_hidden"]), **over)
    keys = [str(k) for k in g["scalar_keys"]]
    assert "train/inv_dyn_loss" in keys
    for u in range(n_updates):
        batch, _ = tu.dev_batch(L, B, A, 11 + u, u8=(u % 2 == 0))
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
        norms = list(zip(("model", "actor", "value"), g[f"u{u}/total_norms"]))
        norms.append(("inv_dynamics", float(g[f"u{u}/inv_dynamics_norm"])))
        for name, w in norms:
            r = abs(agent.last_grad_norms[name] - w) / w
            log(f"[{fname}] update {u} grad-norm {name}: got {agent.last_grad_norms[name]:.6g} ref {w:.6g} rel {r:.2e}")
            assert r < 2e-3
    have = {}
    for m in fx.MODULES + ("inv_dynamics",):
        for k, v in getattr(agent, m).state_dict().items():
            have[f"{m}.{k}"] = (float(v.double().sum()), float(v.double().abs().sum()))
    names = [str(n) for n in g["param_names"]] + [str(n) for n in g["inv_param_names"]]
    assert len(g["inv_param_names"]) == 8
    for n, s_, a_ in zip(names, np.concatenate([g["param_sums"], g["inv_param_sums"]]),
                         np.concatenate([g["param_abssums"], g["inv_param_abssums"]])):
        assert abs(have[n][1] - a_) <= 1e-3 * abs(a_) + 1e-6, (n, have[n][1], a_)
        assert abs(have[n][0] - s_) <= 1e-3 * abs(a_) + 1e-6, (n, have[n][0], s_)


def test_switch_off_builds_nothing_and_an_empty_selection_steps_on_zero():
    agent, _ = tu.make_agent("repo", 8, 4, 5, 6)
    assert not hasattr(agent, "inv_dynamics") and not hasattr(agent, "inv_dynamics_optimizer")
    stride = agent._noise_stride()
    scal = run_updates(agent, 8, 4, 5, 6, 1)
    assert "train/inv_dyn_loss" not in scal and "inv_dynamics" not in agent.last_grad_norms
    on, _ = make_inv_agent("repo", 8, 4, 5, 6, 64)
    assert on._noise_stride() == stride
    assert on.inv_dynamics_optimizer in on._steppers()
    # every transition of the batch terminal: nothing selected -- nan is logged, the step runs on a zero gradient
    before = [t.clone() for t in on.inv_dynamics.plist()]
    batch, _ = tu.dev_batch(8, 4, 6, 11)
    on.noise_source, _ = tu.dev_noise(8, 4, 5, 6, 101)
    on.update((batch[0], batch[1], batch[2], torch.ones_like(batch[3])))
    scal = on.last_scalars
    assert math.isnan(scal["train/inv_dyn_loss"]) and on.last_grad_norms["inv_dynamics"] == 0.0
    assert on.inv_dynamics_optimizer.step_count == 1
    for t, b in zip(on.inv_dynamics.plist(), before):
        assert torch.equal(t, b)            # Adam on a zero gradient from zero moments moves nothing, and nothing is NaN
    assert not torch.isnan(on.inv_dynamics_optimizer.exp_avg).any()


# ----------------------------------------------------------------------------- checkpoints
def test_checkpoint_round_trip_and_a_checkpoint_without_the_keys():
    L, B, H, A = 8, 4, 5, 6
    a, _ = make_inv_agent("repo", L, B, H, A, 64)
    run_updates(a, L, B, H, A, 2)
    ck = a.get_param_dict()
    assert "inv_dynamics" in ck and "inv_dynamics_optimizer" in ck
    assert list(ck["inv_dynamics"].keys()) == [f"fc{i}.{w}" for i in (1, 2, 3, 4) for w in ("weight", "bias")]
    assert sorted(ck["inv_dynamics_optimizer"]["state"].keys()) == list(range(8))
    b, _ = tu.make_agent("repo", L, B, H, A, inv_dynamics_hidden_size=64, **INV_CFG)
    assert not torch.equal(b.inv_dynamics_optimizer.flat, a.inv_dynamics_optimizer.flat)
    b.load_param_dict(ck)
    oa, ob = a.inv_dynamics_optimizer, b.inv_dynamics_optimizer
    for name in ("flat", "exp_avg", "exp_avg_sq"):
        assert torch.equal(getattr(oa, name), getattr(ob, name)), name
    assert ob.step_count == oa.step_count == 2 and (ob.lr, ob.betas, ob.eps) == (oa.lr, oa.betas, oa.eps)
    # a checkpoint written without the auxiliary loads: the module keeps its weights
    keep = b.inv_dynamics_optimizer.flat.clone()
    b.load_param_dict({k: v for k, v in ck.items() if not k.startswith("inv_dynamics")})
    assert torch.equal(b.inv_dynamics_optimizer.flat, keep)


def test_finetuned_repo_builds_and_checkpoints_but_never_trains_the_module():
    from repo_amd.algorithms.repo import FinetunedRePo
    from repo_amd.common.utils import set_gpu_mode

    set_gpu_mode(True)
    cfg = fx.default_config(algo="repo", batch_size=4, chunk_size=8, horizon=5, inv_dynamics_hidden_size=64, **INV_CFG)
    agent = FinetunedRePo(cfg, tu.Env(6), tu.Env(6), tu.Logger())
    before = agent.inv_dynamics_optimizer.flat.clone()
    batch, _ = tu.dev_batch(8, 4, 6, 11)
    agent.noise_source, _ = tu.dev_noise(8, 4, 5, 6, 101)
    agent.train_encoder(batch[0], batch[1], batch[2], 1.0 - batch[3])
    assert "train/inv_dyn_loss" not in agent.last_scalars
    assert torch.equal(agent.inv_dynamics_optimizer.flat, before) and agent.inv_dynamics_optimizer.step_count == 0
    assert "inv_dynamics" in agent.get_param_dict()


# ----------------------------------------------------------------------------- refusals
def test_refusals():
    from repo_amd.algorithms.repo import TIA, MultitaskRePo
    from repo_amd.common.utils import set_gpu_mode

    set_gpu_mode(True)
    with pytest.raises(NotImplementedError, match="disag_model"):
        tu.make_agent("repo", 8, 4, 5, 6, disag_model=True)
    with pytest.raises(NotImplementedError, match="disag_model"):
        tu.make_agent("dreamer", 8, 4, 5, 6, disag_model=True, inv_dynamics_hidden_size=64, **INV_CFG)
    cfg = fx.default_config(algo="tia", batch_size=4, chunk_size=8, horizon=5, inv_dynamics_hidden_size=64, **INV_CFG)
    with pytest.raises(NotImplementedError, match="TIA"):
        TIA(cfg, tu.Env(6), tu.Env(6), tu.Logger())
    cfg = fx.default_config(algo="repo_multitask", batch_size=4, chunk_size=8, horizon=5, share_repr=False,
                            inv_dynamics_hidden_size=64, **INV_CFG)
    env = tu.Env(6)
    env.num_tasks = 3
    with pytest.raises(NotImplementedError, match="MultitaskRePo"):
        MultitaskRePo(cfg, env, env, tu.Logger())
