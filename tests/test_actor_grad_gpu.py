"""config.actor_grad on the GPU: repo_tanh_normal_reinforce against float64 on the float32-rounded inputs,
whole updates of RePo and Dreamer against tests/actor_grad_ref.py's OracleActorGrad (tied to oracle.repo_oracle and
autograd by tests/test_actor_grad_cpu.py), the combined configuration with pcont and the slow value target, the untouched
default path, the families that refuse, and determinism.

Bounds: tests/test_pcont_gpu.py's.  Kernel: sums FTOL = 1e-5 of sum |terms|, gradients GTOL = 1e-4 normwise.  Updates:
scalars 1e-3, flat gradients 1e-3, per-tensor gradients 5e-3."""
import numpy as np
import pytest
import torch

from oracle import fixtures as fx
from oracle import repo_oracle as ro
from tests import act_ref as ar
from tests import actor_grad_ref as ag
from tests import pcont_ref as pr
from tests import reduce_ref as rr
from tests import slow_value_ref as sv
from tests import test_update_gpu as tu
from tests.util import has, l2err, log, traced

pytestmark = pytest.mark.gpu

FTOL = 1e-5
GTOL = 1e-4
E_BADARG, E_SHAPE, E_WS_TOO_SMALL = -1, -2, -4   # include/repo_hip.h
KERNEL = "tanh_normal_reinforce"


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


# ----------------------------------------------------------------------------- 1. grid regimes
KERNEL_CASES = [(1, 1), (5, 6), (2731, 6), (43691, 6)]


def test_grid_regimes():
    """One thread per element, 256 per block: 16384 elements are the last that finish in their own launch, 16385 take the
    follow-up launch; 262144 fill the 1024-block grid and more take the stride loop.  The cases cover all three."""
    assert rr.finishes_in_launch(ag.reinforce_blocks(16384, 1)) and not rr.finishes_in_launch(ag.reinforce_blocks(16385, 1))
    assert ag.reinforce_blocks(262144, 1) == rr.RED_BLOCKS == ag.reinforce_blocks(262145, 1)
    blocks = [ag.reinforce_blocks(r, a) for r, a in KERNEL_CASES]
    assert blocks == [1, 1, 65, 1024]
    assert rr.finishes_in_launch(blocks[1]) and not rr.finishes_in_launch(blocks[2])
    assert 2731 * 6 == 16386 and 43691 * 6 == 262146 > 1024 * 256


# ----------------------------------------------------------------------------- 2. the kernel against the reference
def _kernel_inputs(rows, A):
    rs = np.random.RandomState(1000 * A + rows % 997)
    mean = rs.uniform(-2.0, 2.0, (rows, A)).astype(np.float32)
    std = rs.uniform(0.1, 1.6, (rows, A)).astype(np.float32)
    eps = rs.standard_normal((rows, A)).astype(np.float32)
    ret = rs.standard_normal(rows).astype(np.float32)
    base = rs.standard_normal(rows).astype(np.float32)
    w = rs.uniform(0.0, 1.0, rows).astype(np.float32)
    if rows >= 5:
        std[0], eps[0] = 0.1, 4.0          # the largest dlogp/dstd of the lot: (16 - 1) / 0.1
        std[1], eps[1] = 0.1, -4.0
        mean[2, 0], mean[2, -1] = 5.0, -5.0
        mean[3], std[3], eps[3] = 5.0, 1.0, 4.0      # u = +9
        mean[3, -1], eps[3, -1] = -5.0, -4.0         # u = -9
        base[4] = ret[4]                             # adv = 0
        w[rows // 2] = 0.0                           # weights exactly 0 (rows // 2 is 2 at rows = 5: the mean = +-5 row)
        w[-1] = 0.0
    return mean, std, eps, ret, base, w


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("rows,A", KERNEL_CASES)
def test_kernel_against_reference(ops, rows, A, weighted):
    mean, std, eps, ret, base, w = _kernel_inputs(rows, A)
    gscale = -0.9 / rows
    t64 = [torch.from_numpy(a).double() for a in (mean, std, eps, ret, base, w)]
    want_dm, want_ds, want_sums, terms = ag.reinforce_grads(t64[0], t64[1], t64[2], t64[3], t64[4],
                                                            t64[5] if weighted else None, gscale)
    if rows >= 5:
        u = t64[0] + t64[1] * t64[2]
        assert abs(float(u[3, 0]) - 9.0) < 1e-6 and abs(float(u[3, -1]) + 9.0) < 1e-6
    d = [torch.from_numpy(a).cuda() for a in (mean, std, eps, ret, base, w)]
    wd = d[5] if weighted else None
    sums, dm, ds = ops.tanh_normal_reinforce(d[0], d[1], d[2], d[3], d[4], wd, gscale=gscale)
    again = ops.tanh_normal_reinforce(d[0], d[1], d[2], d[3], d[4], wd, gscale=gscale)
    for a, b in zip((sums, dm, ds), again):
        assert torch.equal(a, b), "two runs differ"
    for t in (sums, dm, ds):
        assert torch.isfinite(t).all()
    errs = {"sum w adv logp": abs(float(sums[0]) - float(want_sums[0])) / float(terms[0].abs().sum()),
            "sum logp": abs(float(sums[1]) - float(want_sums[1])) / float(terms[1].abs().sum()),
            "dmean": l2err(dm, want_dm), "dstd": l2err(ds, want_ds)}
    log(f"tanh_normal_reinforce rows={rows} A={A} weighted={weighted}: " + " ".join(f"{k} {e:.2e}" for k, e in errs.items()))
    assert errs["sum w adv logp"] < FTOL and errs["sum logp"] < FTOL, errs
    assert errs["dmean"] < GTOL and errs["dstd"] < GTOL, errs
    if rows >= 5:
        assert (dm[4] == 0).all() and (ds[4] == 0).all(), "adv = 0"
        if weighted:
            assert (dm[-1] == 0).all() and (ds[rows // 2] == 0).all(), "w = 0"
    # no gradient buffers: the same sums
    s2, none1, none2 = ops.tanh_normal_reinforce(d[0], d[1], d[2], d[3], d[4], wd, gscale=gscale, want_grads=False)
    assert none1 is None and none2 is None and torch.equal(s2, sums)


@pytest.mark.parametrize("rows,A", KERNEL_CASES)
def test_kernel_noise_paths_agree_in_bits(ops, rows, A):
    """eps = NULL + (seed, offset) against the tensor repo_philox_normal writes for the same (seed, offset): element
    e = row * A + a is normal number offset + e -- equal bits in dmean, dstd and both sums."""
    mean, std, _, ret, base, w = _kernel_inputs(rows, A)
    d = [torch.from_numpy(a).cuda() for a in (mean, std, ret, base, w)]
    seed, offset = 0x9E3779B97F4A7C15, 12345 + rows      # (an offset that is no multiple of 4: mid counter block)
    eps = ops.philox_normal(rows * A, seed, offset, d[0].device).view(rows, A)
    a = ops.tanh_normal_reinforce(d[0], d[1], eps, d[2], d[3], d[4], gscale=-0.5)
    b = ops.tanh_normal_reinforce(d[0], d[1], None, d[2], d[3], d[4], gscale=-0.5, noise=(seed, offset))
    for x, y in zip(a, b):
        assert torch.isfinite(x).all() and torch.equal(x, y)
    assert float(a[1].abs().max()) > 0.0


# ----------------------------------------------------------------------------- 3. error codes
def test_error_codes(ops):
    from repo_amd._lib import lib

    rows, A = 4, 3
    bufs = [torch.ones(rows, A, device="cuda") for _ in range(5)]
    vec = [torch.zeros(rows, device="cuda") for _ in range(3)]
    out = torch.zeros(2, device="cuda")
    ws = ops.reduce_ws(out.device)
    st = torch.cuda.current_stream().cuda_stream
    mean, std, eps, dm, ds = (b.data_ptr() for b in bufs)
    ret, base, w = (v.data_ptr() for v in vec)
    call = lib().repo_tanh_normal_reinforce
    tail = (out.data_ptr(), ws.data_ptr(), ws.numel(), st)
    ok = lambda r, a: call(r, a, mean, std, eps, 0, 0, ret, base, w, 1.0, dm, ds, *tail)   # noqa: E731
    assert ok(0, A) == E_SHAPE and ok(rows, 0) == E_SHAPE and ok(-1, A) == E_SHAPE
    assert ok(2 ** 31 // 3 + 1, 3) == E_SHAPE and ok(2 ** 40, 2 ** 40) == E_SHAPE       # the element index overflows
    for null in range(4):   # mean, std, returns, baseline
        ptrs = [mean, std, ret, base]
        ptrs[null] = None
        assert call(rows, A, ptrs[0], ptrs[1], eps, 0, 0, ptrs[2], ptrs[3], w, 1.0, dm, ds, *tail) == E_BADARG, null
    assert call(rows, A, mean, std, eps, 0, 0, ret, base, w, 1.0, dm, ds, None, ws.data_ptr(), ws.numel(), st) == E_BADARG
    assert call(rows, A, mean, std, eps, 0, 0, ret, base, w, 1.0, dm, None, *tail) == E_BADARG
    assert call(rows, A, mean, std, eps, 0, 0, ret, base, w, 1.0, None, ds, *tail) == E_BADARG
    need = lib().repo_reduce_workspace_bytes()
    assert call(rows, A, mean, std, eps, 0, 0, ret, base, w, 1.0, dm, ds, out.data_ptr(), ws.data_ptr(), need - 1, st) \
        == E_WS_TOO_SMALL
    assert call(rows, A, mean, std, eps, 0, 0, ret, base, w, 1.0, dm, ds, out.data_ptr(), None, need, st) == E_WS_TOO_SMALL
    # eps, weights and both gradients are the optional ones
    assert call(rows, A, mean, std, None, 1, 2, ret, base, None, 1.0, None, None, *tail) == 0
    assert ok(rows, A) == 0
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- 4. whole updates against the oracle
def _flat(grads):
    return torch.cat([g.reshape(-1) for g in grads])


def check_against_oracle(agent, oracle, oscal, snap, names, tag):
    """tests/test_pcont_gpu.py::test_update_matches_oracle's bounds on the scalars in `oscal` and the optimisers in `names`."""
    assert set(oscal) <= set(agent.last_scalars), set(oscal) - set(agent.last_scalars)
    for k, w in oscal.items():
        got = agent.last_scalars[k]
        log(f"{tag} {k}: got {got:.7g} oracle {w:.7g} rel {abs(got - w) / (abs(w) + 1e-12):.2e}")
        assert abs(got - w) <= 1e-3 * abs(w) + 1e-7, (tag, k, got, w)
    for name in names:
        grads = oracle.last[f"{name}_grads"]
        opt = getattr(agent, f"{name}_optimizer")
        want = torch.zeros(opt.numel)
        for gr, o, q in zip(grads, opt.offsets, opt.params):
            if gr is not None:
                want[o : o + q.numel()] = gr.reshape(-1)
        e = ((snap[name].cpu() - want).norm() / want.norm()).item()
        errs = tu.per_tensor_errors(snap[name], grads, opt)
        log(f"{tag} {name}: flat {e:.2e}; per-tensor worst {max(x for _, x in errs):.2e}")
        assert e < 1e-3, (tag, name, e)
        for shape, x in errs:
            assert x < 5e-3, (tag, name, shape, x)


@pytest.mark.parametrize("name,mix", [("reinforce", None), ("both", 0.1)])
@pytest.mark.parametrize("algo", ["repo", "dreamer"])
def test_update_matches_oracle(algo, name, mix):
    L, B, H, A = 10, 5, 6, 6
    over = {"actor_grad": name} if mix is None else {"actor_grad": name, "actor_grad_mix": mix}
    agent, cfg = tu.make_agent(algo, L, B, H, A, **over)
    oracle = ag.OracleActorGrad(cfg, A, params=fx.make_params(A, 7))
    assert oracle.mix == (0.0 if name == "reinforce" else 0.1) == agent._actor_mix
    for u in range(2):
        batch, host = tu.dev_batch(L, B, A, 60 + u, u8=(u == 0))
        agent.noise_source, nz = tu.dev_noise(L, B, H, A, 160 + u)
        if u == 0 and name == "reinforce":
            # what the comparison below relies on: at this point the estimator moves the actor's gradient and loss by far
            # more than the bounds, so an agent that silently kept the dynamics path cannot pass
            plain = ro.OracleAgent(cfg, A, params=fx.make_params(A, 7))
            pscal = plain.update(*host, nz)[2]
        with tu.grad_snapshots(agent) as snap:
            beliefs, post = agent.train_dynamics(batch[0], batch[1], batch[2], 1.0 - batch[3])
            agent.train_actor_critic(beliefs.flatten(0, 1), post.flatten(0, 1))
        _, _, oscal = oracle.update(*host, nz)
        assert "train/actor_logprob" in oscal
        if u == 0 and name == "reinforce":
            sharp_g = l2err(_flat(oracle.last["actor_grads"]), _flat(plain.last["actor_grads"]))
            sharp_l = abs(oscal["train/actor_loss"] - pscal["train/actor_loss"]) / abs(pscal["train/actor_loss"])
            log(f"[oracle actor_grad {algo}] reinforce against dynamics, oracle side: actor gradient {sharp_g:.3g} "
                f"actor_loss {sharp_l:.3g}")
            assert sharp_g > 0.05 and sharp_l > 0.05
        check_against_oracle(agent, oracle, oscal, snap, ("model", "actor", "value"),
                             f"[oracle actor_grad {algo} {name}] update {u}")
        torch.cuda.synchronize()
        with torch.no_grad():   # the oracle takes the agent's parameters: the second update is compared at the same point
            for m in fx.MODULES:
                for k, v in getattr(agent, m).state_dict().items():
                    oracle.p[m][k].copy_(v.cpu())
            if algo == "repo":
                oracle.log_beta.copy_(agent.log_beta.cpu().reshape(oracle.log_beta.shape))


# ----------------------------------------------------------------------------- 5. with pcont and the slow value target
@pytest.mark.parametrize("name,mix", [("both", 0.1), ("reinforce", 0.0)])
def test_with_pcont_and_slow_value_target(name, mix):
    """pcont, a slow target from another seed (every 2, fraction 0.5) and "both" at mix 0.1 (and "reinforce": the returns'
    kernel without gradients, no chain through the target or the continuation head): the actor-critic half against
    OracleActorGradSlowPcont from the agent's own latents and post-model-step parameters, as 6l's combined case does.  The
    oracle's baseline is the TARGET head's and its score-function term carries 6k's weights."""
    from tests import test_slow_value_gpu as tsv

    L, B, H, A = 10, 5, 6, 6
    agent, cfg = tu.make_agent("repo", L, B, H, A, pcont=True, slow_value_target=True, slow_value_update=2,
                               slow_value_fraction=0.5, actor_grad=name, actor_grad_mix=0.1)
    head = pr.make_pcont_params(cfg.belief_size, cfg.state_size, cfg.hidden_size)
    agent._load_module(agent.pcont_model, tsv.torch_sd(head))
    slow = sv.make_slow_params(cfg.belief_size, cfg.state_size, cfg.hidden_size)
    tsv.load_target(agent, slow)
    oracle = ag.OracleActorGradSlowPcont(cfg, A, params=fx.make_params(A, 7), pcont_params=head, slow_params=slow)
    assert oracle.mix == mix == agent._actor_mix and (oracle.every, oracle.fraction) == (2, 0.5) and oracle.act == "elu"
    batch, _ = tu.dev_batch(L, B, A, 60)
    agent.noise_source, nz = tu.dev_noise(L, B, H, A, 160)
    with tu.grad_snapshots(agent) as snap:
        beliefs, post = agent.train_dynamics(batch[0], batch[1], batch[2], 1.0 - batch[3])
        torch.cuda.synchronize()
        with torch.no_grad():
            for m in ("transition_model", "reward_model", "actor_model", "value_model", "pcont_model"):
                for k, v in getattr(agent, m).state_dict().items():
                    oracle.p[m][k].copy_(v.cpu())
        agent.train_actor_critic(beliefs.flatten(0, 1), post.flatten(0, 1))
    t ={k: torch.as_tensor(v) for k, v in nz.items()}
    oscal = oracle.train_actor_critic(beliefs.flatten(0, 1).cpu(), post.flatten(0, 1).cpu(), t["img_act"], t["img_prior"],
                                      t["entropy"])
    assert all(np.isfinite(v) for v in agent.last_scalars.values()) and not agent.logger.nonfinite
    # the case tells the target's baseline from the online head's, and weighted from unweighted, on the oracle side
    wts = oracle.last["weights"]
    assert float(wts.min()) < 0.9 and float(wts[0].min()) == 1.0
    with torch.no_grad():   # (the online head has taken one step of 8e-5 since: nothing against the 0.05 asked here)
        online = ar.mlp_head(oracle.p["value_model"], oracle.last["score_inputs"][0], 4, "elu").reshape(-1)
    assert l2err(online, oracle.last["baseline"].reshape(-1)) > 0.05
    check_against_oracle(agent, oracle, oscal, snap, ("actor", "value"), f"[actor_grad combined {name}]")


# ----------------------------------------------------------------------------- 6. the default path
def _run_updates(agent, L, B, H, A, n):
    for u in range(n):
        batch, _ = tu.dev_batch(L, B, A, 11 + u)
        agent.noise_source, _ = tu.dev_noise(L, B, H, A, 101 + u)
        agent.update(batch)
    return agent.last_scalars


def test_default_path_is_untouched():
    L, B, H, A = 8, 4, 5, 6
    plain, cfg = tu.make_agent("repo", L, B, H, A)
    assert not hasattr(cfg, "actor_grad") and not hasattr(cfg, "actor_grad_mix")
    named, _ = tu.make_agent("repo", L, B, H, A, actor_grad="dynamics")
    one, _ = tu.make_agent("repo", L, B, H, A, actor_grad="both", actor_grad_mix=1.0)
    for agent in (plain, named, one):
        assert agent._actor_mix == 1.0
        _run_updates(agent, L, B, H, A, 2)
    torch.cuda.synchronize()
    for other in (named, one):
        for name in ("model", "actor", "value"):
            a, b = getattr(other, f"{name}_optimizer"), getattr(plain, f"{name}_optimizer")
            assert torch.equal(a.flat, b.flat) and torch.equal(a.exp_avg, b.exp_avg), name
        assert other.last_scalars == plain.last_scalars
    assert "train/actor_logprob" not in plain.last_scalars
    batch, _ = tu.dev_batch(L, B, A, 13)
    noise, _ = tu.dev_noise(L, B, H, A, 103)
    for agent in (plain, one):
        agent.noise_source = noise
        _, names = traced(lambda: agent.update(batch))
        assert has(names, "lambda_return_kernel") and not has(names, KERNEL), names
    # ... and the name would show: the switched-on agents launch it, once per update.  A trace can lose events, those of
    # its tail above all (tests/test_slow_value_gpu.py::counted), which can only hide a kernel: three
    # updates are traced with fill kernels behind them, and one surviving event is asked for.
    from tests import test_slow_value_gpu as tsv

    def three_updates(agent):
        for _ in range(3):
            agent.update(batch)

    for over in ({"actor_grad": "reinforce"}, {"actor_grad": "both"}):
        on, _ = tu.make_agent("repo", L, B, H, A, **over)
        on.noise_source = noise
        _, names = tsv.counted(lambda: three_updates(on))
        assert has(names, KERNEL + "_kernel"), names
        assert "train/actor_logprob" in on.last_scalars and np.isfinite(on.last_scalars["train/actor_logprob"])


# ----------------------------------------------------------------------------- 7. refusals
@pytest.mark.parametrize("family", ["FinetunedRePo", "CalibratedRePo", "TIA", "MultitaskDreamer", "MultitaskRePo"])
def test_other_families_refuse(family):
    from tests import test_pcont_gpu as tp

    build = tp._family_builders()[family]
    with pytest.raises(NotImplementedError, match="actor_grad"):
        build(actor_grad="reinforce")
    with pytest.raises(NotImplementedError, match="actor_grad"):
        build(actor_grad="both")
    agent = build(actor_grad="dynamics")
    assert type(agent).__name__ == family and agent._actor_mix == 1.0


@pytest.mark.parametrize("over", [{"actor_grad": "foo"}, {"actor_grad": "both", "actor_grad_mix": -0.1},
                                  {"actor_grad": "both", "actor_grad_mix": 1.1},
                                  {"actor_grad": "both", "actor_grad_mix": float("nan")}])
@pytest.mark.parametrize("algo", ["repo", "dreamer"])
def test_unknown_names_and_mixes_raise(algo, over):
    with pytest.raises(ValueError, match="actor_grad"):
        tu.make_agent(algo, 8, 4, 5, 6, **over)


# ----------------------------------------------------------------------------- 8. determinism
def test_two_seeded_reinforce_agents_are_bit_equal():
    """Philox noise: the kernel draws the rollout's action noise again from the rollout's (seed, offset)."""
    L, B, H, A = 8, 4, 5, 6
    batches = [tu.dev_batch(L, B, A, 300 + i)[0] for i in range(2)]
    finals = []
    for _ in range(2):
        agent, _cfg = tu.make_agent("dreamer", L, B, H, A, actor_grad="reinforce")
        agent.seed_noise(99)
        for b in batches:
            agent.update(b, join=False)
        agent.synchronize()
        torch.cuda.synchronize()
        assert all(np.isfinite(v) for v in agent.last_scalars.values())
        finals.append([o.flat.clone() for o in (agent.model_optimizer, agent.actor_optimizer, agent.value_optimizer)]
                      + [torch.tensor([agent.last_scalars["train/actor_logprob"], agent.last_scalars["train/actor_loss"]])])
    for a, b in zip(*finals):
        assert torch.equal(a, b)
