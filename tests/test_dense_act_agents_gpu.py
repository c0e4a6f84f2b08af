"""dense_activation_function="relu" at the module and agent level: construction, whole updates of RePo and Dreamer against
the REFERENCE's own relu goldens (tests/golden/gen_golden_act.py), and the acting path (captured graph against eager
against the restatement of tests/act_ref.py)."""
import os

import numpy as np
import pytest
import torch

from oracle import fixtures as fx
from oracle import repo_oracle as ro
from tests import act_ref as ar
from tests import test_update_gpu as tu
from tests.util import log

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _poison_lds():
    """Start every test from NaN-filled LDS on all CUs: reads of never-written LDS cannot hide."""
    from repo_amd._lib import lib

    assert lib().repo_debug_poison_lds(torch.cuda.current_stream().cuda_stream) == 0
    yield


def test_modules_build_with_relu_and_refuse_other_names():
    """RewardModel's default argument IS "relu" (the reference's): the plain call must build."""
    from repo_amd import ops
    from repo_amd.algorithms.repo.models.actor_critic import ValueModel
    from repo_amd.algorithms.repo.models.decoder import RewardModel
    from repo_amd.algorithms.repo.models.rssm import TransitionModel

    assert RewardModel(200, 30, 200).act == ops.ACT_RELU
    assert ValueModel(200, 30, 200, "relu").act == ops.ACT_RELU
    assert TransitionModel(200, 30, 6, 200, 1024, "relu").act == ops.ACT_RELU
    for make in (lambda: RewardModel(200, 30, 200, "tanh"), lambda: ValueModel(200, 30, 200, "tanh"),
                 lambda: TransitionModel(200, 30, 6, 200, 1024, "tanh")):
        with pytest.raises(NotImplementedError, match="'elu' or 'relu'"):
            make()


def test_relu_agent_stores_the_ids_and_keeps_the_actor_on_elu():
    from repo_amd import ops

    agent, _ = tu.make_agent("repo", 8, 4, 5, 6, dense_activation_function="relu")
    assert (agent.transition_model.act, agent.reward_model.act, agent.value_model.act) == (ops.ACT_RELU,) * 3
    assert agent.actor_model.act == ops.ACT_ELU   # the reference's quirk: the config's value lands in `dist`


@pytest.mark.parametrize("fname,algo", [("repo_relu_tiny.npz", "repo"), ("dreamer_relu_tiny.npz", "dreamer")])
def test_relu_update_matches_reference_goldens(golden_dir, fname, algo):
    """The bounds of tests/test_update_gpu.py::test_update_matches_reference_goldens on the ELU goldens: logged scalars
    1e-3, log_beta 1e-5 absolute, per-module gradient norms 2e-3 (RePo) / 1e-2 (Dreamer), clip totals 2e-3, latents 1e-4
    after the first update and 2e-3 after later ones, parameter checksums 1e-3 of the tensor's absolute sum."""
    g = np.load(os.path.join(golden_dir, fname))
    L, B, H, A, n_updates = (int(x) for x in g["meta"])
    agent, cfg = tu.make_agent(algo, L, B, H, A, dense_activation_function="relu")
    keys = [str(k) for k in g["scalar_keys"]]
    mtol = 2e-3 if algo == "repo" else 1e-2
    for u in range(n_updates):
        batch, _ = tu.dev_batch(L, B, A, 11 + u, u8=(u % 2 == 0))
        agent.noise_source, _ = tu.dev_noise(L, B, H, A, 101 + u)
        with tu.grad_snapshots(agent) as snap:
            beliefs, post = agent.train_dynamics(batch[0], batch[1], batch[2], 1.0 - batch[3])
            agent.train_actor_critic(beliefs.flatten(0, 1), post.flatten(0, 1))
        for mod, got, w in zip(fx.MODULES, tu.module_grad_norms(agent, snap), g[f"u{u}/module_grad_norms"]):
            r = abs(got - w) / w
            log(f"[{fname}] update {u} module grad-norm {mod}: got {got:.6g} ref {w:.6g} rel {r:.2e}")
            assert r < mtol, (fname, u, mod, got, w)
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
    for n, s_, a_ in zip((str(n) for n in g["param_names"]), g["param_sums"], g["param_abssums"]):
        assert abs(have[n][1] - a_) <= 1e-3 * abs(a_) + 1e-6, (n, have[n][1], a_)
        assert abs(have[n][0] - s_) <= 1e-3 * abs(a_) + 1e-6, (n, have[n][0], s_)


def test_relu_goldens_differ_from_the_elu_goldens(golden_dir):
    """(the relu fixtures are not the ELU ones under another name)"""
    a, b = np.load(os.path.join(golden_dir, "repo_relu_tiny.npz")), np.load(os.path.join(golden_dir, "repo_tiny.npz"))
    assert sorted(a.files) == sorted(b.files)
    assert not np.allclose(a["u0/beliefs"], b["u0/beliefs"], rtol=1e-3, atol=1e-4)


def test_relu_acting_path_graph_equals_eager_and_matches_the_restatement():
    """B = 1, two consecutive steps: the captured graph's belief equals the eager path's bit for bit (the belief carries no
    noise; the posterior sample and the action draw theirs), and equals the restatement within the acting-path test's
    bound (tests/test_host_gpu.py: rtol 1e-4, atol 1e-5); then, with injected noise, the posterior state and both actions
    against the restatement at the same bound."""
    A, D, S = 6, 200, 30
    agent, cfg = tu.make_agent("repo", 8, 4, 5, A, dense_activation_function="relu")
    params = fx.make_params(A, 7)
    p64 = {k: torch.tensor(v, dtype=torch.float64) for k, v in params["transition_model"].items()}
    penc = {k: torch.tensor(v) for k, v in params["encoder"].items()}
    rs = np.random.RandomState(5)
    lat = (torch.from_numpy(rs.standard_normal((1, D)).astype(np.float32) * 0.3).cuda(),
           torch.from_numpy(rs.standard_normal((1, S)).astype(np.float32)).cuda(),
           torch.from_numpy(rs.uniform(-1, 1, (1, A)).astype(np.float32)).cuda())
    assert agent._act_graph_enabled
    for step in range(2):
        frame = torch.from_numpy(fx.preprocess_u8(rs.randint(0, 256, (1, 3, 64, 64)).astype(np.uint8)))
        with torch.no_grad():
            eager = agent._act_eager(*lat, frame.cuda(), False)
        graph = agent.update_latent_and_select_action(*lat, frame.cuda(), False)
        torch.cuda.synchronize()
        assert agent._act_graphs, "the acting path did not capture a graph"
        assert torch.equal(graph[0], eager[0]), step
        assert all(bool(torch.isfinite(t).all()) for t in graph)
        with torch.no_grad():
            emb = ro.encoder_fwd(penc, frame).double()
            z = torch.zeros(1, 1, S, dtype=torch.float64)
            want = ar.observe(p64, lat[0].cpu().double(), lat[1].cpu().double(), lat[2].cpu().double()[None], emb[None],
                              torch.ones(1, 1, 1, dtype=torch.float64), z, z, "relu")[0][0]
        np.testing.assert_allclose(graph[0].cpu().numpy(), want.numpy(), rtol=1e-4, atol=1e-5)
        lat = tuple(t.clone() for t in eager)   # both paths continue from the eager step's latents
    # the same path with the noise injected (as tests/test_host_gpu.py's acting-path test does): the posterior hidden
    # layer's relu, the posterior state, and the actions of the (ELU) actor on the relu RSSM's latents
    pact = {k: torch.tensor(v, dtype=torch.float64) for k, v in params["actor_model"].items()}
    e1, e2 = (torch.from_numpy(rs.standard_normal((1, 1, S)).astype(np.float32)) for _ in range(2))
    ea = torch.from_numpy(rs.standard_normal((1, A)).astype(np.float32))
    es = torch.from_numpy(rs.standard_normal((100, 1, A)).astype(np.float32))
    frame = torch.from_numpy(fx.preprocess_u8(rs.randint(0, 256, (1, 3, 64, 64)).astype(np.uint8)))
    with torch.no_grad():
        emb = ro.encoder_fwd(penc, frame).double()
        outs = ar.observe(p64, lat[0].cpu().double(), lat[1].cpu().double(), lat[2].cpu().double()[None], emb[None],
                          torch.ones(1, 1, 1, dtype=torch.float64), e1.double(), e2.double(), "relu")
        ob, os_ = outs[0][0], outs[4][0]
        mean, std, _ = ar.actor_fwd(pact, ob, os_, "elu")
        want_explore = torch.tanh(mean + std * ea.double())
        ys = torch.tanh(mean + std * es.double())
        want_mode = ys[ro.tanh_normal_log_prob(ys, mean, std).argmax(0), torch.arange(1)]
        emb_g = agent.encoder(frame.cuda())
        outs_g = agent.transition_model.observe(lat[0], lat[1], lat[2][None], emb_g[None], noise=(e1.cuda(), e2.cuda()))
        b_g, s_g = outs_g[0][0], outs_g[4][0]
        a_explore = agent.actor_model.get_action(b_g, s_g, det=False, eps=ea.cuda())
        a_mode = agent.actor_model.get_action(b_g, s_g, det=True, eps=es.cuda())
    for name, got, want in (("belief", b_g, ob), ("posterior state", s_g, os_), ("explore action", a_explore, want_explore),
                            ("mode action", a_mode, want_mode)):
        np.testing.assert_allclose(got.cpu().numpy(), want.numpy(), rtol=1e-4, atol=1e-5, err_msg=name)
