"""config.conv_precision on the agents: Dreamer and RePo run train_dynamics, the acting path and _reconstruct at
the configured precision; the first update under "high" keeps the committed goldens' losses and the oracle's model gradient at
the bounds the existing tests apply; the other families refuse the key by name."""
import os

import numpy as np
import pytest
import torch

from oracle import fixtures as fx
from oracle.repo_oracle import OracleAgent
from tests import test_conv_precision_gpu as cp
from tests import test_update_gpu as tu
from tests.util import log, traced

pytestmark = pytest.mark.gpu

BF_KERNELS = ("bconv_down_kernel", "tconv_down_kernel", "buconv_scatter_kernel", "tconv_up_kernel", "bconv_wgrad_kernel",
              "tconv_wgrad_kernel", cp.NLL_KERNEL)


@pytest.fixture(autouse=True)
def _poison_lds():
    from repo_amd._lib import lib

    assert lib().repo_debug_poison_lds(torch.cuda.current_stream().cuda_stream) == 0
    yield


def conv_products(names):
    """{kernel: product counts} of the bf16 conv kernels in a trace; uint8 frames' bconv instantiation aside (3 | 2)."""
    out = {}
    for k in BF_KERNELS:
        float_names = [n for n in names if not (k == "bconv_down_kernel" and "unsigned char" in n)]
        got = cp.products(float_names, k)
        if got:
            out[k] = got
    u8 = cp.products([n for n in names if "bconv_down_kernel" in n and "unsigned char" in n], "bconv_down_kernel")
    return out, u8


@pytest.mark.parametrize("fname,algo", [("repo_tiny.npz", "repo"), ("dreamer_tiny.npz", "dreamer")])
def test_first_update_in_high_keeps_the_goldens_losses_and_the_oracles_gradient(golden_dir, fname, algo):
    """The goldens' L, B, H.  Logged losses of the first update within 1e-3 of the reference's (the bound of
    tests/test_update_gpu.py::test_update_matches_reference_goldens); the flat model gradient within 1e-3 (normwise) of the
    CPU oracle's on the same batch, the bar of test_update_matches_oracle_latents_and_grads; the update's trace lists
    three-product conv kernels (two-product against the uint8 frames) and no six-product one."""
    g = np.load(os.path.join(golden_dir, fname))
    L, B, H, A, _ = (int(x) for x in g["meta"])
    agent, cfg = tu.make_agent(algo, L, B, H, A, conv_precision="high")
    oracle = OracleAgent(cfg, A, seed=7)
    batch, host = tu.dev_batch(L, B, A, 11, u8=True)
    agent.noise_source, nz = tu.dev_noise(L, B, H, A, 101)

    def update():
        with tu.grad_snapshots(agent) as snap:
            beliefs, post = agent.train_dynamics(batch[0], batch[1], batch[2], 1.0 - batch[3])
            agent.train_actor_critic(beliefs.flatten(0, 1), post.flatten(0, 1))
        return snap

    snap, names = traced(update)
    ran, u8 = conv_products(names)
    log(f"[conv_precision high {fname}] conv kernels {ran} uint8 {u8}")
    assert ran and all(v == {3} for v in ran.values()), (ran, names)
    assert u8 <= {2}, u8
    scal = agent.last_scalars
    for k, w in zip((str(k) for k in g["scalar_keys"]), g["u0/scalars"]):
        r = abs(scal[k] - w) / (abs(w) + 1e-12)
        log(f"[conv_precision high {fname}] {k}: got {scal[k]:.7g} ref {w:.7g} rel {r:.2e}")
        assert r < 1e-3, (fname, k, scal[k], w)
    oracle.update(*host, nz)
    opt = agent.model_optimizer
    want = torch.zeros(opt.numel)
    for gr, o, q in zip(oracle.last["model_grads"], opt.offsets, opt.params):
        if gr is not None:
            want[o : o + q.numel()] = gr.reshape(-1)
    e = ((snap["model"].cpu() - want).norm() / want.norm()).item()
    errs = tu.per_tensor_errors(snap["model"], oracle.last["model_grads"], opt)
    log(f"[conv_precision high {fname}] flat model grad {e:.2e}; per-tensor worst {max(x for _, x in errs):.2e} "
        + " ".join(f"{x:.1e}" for _, x in errs))
    assert e < 1e-3, e


@pytest.mark.parametrize("algo", ["repo", "dreamer"])
def test_default_agent_is_bit_identical_to_highest_and_differs_from_high(algo):
    L, B, H, A = 10, 5, 6, 6
    batch, _ = tu.dev_batch(L, B, A, 40, u8=True)
    out = {}
    for name, over in (("default", {}), ("highest", dict(conv_precision="highest")), ("high", dict(conv_precision="high"))):
        agent, _ = tu.make_agent(algo, L, B, H, A, **over)
        agent.noise_source, _ = tu.dev_noise(L, B, H, A, 140)
        with tu.grad_snapshots(agent, ("model",)) as snap:
            beliefs, post = agent.train_dynamics(batch[0], batch[1], batch[2], 1.0 - batch[3])
        out[name] = (beliefs.clone(), post.clone(), snap["model"])
    if cp.DEFAULT == "highest":
        assert all(torch.equal(a, b) for a, b in zip(out["default"], out["highest"]))
    assert not torch.equal(out["high"][2], out["highest"][2]), "the key changed nothing"


def test_128_stack_accepts_the_key():
    """The 128 x 128 stack's layers 4, 5 (decoder 13 x 13, 30 x 30) are the 64 x 64 stack's: they run three-product kernels."""
    L, B, H, A = 7, 3, 5, 7
    agent, _ = tu.make_agent("repo", L, B, H, A, image=128, conv_precision="high")
    batch, _ = tu.dev_batch(L, B, A, 40, u8=True, image=128)
    agent.noise_source, _ = tu.dev_noise(L, B, H, A, 140)
    _, names = traced(lambda: agent.train_dynamics(batch[0], batch[1], batch[2], 1.0 - batch[3]))
    ran, u8 = conv_products(names)
    assert ran and all(v == {3} for v in ran.values()) and u8 <= {2}, (ran, u8)
    assert all(np.isfinite(v) for v in agent.last_scalars.values())


def test_acting_graph_captured_in_high_replays_the_eager_high_result():
    """One uint8 frame: encoder conv1 runs bconv.h's uint8 form (961 pixels), so the mode reaches the acting path; the
    captured graph's belief equals the eager step's bit for bit, and both ran the two-product instantiation."""
    A = 6
    agent, _ = tu.make_agent("repo", 8, 4, 5, A, conv_precision="high")
    twin, _ = tu.make_agent("repo", 8, 4, 5, A)
    rs = np.random.RandomState(5)
    lat = (torch.from_numpy(rs.standard_normal((1, 200)).astype(np.float32) * 0.3).cuda(),
           torch.from_numpy(rs.standard_normal((1, 30)).astype(np.float32)).cuda(),
           torch.from_numpy(rs.uniform(-1, 1, (1, A)).astype(np.float32)).cuda())
    frame = torch.from_numpy(rs.randint(0, 256, (1, 3, 64, 64)).astype(np.uint8)).cuda()
    from repo_amd import ops

    with ops.conv_precision("high"):
        eager, names = traced(lambda: agent._act_eager(*lat, frame, False))
    assert cp.products(names, "bconv_down_kernel") == {2}, names
    graph = agent.update_latent_and_select_action(*lat, frame, False)
    again, names_g = traced(lambda: agent.update_latent_and_select_action(*lat, frame, False))   # the captured graph's replay
    assert cp.products(names_g, "bconv_down_kernel") == {2}, names_g
    assert agent._act_graphs, "the acting path did not capture a graph"
    assert ops.get_conv_precision() == cp.DEFAULT
    assert torch.equal(graph[0], eager[0]) and torch.equal(again[0], eager[0])
    # (the belief of one step does not read the frame; the embedding the posterior is drawn from does)
    with torch.no_grad(), ops.conv_precision("high"):
        emb = agent.encoder(frame)
    with torch.no_grad(), ops.conv_precision("highest"):
        assert not torch.equal(twin.encoder(frame), emb), "the mode changed nothing on the acting path's encoder"
    recon = agent._reconstruct(graph[0], graph[1])
    assert recon.shape == (1, 3, 64, 64) and bool(torch.isfinite(recon).all())


def test_symbolic_agents_accept_and_ignore_the_key():
    from repo_amd.algorithms.repo import RePo
    from repo_amd.common.utils import set_gpu_mode

    set_gpu_mode(True)
    cfg = fx.default_config(algo="repo", batch_size=4, chunk_size=8, horizon=5, pixel_obs=False, conv_precision="high")

    class Env:
        observation_space = tu.Space((17,))
        action_space = tu.Space((6,))

    agent = RePo(cfg, Env(), Env(), tu.Logger())
    assert agent._conv_precision == "high"


def test_unknown_name_in_the_config_is_a_value_error():
    with pytest.raises(ValueError, match='"highest" or "high"'):
        tu.make_agent("repo", 8, 4, 5, 6, conv_precision="tf32")


def _family(name):
    from repo_amd.algorithms import repo as pkg

    return getattr(pkg, name)


@pytest.mark.parametrize("name", ["FinetunedRePo", "CalibratedRePo", "TIA", "MultitaskDreamer", "MultitaskRePo"])
def test_other_families_refuse_the_key_by_name(name):
    from repo_amd.common.utils import set_gpu_mode

    set_gpu_mode(True)
    cls = _family(name)
    algo = {"TIA": "tia", "MultitaskDreamer": "dreamer_multitask", "MultitaskRePo": "repo_multitask"}.get(name, "repo")
    extra = dict(inv_dynamics=True) if name == "CalibratedRePo" else {}   # (its constructor asks for one of its two auxiliaries)
    cfg = fx.default_config(algo=algo, batch_size=4, chunk_size=8, horizon=5, conv_precision="high", **extra)
    env = tu.Env(6)
    env.num_tasks = 3
    args = (cfg, env, env, env, tu.Logger()) if name == "CalibratedRePo" else (cfg, env, env, tu.Logger())
    with pytest.raises(NotImplementedError, match="conv_precision"):
        cls(*args)
    # ... and build at "highest", named or not: the guard is on the value, not on the key
    assert cls._BUILDS_CONV_PRECISION is False
