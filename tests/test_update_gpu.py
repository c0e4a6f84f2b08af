"""Whole-update parity on the GPU: the HIP agent (through the C ABI) against
 (a) the committed golden vectors produced by the REFERENCE (tests/golden/*.npz), and
 (b) the CPU oracle run on the same seeded batches and noise.

Tolerance (north_star): every per-step loss within 1e-3 relative of the reference on identical
replay batches; log_beta within 1e-5 absolute.  Latents after the first update are compared at
1e-4; after later updates at 2e-3 absolute (Adam's sign-like early steps amplify fp32 rounding;
see tests/test_oracle_golden.py for the same effect between two CPU runs).
"""
import math
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from oracle import fixtures as fx
from oracle.repo_oracle import OracleAgent
from tests.util import log

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _poison_lds():
    """Start every test from NaN-filled LDS on all CUs: reads of never-written LDS cannot hide."""
    from repo_amd._lib import lib

    assert lib().repo_debug_poison_lds(torch.cuda.current_stream().cuda_stream) == 0
    yield


class Space:
    def __init__(self, shape):
        self.shape = shape


class Env:
    def __init__(self, A, image=64):
        self.observation_space = Space((3, image, image))
        self.action_space = Space((A,))


class Logger:
    dir = "/tmp"

    def __init__(self):
        self.kv = {}
        self.nonfinite = []

    def record(self, k, v, exclude=None):
        self.kv[k] = v
        if isinstance(v, (float, np.floating)) and not math.isfinite(v):
            self.nonfinite.append((k, float(v)))    # every non-finite scalar ever logged, not only the last value per key

    def dump(self, step=None):
        pass


def make_agent(algo, L, B, H, A, seed=7, image=64, **over):
    from repo_amd.algorithms.repo import Dreamer, RePo
    from repo_amd.common.utils import set_gpu_mode

    set_gpu_mode(True)
    cfg = fx.default_config(algo=algo, batch_size=B, chunk_size=L, horizon=H, **over)
    agent = (RePo if algo == "repo" else Dreamer)(cfg, Env(A, image), Env(A, image), Logger())
    params = fx.make_params(A, seed, image, belief=cfg.belief_size, state=cfg.state_size, hidden=cfg.hidden_size)
    for mod in fx.MODULES:
        sd = {k: torch.from_numpy(v) for k, v in params[mod].items()}
        agent._load_module(getattr(agent, mod), sd)
    return agent, cfg


def dev_batch(L, B, A, seed, u8=True, image=64):
    obs, act, rew, done = fx.make_batch(L, B, A, seed=seed, image=image)
    o = torch.from_numpy(obs if u8 else fx.preprocess_u8(obs)).cuda()
    return (o, torch.from_numpy(act).cuda(), torch.from_numpy(rew).cuda(), torch.from_numpy(done).cuda()), (obs, act, rew, done)


def dev_noise(L, B, H, A, seed, state=30):
    n = fx.make_noise(L, B, H, A, state=state, seed=seed)
    return {k: torch.from_numpy(v).cuda() for k, v in n.items()}, n


class grad_snapshots:
    """Inside the block, every optimiser in `names` copies its flat gradient as it enters clip_and_step (pre-clip:
    repo_clip_adam reads the gradient as const) into self.snap[name]; leaving it waits for the device (the copies are
    made on whichever stream the agent steps that optimiser on)."""

    def __init__(self, agent, names=("model", "actor", "value")):
        self.agent, self.names, self.snap = agent, names, {}

    def __enter__(self):
        for name in self.names:
            opt = getattr(self.agent, f"{name}_optimizer")
            orig = opt.clip_and_step

            def hooked(norm, opt=opt, orig=orig, name=name):
                self.snap[name] = opt.grad.clone()
                orig(norm)

            opt.clip_and_step = hooked
        return self.snap

    def __exit__(self, *exc):
        for name in self.names:
            del getattr(self.agent, f"{name}_optimizer").clip_and_step
        torch.cuda.synchronize()


_OPT_OF = {"actor_model": "actor", "value_model": "value"}   # every other module's parameters are the model optimiser's


def module_grad_norms(agent, snap):
    """2-norms of each module's pre-clip gradient in fx.MODULES order (the goldens' u*/module_grad_norms)."""
    out = []
    for mod in fx.MODULES:
        name = _OPT_OF.get(mod, "model")
        opt = getattr(agent, f"{name}_optimizer")
        where = {id(q): o for q, o in zip(opt.params, opt.offsets)}
        sq = sum(float(snap[name][where[id(q)] : where[id(q)] + q.numel()].double().pow(2).sum())
                 for q in getattr(agent, mod).parameters())
        out.append(math.sqrt(sq))
    return out


def per_tensor_errors(got, grads, opt):
    """Normwise relative error of each parameter tensor's slice of the flat gradient `got` against the oracle's."""
    out = []
    for gr, o, q in zip(grads, opt.offsets, opt.params):
        if gr is not None:
            a = got[o : o + q.numel()].cpu()
            out.append((tuple(q.shape), ((a - gr.reshape(-1)).norm() / (gr.norm() + 1e-12)).item()))
    return out


CASES = [("repo_tiny.npz", "repo"), ("dreamer_tiny.npz", "dreamer"), ("repo_odd.npz", "repo"), ("repo_c1.npz", "repo")]


@pytest.mark.parametrize("fname,algo", CASES)
def test_update_matches_reference_goldens(golden_dir, fname, algo):
    g = np.load(os.path.join(golden_dir, fname))
    L, B, H, A, n_updates = (int(x) for x in g["meta"])
    agent, cfg = make_agent(algo, L, B, H, A)
    keys = [str(k) for k in g["scalar_keys"]]
    full = fname != "repo_c1.npz"
    worst = 0.0
    # per-module gradient norms: the bound of the totals for RePo; for Dreamer the CPU oracle's own bound against the same
    # golden (tests/test_oracle_golden.py: ReLU flips in the attached decoder reach the encoder and the RSSM)
    mtol = 2e-3 if algo == "repo" else 1e-2
    for u in range(n_updates):
        batch, _ = dev_batch(L, B, A, 11 + u, u8=(u % 2 == 0))  # alternate uint8 / float32 frames
        agent.noise_source, _ = dev_noise(L, B, H, A, 101 + u)
        with grad_snapshots(agent) as snap:
            beliefs, post = agent.train_dynamics(batch[0], batch[1], batch[2], 1.0 - batch[3])
            agent.train_actor_critic(beliefs.flatten(0, 1), post.flatten(0, 1))
        for mod, got, w in zip(fx.MODULES, module_grad_norms(agent, snap), g[f"u{u}/module_grad_norms"]):
            r = abs(got - w) / w
            log(f"[{fname}] update {u} module grad-norm {mod}: got {got:.6g} ref {w:.6g} rel {r:.2e}")
            assert r < mtol, (fname, u, mod, got, w)
        scal = agent.last_scalars
        bl, ps = beliefs.cpu().numpy(), post.cpu().numpy()
        if not full:
            bl, ps = bl[::7, ::3, :8], ps[::7, ::3, :8]
        atol = 1e-4 if u == 0 else 2e-3
        np.testing.assert_allclose(bl, g[f"u{u}/beliefs"], rtol=1e-3, atol=atol)
        np.testing.assert_allclose(ps, g[f"u{u}/posterior_states"], rtol=1e-3, atol=atol)
        want = g[f"u{u}/scalars"]
        for k, w in zip(keys, want):
            got = scal[k]
            r = abs(got - w) / (abs(w) + 1e-12)
            worst = max(worst, r)
            log(f"[{fname}] update {u} {k}: got {got:.7g} ref {w:.7g} rel {r:.2e}")
            assert r < 1e-3, (fname, u, k, got, w)
        if algo == "repo":
            assert abs(float(agent.log_beta) - float(g[f"u{u}/log_beta"])) < 1e-5
        tn = g[f"u{u}/total_norms"]
        gn = agent.last_grad_norms
        for name, w in zip(("model", "actor", "value"), tn):
            r = abs(gn[name] - w) / w
            log(f"[{fname}] update {u} grad-norm {name}: got {gn[name]:.6g} ref {w:.6g} rel {r:.2e}")
            assert r < 2e-3
    log(f"[{fname}] worst scalar rel err {worst:.2e}")
    # parameter checksums after the last Adam step
    names = [str(n) for n in g["param_names"]]
    have = {}
    for m in fx.MODULES:
        for k, v in getattr(agent, m).state_dict().items():
            have[f"{m}.{k}"] = (float(v.double().sum()), float(v.double().abs().sum()))
    for n, s_, a_ in zip(names, g["param_sums"], g["param_abssums"]):
        assert abs(have[n][1] - a_) <= 1e-3 * abs(a_) + 1e-6, (n, have[n][1], a_)
        assert abs(have[n][0] - s_) <= 1e-3 * abs(a_) + 1e-6, (n, have[n][0], s_)


# image=128: the build-defined 128 x 128 conv stack (BASELINE config 4's frame size).  The reference has no such
# model (its flatten hard-codes 64 x 64), so this variant's parity is pinned by the oracle only -- "parity unpinned
# by the reference" (DESIGN.md section 6).
# (L, B, H): (L - 1) * B decoder rows -- 45 and 18 run its two-layer form; 512 (L = 33, B = 16) the composed head
# (functional._DEC_COMPOSE_MIN_ROWS)
@pytest.mark.parametrize("algo,image,A,LBH", [
    pytest.param("repo", 64, 6, (10, 5, 6), id="repo-64-6"),
    pytest.param("dreamer", 64, 6, (10, 5, 6), id="dreamer-64-6"),
    pytest.param("repo", 128, 7, (7, 3, 5), id="repo-128-7"),
    pytest.param("dreamer", 128, 7, (7, 3, 5), id="dreamer-128-7"),
    pytest.param("repo", 64, 6, (33, 16, 5), id="repo-64-6-512rows"),
    pytest.param("dreamer", 64, 6, (33, 16, 5), id="dreamer-64-6-512rows"),
])
def test_update_matches_oracle_latents_and_grads(algo, image, A, LBH):
    L, B, H = LBH
    agent, cfg = make_agent(algo, L, B, H, A, image=image)
    oracle = OracleAgent(cfg, A, seed=7, image=image)
    # At 512 rows a few decoder ReLU decisions within rounding of zero differ between the GPU and the fp32 CPU oracle (the
    # first update's per-tensor errors: up to 5e-4, decoder fc1 / conv1 and encoder conv1); Adam's sign-like first step
    # turns them into parameter differences of up to 2 lr, and the SECOND update's per-tensor gradients then differed by
    # up to 1.3e-2 on those tensors -- a property of the two trajectories, not of the kernels (the decoder alone is within
    # 1e-5 of fp64 there: tests/test_ops_gpu.py).  These cases hand the oracle the agent's parameters (and dual variable)
    # after each update, so that every update's gradients are compared at the same point.
    resync = (L - 1) * B >= 512
    for u in range(2):
        batch, host = dev_batch(L, B, A, 40 + u, u8=(u == 0), image=image)
        agent.noise_source, nz = dev_noise(L, B, H, A, 140 + u)
        # gradients of THIS update before the optimiser touches them: snapshot via a hook on step
        beliefs, post = agent.train_dynamics(batch[0], batch[1], batch[2], 1.0 - batch[3])
        g_model = agent.model_optimizer.grad.clone()
        agent.train_actor_critic(beliefs.flatten(0, 1), post.flatten(0, 1))
        g_actor = agent.actor_optimizer.grad.clone()
        g_value = agent.value_optimizer.grad.clone()
        ob, op_, oscal = oracle.update(*host, nz)
        tol = 1e-4 if u == 0 else 2e-3
        np.testing.assert_allclose(beliefs.cpu().numpy(), ob.numpy(), rtol=1e-3, atol=tol)
        np.testing.assert_allclose(post.cpu().numpy(), op_.numpy(), rtol=1e-3, atol=tol)
        for k, w in oscal.items():
            got = agent.last_scalars[k]
            assert abs(got - w) <= 1e-3 * abs(w) + 1e-7, (u, k, got, w)

        def flat(grads, opt):
            out = torch.zeros(opt.numel)
            for gr, o, p in zip(grads, opt.offsets, opt.params):
                if gr is not None:
                    out[o : o + p.numel()] = gr.reshape(-1)
            return out

        for name, got, want in (
            ("model", g_model, flat(oracle.last["model_grads"], agent.model_optimizer)),
            ("actor", g_actor, flat(oracle.last["actor_grads"], agent.actor_optimizer)),
            ("value", g_value, flat(oracle.last["value_grads"], agent.value_optimizer)),
        ):
            e = ((got.cpu() - want).norm() / want.norm()).item()
            log(f"[oracle {algo} {image}x{image} L={L} B={B}] update {u} flat grad {name}: l2 rel {e:.2e}")
            # normwise (a ReLU unit within rounding of zero may flip between two fp32 runs); observed 2e-7 .. 3e-6
            assert e < 1e-3, (name, e)
        # ... and per parameter tensor (a wrong bias or FiLM-sized tensor vanishes in the flat norm)
        for name, got, grads in (("model", g_model, oracle.last["model_grads"]), ("actor", g_actor, oracle.last["actor_grads"]),
                                 ("value", g_value, oracle.last["value_grads"])):
            errs = per_tensor_errors(got, grads, getattr(agent, f"{name}_optimizer"))
            log(f"[oracle {algo} {image}x{image} L={L} B={B}] update {u} per-tensor {name}: worst "
                f"{max(e for _, e in errs):.2e} " + " ".join(f"{e:.1e}" for _, e in errs))
            for shape, e in errs:
                assert e < 5e-3, (name, shape, e)
        if resync:
            torch.cuda.synchronize()
            with torch.no_grad():
                for m in fx.MODULES:
                    for k, v in getattr(agent, m).state_dict().items():
                        oracle.p[m][k].copy_(v.cpu())
                if algo == "repo":
                    oracle.log_beta.copy_(agent.log_beta.cpu().reshape(oracle.log_beta.shape))


# Other latent widths (cfg.belief_size / state_size): F = belief + state = 232 and 240 give the composed decoder head
# other pads than the default's 232 (functional.DecHead.pad).  The world-model half only: latents and pre-clip model
# gradients against the oracle built on the same parameters.
@pytest.mark.parametrize("algo", ["repo", "dreamer"])
@pytest.mark.parametrize("belief,state", [(200, 32), (208, 32)])
def test_train_dynamics_at_other_latent_widths_matches_oracle(algo, belief, state):
    L, B, H, A = 33, 16, 5, 6
    agent, cfg = make_agent(algo, L, B, H, A, belief_size=belief, state_size=state)
    oracle = OracleAgent(cfg, A, params=fx.make_params(A, 7, belief=belief, state=state))
    batch, host = dev_batch(L, B, A, 45, u8=True)
    agent.noise_source, nz = dev_noise(L, B, H, A, 145, state=state)
    with grad_snapshots(agent, ("model",)) as snap:
        beliefs, post = agent.train_dynamics(batch[0], batch[1], batch[2], 1.0 - batch[3])
    obs, act, rew, done = (torch.from_numpy(x) for x in (fx.preprocess_u8(host[0]), *host[1:]))
    ob, op_, _ = oracle.train_dynamics(obs, act, rew, 1 - done, torch.from_numpy(nz["obs_prior"]),
                                           torch.from_numpy(nz["obs_post"]))
    assert beliefs.shape == (L - 1, B, belief) and post.shape == (L - 1, B, state)
    np.testing.assert_allclose(beliefs.cpu().numpy(), ob.numpy(), rtol=1e-3, atol=1e-4)
    np.testing.assert_allclose(post.cpu().numpy(), op_.numpy(), rtol=1e-3, atol=1e-4)
    opt = agent.model_optimizer
    want = torch.zeros(opt.numel)
    for gr, o, q in zip(oracle.last["model_grads"], opt.offsets, opt.params):
        if gr is not None:
            want[o : o + q.numel()] = gr.reshape(-1)
    e = ((snap["model"].cpu() - want).norm() / want.norm()).item()
    errs = per_tensor_errors(snap["model"], oracle.last["model_grads"], opt)
    log(f"[oracle {algo} belief={belief} state={state} L={L} B={B}] train_dynamics flat model grad {e:.2e}; per-tensor "
        f"worst {max(x for _, x in errs):.2e} " + " ".join(f"{x:.1e}" for _, x in errs))
    assert e < 1e-3, e
    for shape, x in errs:
        assert x < 5e-3, (shape, x)


# The whole update -- train_dynamics AND train_actor_critic (rollout, actor, value) -- at the widths of
# tests/test_widths_gpu.py that take other engines than the default: (belief, hidden, state, action).
WIDTH_UPDATES = [
    pytest.param(208, 208, 32, 16, id="full-blocks"),
    pytest.param(200, 208, 30, 6, id="hidden-ne-belief"),
    pytest.param(200, 200, 31, 6, id="odd-state"),
    pytest.param(200, 200, 30, 1, id="cartpole"),
    pytest.param(200, 200, 30, 21, id="humanoid"),
    pytest.param(256, 256, 32, 6, id="max-width"),
]


@pytest.mark.parametrize("belief,hidden,state,A", WIDTH_UPDATES)
def test_update_at_other_widths_matches_oracle(belief, hidden, state, A):
    L, B, H = 10, 5, 6
    over = dict(belief_size=belief, hidden_size=hidden, state_size=state)
    agent, cfg = make_agent("repo", L, B, H, A, **over)
    oracle = OracleAgent(cfg, A, params=fx.make_params(A, 7, belief=belief, state=state, hidden=hidden))
    tag = f"[oracle widths belief={belief} hidden={hidden} state={state} A={A}]"
    for u in range(2):
        batch, host = dev_batch(L, B, A, 60 + u, u8=(u == 0))
        agent.noise_source, nz = dev_noise(L, B, H, A, 160 + u, state=state)
        with grad_snapshots(agent) as snap:
            beliefs, post = agent.train_dynamics(batch[0], batch[1], batch[2], 1.0 - batch[3])
            agent.train_actor_critic(beliefs.flatten(0, 1), post.flatten(0, 1))
        ob, op_, oscal = oracle.update(*host, nz)
        assert beliefs.shape == (L - 1, B, belief) and post.shape == (L - 1, B, state)
        tol = 1e-4 if u == 0 else 2e-3
        np.testing.assert_allclose(beliefs.cpu().numpy(), ob.numpy(), rtol=1e-3, atol=tol)
        np.testing.assert_allclose(post.cpu().numpy(), op_.numpy(), rtol=1e-3, atol=tol)
        for k, w in oscal.items():
            got = agent.last_scalars[k]
            assert abs(got - w) <= 1e-3 * abs(w) + 1e-7, (u, k, got, w)
        for name, grads in (("model", oracle.last["model_grads"]), ("actor", oracle.last["actor_grads"]),
                            ("value", oracle.last["value_grads"])):
            opt = getattr(agent, f"{name}_optimizer")
            want = torch.zeros(opt.numel)
            for gr, o, q in zip(grads, opt.offsets, opt.params):
                if gr is not None:
                    want[o : o + q.numel()] = gr.reshape(-1)
            e = ((snap[name].cpu() - want).norm() / want.norm()).item()
            errs = per_tensor_errors(snap[name], grads, opt)
            log(f"{tag} update {u} {name}: flat {e:.2e}; per-tensor worst {max(x for _, x in errs):.2e} "
                + " ".join(f"{x:.1e}" for _, x in errs))
            assert e < 1e-3, (name, e)
            for shape, x in errs:
                assert x < 5e-3, (name, shape, x)
        # as in test_update_matches_oracle_latents_and_grads at 512 rows: the oracle takes the agent's parameters, so the
        # second update's gradients are compared at the same point (encoder ReLU ties within rounding of zero, turned into
        # parameter differences by Adam's sign-like first step, moved conv1's second gradient by up to 1.2e-2)
        torch.cuda.synchronize()
        with torch.no_grad():
            for m in fx.MODULES:
                for k, v in getattr(agent, m).state_dict().items():
                    oracle.p[m][k].copy_(v.cpu())
            oracle.log_beta.copy_(agent.log_beta.cpu().reshape(oracle.log_beta.shape))


@pytest.mark.parametrize("belief,state,A,entry", [(264, 30, 6, "repo_rssm_observe_fwd"),
                                                  (200, 30, 40, "repo_rssm_observe_fwd")])
def test_update_at_unsupported_widths_raises_and_leaves_the_model(belief, state, A, entry):
    """belief_size above the row scan's 256 features, and state + action above its 64 columns: the first update raises
    RepoHipError naming the entry point that refused the shape -- no NaN or stale numbers, and no optimiser has stepped."""
    from repo_amd._lib import RepoHipError

    L, B, H = 6, 3, 4
    agent, cfg = make_agent("repo", L, B, H, A, belief_size=belief, state_size=state)
    batch, _ = dev_batch(L, B, A, 70)
    agent.noise_source, _ = dev_noise(L, B, H, A, 170, state=state)
    opts = (agent.model_optimizer, agent.actor_optimizer, agent.value_optimizer)
    before = [t.clone() for o in opts for t in (o.flat, o.exp_avg, o.exp_avg_sq)] + [agent.log_beta.clone()]
    steps = [o.step_count for o in opts]
    with pytest.raises(RepoHipError, match=entry):
        agent.update(batch)
        agent.last_scalars
    torch.cuda.synchronize()
    after = [t for o in opts for t in (o.flat, o.exp_avg, o.exp_avg_sq)] + [agent.log_beta]
    assert [o.step_count for o in opts] == steps
    for i, (a, b) in enumerate(zip(before, after)):
        assert torch.equal(a, b), i


def test_full_size_update_properties():
    """BASELINE config 2 shapes (B=50, L=50, H=15): size-independent properties."""
    L, B, H, A = 50, 50, 15, 6
    agent, cfg = make_agent("repo", L, B, H, A)
    batch, _ = dev_batch(L, B, A, 1234)
    p0 = agent.model_optimizer.flat.clone()
    agent.update(batch)
    s1 = dict(agent.last_scalars)
    assert all(np.isfinite(v) for v in s1.values()), s1
    # sanity anchors observed on the reference with uniform-random frames
    assert 13000 < s1["train/obs_loss"] < 13800
    assert 0.05 < s1["train/kl_div"] < 1.0
    assert abs(s1["train/beta"] - 1e-5) < 1e-7
    # every parameter moved by at most ~lr (Adam's first step is sign-like) and most of them did move
    dlt = (agent.model_optimizer.flat - p0).abs()
    assert float(dlt.max()) <= 3e-4 * 1.01
    assert float((dlt > 0).float().mean()) > 0.9
    # determinism: same batch + same injected noise on a fresh agent gives bit-identical scalars
    noise, _ = dev_noise(L, B, H, A, 5)
    outs = []
    for _ in range(2):
        ag, _ = make_agent("repo", L, B, H, A)
        ag.noise_source = noise
        ag.update(batch)
        outs.append(dict(ag.last_scalars))
    assert outs[0] == outs[1], (outs[0], outs[1])


@pytest.mark.parametrize("image", [64, 128])
def test_module_autograd_wrappers(image):
    """encoder / obs_model / reward_model / transition_model.observe as autograd nodes."""
    from repo_amd.algorithms.repo.models.utils import bottle
    from oracle import repo_oracle as ro

    L, B, H, A = 6, 3, 4, 6
    agent, cfg = make_agent("dreamer", L, B, H, A, image=image)
    batch, host = dev_batch(L, B, A, 77, u8=False, image=image)
    obs, act, rew, done = batch
    nz, nzh = dev_noise(L, B, H, A, 177)
    T = L - 1
    embeds = bottle(agent.encoder, (obs,))
    b0 = torch.zeros(B, cfg.belief_size, device="cuda")
    s0 = torch.zeros(B, cfg.state_size, device="cuda")
    outs = agent.transition_model.observe(b0, s0, act[:-1], embeds[1:], 1 - done[:-1], noise=(nz["obs_prior"], nz["obs_post"]))
    beliefs, post = outs[0], outs[4]
    recon = bottle(agent.obs_model, (beliefs, post))
    rp = bottle(agent.reward_model, (beliefs, post))
    loss = (0.5 * (recon - obs[1:]) ** 2).sum((2, 3, 4)).mean() + (rp**2).mean() + outs[2].pow(2).mean()
    for p in agent.model_params:
        p.grad = None
    loss.backward()
    # oracle
    o = OracleAgent(cfg, A, seed=7, image=image)
    ho = torch.from_numpy(fx.preprocess_u8(host[0]))
    oe = ro.encoder_fwd(o.p["encoder"], ho.reshape(L * B, 3, image, image)).reshape(L, B, -1)
    oo = ro.observe(o.p["transition_model"], torch.zeros(B, 200), torch.zeros(B, 30), torch.from_numpy(host[1])[:-1], oe[1:],
                    1 - torch.from_numpy(host[3])[:-1], torch.from_numpy(nzh["obs_prior"]), torch.from_numpy(nzh["obs_post"]))
    fb, fs = oo[0].reshape(T * B, -1), oo[4].reshape(T * B, -1)
    orec = ro.decoder_fwd(o.p["obs_model"], fb, fs).reshape(T, B, 3, image, image)
    orp = ro.scalar_head(o.p["reward_model"], fb, fs).reshape(T, B)
    ol = (0.5 * (orec - ho[1:]) ** 2).sum((2, 3, 4)).mean() + (orp**2).mean() + oo[2].pow(2).mean()
    ol.backward()
    assert abs(loss.item() - ol.item()) < 1e-4 * abs(ol.item())
    got = torch.cat([p.grad.reshape(-1) for p in agent.model_params]).cpu()
    want = torch.cat([q.grad.reshape(-1) for q in o.model_params])
    e = ((got - want).norm() / want.norm()).item()
    log(f"[autograd wrappers] loss {loss.item():.6g} vs {ol.item():.6g}; model grad l2 rel {e:.2e}")
    assert e < 5e-3


def test_pipelined_updates_are_bit_deterministic():
    """Two identically seeded agents, 25 pipelined updates each (in-kernel Philox noise, two 16-row groups in the
    column-split scans): bit-identical parameters.  A stale or torn read in the scans' all-gathers through L2
    (csrc/scan_cs.hip), or any other race between the update's streams, would show here (tools/determinism_soak.py is
    the long version: 400 updates at B=50, 600 at B=7)."""
    L, B, H, A = 12, 20, 6, 6
    batches = [dev_batch(L, B, A, 300 + i)[0] for i in range(3)]
    finals = []
    for _ in range(2):
        agent, _cfg = make_agent("repo", L, B, H, A)
        agent.seed_noise(99)
        for i in range(25):
            agent.update(batches[i % 3], join=False)
        agent.synchronize()
        torch.cuda.synchronize()
        assert all(np.isfinite(v) for v in agent.last_scalars.values())
        finals.append([o.flat.clone() for o in (agent.model_optimizer, agent.actor_optimizer, agent.value_optimizer)]
                      + [agent.log_beta.clone().reshape(1)])
    for a, b in zip(*finals):
        assert torch.equal(a, b)
