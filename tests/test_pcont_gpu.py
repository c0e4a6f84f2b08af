"""config.pcont on the GPU: the two kernels of csrc/loss.hip against float64 on the float32-rounded inputs,
common.utils.lambda_return on a discount tensor, whole updates of RePo and Dreamer against tests/pcont_ref.py's OraclePcont
(tied to torch's own functions by tests/test_pcont_cpu.py), the combined configuration, the untouched default path,
checkpoints, the families that refuse, and determinism.

Bounds.  Kernels: tests/test_widths_gpu.py's -- forward values FTOL = 1e-5 of the largest element, gradients GTOL = 1e-4
normwise, sums FTOL of sum |terms|.  Updates: tests/test_update_gpu.py::test_update_at_other_widths_matches_oracle's --
scalars 1e-3, latents rtol 1e-3 / atol 1e-4 then 2e-3, flat gradients 1e-3, per-tensor gradients 5e-3."""
import numpy as np
import pytest
import torch

from oracle import fixtures as fx
from oracle import repo_oracle as ro
from tests import act_ref as ar
from tests import pcont_ref as pr
from tests import reduce_ref as rr
from tests import test_update_gpu as tu
from tests.util import has, l2err, log, relerr, traced

pytestmark = pytest.mark.gpu

FTOL = 1e-5
GTOL = 1e-4
E_SHAPE = -2   # include/repo_hip.h


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


# ----------------------------------------------------------------------------- 1. repo_bernoulli_nll
def test_bernoulli_grid_regimes():
    """65536 elements are the last that finish in their own launch; 65537 take the follow-up launch."""
    assert rr.finishes_in_launch(rr.red_blocks(65536, 1024)) and not rr.finishes_in_launch(rr.red_blocks(65537, 1024))


@pytest.mark.parametrize("n", [1, 255, 257, 65537])
def test_bernoulli_nll(ops, n):
    rs = np.random.RandomState(n)
    logit = (rs.standard_normal(n) * 3.0).astype(np.float32)
    planted = [90.0, -90.0, 40.0, -40.0][:n] if n < 8 else [40.0, -40.0, 90.0, -90.0, 90.0, -90.0, 40.0, -40.0]
    logit[:len(planted)] = planted
    base = (rs.uniform(size=n) < 0.7).astype(np.float32)
    if n >= 8:
        base[:8] = [1, 1, 1, 1, 0, 0, 0, 0]      # each planted logit against both targets
    gamma, scale = 0.99, 10.0 / n
    l64 = torch.from_numpy(logit).double().requires_grad_(True)
    y64 = float(np.float32(gamma)) * torch.from_numpy(base).double()
    terms = pr.bernoulli_nll(l64, y64)
    (terms.sum() * scale).backward()
    ld, bd = torch.from_numpy(logit).cuda(), torch.from_numpy(base).cuda()
    s1, d1 = ops.bernoulli_nll(ld, bd, gamma, scale)
    s2, d2 = ops.bernoulli_nll(ld, bd, gamma, scale)
    assert torch.equal(s1, s2) and torch.equal(d1, d2), "two runs differ"
    assert torch.isfinite(s1).all() and torch.isfinite(d1).all()
    e_s = abs(float(s1) - float(terms.sum())) / float(terms.abs().sum())
    e_g = l2err(d1, l64.grad)
    log(f"bernoulli_nll n={n}: sum {e_s:.2e} dlogit {e_g:.2e}")
    assert e_s < FTOL and e_g < GTOL
    s3, none = ops.bernoulli_nll(ld, bd, gamma, scale, want_grad=False)
    assert none is None and torch.equal(s3, s1)


# ----------------------------------------------------------------------------- 2. repo_lambda_return_disc
RET_CASES = [(2, 1), (3, 5), (14, 257), (14, 16385)]


def test_lambda_return_disc_grid_regimes():
    """16385 is the first N that takes the follow-up launch (one thread per column, 256 per block, 64 blocks)."""
    assert rr.finishes_in_launch(rr.red_blocks(16384, 256)) and not rr.finishes_in_launch(rr.red_blocks(16385, 256))
    assert rr.red_blocks(16385, 256) == rr.lambda_return_blocks(16385)


def _ret_inputs(Hm, N):
    rs = np.random.RandomState(100 * Hm + N % 97)
    r = rs.standard_normal((Hm, N)).astype(np.float32)
    v = rs.standard_normal((Hm, N)).astype(np.float32)
    logit = (rs.standard_normal((Hm, N)) * 2.0 + 2.0).astype(np.float32)
    if N >= 5:
        logit[:, 1] = -40.0     # the weights collapse to 0 behind the first step
        logit[:, 2] = 40.0      # p = 1 to rounding
    return r, v, logit


@pytest.mark.parametrize("is_logit", [0, 1])
@pytest.mark.parametrize("lam", [0.0, 0.95, 1.0])
@pytest.mark.parametrize("Hm,N", RET_CASES)
def test_lambda_return_disc(ops, Hm, N, lam, is_logit):
    r, v, logit = _ret_inputs(Hm, N)
    disc = logit if is_logit else torch.sigmoid(torch.from_numpy(logit).double()).float().numpy()
    gret = -1.0 / ((Hm - 1) * N)
    r64, v64, d64 = (torch.from_numpy(a).double().requires_grad_(True) for a in (r, v, disc))
    p64 = torch.sigmoid(d64) if is_logit else d64
    R, w = pr.weighted_returns(r64[:-1], v64[:-1], p64[:-1], v64[-1], lam)
    w = w.detach()
    (gret * (w * R).sum()).backward()
    rd, vd, dd = (torch.from_numpy(a).cuda() for a in (r, v, disc))
    # the rows the kernel must not read: NaN would reach every output that read them
    rd[-1], dd[-1] = float("nan"), float("nan")
    returns, weights, dr, dv, dc, sums = ops.lambda_return_disc(rd, vd, dd, lam, gret, disc_is_logit=bool(is_logit))
    again = ops.lambda_return_disc(rd, vd, dd, lam, gret, disc_is_logit=bool(is_logit))
    for a, b in zip((returns, weights, dr, dv, dc, sums), again):
        assert torch.equal(a, b), "two runs differ"
    for t in (returns, weights, dr, dv, dc, sums):
        assert torch.isfinite(t).all()
    errs = {"returns": relerr(returns, R), "weights": relerr(weights, w),
            "sum wR": abs(float(sums[0]) - float((w * R).sum())) / float((w * R).abs().sum()),
            "sum w": abs(float(sums[1]) - float(w.sum())) / float(w.sum()),
            "drewards": l2err(dr, r64.grad), "dvalues": l2err(dv, v64.grad), "ddisc": l2err(dc, d64.grad)}
    log(f"lambda_return_disc Hm={Hm} N={N} lam={lam} logit={is_logit}: " + " ".join(f"{k} {e:.2e}" for k, e in errs.items()))
    for k in ("returns", "weights", "sum wR", "sum w"):
        assert errs[k] < FTOL, (k, errs[k])
    for k in ("drewards", "dvalues", "ddisc"):
        assert errs[k] < GTOL, (k, errs[k])
    assert (dr[-1] == 0).all() and (dc[-1] == 0).all() and (dv[0] == 0).all()
    if N >= 5:
        assert float(weights[1:, 1].abs().max()) < 1e-15      # (every case with these columns has Hm >= 3)
        assert torch.equal(weights[:, 2], torch.ones_like(weights[:, 2]))
    # forward only: no gradient buffer exists to write, the forward outputs are the same bits
    f = ops.lambda_return_disc(rd, vd, dd, lam, gret, disc_is_logit=bool(is_logit), want_grads=False)
    assert f[2] is None and f[3] is None and f[4] is None
    assert torch.equal(f[0], returns) and torch.equal(f[1], weights) and torch.equal(f[5], sums)


def test_lambda_return_disc_refuses_one_row_and_partial_gradients(ops):
    from repo_amd._lib import lib

    N = 4
    bufs = [torch.zeros(2, N, device="cuda") for _ in range(8)]
    out = torch.zeros(2, device="cuda")
    ws = ops.reduce_ws(out.device)
    st = torch.cuda.current_stream().cuda_stream
    p = [b.data_ptr() for b in bufs]
    call = lib().repo_lambda_return_disc
    assert call(1, N, p[0], p[1], p[2], 1, 0.95, 0.0, p[3], p[4], None, None, None, out.data_ptr(), ws.data_ptr(),
                ws.numel(), st) == E_SHAPE
    # the three gradients come together or not at all
    assert call(2, N, p[0], p[1], p[2], 1, 0.95, 0.0, p[3], p[4], p[5], p[6], None, out.data_ptr(), ws.data_ptr(),
                ws.numel(), st) == -1
    assert call(2, N, p[0], p[1], p[2], 1, 0.95, 0.0, p[3], p[4], p[5], p[6], p[7], out.data_ptr(), ws.data_ptr(),
                ws.numel(), st) == 0
    torch.cuda.synchronize()


# ----------------------------------------------------------------------------- 3. common.utils.lambda_return
def test_public_lambda_return_takes_a_discount_tensor(ops):
    from repo_amd.common.utils import lambda_return

    rs = np.random.RandomState(3)
    L, N, lam = 6, 37, 0.95
    r, v = (torch.from_numpy(rs.standard_normal((L, N)).astype(np.float32)) for _ in range(2))
    boot = torch.from_numpy(rs.standard_normal(N).astype(np.float32))
    disc = torch.from_numpy(rs.uniform(0.5, 1.0, (L, N)).astype(np.float32))
    got = lambda_return(r.cuda(), v.cuda(), disc.cuda(), boot.cuda(), lam)
    want = ro.lambda_return(r.double(), v.double(), disc.double(), boot.double(), lam)
    assert got.shape == want.shape and relerr(got, want) < FTOL
    # a constant tensor keeps the one-discount kernel, bit for bit
    const = torch.full((L, N), 0.99)
    got = lambda_return(r.cuda(), v.cuda(), const.cuda(), boot.cuda(), lam)
    pad = torch.zeros(1, N)
    same = ops.lambda_return(torch.cat([r, pad]).cuda(), torch.cat([v, boot[None]]).cuda(), 0.99, lam, want_grads=False)[0]
    assert torch.equal(got, same)
    assert relerr(got, ro.lambda_return(r.double(), v.double(), const.double(), boot.double(), lam)) < FTOL


# ----------------------------------------------------------------------------- agents
def make_pcont_agent(algo, L, B, H, A, **over):
    agent, cfg = tu.make_agent(algo, L, B, H, A, pcont=True, **over)
    head = pr.make_pcont_params(cfg.belief_size, cfg.state_size, cfg.hidden_size)
    assert list(agent.pcont_model.state_dict().keys()) == list(head.keys())
    agent._load_module(agent.pcont_model, {k: torch.from_numpy(v) for k, v in head.items()})
    return agent, cfg


def run_updates(agent, L, B, H, A, n):
    for u in range(n):
        batch, _ = tu.dev_batch(L, B, A, 11 + u)
        agent.noise_source, _ = tu.dev_noise(L, B, H, A, 101 + u)
        agent.update(batch)
    return agent.last_scalars


# ----------------------------------------------------------------------------- 4. whole updates against the oracle
@pytest.mark.parametrize("algo", ["repo", "dreamer"])
def test_update_matches_oracle(algo):
    L, B, H, A = 10, 5, 6, 6
    agent, cfg = make_pcont_agent(algo, L, B, H, A)
    oracle = pr.OraclePcont(cfg, A, params=fx.make_params(A, 7))
    mods = fx.MODULES + ("pcont_model",)
    assert [tuple(q.shape) for q in agent.model_optimizer.params[-8:]] == [tuple(q.shape) for q in oracle.model_params[-8:]]
    tag = f"[oracle pcont {algo}]"
    for u in range(2):
        batch, host = tu.dev_batch(L, B, A, 60 + u, u8=(u == 0))
        dones = host[3][:, :, 0]
        assert dones.max() == 1.0 and (dones.sum(0) == 0).any(), "the batch needs a terminal step and a column without one"
        agent.noise_source, nz = tu.dev_noise(L, B, H, A, 160 + u)
        with tu.grad_snapshots(agent) as snap:
            beliefs, post = agent.train_dynamics(batch[0], batch[1], batch[2], 1.0 - batch[3])
            agent.train_actor_critic(beliefs.flatten(0, 1), post.flatten(0, 1))
        ob, op_, oscal = oracle.update(*host, nz)
        tol = 1e-4 if u == 0 else 2e-3
        np.testing.assert_allclose(beliefs.cpu().numpy(), ob.numpy(), rtol=1e-3, atol=tol)
        np.testing.assert_allclose(post.cpu().numpy(), op_.numpy(), rtol=1e-3, atol=tol)
        assert "train/pcont_loss" in oscal
        for k, w in oscal.items():
            got = agent.last_scalars[k]
            log(f"{tag} update {u} {k}: got {got:.7g} oracle {w:.7g} rel {abs(got - w) / (abs(w) + 1e-12):.2e}")
            assert abs(got - w) <= 1e-3 * abs(w) + 1e-7, (u, k, got, w)
        for name, grads in (("model", oracle.last["model_grads"]), ("actor", oracle.last["actor_grads"]),
                            ("value", oracle.last["value_grads"])):
            opt = getattr(agent, f"{name}_optimizer")
            want = torch.zeros(opt.numel)
            for gr, o, q in zip(grads, opt.offsets, opt.params):
                if gr is not None:
                    want[o : o + q.numel()] = gr.reshape(-1)
            e = ((snap[name].cpu() - want).norm() / want.norm()).item()
            errs = tu.per_tensor_errors(snap[name], grads, opt)
            log(f"{tag} update {u} {name}: flat {e:.2e}; per-tensor worst {max(x for _, x in errs):.2e} "
                + " ".join(f"{x:.1e}" for _, x in errs))
            assert e < 1e-3, (name, e)
            if name == "model":
                assert len(errs) == len(opt.params) and all(g is not None for g in grads[-8:])   # the head's eight included
            for shape, x in errs:
                assert x < 5e-3, (name, shape, x)
        torch.cuda.synchronize()
        with torch.no_grad():   # the oracle takes the agent's parameters: the second update is compared at the same point
            for m in mods:
                for k, v in getattr(agent, m).state_dict().items():
                    oracle.p[m][k].copy_(v.cpu())
            if algo == "repo":
                oracle.log_beta.copy_(agent.log_beta.cpu().reshape(oracle.log_beta.shape))


# ----------------------------------------------------------------------------- 5. the combined configuration
def test_pcont_with_inverse_dynamics_relu_and_state_vectors():
    from tests import test_symbolic_gpu as ts

    L, B, H, A = 8, 4, 5, 6
    agent, cfg = ts.make_sym_agent("repo", L, B, H, A, pcont=True, dense_activation_function="relu", inv_dynamics=True,
                                   inv_dynamics_lr=3e-4, inv_dynamics_hidden_size=64)
    head = pr.make_pcont_params(cfg.belief_size, cfg.state_size, cfg.hidden_size)
    agent._load_module(agent.pcont_model, {k: torch.from_numpy(v) for k, v in head.items()})
    batch = ts.sym_batch(L, B, A, 11)
    agent.noise_source, _ = tu.dev_noise(L, B, H, A, 101)
    nonterms = 1.0 - batch[3]
    beliefs, post = agent.train_dynamics(batch[0], batch[1], batch[2], nonterms)
    agent.train_actor_critic(beliefs.flatten(0, 1), post.flatten(0, 1))
    scal = agent.last_scalars
    assert all(np.isfinite(v) for v in scal.values()), scal
    assert not agent.logger.nonfinite
    assert "train/inv_dyn_loss" in scal and "inv_dynamics" in agent.last_grad_norms
    # the restatement on the agent's own latents and the head's pre-step parameters
    p64 = {k: torch.from_numpy(v).double() for k, v in head.items()}
    x = torch.cat([beliefs, post], 2).flatten(0, 1).double().cpu()
    logit = ar.mlp_head(p64, x, 4, "relu").reshape(-1)
    want = cfg_scale(cfg) * pr.bernoulli_nll(logit, cfg.gamma * nonterms[:-1].reshape(-1).double().cpu()).mean().item()
    got = scal["train/pcont_loss"]
    log(f"[pcont combined] pcont_loss got {got:.7g} restated {want:.7g}")
    assert abs(got - want) <= 1e-3 * abs(want)
    parts = scal["train/obs_loss"] + scal["train/reward_loss"] + scal["train/kl_loss"] + got
    assert abs(scal["train/model_loss"] - parts) <= 1e-6 * abs(parts)


def cfg_scale(cfg):
    return float(getattr(cfg, "pcont_scale", 10.0))


# ----------------------------------------------------------------------------- 6. the default path
def test_default_path_is_untouched():
    L, B, H, A = 8, 4, 5, 6
    off, _ = tu.make_agent("repo", L, B, H, A, pcont=False)
    plain, cfg = tu.make_agent("repo", L, B, H, A)
    assert not hasattr(cfg, "pcont") and not hasattr(off, "pcont_model") and not hasattr(plain, "pcont_model")
    run_updates(off, L, B, H, A, 2)
    run_updates(plain, L, B, H, A, 2)
    torch.cuda.synchronize()
    for name in ("model", "actor", "value"):
        a, b = getattr(off, f"{name}_optimizer"), getattr(plain, f"{name}_optimizer")
        assert torch.equal(a.flat, b.flat) and torch.equal(a.exp_avg, b.exp_avg), name
    assert off.last_scalars == plain.last_scalars and "train/pcont_loss" not in plain.last_scalars
    assert list(off.get_param_dict().keys()) == list(plain.get_param_dict().keys())
    batch, _ = tu.dev_batch(L, B, A, 13)
    plain.noise_source, _ = tu.dev_noise(L, B, H, A, 103)
    _, names = traced(lambda: plain.update(batch))
    assert has(names, "lambda_return_kernel") and has(names, "scalar_nll_kernel")
    assert not has(names, "bernoulli_nll") and not has(names, "lambda_return_disc"), names
    # ... and the names would show: the switched-on agent launches both
    on, _ = make_pcont_agent("repo", L, B, H, A)
    on.noise_source = plain.noise_source
    _, names = traced(lambda: on.update(batch))
    assert has(names, "bernoulli_nll_kernel") and has(names, "lambda_return_disc_kernel"), names
    assert not has(names, r"\blambda_return_kernel")


# ----------------------------------------------------------------------------- 7. checkpoints
def test_checkpoint_key_and_round_trip(golden_dir):
    import json
    import os

    L, B, H, A = 8, 4, 5, 6
    a, _ = make_pcont_agent("repo", L, B, H, A)
    plain, _ = tu.make_agent("repo", L, B, H, A)
    assert "pcont_model" not in plain.get_param_dict()
    with open(os.path.join(golden_dir, "checkpoint_manifest.json")) as f:
        assert list(plain.get_param_dict().keys()) == json.load(f)["repo"]["top_keys"]   # the default config's key list
    run_updates(a, L, B, H, A, 2)
    ck = a.get_param_dict()
    assert list(ck["pcont_model"].keys()) == pr.HEAD_KEYS
    assert set(ck.keys()) == set(plain.get_param_dict().keys()) | {"pcont_model"}
    b, _ = tu.make_agent("repo", L, B, H, A, pcont=True)
    assert not torch.equal(b.model_optimizer.flat, a.model_optimizer.flat)
    b.load_param_dict(ck)
    for name in ("flat", "exp_avg", "exp_avg_sq"):
        assert torch.equal(getattr(a.model_optimizer, name), getattr(b.model_optimizer, name)), name
    for (k, v), w in zip(b.pcont_model.state_dict().items(), ck["pcont_model"].values()):
        assert torch.equal(v, w), k
    # a checkpoint without the entry loads: the head keeps its weights
    keep = [t.clone() for t in b.pcont_model.plist()]
    b.load_param_dict({k: v for k, v in ck.items() if k != "pcont_model"})
    for t, w in zip(b.pcont_model.plist(), keep):
        assert torch.equal(t, w)


# ----------------------------------------------------------------------------- 8. the other families
def _family_builders():
    from repo_amd.algorithms.repo import FinetunedRePo
    from repo_amd.common.utils import set_gpu_mode
    from tests import test_calib_gpu as tc
    from tests import test_mt_gpu as tm
    from tests import test_tia_gpu as tt

    set_gpu_mode(True)

    def finetuned(**over):
        cfg = fx.default_config(algo="repo", batch_size=4, chunk_size=8, horizon=5, **over)
        return FinetunedRePo(cfg, tu.Env(6), tu.Env(6), tu.Logger())

    return {"FinetunedRePo": finetuned,
            "CalibratedRePo": lambda **over: tc.make_calib_agent("js", **over)[0],
            "TIA": lambda **over: tt.make_tia(8, 4, 5, 6, **over)[0],
            "MultitaskDreamer": lambda **over: tm.make_mt("dreamer_multitask", 8, 4, 5, 6, 3, **over)[0],
            "MultitaskRePo": lambda **over: tm.make_mt("repo_multitask", 8, 4, 5, 6, 3, **over)[0]}


@pytest.mark.parametrize("family", ["FinetunedRePo", "CalibratedRePo", "TIA", "MultitaskDreamer", "MultitaskRePo"])
def test_other_families_refuse(family):
    build = _family_builders()[family]
    with pytest.raises(NotImplementedError, match="pcont"):
        build(pcont=True)
    agent = build(pcont=False)
    assert type(agent).__name__ == family and not hasattr(agent, "pcont_model")


# ----------------------------------------------------------------------------- 9. determinism
def test_two_seeded_agents_are_bit_equal():
    L, B, H, A = 8, 4, 5, 6
    batches = [tu.dev_batch(L, B, A, 300 + i)[0] for i in range(2)]
    finals = []
    for _ in range(2):
        agent, _cfg = make_pcont_agent("dreamer", L, B, H, A)
        agent.seed_noise(99)
        for b in batches:
            agent.update(b, join=False)
        agent.synchronize()
        torch.cuda.synchronize()
        assert all(np.isfinite(v) for v in agent.last_scalars.values())
        finals.append([o.flat.clone() for o in (agent.model_optimizer, agent.actor_optimizer, agent.value_optimizer)]
                      + [torch.tensor([agent.last_scalars["train/pcont_loss"]])])
    for a, b in zip(*finals):
        assert torch.equal(a, b)
