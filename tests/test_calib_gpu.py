"""CalibratedRePo's discriminator on the GPU: the kernels of csrc/vdb.hip and the LeakyReLU dense chain behind
repo_amd.common.models.gans.VDBDiscriminator against the float64 restatement of tests/calib_ref.py (tied to the reference's
own modules by tests/test_calib_cpu.py), in both alignment modes.

Bounds:
 * d, mean, logstd, the four losses, the penalty's value, beta: FTOL = 1e-5 (tests/test_dense_act_gpu.py);
 * every parameter gradient WITHOUT the penalty, and the input gradient: per tensor GTOL = 1e-4 in the l2 norm;
 * the penalty's own parameter gradients: max(GTOL, 4 x the per-tensor l2 error of the restatement run in float32 on the
   CPU against its float64 self at the same case) -- that chain is three times as long, the GPU sums in another order
   and splits bf16.  Measured (max over the tensors of a case; JS / support mode), PEN_F32 below:
       (37, 37, 1024, 32, 8) 2.6e-7   (2, 2, 1024, 256, 64) 7.9e-7   (16, 48, 40, 24, 5) 2.8e-7   (1, 1, 8, 4, 1) 3.0e-7
   (the same in both modes: the penalty does not depend on the mode), the largest tensor of a case being a weight of
   the first layers; 4 x the measurement is at most 3.2e-6, so the bound is GTOL = 1e-4 in every case.
 * the reference-width case runs 2 + 2 rows: of the first 64 seeds none met the margin at 5 or 4 or 3 rows (10.9 k
   activation inputs at 5), seed 36 does at 2.
 * parameters after the Adam step: 1e-2 lr (an Adam step moves every weight by about lr whatever the gradient's
   size, so a gradient element that is pure rounding noise may flip its step: only elements with |g| >= 1e-2 max|g| of
   their tensor are compared, the others are bounded by the step size).

Condition: each case asserts min |pre| >= PRE_MARGIN over every LeakyReLU input the restatement formed, `lat` included;
the seeds below were picked on the CPU (the first of 0..63 that meets it)."""
import functools

import numpy as np
import pytest
import torch

from tests import calib_ref as cr
from tests.util import has, l2err, log, relerr, traced

pytestmark = pytest.mark.gpu

FTOL = 1e-5   # tests/test_dense_act_gpu.py FTOL
GTOL = 1e-4   # tests/test_dense_act_gpu.py GTOL
LR = 1e-4
BETA0 = 0.1

# (N_real, N_fake, E, Hf, Z)
CASES = [(37, 37, 1024, 32, 8), (2, 2, 1024, 256, 64), (16, 48, 40, 24, 5), (1, 1, 8, 4, 1)]
# (case index, support) -> seed of the inputs: the first of 0..63 with min |pre| >= PRE_MARGIN (picked on the CPU)
SEEDS = {(0, False): 1, (0, True): 1, (1, False): 36, (1, True): 36, (2, False): 8, (2, True): 8, (3, False): 0, (3, True): 0}
# (case index, support) -> max over the parameter tensors of the l2 error of the PENALTY's gradient, restatement in float32
# on the CPU against float64
PEN_F32 = {(0, False): 2.6e-07, (0, True): 2.6e-07, (1, False): 7.9e-07, (1, True): 7.9e-07, (2, False): 2.8e-07,
           (2, True): 2.8e-07, (3, False): 3e-07, (3, True): 3e-07}
PARAMS = [(i, s) for i in range(len(CASES)) for s in (False, True)]


def make_case(ci, support, seed):
    """Seeded float32 inputs of a case: x_real, x_fake, eps_real, eps_fake, tau (support mode) or None."""
    Nr, Nf, E, Hf, Z = CASES[ci]
    rs = np.random.RandomState(1000 * ci + seed)
    t = lambda *s: torch.from_numpy(rs.standard_normal(s).astype(np.float32))  # noqa: E731
    xr, xf, er, ef = t(Nr, E), t(Nf, E), t(Nr, Z), t(Nf, Z)
    tau = torch.exp(0.3 * t(Nr)) if support else None
    return xr, xf, er, ef, tau


def restate(ci, support, seed, dtype=torch.float64):
    """Everything the tests compare, from the restatement at `dtype` on the CPU."""
    Nr, Nf, E, Hf, Z = CASES[ci]
    xr, xf, er, ef, tau = (None if v is None else v.to(dtype) for v in make_case(ci, support, seed))
    params = cr.make_disc_params(E, Hf, Z)
    p = {k: torch.from_numpy(v).to(dtype).requires_grad_(True) for k, v in params.items()}
    pre = []
    out = cr.disc_losses(p, xr, xf, er, ef, BETA0, tau=tau, pre=pre)
    names = list(p.keys())
    g_main = torch.autograd.grad(out["real"] + out["fake"] + out["kl_loss"], [p[k] for k in names], retain_graph=True)
    g_pen = torch.autograd.grad(out["gp"], [p[k] for k in names], allow_unused=True)
    g_pen = [torch.zeros_like(p[k]) if g is None else g for k, g in zip(names, g_pen)]   # fc.bias: no penalty gradient
    res = {k: float(out[k].detach()) for k in ("real", "fake", "kl", "gp")}
    res["beta"] = cr.beta_step(BETA0, res["kl"])
    res["g_main"] = dict(zip(names, (g.detach() for g in g_main)))
    res["g_pen"] = dict(zip(names, (g.detach() for g in g_pen)))
    res["stepped"] = {k: cr.adam_first_step(p[k].detach(), res["g_main"][k] + res["g_pen"][k], LR) for k in names}
    res["min_pre"] = cr.min_abs_pre(pre)
    # the forward alone, and the generator side: the alignment loss's gradient into the fake rows
    xg = xf.clone().requires_grad_(True)
    pd = {k: v.detach() for k, v in p.items()}
    d, mean, logstd = cr.disc_forward(pd, xg, ef)
    res["d"], res["mean"], res["logstd"] = d.detach(), mean.detach(), logstd.detach()
    gl = cr.generator_loss(d, support)
    res["gen"] = float(gl.detach())
    res["dx"], = torch.autograd.grad(gl, xg)
    return res


@functools.lru_cache(maxsize=None)
def reference(ci, support):
    return restate(ci, support, SEEDS[(ci, support)])


@pytest.fixture(autouse=True)
def _poison_lds():
    from repo_amd._lib import lib

    assert lib().repo_debug_poison_lds(torch.cuda.current_stream().cuda_stream) == 0
    yield


def make_disc(ci):
    from repo_amd.common.models.gans import VDBDiscriminator

    Nr, Nf, E, Hf, Z = CASES[ci]
    params = cr.make_disc_params(E, Hf, Z)
    disc = VDBDiscriminator(E, [Hf] * 4, Z, lr=LR, init_beta=BETA0, device="cuda")
    assert [(k, tuple(v.shape)) for k, v in disc.state_dict().items()] == [(k, v.shape) for k, v in params.items()]
    disc.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    return disc, list(params.keys())


def dev_case(ci, support):
    xr, xf, er, ef, tau = make_case(ci, support, SEEDS[(ci, support)])
    return xr.cuda(), xf.cuda(), (er.cuda(), ef.cuda()), None if tau is None else tau.cuda()


@pytest.mark.parametrize("ci,support", PARAMS)
def test_forward_and_generator_side_match_the_restatement(ci, support):
    from repo_amd import ops

    ref = reference(ci, support)
    assert ref["min_pre"] >= cr.PRE_MARGIN, ref["min_pre"]
    disc, _ = make_disc(ci)
    xr, xf, eps, tau = dev_case(ci, support)
    d, mean, logstd = disc(xf, eps=eps[1])
    for name, got in (("d", d[:, 0]), ("mean", mean), ("logstd", logstd)):
        e = relerr(got, ref[name])
        log(f"[vdb fwd {CASES[ci]} support={support}] {name}: relerr {e:.2e}")
        assert e < FTOL, (name, e)
    # the generator side through the frozen discriminator: loss and input gradient
    sv = disc.fwd(xf, eps=eps[1], want_kl=False)
    s, dd = ops.vdb_loss(sv.d, ops.VDB_NEG_CHI if support else ops.VDB_BCE1, 1.0 / xf.shape[0])
    got = float(s) / xf.shape[0]
    assert abs(got - ref["gen"]) <= FTOL * abs(ref["gen"]), (got, ref["gen"])
    before = disc.optimizer.grad.clone()
    dx = disc.input_grad(sv, dd)
    e = l2err(dx, ref["dx"])
    log(f"[vdb fwd {CASES[ci]} support={support}] dx: l2err {e:.2e}")
    assert e < GTOL, e
    assert torch.equal(disc.optimizer.grad, before)   # a frozen pass writes no parameter gradient
    if not support:
        assert abs(float(disc._bce_with_logits(sv.d, 1)) - ref["gen"]) <= FTOL * abs(ref["gen"])


def pen_tol(ci, support):
    return max(GTOL, 4.0 * PEN_F32[(ci, support)])


@pytest.mark.parametrize("ci,support", PARAMS)
def test_losses_and_gradients_match_the_restatement(ci, support):
    ref = reference(ci, support)
    assert ref["min_pre"] >= cr.PRE_MARGIN, ref["min_pre"]
    disc, names = make_disc(ci)
    xr, xf, eps, tau = dev_case(ci, support)
    Nr, Nf = xr.shape[0], xf.shape[0]
    # without the penalty: the first-order gradients
    buf, svr, svf = disc.loss_and_grad(xr, xf, tau, eps=eps, penalty=False)
    g_main = [g.clone() for g in disc._pg()[1]]
    real, fake = float(buf[0]) / Nr, float(buf[1]) / Nf
    kl = 0.5 * (float(svr.kl) / Nr + float(svf.kl) / Nf)
    for name, got in (("real", real), ("fake", fake), ("kl", kl)):
        r = abs(got - ref[name]) / abs(ref[name])
        log(f"[vdb {CASES[ci]} support={support}] {name}: got {got:.7g} ref {ref[name]:.7g} rel {r:.2e}")
        assert r < FTOL, (name, got, ref[name])
    for k, g in zip(names, g_main):
        e = l2err(g, ref["g_main"][k])
        log(f"[vdb {CASES[ci]} support={support}] d/d {k}: l2err {e:.2e}")
        assert e < GTOL, (k, e)
    # the penalty alone: its value, and its own parameter gradient through a reverse pass that carries nothing else
    disc.optimizer.zero_grad()
    sq, extra = disc._grad_penalty(svr)
    disc.bwd(svr, torch.zeros(Nr, device="cuda"), extra=extra)
    gp = float(sq) * disc.gp_weight / Nr
    r = abs(gp - ref["gp"]) / abs(ref["gp"])
    log(f"[vdb {CASES[ci]} support={support}] gp: got {gp:.7g} ref {ref['gp']:.7g} rel {r:.2e}")
    assert r < FTOL, (gp, ref["gp"])
    tol = pen_tol(ci, support)
    for k, g in zip(names, disc._pg()[1]):
        if k == "fc.bias":
            assert float(g.abs().max()) == 0.0   # the penalty has no gradient into fc.bias
            continue
        e = l2err(g, ref["g_pen"][k])
        log(f"[vdb {CASES[ci]} support={support}] penalty d/d {k}: l2err {e:.2e} (bound {tol:.1e})")
        assert e < tol, (k, e, tol)


@pytest.mark.parametrize("ci,support", PARAMS)
def test_train_steps_parameters_and_beta_and_repeats_bit_for_bit(ci, support):
    ref = reference(ci, support)
    assert ref["min_pre"] >= cr.PRE_MARGIN, ref["min_pre"]
    xr, xf, eps, tau = dev_case(ci, support)
    runs = []
    for _ in range(2):
        disc, names = make_disc(ci)
        (info, kernels) = traced(lambda: disc.train(xr, xf, tau, eps=eps))
        runs.append((disc.optimizer.flat.clone(), disc.optimizer.grad.clone(), info.buf.clone(), disc.beta.clone()))
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(a, b)   # fixed summation order, no float atomics
    for pat in ("vdb_head_fwd_kernel", "vdb_loss_kernel", "vdb_colsum_kernel<false>", "vdb_colsum_kernel<true>",
                "vdb_colsum_finish_kernel", "vdb_gp_delta_kernel", "vdb_gp_norm_kernel", "vdb_beta_step_kernel", "clip_adam"):
        assert has(kernels, pat), (pat, kernels)
    for k in ("real_loss", "fake_loss", "kl", "gp", "beta"):
        want = ref[{"real_loss": "real", "fake_loss": "fake"}.get(k, k)]
        assert abs(info[k] - want) <= FTOL * abs(want), (k, info[k], want)
    assert abs(float(disc.beta) - ref["beta"]) <= FTOL * ref["beta"]
    assert disc.optimizer.step_count == 1
    for k, p in zip(names, disc.plist()):
        g = ref["g_main"][k] + ref["g_pen"][k]
        want, p0 = ref["stepped"][k], torch.from_numpy(cr.make_disc_params(*CASES[ci][2:])[k]).double()
        got = p.detach().double().cpu()
        sure = g.abs() >= 1e-2 * g.abs().max()
        assert float(((got - want).abs() * sure).max()) <= 1e-2 * LR, k          # the step is the restatement's
        assert float((got - p0).abs().max()) <= LR * (1 + 1e-3), k                # and nowhere larger than lr


def test_in_kernel_noise_runs_and_advances_the_stream():
    disc, _ = make_disc(2)
    xr, xf, _, _ = dev_case(2, False)
    info = disc.train(xr, xf)
    assert disc._noise_counter == (xr.shape[0] + xf.shape[0]) * disc.latent_dim
    assert all(np.isfinite(info[k]) for k in info.keys())
    from repo_amd import ops

    # the Philox form of a forward equals the explicit form on the materialised normals
    n = xf.shape[0] * disc.latent_dim
    d1, _, _ = disc(xf, noise=(5, 64))
    d2, _, _ = disc(xf, eps=ops.philox_normal(n, 5, 64, "cuda").view(xf.shape[0], -1))
    assert torch.equal(d1, d2)


# ----------------------------------------------------------------------------- the agent
# Bounds of the golden comparison: those of tests/test_inv_dyn_gpu.py for its goldens -- scalars 1e-3 relative, gradient
# norms 2e-3, checksums 1e-3 |a| + 1e-6.
class PairedEnv:
    """A calibration environment stand-in: 6-channel paired frames (source view | target view), seeded, an episode of
    `horizon` steps."""

    def __init__(self, A, horizon=7, seed=0):
        from tests import test_update_gpu as tu

        self.observation_space = tu.Space((6, 64, 64))
        self.action_space = tu.Space((A,))
        self.action_space.sample = lambda: self.rs.uniform(-1, 1, A).astype(np.float32)
        self.rs, self.horizon, self.t = np.random.RandomState(seed), horizon, 0
        self.frames, self.actions, self.dones = [], [], []

    def _frame(self):
        f = self.rs.randint(0, 256, (6, 64, 64)).astype(np.uint8)
        self.frames.append(f)
        return f

    def reset(self):
        self.t = 0
        return self._frame()

    def step(self, action):
        self.t += 1
        done = self.t == self.horizon
        self.actions.append(np.asarray(action).copy())
        self.dones.append(done)
        return self._frame(), float(self.t), done, {}


def make_calib_agent(mode, L=8, B=4, H=5, A=6, **over):
    from oracle import fixtures as fx
    from repo_amd.algorithms.repo import CalibratedRePo
    from repo_amd.common.utils import set_gpu_mode
    from tests import test_update_gpu as tu

    set_gpu_mode(True)
    cfg = fx.default_config(algo="repo_calibrate", batch_size=B, chunk_size=L, horizon=H, alignment_mode=mode,
                            **{**cr.CALIB_CFG, **over})
    agent = CalibratedRePo(cfg, tu.Env(A), tu.Env(A), PairedEnv(A), tu.Logger())
    params = fx.make_params(A, 7)
    for mod in fx.MODULES:
        agent._load_module(getattr(agent, mod), {k: torch.from_numpy(v) for k, v in params[mod].items()})
    agent._load_module(agent.src_encoder, {k: torch.from_numpy(v) for k, v in params["encoder"].items()})
    agent._load_module(agent.encoder, {k: torch.from_numpy(v) for k, v in fx.make_params(A, 9)["encoder"].items()})
    for mod, p in ((agent.disc, cr.make_disc_params(cfg.embedding_size, cfg.f_hidden_size, cfg.f_latent_size)),
                   (agent.log_tau, cr.make_tau_params(cfg.embedding_size, cfg.f_hidden_size))):
        assert list(mod.state_dict().keys()) == list(p.keys())
        agent._load_module(mod, {k: torch.from_numpy(v) for k, v in p.items()})
    return agent, cfg


def calib_step(agent, cfg, u, inject=True):
    L, B = cfg.chunk_size, cfg.batch_size
    frames, noise = cr.make_calib_inputs(L, B, 6, cfg.f_latent_size, u)
    agent.noise_source = {k: torch.from_numpy(v).cuda() for k, v in noise.items()} if inject else None
    f = {k: torch.from_numpy(v).cuda() for k, v in frames.items()}
    agent.calibration_step(f["aln_src"], f["aln_tgt"], f["cal_src"], f["cal_tgt"])
    return agent.last_scalars


@pytest.mark.parametrize("mode", ["js", "support"])
def test_calibration_steps_match_the_reference_goldens(golden_dir, mode):
    import os

    fname = f"calib_{mode}_tiny.npz"
    g = np.load(os.path.join(golden_dir, fname))
    L, B, H, A, n_updates = (int(x) for x in g["meta"])
    agent, cfg = make_calib_agent(mode, L, B, H, A)
    assert not agent._BUILDS_SYMBOLIC
    keys = [str(k) for k in g["scalar_keys"]]
    modules = [str(m) for m in g["grad_norm_modules"]]
    for u in range(n_updates):
        scal = calib_step(agent, cfg, u)
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
    for m in ("encoder", "disc", "log_tau", "src_encoder"):
        for k, v in getattr(agent, m).state_dict().items():
            have[f"{m}.{k}"] = (float(v.double().sum()), float(v.double().abs().sum()))
    names = [str(n) for n in g["param_names"]]
    assert sorted(names) == sorted(have)
    for n, s_, a_ in zip(names, g["param_sums"], g["param_abssums"]):
        assert abs(have[n][1] - a_) <= 1e-3 * abs(a_) + 1e-6, (n, have[n][1], a_)
        assert abs(have[n][0] - s_) <= 1e-3 * abs(a_) + 1e-6, (n, have[n][0], s_)


@pytest.mark.parametrize("mode", ["js", "support"])
def test_a_step_with_in_kernel_noise_gives_finite_scalars(mode):
    agent, cfg = make_calib_agent(mode)
    before = agent._noise_counter
    scal = calib_step(agent, cfg, 0, inject=False)
    assert scal and all(np.isfinite(v) for v in scal.values()), scal
    n = cfg.chunk_size * cfg.batch_size * cfg.f_latent_size
    assert agent._noise_counter - before == (4 if mode == "support" else 3) * n <= agent._noise_stride()


def _fill_rings(agent, n=40, seed=5):
    rs = np.random.RandomState(seed)
    for i in range(n):
        a, r, d = rs.uniform(-1, 1, 6).astype(np.float32), float(rs.randn()), float(i % 13 == 12)
        agent.src_buffer.push(rs.randint(0, 256, (3, 64, 64)).astype(np.uint8), a, r, d)
        agent.buffer.push(rs.randint(0, 256, (3, 64, 64)).astype(np.uint8), a, r, d)
        agent.calib_buffer.push(rs.randint(0, 256, (6, 64, 64)).astype(np.uint8), a, r, d)


def test_train_agent_moves_the_target_encoder_and_nothing_else_of_the_source_agent():
    from oracle import fixtures as fx

    agent, cfg = make_calib_agent("support", train_steps=2)
    _fill_rings(agent)
    frozen = [m for m in fx.MODULES if m != "encoder"] + ["src_encoder", "inv_dynamics"]
    before = {m: {k: v.clone() for k, v in getattr(agent, m).state_dict().items()} for m in frozen + ["encoder"]}
    log_beta = agent.log_beta.clone()
    np.random.seed(3)
    agent.train_agent()
    torch.cuda.synchronize()
    for m in frozen:
        for k, v in getattr(agent, m).state_dict().items():
            assert torch.equal(v, before[m][k]), (m, k)
    assert torch.equal(agent.log_beta, log_beta)
    assert any(not torch.equal(v, before["encoder"][k]) for k, v in agent.encoder.state_dict().items())
    assert agent.encoder_optimizer.step_count == agent.disc.optimizer.step_count == agent.tau_optimizer.step_count == 2
    assert agent.u_optimizer.step_count == 2 and agent.model_optimizer.step_count == 0
    assert all(np.isfinite(v) for v in agent.last_scalars.values())
    assert set(agent.get_param_dict().keys()) == set(make_calib_agent("js")[0].get_param_dict().keys())
    assert not any(k.startswith(("disc", "log_tau", "src_encoder")) for k in agent.get_param_dict())


@pytest.mark.parametrize("expert", [False, True])
def test_collect_calibration_data_fills_both_rings_with_the_reference_split(expert):
    n = 12
    agent, cfg = make_calib_agent("js", calibration_buffer_size=n, calib_time_limit=5)
    env = agent.calib_env
    agent.collect_calibration_data(expert=expert)
    # every frame the environment produced, in order, minus the ones a reset replaced: rebuild the pushed sequence
    pushed, k = [], 0
    frames, dones, t_limit = env.frames, [], 0
    for i in range(n):
        pushed.append(frames[k])
        done = env.dones[i]
        if expert:
            t_limit += 1
            if t_limit == cfg.calib_time_limit:
                done, t_limit = True, 0
        dones.append(float(done))
        k += 2 if done else 1   # a finished episode's last frame is dropped for the reset's
    pushed = np.stack(pushed)
    assert agent.calib_buffer.pos == n % agent.calib_buffer.capacity and len(agent.buffer) == n
    assert np.array_equal(agent.calib_buffer.observations[:n], pushed)
    assert np.array_equal(agent.buffer.observations[:n], pushed[:, 3:])
    assert np.array_equal(agent.calib_buffer.actions[:n], np.stack(env.actions[:n]))
    assert np.array_equal(agent.buffer.actions[:n], agent.calib_buffer.actions[:n])
    assert agent.calib_buffer.dones[:n, 0].tolist() == dones == agent.buffer.dones[:n, 0].tolist()
    assert sum(dones) >= (2 if expert else 1)
    if not expert:
        np.random.seed(1)
        src, tgt = agent.calib_buffer.sample(2, 4)[:2]
        assert src.shape == tgt.shape == (4, 2, 3, 64, 64)
        dev = agent.calib_buffer.sample_to_device(2, 4, agent.device)
        assert dev[0].shape == dev[1].shape == (4, 2, 3, 64, 64) and dev[0].is_contiguous() and dev[1].is_contiguous()
