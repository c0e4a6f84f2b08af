"""config.slow_value_target on the GPU: repo_clip_adam_target against repo_clip_adam and float64, its skip
word and argument checks, FlatAdam's schedule, whole updates of RePo and Dreamer against tests/slow_value_ref.py's
OracleSlowValue (tied to OracleAgent by tests/test_slow_value_cpu.py), the equal-target sanity check, the combined
configuration, the untouched default path, checkpoints, and the families that refuse.

Bounds.  The kernel's parameters and moments: the bits of repo_clip_adam.  Its target: MIX_BOUND = 2^-22 * max(|p_new|, |t|)
elementwise against float64 formed from the kernel's own p_new -- one rounding in d = p_new - t (at most 2^-24 (|p_new| +
|t|), scaled by fraction <= 1) and one in the fused multiply-add (at most 2^-24 |t_new|, |t_new| <= max): at most
3 * 2^-24 * max.  Updates: tests/test_pcont_gpu.py::test_update_matches_oracle's -- scalars 1e-3, flat gradients 1e-3,
per-tensor gradients 5e-3; the target 1e-6 normwise per tensor."""
import collections
import json
import os
import re

import numpy as np
import pytest
import torch

from oracle import fixtures as fx
from oracle import repo_oracle as ro
from tests import pcont_ref as pr
from tests import slow_value_ref as sv
from tests import test_update_gpu as tu
from tests.util import has, l2err, log, rnd, traced

pytestmark = pytest.mark.gpu

E_BADARG, E_SHAPE = -1, -2   # include/repo_hip.h
F32 = np.float32
BETAS = (float(F32(0.9)), float(F32(0.999)))
LR = 1e-2
TARGET_KERNEL, PLAIN_KERNEL = r"\bclip_adam_target_kernel\b", r"\bclip_adam_kernel\b"


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


def dev(t):
    return t.cuda()


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def mix_check(t_new, t_old, p_new, fraction, tag):
    """The target's elementwise bound (module docstring); -> the worst error as a fraction of its bound."""
    t64, p64 = t_old.double().cpu(), p_new.double().cpu()
    want = sv.slow_mix(t64, p64, float(F32(fraction)))
    err = (t_new.double().cpu() - want).abs()
    bound = 2.0 ** -22 * torch.maximum(p64.abs(), t64.abs())
    worst = float((err / bound.clamp(min=1e-300)).max())
    log(f"{tag}: target max |t - t64| {float(err.max()):.2e}, worst error / bound {worst:.3f}")
    assert bool((err <= bound).all()), (tag, worst)
    return worst


def kernel_inputs(n, seed):
    """NaN-free random contents for every buffer (an overwrite shows), moments of a second step, a gradient that clips."""
    rs = np.random.RandomState(seed)
    p0, t0, g = rnd(rs, n, scale=0.3), rnd(rs, n, scale=0.3), rnd(rs, n, scale=5.0)
    m0, v0 = rnd(rs, n, scale=0.1), rnd(rs, n, scale=0.1).abs()
    return [dev(x) for x in (p0, g, m0, v0, t0)]


# ----------------------------------------------------------------------------- 1. the kernel against repo_clip_adam
@pytest.mark.parametrize("fraction", [1.0, 0.5, 2.0 ** -7])
@pytest.mark.parametrize("n", [1, 257, 524547])
def test_kernel_against_clip_adam(ops, n, fraction):
    """One block, two blocks, and the grid-stride loop (2050 blocks' worth on 2048); step 2 from non-zero moments, clipped."""
    assert min(2048, -(-n // 256)) == {1: 1, 257: 2, 524547: 2048}[n] and -(-524547 // 256) == 2050
    p0, g, m0, v0, t0 = kernel_inputs(n, n)
    max_norm = 1.0
    sq = ops.grad_sqnorm(g)
    assert float(sq) > max_norm ** 2, "the step must clip"
    a = [p0.clone(), m0.clone(), v0.clone()]
    ops.clip_adam(a[0], g, a[1], a[2], sq, max_norm, LR, 2, betas=BETAS)
    b = [p0.clone(), m0.clone(), v0.clone(), t0.clone()]
    _, names = traced(lambda: ops.clip_adam_target(b[0], g, b[1], b[2], sq, max_norm, LR, 2, b[3], fraction, betas=BETAS))
    assert has(names, TARGET_KERNEL) and not has(names, PLAIN_KERNEL), names
    assert not same_bits(a[0], p0)
    for x, y, what in zip(a, b, "pmv"):
        assert same_bits(x, y), (what, n, fraction)
    if fraction == 1.0:
        assert same_bits(b[3], b[0])
    else:
        assert not same_bits(b[3], t0) and not same_bits(b[3], b[0])
        mix_check(b[3], t0, b[0], fraction, f"clip_adam_target n={n} fraction={fraction:g}")


@pytest.mark.parametrize("fraction", [1.0, 0.5])
def test_kernel_without_a_norm_steps_unclipped(ops, fraction):
    n = 257
    p0, g, m0, v0, t0 = kernel_inputs(n, 5)
    sq = ops.grad_sqnorm(g)
    clipped = [p0.clone(), m0.clone(), v0.clone()]
    ops.clip_adam(clipped[0], g, clipped[1], clipped[2], sq, 1.0, LR, 2, betas=BETAS)
    a = [p0.clone(), m0.clone(), v0.clone()]
    ops.clip_adam(a[0], g, a[1], a[2], None, 1.0, LR, 2, betas=BETAS)
    b = [p0.clone(), m0.clone(), v0.clone(), t0.clone()]
    ops.clip_adam_target(b[0], g, b[1], b[2], None, 1.0, LR, 2, b[3], fraction, betas=BETAS)
    assert not same_bits(a[1], clipped[1]), "the unclipped step is another step"
    for x, y, what in zip(a, b, "pmv"):
        assert same_bits(x, y), what
    if fraction == 1.0:
        assert same_bits(b[3], b[0])
    else:
        mix_check(b[3], t0, b[0], fraction, f"clip_adam_target sqnorm=None fraction={fraction:g}")


# ----------------------------------------------------------------------------- 2. the skip word
@pytest.mark.parametrize("fraction", [1.0, 0.5])
def test_skip_word(ops, fraction):
    n = 257
    p0, g, m0, v0, t0 = kernel_inputs(n, 9)
    sq = ops.grad_sqnorm(g)
    runs = []
    for skip in (None, torch.zeros(1, dtype=torch.int32, device="cuda"), torch.full((1,), 4, dtype=torch.int32, device="cuda")):
        bufs = [p0.clone(), m0.clone(), v0.clone(), t0.clone()]
        ops.clip_adam_target(bufs[0], g, bufs[1], bufs[2], sq, 1.0, LR, 3, bufs[3], fraction, betas=BETAS, skip=skip)
        runs.append(bufs)
    none, zero, four = runs
    assert all(not same_bits(x, y) for x, y in zip(none, (p0, m0, v0, t0))), "the step writes all four buffers"
    assert all(same_bits(x, y) for x, y in zip(none, zero)), "skip word 0 is no skip word"
    assert all(same_bits(x, y) for x, y in zip(four, (p0, m0, v0, t0))), "a non-zero skip word: nothing is written"


# ----------------------------------------------------------------------------- 3. argument errors
def test_argument_errors(ops):
    from repo_amd._lib import lib

    n = 8
    p, g, m, v, t = (x.clone() for x in kernel_inputs(n, 1))
    keep = [x.clone() for x in (p, m, v, t)]
    st = torch.cuda.current_stream().cuda_stream
    call = lib().repo_clip_adam_target

    def run(n_, target, fraction):
        return call(n_, p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), None, 1.0, LR, BETAS[0], BETAS[1], 1e-8, 1,
                    None, target, fraction, st)

    assert run(n, None, 0.5) == E_BADARG
    assert run(n, t.data_ptr(), 0.0) == E_BADARG
    assert run(n, t.data_ptr(), 1.5) == E_BADARG
    assert run(n, t.data_ptr(), float("nan")) == E_BADARG
    assert run(0, t.data_ptr(), 0.5) == E_SHAPE
    torch.cuda.synchronize()
    assert all(same_bits(x, y) for x, y in zip((p, m, v, t), keep)), "a refused call launches nothing"
    assert run(n, t.data_ptr(), 1.0) == 0
    torch.cuda.synchronize()
    assert same_bits(t, p) and not same_bits(p, keep[0])


# ----------------------------------------------------------------------------- 4. FlatAdam's schedule
def test_flat_adam_schedule_and_state_dict_phase(ops):
    """n = 257, every = 3, fraction = 0.5, seven steps: the target moves behind steps 3 and 6 only, in the fused kernel; an
    optimiser rebuilt from the state_dict after step 4 mixes at step 6, not at its own third step."""
    from repo_amd.algorithms.repo.models.utils import FlatAdam

    n, every, fraction = 257, 3, 0.5
    rs = np.random.RandomState(4)
    w0 = rnd(rs, n, scale=0.3)

    def build(values):
        opt = FlatAdam([torch.nn.Parameter(values.clone().cuda())], lr=LR)
        return opt

    opt = build(w0)
    assert opt.numel == 260
    target = dev(rnd(rs, opt.numel, scale=0.3))
    opt.track_target(target, every, fraction)
    for step in range(1, 8):
        if step == 5:   # a round trip in between keeps the phase: the step count travels in the Adam state
            sd, values = opt.state_dict(), opt.flat[:n].clone()
            opt = build(values.cpu())
            opt.load_state_dict(sd)
            assert opt.step_count == 4
            opt.track_target(target, every, fraction)
        opt.grad[:n].copy_(dev(rnd(rs, n, scale=5.0 if step % 2 else 0.01)))
        before = target.clone()
        _, names = traced(lambda: opt.clip_and_step(1.0))
        mixed = sv.mixes(step, every)
        assert mixed == (step in (3, 6))
        assert has(names, TARGET_KERNEL) == mixed and has(names, PLAIN_KERNEL) == (not mixed), (step, names)
        if mixed:
            assert not same_bits(target, before)
            mix_check(target, before, opt.flat, fraction, f"FlatAdam step {step}")
        else:
            assert same_bits(target, before), step
    assert opt.step_count == 7
    # step() (no clipping) follows the same schedule
    opt.track_target(target, 2, 1.0)
    opt.grad[:n].copy_(dev(rnd(rs, n)))
    _, names = traced(opt.step)
    assert opt.step_count == 8 and has(names, TARGET_KERNEL) and same_bits(target, opt.flat)


# ----------------------------------------------------------------------------- agents
def counted(fn):
    """tests/util.py's traced() with multiplicity: (fn(), Counter of the device kernels' names).  An update's optimiser steps
    are its LAST launches; a few fill kernels behind them keep them off the tail of the trace, where a record can be lost
    when the profiler stops."""
    from torch.profiler import ProfilerActivity, profile

    pad = torch.zeros(64, device="cuda")
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        out = fn()
        torch.cuda.synchronize()
        for _ in range(8):
            pad.add_(1.0)
        torch.cuda.synchronize()
    names = collections.Counter(e.name for e in prof.events() if "kernel" in e.name.lower() and "hipLaunch" not in e.name)
    assert names, "the device trace lists no HIP kernels"
    return out, names


def n_launches(counts, pattern):
    return sum(c for name, c in counts.items() if re.search(pattern, name))


def torch_sd(params):
    return {k: torch.from_numpy(np.asarray(v)) for k, v in params.items()}


def load_target(agent, slow_params):
    """Through load_param_dict: slow_params None = a checkpoint without the entry (the target becomes the value head)."""
    ck = agent.get_param_dict()
    ck.pop("slow_value_model")
    if slow_params is not None:
        ck["slow_value_model"] = torch_sd(slow_params)
    agent.load_param_dict(ck)


def make_slow_agent(algo, L, B, H, A, every, fraction, slow_params="distinct", **over):
    agent, cfg = tu.make_agent(algo, L, B, H, A, slow_value_target=True, slow_value_update=every,
                               slow_value_fraction=fraction, **over)
    if slow_params == "distinct":
        slow_params = sv.make_slow_params(cfg.belief_size, cfg.state_size, cfg.hidden_size)
    load_target(agent, slow_params)
    return agent, cfg


def target_errors(agent, oracle):
    return [(k, l2err(v, oracle.slow[k])) for k, v in agent.slow_value_model.state_dict().items()]


def check_against_oracle(agent, oracle, oscal, snap, names, tag):
    """The bounds of tests/test_pcont_gpu.py::test_update_matches_oracle on the scalars in `oscal` and the optimisers in `names`."""
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
    errs = target_errors(agent, oracle)
    log(f"{tag} target: worst {max(x for _, x in errs):.2e}")
    for k, x in errs:
        assert x < 1e-6, (tag, k, x)


# ----------------------------------------------------------------------------- 5. whole updates against the oracle
@pytest.mark.parametrize("algo", ["repo", "dreamer"])
def test_update_matches_oracle(algo):
    g = sv.GPU_CASE
    L, B, H, A = g["L"], g["B"], g["H"], g["A"]
    agent, cfg = make_slow_agent(algo, L, B, H, A, g["every"], g["fraction"])
    oracle = sv.OracleSlowValue(cfg, A, params=fx.make_params(A, 7), slow_params=sv.make_slow_params())
    assert (oracle.every, oracle.fraction) == (2, 0.5)
    assert all(e == 0.0 for _, e in target_errors(agent, oracle)), "the target came through load_param_dict"
    for u in range(g["updates"]):
        batch, host = tu.dev_batch(L, B, A, g["batch_seed"] + u, u8=(u == 0))
        agent.noise_source, nz = tu.dev_noise(L, B, H, A, g["noise_seed"] + u)

        def update():
            beliefs, post = agent.train_dynamics(batch[0], batch[1], batch[2], 1.0 - batch[3])
            agent.train_actor_critic(beliefs.flatten(0, 1), post.flatten(0, 1))

        with tu.grad_snapshots(agent) as snap:
            _, counts = counted(update)
        assert n_launches(counts, TARGET_KERNEL) == (1 if u == 1 else 0), (u, counts)
        assert n_launches(counts, PLAIN_KERNEL) >= 1, (u, counts)   # the other optimisers' steps stay the plain kernel
        _, _, oscal = oracle.update(*host, nz)
        check_against_oracle(agent, oracle, oscal, snap, ("model", "actor", "value"), f"[oracle slow value {algo}] update {u}")
        torch.cuda.synchronize()
        with torch.no_grad():   # the oracle takes the agent's ONLINE parameters; its target stays its own
            for m in fx.MODULES:
                for k, v in getattr(agent, m).state_dict().items():
                    oracle.p[m][k].copy_(v.cpu())
            if algo == "repo":
                oracle.log_beta.copy_(agent.log_beta.cpu().reshape(oracle.log_beta.shape))
    assert agent.value_optimizer.step_count == 3


# ----------------------------------------------------------------------------- 6. equal target: the plain agent's numbers
def test_equal_target_is_the_plain_update_to_rounding():
    """every = 1, fraction = 1, target == online head: the target is the online head before every update, so the update is
    the plain one computed through two chains instead of one -- equal to rounding, not in bits."""
    L, B, H, A = 8, 4, 5, 6
    on, _ = make_slow_agent("repo", L, B, H, A, 1, 1.0, slow_params=None)
    plain, _ = tu.make_agent("repo", L, B, H, A)
    assert torch.equal(on._slow_value_flat, on.value_optimizer.flat) and torch.equal(on.value_optimizer.flat, plain.value_optimizer.flat)
    for u in range(2):
        batch, _ = tu.dev_batch(L, B, A, 11 + u)
        noise, _ = tu.dev_noise(L, B, H, A, 101 + u)
        snaps = []
        for agent in (on, plain):
            agent.noise_source = noise
            with tu.grad_snapshots(agent) as snap:
                agent.update(batch)
            snaps.append(snap)
        for k, w in plain.last_scalars.items():
            got = on.last_scalars[k]
            log(f"[equal target] update {u} {k}: on {got:.7g} plain {w:.7g} rel {abs(got - w) / (abs(w) + 1e-12):.2e}")
            assert abs(got - w) <= 1e-5 * abs(w), (u, k, got, w)
        for name in ("model", "actor", "value"):
            e = l2err(snaps[0][name], snaps[1][name])
            log(f"[equal target] update {u} {name} gradient: {e:.2e}")
            assert e < 1e-4, (u, name, e)
        assert torch.equal(on._slow_value_flat, on.value_optimizer.flat), "fraction 1 after every step: a bit copy"


# ----------------------------------------------------------------------------- 7. the combined configuration
def test_slow_value_with_pcont_relu_and_state_vectors():
    """pcont, ReLU heads and state-vector observations, one update with a mixing step.  The oracle restates the actor-critic
    half (tests/slow_value_ref.py: its train_dynamics knows neither ReLU nor state vectors, and the feature does not touch
    that half): it starts from the agent's own latents and post-model-step parameters."""
    from tests import test_symbolic_gpu as ts

    L, B, H, A = 8, 4, 5, 6
    agent, cfg = ts.make_sym_agent("repo", L, B, H, A, pcont=True, dense_activation_function="relu",
                                   slow_value_target=True, slow_value_update=1, slow_value_fraction=0.5)
    head = pr.make_pcont_params(cfg.belief_size, cfg.state_size, cfg.hidden_size)
    agent._load_module(agent.pcont_model, torch_sd(head))
    slow = sv.make_slow_params(cfg.belief_size, cfg.state_size, cfg.hidden_size)
    load_target(agent, slow)
    oracle = sv.OracleSlowValuePcont(cfg, A, params=fx.make_params(A, 7), pcont_params=head, slow_params=slow)
    assert oracle.act == "relu" and (oracle.every, oracle.fraction) == (1, 0.5)
    batch = ts.sym_batch(L, B, A, 11)
    agent.noise_source, nz = tu.dev_noise(L, B, H, A, 101)
    with tu.grad_snapshots(agent) as snap:
        beliefs, post = agent.train_dynamics(batch[0], batch[1], batch[2], 1.0 - batch[3])
        torch.cuda.synchronize()
        with torch.no_grad():
            for m in ("transition_model", "reward_model", "actor_model", "value_model", "pcont_model"):
                for k, v in getattr(agent, m).state_dict().items():
                    oracle.p[m][k].copy_(v.cpu())
        _, counts = counted(lambda: agent.train_actor_critic(beliefs.flatten(0, 1), post.flatten(0, 1)))
    assert n_launches(counts, TARGET_KERNEL) == 1 and has(counts, r"lambda_return_disc_kernel"), counts
    t = {k: torch.as_tensor(v) for k, v in nz.items()}
    oscal = oracle.train_actor_critic(beliefs.flatten(0, 1).cpu(), post.flatten(0, 1).cpu(), t["img_act"], t["img_prior"],
                                      t["entropy"])
    assert all(np.isfinite(v) for v in agent.last_scalars.values()) and not agent.logger.nonfinite
    check_against_oracle(agent, oracle, oscal, snap, ("actor", "value"), "[slow value combined]")


# ----------------------------------------------------------------------------- 8. the default path
def test_default_path_is_untouched():
    L, B, H, A = 8, 4, 5, 6
    torch.manual_seed(3)
    off, _ = tu.make_agent("repo", L, B, H, A, slow_value_target=False)
    plain, cfg = tu.make_agent("repo", L, B, H, A)
    assert not hasattr(cfg, "slow_value_target")
    assert not hasattr(off, "slow_value_model") and not hasattr(plain, "slow_value_model")
    assert off.value_optimizer.target is None
    for agent in (off, plain):
        for u in range(2):
            batch, _ = tu.dev_batch(L, B, A, 11 + u)
            agent.noise_source, _ = tu.dev_noise(L, B, H, A, 101 + u)
            agent.update(batch)
    torch.cuda.synchronize()
    for name in ("model", "actor", "value"):
        a, b = getattr(off, f"{name}_optimizer"), getattr(plain, f"{name}_optimizer")
        assert torch.equal(a.flat, b.flat) and torch.equal(a.exp_avg, b.exp_avg), name
    assert off.last_scalars == plain.last_scalars
    assert list(off.get_param_dict().keys()) == list(plain.get_param_dict().keys())
    batch, _ = tu.dev_batch(L, B, A, 13)
    plain.noise_source, _ = tu.dev_noise(L, B, H, A, 103)
    _, names = traced(lambda: plain.update(batch))
    assert has(names, PLAIN_KERNEL) and not has(names, "clip_adam_target"), names


def test_seeded_construction_draws_nothing_for_the_target():
    """Same seed, key on and off, no parameters loaded: the online parameters and torch's generator end up bit-equal, and
    the target is a bit copy of the online head in the value optimiser's layout."""
    from repo_amd.algorithms.repo import RePo
    from repo_amd.common.utils import set_gpu_mode

    set_gpu_mode(True)
    L, B, H, A = 8, 4, 5, 6
    built = []
    for over in ({}, {"slow_value_target": True}):
        torch.manual_seed(5)
        cfg = fx.default_config(algo="repo", batch_size=B, chunk_size=L, horizon=H, **over)
        agent = RePo(cfg, tu.Env(A), tu.Env(A), tu.Logger())
        built.append((agent, torch.get_rng_state().clone(), agent._noise_counter))
    (plain, rng_a, ctr_a), (on, rng_b, ctr_b) = built
    assert torch.equal(rng_a, rng_b) and ctr_a == ctr_b
    for name in ("model", "actor", "value"):
        assert torch.equal(getattr(plain, f"{name}_optimizer").flat, getattr(on, f"{name}_optimizer").flat), name
    opt = on.value_optimizer
    qs = on.slow_value_model.plist()
    assert [tuple(q.shape) for q in qs] == [tuple(q.shape) for q in opt.params]
    assert type(on.slow_value_model) is type(on.value_model) and on.slow_value_model.act == on.value_model.act
    for q, o in zip(qs, opt.offsets):   # views into ONE float32 buffer at the optimiser's offsets
        assert q.dtype == torch.float32 and q.data_ptr() - qs[0].data_ptr() == 4 * o and not q.requires_grad and q.grad is None
    assert on._slow_value_flat.numel() == opt.numel and qs[0].data_ptr() == on._slow_value_flat.data_ptr()
    assert same_bits(on._slow_value_flat, opt.flat)
    held = {id(q) for o in (on.model_optimizer, on.actor_optimizer, on.value_optimizer) for q in o.params}
    assert not held & {id(q) for q in qs}, "the target is in no optimiser"


# ----------------------------------------------------------------------------- 9. checkpoints
def test_checkpoint_key_and_round_trip(golden_dir):
    L, B, H, A = 8, 4, 5, 6
    a, _ = make_slow_agent("repo", L, B, H, A, 2, 0.5)
    plain, _ = tu.make_agent("repo", L, B, H, A)
    assert "slow_value_model" not in plain.get_param_dict()
    with open(os.path.join(golden_dir, "checkpoint_manifest.json")) as f:
        assert list(plain.get_param_dict().keys()) == json.load(f)["repo"]["top_keys"]   # the default config's key list

    def update(agent, u):
        batch, _ = tu.dev_batch(L, B, A, 11 + u)
        agent.noise_source, _ = tu.dev_noise(L, B, H, A, 101 + u)
        agent.update(batch)

    update(a, 0)
    ck = a.get_param_dict()
    assert list(ck["slow_value_model"].keys()) == sv.HEAD_KEYS == list(ck["value_model"].keys())
    assert set(ck.keys()) == set(plain.get_param_dict().keys()) | {"slow_value_model"}
    b, _ = tu.make_agent("repo", L, B, H, A, seed=8, slow_value_target=True, slow_value_update=2, slow_value_fraction=0.5)
    assert not torch.equal(b.value_optimizer.flat, a.value_optimizer.flat)
    b.load_param_dict(ck)
    assert same_bits(a._slow_value_flat, b._slow_value_flat)
    for name in ("flat", "exp_avg", "exp_avg_sq"):
        assert same_bits(getattr(a.value_optimizer, name), getattr(b.value_optimizer, name)), name
    assert a.value_optimizer.step_count == b.value_optimizer.step_count == 1
    before = a._slow_value_flat.clone()
    for agent in (a, b):   # the next mixing step falls on the same update: the second
        update(agent, 1)
    torch.cuda.synchronize()
    assert not same_bits(a._slow_value_flat, before) and same_bits(a._slow_value_flat, b._slow_value_flat)
    assert same_bits(a.value_optimizer.flat, b.value_optimizer.flat)
    # a checkpoint without the entry: the target becomes a bit copy of the loaded value head
    c, _ = tu.make_agent("repo", L, B, H, A, seed=8, slow_value_target=True)
    c.load_param_dict({k: v for k, v in ck.items() if k != "slow_value_model"})
    for (k, v), w in zip(c.slow_value_model.state_dict().items(), ck["value_model"].values()):
        assert torch.equal(v, w.to(v.device)), k
    assert same_bits(c._slow_value_flat, c.value_optimizer.flat)
    # key off: the entry is ignored
    plain.load_param_dict(ck)
    assert not hasattr(plain, "slow_value_model") and same_bits(plain.value_optimizer.flat, c.value_optimizer.flat)


# ----------------------------------------------------------------------------- 10. refusals
@pytest.mark.parametrize("family", ["FinetunedRePo", "CalibratedRePo", "TIA", "MultitaskDreamer", "MultitaskRePo"])
def test_other_families_refuse(family):
    from tests import test_pcont_gpu as tp

    build = tp._family_builders()[family]
    with pytest.raises(NotImplementedError, match="slow_value_target"):
        build(slow_value_target=True)
    agent = build(slow_value_target=False)
    assert type(agent).__name__ == family and not hasattr(agent, "slow_value_model")


@pytest.mark.parametrize("over", [{"slow_value_update": 0}, {"slow_value_fraction": 0.0}, {"slow_value_fraction": 1.5},
                                  {"slow_value_update": 2.5}])
@pytest.mark.parametrize("algo", ["repo", "dreamer"])
def test_out_of_range_keys_raise(algo, over):
    with pytest.raises(ValueError, match=next(iter(over))):
        tu.make_agent(algo, 8, 4, 5, 6, slow_value_target=True, **over)
