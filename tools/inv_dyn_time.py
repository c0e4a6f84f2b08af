"""What config.inv_dynamics costs: one RePo update at the bench shapes (B=50, L=50, H=15, A=6, inv_dynamics_hidden_size
512) with the switch off and on -- the train_agent() loop tools/dense_act_time.py times (replay ring mirrored in HBM, a
fresh batch every step, pipelined updates), 10 warm-up + 40 timed updates.  Each measurement runs in a fresh child process,
alternating off, on, off, on.
usage: python tools/inv_dyn_time.py                  off / on, alternating, then the auxiliary's kernels
       python tools/inv_dyn_time.py --against DIR    the switch OFF in this tree against the checkout at DIR (built there:
                                                     python -m repo_amd.build), alternating this, DIR, this, DIR, ...
       python tools/inv_dyn_time.py off|on|kernels [ROOT]   one measurement in this process, on the package under ROOT"""
import os, subprocess, sys, time
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 and sys.argv[1] in ("off", "on", "kernels") else HERE
sys.path.insert(0, ROOT)


def make_agent(on):
    import numpy as np
    import bench
    from repo_amd.algorithms.repo.repo import RePo
    cfg = bench.config("repo")
    cfg.inv_dynamics = on
    cfg.inv_dynamics_lr, cfg.inv_dynamics_hidden_size = 3e-4, 512
    agent = RePo(cfg, bench.Env(), bench.Env(), bench.NullLogger())
    buf = type(agent.buffer)(20000, (3, 64, 64), (6,), obs_type=np.uint8)
    rs = np.random.RandomState(0)
    buf.observations[:] = rs.randint(0, 256, size=buf.observations.shape, dtype=np.uint8)
    buf.actions[:] = rs.uniform(-1, 1, buf.actions.shape)
    buf.rewards[:] = rs.uniform(0, 1, buf.rewards.shape)
    buf.dones[:] = rs.uniform(size=buf.dones.shape) < 0.002   # episodes of ~500 steps: the mask drops a few rows
    buf.pos, buf.full = 0, True
    buf.enable_device_mirror(agent.device)
    buf.invalidate_mirror()
    agent.buffer = buf
    return agent, cfg


def measure(on):
    import torch
    agent, cfg = make_agent(on)
    cfg.train_steps = 10
    agent.train_agent(); torch.cuda.synchronize()
    cfg.train_steps = 40
    t0 = time.perf_counter()
    agent.train_agent(); torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    extra = f" inv_dyn_loss {agent.last_scalars['train/inv_dyn_loss']:.4f}" if on else ""
    print(f"[{os.path.basename(ROOT)}] inv_dynamics={on}: {dt/40*1e3:.3f} ms per update ({40/dt:.1f} updates/s) incl. "
          f"sampling + H2D{extra}", flush=True)


def kernels():
    """Device time of every kernel of ONE train_inv_dynamics call on an idle device (mean of 20 calls)."""
    import torch
    from torch.profiler import ProfilerActivity, profile
    agent, cfg = make_agent(True)
    cfg.train_steps = 3
    agent.train_agent(); torch.cuda.synchronize()
    L, B, D, S = cfg.chunk_size, cfg.batch_size, cfg.belief_size, cfg.state_size
    g = torch.Generator(device="cuda").manual_seed(0)
    featx = torch.randn(L - 1, B, D + S, device="cuda", generator=g)
    actions = torch.rand(L, B, 6, device="cuda", generator=g) * 2 - 1
    nonterms = (torch.rand(L, B, 1, device="cuda", generator=g) > 0.002).float()
    agent._take_status()
    call = lambda: agent.train_inv_dynamics(featx[:, :, :D], featx[:, :, D:], actions, nonterms)  # noqa: E731
    for _ in range(5):
        call()
    torch.cuda.synchronize()
    n = 20
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(n):
            call()
        torch.cuda.synchronize()
    rows = {}
    for e in prof.events():
        if e.device_time_total > 0 and "Memcpy" not in e.name and "Memset" not in e.name:
            c = rows.setdefault(e.name, [0, 0.0])
            c[0] += 1
            c[1] += e.device_time_total
    total = sum(t for _, t in rows.values())
    print(f"train_inv_dynamics: {total / n:.1f} us of kernel time per call, {sum(c for c, _ in rows.values()) // n} launches")
    for name, (c, t) in sorted(rows.items(), key=lambda kv: -kv[1][1]):
        print(f"  {t / n:8.1f} us  x{c // n:<3d} {name[:150]}")


if __name__ == "__main__":
    me = os.path.abspath(__file__)
    if len(sys.argv) > 1 and sys.argv[1] in ("off", "on"):
        measure(sys.argv[1] == "on")
    elif len(sys.argv) > 1 and sys.argv[1] == "kernels":
        kernels()
    elif len(sys.argv) > 2 and sys.argv[1] == "--against":
        other = os.path.abspath(sys.argv[2])
        for root in (HERE, other) * 3:
            subprocess.run([sys.executable, me, "off", root], cwd=root, check=True, timeout=240)
    else:
        for mode in ("off", "on", "off", "on"):
            subprocess.run([sys.executable, me, mode], cwd=HERE, check=True, timeout=240)
        subprocess.run([sys.executable, me, "kernels"], cwd=HERE, check=True, timeout=240)
