"""What config.value_dist = "twohot" costs: one RePo update at the bench shapes (B=50, L=50, H=15, A=6) with the scalar head
("normal") and the two-hot head (value_bins 255) -- the train_agent() loop tools/return_norm_time.py times (replay ring
mirrored in HBM, a fresh batch every step, pipelined updates), 10 warm-up + 40 timed updates.  Each measurement runs in a
fresh child process under a time limit, alternating normal / twohot three times, with a closing normal line (the normal
lines give the run's own spread); the first child that fails ends the run.  The lines are printed and written to
profiles/twohot_time.txt.
usage: python tools/twohot_time.py [--out FILE]        the seven measurements
       python tools/twohot_time.py normal|twohot       one measurement in this process"""
import os, subprocess, sys, time
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
CHILD_TIMEOUT = 240   # seconds: a measurement takes ~15 s, most of it start-up
DISTS = ("normal", "twohot")


def make_agent(dist):
    """tools/return_norm_time.py's agent and synthetic replay ring, with the key in the config it is built from."""
    import numpy as np
    import bench
    from repo_amd.algorithms.repo.repo import RePo
    cfg = bench.config("repo")
    cfg.value_dist = dist
    agent = RePo(cfg, bench.Env(), bench.Env(), bench.NullLogger())
    buf = type(agent.buffer)(20000, (3, 64, 64), (6,), obs_type=np.uint8)
    rs = np.random.RandomState(0)
    buf.observations[:] = rs.randint(0, 256, size=buf.observations.shape, dtype=np.uint8)
    buf.actions[:] = rs.uniform(-1, 1, buf.actions.shape)
    buf.rewards[:] = rs.uniform(0, 1, buf.rewards.shape)
    buf.dones[:] = rs.uniform(size=buf.dones.shape) < 0.002
    buf.pos, buf.full = 0, True
    buf.enable_device_mirror(agent.device)
    buf.invalidate_mirror()
    agent.buffer = buf
    return agent, cfg


def measure(dist):
    import torch
    agent, cfg = make_agent(dist)
    assert agent._value_dist == dist and (dist == "normal" or agent._value_bins == 255)
    cfg.train_steps = 10
    agent.train_agent(); torch.cuda.synchronize()
    cfg.train_steps = 40
    t0 = time.perf_counter()
    agent.train_agent(); torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    s = agent.last_scalars
    print(f"value_dist={dist}: {dt/40*1e3:.3f} ms per update ({40/dt:.1f} updates/s) incl. sampling + H2D; "
          f"actor_loss {s['train/actor_loss']:.4f} value_loss {s['train/value_loss']:.4f}", flush=True)


if __name__ == "__main__":
    me = os.path.abspath(__file__)
    if len(sys.argv) > 1 and sys.argv[1] in DISTS:
        measure(sys.argv[1])
        sys.exit(0)
    out = sys.argv[2] if len(sys.argv) > 2 and sys.argv[1] == "--out" else os.path.join(HERE, "profiles", "twohot_time.txt")
    lines = []
    for dist in DISTS * 3 + ("normal",):
        r = subprocess.run([sys.executable, me, dist], cwd=HERE, timeout=CHILD_TIMEOUT, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True)
        print(r.stdout, end="", flush=True)
        if r.returncode != 0:   # nothing more is started on the device behind a child that failed
            sys.exit(f"twohot_time: the `{dist}` measurement exited with {r.returncode}; stopping")
        lines += [ln for ln in r.stdout.splitlines() if ln.startswith("value_dist=")]
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
