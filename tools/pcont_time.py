"""What config.pcont costs: one RePo update at the bench shapes (B=50, L=50, H=15, A=6) with the switch off and on -- the
train_agent() loop tools/inv_dyn_time.py times (replay ring mirrored in HBM, a fresh batch every step, pipelined updates),
10 warm-up + 40 timed updates.  Each measurement runs in a fresh child process under a time limit, alternating off, on,
off, on; the first child that fails ends the run.  The lines are printed and written to profiles/pcont_time.txt.
usage: python tools/pcont_time.py [--out FILE]     off / on, alternating
       python tools/pcont_time.py off|on            one measurement in this process"""
import os, subprocess, sys, time
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
CHILD_TIMEOUT = 240   # seconds: a measurement takes ~15 s, most of it start-up


def make_agent(on):
    import numpy as np
    import bench
    from repo_amd.algorithms.repo.repo import RePo
    cfg = bench.config("repo")
    cfg.pcont = on
    agent = RePo(cfg, bench.Env(), bench.Env(), bench.NullLogger())
    buf = type(agent.buffer)(20000, (3, 64, 64), (6,), obs_type=np.uint8)
    rs = np.random.RandomState(0)
    buf.observations[:] = rs.randint(0, 256, size=buf.observations.shape, dtype=np.uint8)
    buf.actions[:] = rs.uniform(-1, 1, buf.actions.shape)
    buf.rewards[:] = rs.uniform(0, 1, buf.rewards.shape)
    buf.dones[:] = rs.uniform(size=buf.dones.shape) < 0.002   # episodes of ~500 steps: a few soft targets of 0 per batch
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
    extra = f" pcont_loss {agent.last_scalars['train/pcont_loss']:.4f}" if on else ""
    print(f"pcont={on}: {dt/40*1e3:.3f} ms per update ({40/dt:.1f} updates/s) incl. sampling + H2D{extra}", flush=True)


if __name__ == "__main__":
    me = os.path.abspath(__file__)
    if len(sys.argv) > 1 and sys.argv[1] in ("off", "on"):
        measure(sys.argv[1] == "on")
        sys.exit(0)
    out = sys.argv[2] if len(sys.argv) > 2 and sys.argv[1] == "--out" else os.path.join(HERE, "profiles", "pcont_time.txt")
    lines = []
    for mode in ("off", "on", "off", "on"):
        r = subprocess.run([sys.executable, me, mode], cwd=HERE, timeout=CHILD_TIMEOUT, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True)
        print(r.stdout, end="", flush=True)
        if r.returncode != 0:   # nothing more is started on the device behind a child that failed
            sys.exit(f"pcont_time: the `{mode}` measurement exited with {r.returncode}; stopping")
        lines += [ln for ln in r.stdout.splitlines() if ln.startswith("pcont=")]
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
