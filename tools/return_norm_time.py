"""What config.return_norm costs: one RePo update at the bench shapes (B=50, L=50, H=15, A=6) with the key off and on, for
each actor_grad mode -- the train_agent() loop tools/actor_grad_time.py times (replay ring mirrored in HBM, a fresh batch
every step, pipelined updates), 10 warm-up + 40 timed updates.  Each measurement runs in a fresh child process under a time
limit, alternating off and on per mode, with a second dynamics/off line at the end (the two give the run's own spread); the
first child that fails ends the run.  The lines are printed and written to profiles/return_norm_time.txt.
usage: python tools/return_norm_time.py [--out FILE]                      the seven measurements
       python tools/return_norm_time.py dynamics|reinforce|both off|on    one measurement in this process"""
import os, subprocess, sys, time
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
CHILD_TIMEOUT = 240   # seconds: a measurement takes ~15 s, most of it start-up
MODES = ("dynamics", "reinforce", "both")


def make_agent(mode, on):
    """tools/actor_grad_time.py's agent and synthetic replay ring, with the key in the config it is built from."""
    import numpy as np
    import bench
    from repo_amd.algorithms.repo.repo import RePo
    cfg = bench.config("repo")
    cfg.actor_grad = mode
    if on:
        cfg.return_norm = True
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


def measure(mode, on):
    import torch
    agent, cfg = make_agent(mode, on)
    assert agent._return_norm == on
    cfg.train_steps = 10
    agent.train_agent(); torch.cuda.synchronize()
    cfg.train_steps = 40
    t0 = time.perf_counter()
    agent.train_agent(); torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    s = agent.last_scalars
    extra = (f" return_scale {s['train/return_scale']:.4f} lo {s['train/return_lo']:.4f} hi {s['train/return_hi']:.4f}"
             if on else "")
    print(f"actor_grad={mode} return_norm={'on' if on else 'off'}: {dt/40*1e3:.3f} ms per update ({40/dt:.1f} updates/s) "
          f"incl. sampling + H2D; actor_loss {s['train/actor_loss']:.4f}{extra}", flush=True)


if __name__ == "__main__":
    me = os.path.abspath(__file__)
    if len(sys.argv) > 2 and sys.argv[1] in MODES and sys.argv[2] in ("off", "on"):
        measure(sys.argv[1], sys.argv[2] == "on")
        sys.exit(0)
    out = sys.argv[2] if len(sys.argv) > 2 and sys.argv[1] == "--out" else os.path.join(HERE, "profiles", "return_norm_time.txt")
    lines = []
    for mode, key in [(m, k) for m in MODES for k in ("off", "on")] + [("dynamics", "off")]:
        r = subprocess.run([sys.executable, me, mode, key], cwd=HERE, timeout=CHILD_TIMEOUT, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True)
        print(r.stdout, end="", flush=True)
        if r.returncode != 0:   # nothing more is started on the device behind a child that failed
            sys.exit(f"return_norm_time: the `{mode} {key}` measurement exited with {r.returncode}; stopping")
        lines += [ln for ln in r.stdout.splitlines() if ln.startswith("actor_grad=")]
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
