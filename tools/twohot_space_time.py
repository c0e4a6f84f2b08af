"""What the keys of DESIGN.md 6r cost per update, in the manner of tools/wm_losses_time.py: the train_agent() loop (replay
ring mirrored in HBM, a fresh batch every step, pipelined updates), 10 warm-up + 40 timed updates, each measurement in a fresh
child process under a time limit, alternating off / on three times with a closing off line (the off lines give the run's own
spread); the first child that fails ends the run.  The pixel RePo at B = L = 50, H = 15 with value_dist = "twohot":
  reg:    config.value_slow_reg absent against 1.0 (slow_value_update 1, slow_value_fraction 0.02, slow_value_target off: the
          setup that adds the slow copy's forward on the critic's rows);
  space:  config.value_bin_space "symlog" against "symexp".
The lines are printed and written to profiles/twohot_space_time.txt.
usage: python tools/twohot_space_time.py [--out FILE]              the fourteen measurements
       python tools/twohot_space_time.py reg|space off|on           one measurement in this process"""
import os, subprocess, sys, time
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
CHILD_TIMEOUT = 240   # seconds: a measurement takes ~15 s, most of it start-up
WHAT, STATES = ("reg", "space"), ("off", "on")


def make_agent(what, state):
    """tools/wm_losses_time.py's agent and synthetic replay ring, with the key in the config it is built from."""
    import numpy as np
    import bench
    from repo_amd.algorithms.repo.repo import RePo
    cfg = bench.config("repo")
    env = bench.Env()
    cfg.value_dist = "twohot"
    if state == "on" and what == "reg":
        cfg.value_slow_reg, cfg.slow_value_update, cfg.slow_value_fraction = 1.0, 1, 0.02
    if state == "on" and what == "space":
        cfg.value_bin_space = "symexp"
    agent = RePo(cfg, env, env, bench.NullLogger())
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


def measure(what, state):
    import torch
    agent, cfg = make_agent(what, state)
    on = state == "on"
    assert agent._twohot and agent._value_bins == 255
    assert (agent._value_reg > 0.0) == (on and what == "reg") and (agent._value_space == "symexp") == (on and what == "space")
    cfg.train_steps = 10
    agent.train_agent(); torch.cuda.synchronize()
    cfg.train_steps = 40
    t0 = time.perf_counter()
    agent.train_agent(); torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    s = agent.last_scalars
    print(f"{what}={state}: {dt/40*1e3:.3f} ms per update ({40/dt:.1f} updates/s) incl. sampling + H2D; "
          f"value_loss {s['train/value_loss']:.4f} value_reg {s.get('train/value_reg', float('nan')):.4f}", flush=True)


if __name__ == "__main__":
    me = os.path.abspath(__file__)
    if len(sys.argv) > 2 and sys.argv[1] in WHAT and sys.argv[2] in STATES:
        measure(sys.argv[1], sys.argv[2])
        sys.exit(0)
    out = sys.argv[2] if len(sys.argv) > 2 and sys.argv[1] == "--out" else os.path.join(HERE, "profiles", "twohot_space_time.txt")
    lines = []
    for what in WHAT:
        for state in STATES * 3 + ("off",):
            r = subprocess.run([sys.executable, me, what, state], cwd=HERE, timeout=CHILD_TIMEOUT, stdout=subprocess.PIPE,
                               stderr=subprocess.STDOUT, text=True)
            print(r.stdout, end="", flush=True)
            if r.returncode != 0:   # nothing more is started on the device behind a child that failed
                sys.exit(f"twohot_space_time: the `{what} {state}` measurement exited with {r.returncode}; stopping")
            lines += [ln for ln in r.stdout.splitlines() if ln.startswith(f"{what}=")]
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
