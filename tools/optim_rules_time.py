"""What config.grad_clip = "agc" and config.optimizer = "laprop" cost: one RePo update at the bench shapes (B=50, L=50, H=15,
A=6) with the keys off and with each of the three switched-on combinations -- the train_agent() loop tools/twohot_time.py
times (replay ring mirrored in HBM, a fresh batch every step, pipelined updates), 10 warm-up + 40 timed updates.  Each
measurement runs in a fresh child process under a time limit, alternating off / on per combination, with a closing off line
(the off lines give the run's own spread); the first child that fails ends the run.  The lines are printed and written to
profiles/optim_rules_time.txt.
usage: python tools/optim_rules_time.py [--out FILE]          the seven measurements
       python tools/optim_rules_time.py GRAD_CLIP OPTIMIZER   one measurement in this process"""
import os, subprocess, sys, time
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
CHILD_TIMEOUT = 240   # seconds: a measurement takes ~15 s, most of it start-up
OFF = ("norm", "adam")
COMBOS = (("agc", "adam"), ("norm", "laprop"), ("agc", "laprop"))


def make_agent(clip, rule):
    """tools/twohot_time.py's agent and synthetic replay ring, with the keys in the config it is built from (absent when off)."""
    import numpy as np
    import bench
    from repo_amd.algorithms.repo.repo import RePo
    cfg = bench.config("repo")
    if (clip, rule) != OFF:
        cfg.grad_clip, cfg.optimizer = clip, rule
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


def measure(clip, rule):
    import torch
    agent, cfg = make_agent(clip, rule)
    opt = agent.model_optimizer
    assert opt.rule == rule and (opt.agc is not None) == (clip == "agc")
    cfg.train_steps = 10
    agent.train_agent(); torch.cuda.synchronize()
    cfg.train_steps = 40
    t0 = time.perf_counter()
    agent.train_agent(); torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    s = agent.last_scalars
    clipped = "".join(f" {k[len('train/agc_clipped_'):]} {v:.0f}" for k, v in s.items() if k.startswith("train/agc_clipped_"))
    print(f"grad_clip={clip} optimizer={rule}: {dt/40*1e3:.3f} ms per update ({40/dt:.1f} updates/s) incl. sampling + H2D; "
          f"model_loss {s['train/model_loss']:.2f} actor_loss {s['train/actor_loss']:.4f}"
          + (f"; clipped tensors:{clipped}" if clipped else ""), flush=True)


if __name__ == "__main__":
    me = os.path.abspath(__file__)
    if len(sys.argv) == 3 and sys.argv[1] != "--out":
        measure(sys.argv[1], sys.argv[2])
        sys.exit(0)
    out = sys.argv[2] if len(sys.argv) > 2 and sys.argv[1] == "--out" else os.path.join(HERE, "profiles", "optim_rules_time.txt")
    lines = []
    for combo in [c for on in COMBOS for c in (OFF, on)] + [OFF]:
        r = subprocess.run([sys.executable, me, *combo], cwd=HERE, timeout=CHILD_TIMEOUT, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True)
        print(r.stdout, end="", flush=True)
        if r.returncode != 0:   # nothing more is started on the device behind a child that failed
            sys.exit(f"optim_rules_time: the `{' '.join(combo)}` measurement exited with {r.returncode}; stopping")
        lines += [ln for ln in r.stdout.splitlines() if ln.startswith("grad_clip=")]
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
