"""What config.slow_value_target costs: one RePo update at the bench shapes (B=50, L=50, H=15, A=6) with the switch off and
on -- the train_agent() loop tools/pcont_time.py times (replay ring mirrored in HBM, a fresh batch every step, pipelined
updates), 10 warm-up + 40 timed updates.  The switched-on agent mixes every 5 value steps (fraction 0.5) so that the timed
updates hold eight fused steps, and its target starts as the online head.  Each measurement runs in a fresh child process
under a time limit, alternating off, on, off, on; the first child that fails ends the run.  The lines are printed and written
to profiles/slow_value_time.txt, with the off/off spread of the run beside the off/on difference.
usage: python tools/slow_value_time.py [--out FILE]     off / on, alternating
       python tools/slow_value_time.py off|on            one measurement in this process"""
import os, re, subprocess, sys, time
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
CHILD_TIMEOUT = 240   # seconds: a measurement takes ~15 s, most of it start-up


def make_agent(on):
    import numpy as np
    import bench
    from repo_amd.algorithms.repo.repo import RePo
    cfg = bench.config("repo")
    cfg.slow_value_target = on
    cfg.slow_value_update, cfg.slow_value_fraction = 5, 0.5
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


def measure(on):
    import torch
    agent, cfg = make_agent(on)
    cfg.train_steps = 10
    agent.train_agent(); torch.cuda.synchronize()
    cfg.train_steps = 40
    t0 = time.perf_counter()
    agent.train_agent(); torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    extra = f" value_loss {agent.last_scalars['train/value_loss']:.4f} value steps {agent.value_optimizer.step_count}"
    print(f"slow_value_target={on}: {dt/40*1e3:.3f} ms per update ({40/dt:.1f} updates/s) incl. sampling + H2D{extra}",
          flush=True)


if __name__ == "__main__":
    me = os.path.abspath(__file__)
    if len(sys.argv) > 1 and sys.argv[1] in ("off", "on"):
        measure(sys.argv[1] == "on")
        sys.exit(0)
    out = sys.argv[2] if len(sys.argv) > 2 and sys.argv[1] == "--out" else os.path.join(HERE, "profiles", "slow_value_time.txt")
    lines, ms = [], {"off": [], "on": []}
    for mode in ("off", "on", "off", "on"):
        r = subprocess.run([sys.executable, me, mode], cwd=HERE, timeout=CHILD_TIMEOUT, stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, text=True)
        print(r.stdout, end="", flush=True)
        if r.returncode != 0:   # nothing more is started on the device behind a child that failed
            sys.exit(f"slow_value_time: the `{mode}` measurement exited with {r.returncode}; stopping")
        got = [ln for ln in r.stdout.splitlines() if ln.startswith("slow_value_target=")]
        lines += got
        ms[mode] += [float(re.search(r": ([0-9.]+) ms", ln).group(1)) for ln in got]
    if len(ms["off"]) == 2 and len(ms["on"]) == 2:
        off, on = sum(ms["off"]) / 2, sum(ms["on"]) / 2
        lines.append(f"off/off spread {abs(ms['off'][0] - ms['off'][1]):.3f} ms; on/on spread {abs(ms['on'][0] - ms['on'][1]):.3f} ms; "
                     f"mean on - mean off {on - off:+.3f} ms ({(on / off - 1) * 100:+.1f} %)")
        print(lines[-1], flush=True)
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
