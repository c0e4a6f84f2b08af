"""What config.embedding_size costs: one RePo update at the bench shapes (B=50, L=50, H=15, A=6) with embedding_size 1024
(no fc in the encoder: the path every earlier measurement took) and 256 (the reference's fc 1024 -> 256 behind conv4, a
256-wide posterior embedding product and decoder head) -- the train_agent() loop tools/inv_dyn_time.py times (replay ring
mirrored in HBM, a fresh batch every step, pipelined updates), 10 warm-up + 40 timed updates.  Each measurement runs in a
fresh child process, alternating 1024, 256, 1024, 256, ...
usage: python tools/embed_time.py                  1024 / 256, five alternating pairs, then the summary
       python tools/embed_time.py --against DIR    E = 1024 in this tree against the checkout at DIR (built there:
                                                   python -m repo_amd.build): five alternating pairs DIR, DIR (what that
                                                   tree shows against itself), then five pairs this, DIR; both spreads
       python tools/embed_time.py E [ROOT]         one measurement in this process, on the package under ROOT"""
import os, re, subprocess, sys, time
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = os.path.abspath(sys.argv[2]) if len(sys.argv) > 2 and sys.argv[1].isdigit() else HERE
sys.path.insert(0, ROOT)
PAIRS = 5


def make_agent(E):
    import numpy as np
    import bench
    from repo_amd.algorithms.repo.repo import RePo
    cfg = bench.config("repo")
    cfg.embedding_size = E
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


def measure(E):
    import torch
    agent, cfg = make_agent(E)
    cfg.train_steps = 10
    agent.train_agent(); torch.cuda.synchronize()
    cfg.train_steps = 40
    t0 = time.perf_counter()
    agent.train_agent(); torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(f"[{os.path.basename(ROOT)}] embedding_size={E}: {dt/40*1e3:.3f} ms per update ({40/dt:.1f} updates/s) incl. "
          f"sampling + H2D, model_loss {agent.last_scalars['train/model_loss']:.1f}", flush=True)


def child(E, root):
    out = subprocess.run([sys.executable, os.path.abspath(__file__), str(E), root], cwd=root, check=True, timeout=240,
                         stdout=subprocess.PIPE, text=True).stdout
    sys.stdout.write(out); sys.stdout.flush()
    return float(re.search(r"([0-9.]+) ms per update", out).group(1))


def pairs(label_a, run_a, label_b, run_b):
    """PAIRS alternating pairs a, b -> prints each side's values and, per pair, b - a (the spread of a comparison)."""
    a, b = [], []
    for _ in range(PAIRS):
        a.append(run_a()); b.append(run_b())
    d = [y - x for x, y in zip(a, b)]
    fmt = lambda v: " ".join(f"{x:.3f}" for x in v)  # noqa: E731
    print(f"{label_a}: {fmt(a)}  (min {min(a):.3f} median {sorted(a)[PAIRS // 2]:.3f} max {max(a):.3f}) ms")
    print(f"{label_b}: {fmt(b)}  (min {min(b):.3f} median {sorted(b)[PAIRS // 2]:.3f} max {max(b):.3f}) ms")
    print(f"{label_b} - {label_a}, pair by pair: {' '.join(f'{x:+.3f}' for x in d)}  (from {min(d):+.3f} to {max(d):+.3f}, "
          f"median {sorted(d)[PAIRS // 2]:+.3f}) ms", flush=True)


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1].isdigit():
        measure(int(sys.argv[1]))
    elif len(sys.argv) > 2 and sys.argv[1] == "--against":
        other = os.path.abspath(sys.argv[2])
        pairs("parent (first of a pair)", lambda: child(1024, other), "parent (second of a pair)", lambda: child(1024, other))
        pairs("parent E=1024", lambda: child(1024, other), "this tree E=1024", lambda: child(1024, HERE))
    else:
        pairs("E=1024", lambda: child(1024, HERE), "E=256", lambda: child(256, HERE))
