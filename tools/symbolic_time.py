"""What the state-vector path (config.pixel_obs = False) costs, and whether its fused output head pays.
usage: python tools/symbolic_time.py            both measurements
       python tools/symbolic_time.py head       repo_linear_unit_nll at rows = 2450, K = 1024, O in {17, 24, 67}: the fused
                                                kernel against the two-launch form (ops.gemm + ops.scalar_nll) and against
                                                the entry point's own composition, alternating, 3 rounds of 200 calls each
                                                between device events after 20 warm-up calls
       python tools/symbolic_time.py update     one RePo and one Dreamer update on 24-float observations at B = 50,
                                                L = 50, H = 15, A = 6: 10 warm-up + 40 timed pipelined updates on a device
                                                batch, host clock around a device synchronise"""
import os, sys, time
HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)


def _timed(fn, n=200, warm=20):
    import torch
    for _ in range(warm):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3   # us per call


def head():
    import torch
    from repo_amd import ops
    from repo_amd._lib import lib
    rows, K = 2450, 1024
    g = torch.Generator(device="cuda").manual_seed(0)
    for O in (17, 24, 67):
        h = torch.randn(rows, K, device="cuda", generator=g)
        w = torch.randn(O, K, device="cuda", generator=g) / K ** 0.5
        b = torch.randn(O, device="cuda", generator=g)
        t = torch.randn(rows, O, device="cuda", generator=g)
        dpre = torch.empty(rows, O, device="cuda")
        pred = torch.empty(rows, O, device="cuda")

        def entry(mode):
            def run():
                prev = lib().repo_debug_linear_nll(mode)
                ops.linear_unit_nll(h, w, b, t, 1.0 / rows, dpre=dpre)
                lib().repo_debug_linear_nll(prev)
            return run

        def two_launch():
            ops.gemm(h, w, transb=True, bias=b, out=pred)
            ops.scalar_nll(pred.view(-1), t.view(-1), None, 1.0 / rows)

        forms = (("fused", entry(1)), ("gemm + scalar_nll", two_launch), ("composition", entry(2)), ("dispatch", entry(0)))
        res = {name: [] for name, _ in forms}
        for _ in range(3):
            for name, fn in forms:
                res[name].append(_timed(fn))
        fused = lib().repo_linear_unit_nll_fused(rows, O, K, h.data_ptr(), K, w.data_ptr(), K)
        print(f"linear_unit_nll rows={rows} K={K} O={O} (dispatch takes the {'fused kernel' if fused else 'composition'}): "
              + "; ".join(f"{name} {' / '.join(f'{v:.1f}' for v in vs)} us" for name, vs in res.items()), flush=True)


def update():
    import numpy as np
    import torch
    import bench
    from repo_amd.algorithms.repo import Dreamer, RePo

    class Space:
        def __init__(self, shape):
            self.shape = shape

    class Env:
        observation_space = Space((24,))
        action_space = Space((6,))

    for Algo in (RePo, Dreamer):
        cfg = bench.config("repo" if Algo is RePo else "dreamer")
        cfg.pixel_obs = False
        agent = Algo(cfg, Env(), Env(), bench.NullLogger())
        L, B = cfg.chunk_size, cfg.batch_size
        rs = np.random.RandomState(0)
        batch = tuple(torch.from_numpy(x).cuda() for x in (
            rs.standard_normal((L, B, 24)).astype(np.float32), rs.uniform(-1, 1, (L, B, 6)).astype(np.float32),
            rs.uniform(0, 1, (L, B, 1)).astype(np.float32), (rs.uniform(size=(L, B, 1)) < 0.002).astype(np.float32)))
        for _ in range(10):
            agent.update(batch, join=False)
        agent.synchronize(); torch.cuda.synchronize()
        times = []
        for _ in range(3):
            t0 = time.perf_counter()
            for _ in range(40):
                agent.update(batch, join=False)
            agent.synchronize(); torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) / 40 * 1e3)
        s = agent.last_scalars
        print(f"{Algo.__name__} pixel_obs=False obs=24 B={B} L={L} H={cfg.horizon}: "
              f"{' / '.join(f'{t:.3f}' for t in times)} ms per update (3 windows of 40), obs_loss {s['train/obs_loss']:.4f}",
              flush=True)


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "both"
    if what in ("head", "both"):
        head()
    if what in ("update", "both"):
        update()
