"""Isolated times of the fused head chains at update row counts: per call (HIP events) and the chain kernel alone (device trace).

    python tools/mlp32_heads_time.py <tag>          # one line per call; REPO_HIP_LIB selects the library (A/B: alternate processes)
    python tools/mlp32_heads_time.py <tag> plain    # the calls only, 5 each: the run to put under a counter collection
-> profiles/mlp32_heads_isolated.txt, profiles/mlp32_pmc.txt"""
import os, re, sys
import numpy as np
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import fixtures as fx
from repo_amd import ops
from torch.profiler import ProfilerActivity, profile

tag = sys.argv[1]
plain = len(sys.argv) > 2 and sys.argv[2] == "plain"
dev = torch.device("cuda")
P = fx.make_params(6, 7)
vp = [torch.tensor(v).cuda() for v in P["value_model"].values()]
ap = [torch.tensor(v).cuda() for v in P["actor_model"].values()]
g = torch.Generator(device="cuda").manual_seed(1)
r = lambda *s: torch.randn(*s, device=dev, generator=g)
NI, N = 34300, 2450


def measure(name, fn, pat, iters=20):
    for _ in range(3 if not plain else 5):
        fn()
    torch.cuda.synchronize()
    if plain:
        return
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    call = e0.elapsed_time(e1) * 1e3 / iters
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
    ks = [e for e in prof.events() if re.search(pat, e.name)]
    t = sorted(e.device_time for e in ks)
    kname = ks[0].name[:60] if ks else "?"
    print(f"{tag:7s} {name:52s} call {call:7.1f} us  kernel median {t[len(t)//2]:7.1f} min {t[0]:7.1f} max {t[-1]:7.1f} us  n={len(t)}  {kname}", flush=True)


x = r(NI, 230)
out, hid = ops.mlp_fwd(vp, x)
measure("fwd value head 34300 rows", lambda: ops.mlp_fwd(vp, x), r"\bmlp_fwd_kernel")
dout, dx = r(NI, 1), torch.empty(NI, 230, device=dev)
measure("bwd value head dx only 34300 rows", lambda: ops.mlp_bwd(vp, x, hid, dout, dparams=None, dx=dx), r"\bmlp_bwd_kernel")
gp = [torch.zeros_like(v) for v in vp]
dw = r(NI - N, 1)
measure("bwd value head two upstreams 34300/31850 rows", lambda: ops.mlp_bwd(vp, x, hid, dout, dparams=gp, dx=dx, dout_w=dw), r"\bmlp_bwd_kernel")
xa = r(NI + N, 230)
measure("fwd actor head 36750 rows", lambda: ops.mlp_fwd(ap, xa), r"\bmlp_fwd_kernel")
outa, hida = ops.mlp_fwd(ap, xa)
da = r(NI + N, 12)
gpa = [torch.zeros_like(v) for v in ap]
measure("bwd actor trunk weight side 36750 rows", lambda: ops.mlp_bwd(ap, xa, hida, da, dparams=gpa, dx=None), r"\bmlp_bwd_kernel")
