"""Chain kernel time by row count, both engines in one process (REPO_MLP32_MIN_ROWS is read at every call): where the
row thresholds of csrc/mlp32.hip come from.  -> profiles/mlp32_threshold.txt"""
import os, re, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from oracle import fixtures as fx
from repo_amd import ops
from torch.profiler import ProfilerActivity, profile

P = fx.make_params(6, 7)
vp = [torch.tensor(v).cuda() for v in P["value_model"].values()]
ap = [torch.tensor(v).cuda() for v in P["actor_model"].values()]


def ktime(fn, pat, iters=12):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
    t = sorted(e.device_time for e in prof.events() if re.search(pat, e.name))
    return t[len(t) // 2]


print("# rows | value fwd fp32 / bf16x6 | value bwd (dx + saved gradients) fp32 / bf16x6 | actor fwd fp32 / bf16x6   (us, kernel alone, median of 12)")
for rows in (128, 256, 512, 1024, 2048, 4096, 8192, 16384, 34300):
    x = torch.randn(rows, 230, device="cuda")
    res = []
    for prm, O in ((vp, 1), (ap, 12)):
        for eng in (10 ** 9, 0):
            os.environ["REPO_MLP32_MIN_ROWS"] = str(eng)
            out, hid = ops.mlp_fwd(prm, x)
            res.append(ktime(lambda: ops.mlp_fwd(prm, x), r"\bmlp_fwd_kernel"))
            if O == 1:
                dout, dx = torch.randn(rows, 1, device="cuda"), torch.empty(rows, 230, device="cuda")
                gp = [torch.zeros_like(v) for v in prm]
                res.append(ktime(lambda: ops.mlp_bwd(prm, x, hid, dout, dparams=gp, dx=dx), r"\bmlp_bwd_kernel"))
    print(f"{rows:6d} | {res[0]:6.1f} / {res[2]:6.1f} | {res[1]:6.1f} / {res[3]:6.1f} | {res[4]:6.1f} / {res[5]:6.1f}", flush=True)
