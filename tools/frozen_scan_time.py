#!/usr/bin/env python3
"""The reverse observe scan for frozen weights (repo_rssm_observe_bwd_frozen: the scan and d embeds only) against the full
one (the same scan + its eight deferred weight-gradient products), on the same saved forward and the upstream the "pair"
calibration step hands it (dfeat only).  T = 49; B = 100 is the step's [cal_tgt | aln_tgt] scan at batch 50 (row scan),
B = 50 a single block (column-split engine).  Alternating full / frozen, PAIRS pairs of 20 calls each: us per call, then
the medians and the spread of each side.
usage: python tools/frozen_scan_time.py [PAIRS]"""
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from oracle import fixtures as fx
from repo_amd import ops

T, A, D, S, E = 49, 6, 200, 30, 1024
PAIRS = int(sys.argv[1]) if len(sys.argv) > 1 else 7
p = [torch.tensor(v).cuda() for v in fx.make_params(A, 7)["transition_model"].values()]
g = torch.Generator(device="cuda").manual_seed(0)


def timeit(fn, iters=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3


for B in (100, 50):
    r = lambda *s: torch.randn(*s, device="cuda", generator=g)  # noqa: E731
    act, non, emb = r(T, B, A), torch.ones(T, B, device="cuda"), r(T, B, E).relu_()
    sv = ops.rssm_observe_fwd(p, r(B, D) * 0.3, r(B, S), act, non, emb, None, None, 0.1, noise=(1, 0))
    dfeat, dembeds = r(T, B, D + S), torch.empty(T, B, E, device="cuda")
    gp = [torch.zeros_like(t) for t in p]
    full = lambda: ops.rssm_observe_bwd(p, sv, gp, dfeat=dfeat, dembeds=dembeds)  # noqa: E731
    frozen = lambda: ops.rssm_observe_bwd(p, sv, None, dfeat=dfeat, dembeds=dembeds)  # noqa: E731
    print(f"# reverse observe scan T={T} B={B} ({'column-split engine' if sv.cs else 'row scan'}), us per call", flush=True)
    a, b = [], []
    for i in range(PAIRS):
        a.append(timeit(full))
        b.append(timeit(frozen))
        print(f"  pair {i}: full {a[-1]:8.1f}   frozen {b[-1]:8.1f}", flush=True)
    print(f"  median full {statistics.median(a):.1f} (min {min(a):.1f}, max {max(a):.1f});  "
          f"median frozen {statistics.median(b):.1f} (min {min(b):.1f}, max {max(b):.1f})", flush=True)
