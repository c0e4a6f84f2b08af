import os
import re

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG = os.path.join(ROOT, "gpurun_out", "parity_log.txt")


def log(msg):
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    with open(LOG, "a") as f:
        f.write(msg + "\n")
    print(msg)


def relerr(got, want):
    """max |got-want| / max|want| (normwise, robust to near-zero entries)."""
    got = got.detach().double().cpu()
    want = want.detach().double().cpu()
    scale = want.abs().max().item() + 1e-30
    return (got - want).abs().max().item() / scale


def l2err(got, want):
    got = got.detach().double().cpu().flatten()
    want = want.detach().double().cpu().flatten()
    return ((got - want).norm() / (want.norm() + 1e-30)).item()


def rnd(rs, *shape, scale=1.0):
    return torch.from_numpy((rs.standard_normal(shape) * scale).astype(np.float32))


def traced(fn):
    """(fn(), names of the device kernels it launched).  Every traced call launches HIP kernels: a trace that lists none
    cannot confirm an engine, and fails the case."""
    from torch.profiler import ProfilerActivity, profile

    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        out = fn()
        torch.cuda.synchronize()
    names = sorted({e.name for e in prof.events() if "kernel" in e.name.lower() and "hipLaunch" not in e.name})
    assert names, "the device trace lists no HIP kernels: the engine that ran cannot be confirmed"
    return out, names


def has(names, pattern):
    return any(re.search(pattern, n) for n in names)


# One kernel per conv engine (csrc/conv.hip's plans pick exactly one of them per call), and the kernels that finish a weight
# gradient.  The only list of these names in the tests: a new engine is added here.
CONV_ENGINE_KERNELS = ("dconv_down_kernel", "bconv_down_kernel", "tconv_down_kernel", "uconv_scatter_kernel", "buconv_scatter_kernel",
                       "dconv_up_kernel", "tconv_up_kernel", "igemm_kernel", "dconv_wgrad_kernel", "bconv_wgrad_kernel",
                       "tconv_wgrad_kernel")
CONV_REDUCE_KERNELS = ("conv_slab_reduce_kernel", "conv_slab_reduce_wave_kernel", "channel_sum_kernel")

# One kernel per dense engine of repo_gemm (csrc/gemm.hip's dense_plan picks exactly one of them per call): the <= 8-row vector
# kernel, the bf16x6 engine, and the fp32-MFMA tile engines with vector loads / with gathers.
DENSE_ENGINE_KERNELS = ("gemv_small_kernel", "bgemm_kernel", "vgemm_kernel", "igemm_kernel")

# Every kernel a dense weight gradient can run on (csrc/gemm.hip's wgrad_plan / wgrad_group_plan), as patterns for has():
# the two row-range head kernels, the split-K tile engine alone (VWgradOp) and in a group (VWgradGroupOp), the one
# bf16x6 product, and the kernel that sums the slabs of a single job / of a group.
DENSE_WGRAD_KERNELS = (r"\bwgrad_tr_kernel\b", r"\bwgrad_direct_kernel\b", r"\bvgemm_kernel<[^,]*\bVWgradOp\b",
                       r"\bvgemm_kernel<[^,]*\bVWgradGroupOp\b", r"\bbgemm_kernel\b", r"\bslab_reduce_kernel\b",
                       r"\bslab_reduce_group_kernel\b")
