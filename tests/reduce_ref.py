"""The streaming reductions' one summation order and their grids, restated in Python.

`fixed_order_sum` is the order in which `last_block_finishes` (csrc/common.h), `final_sum_kernel` (csrc/loss.hip) and
`sqnorm_final_kernel` (csrc/optim.hip) add a row of per-block partials, all three with blockDim.x = 256 on wave64:

  1. thread t starts from 0 and adds parts[t], parts[t + 256], ... in sequence;
  2. each 64-lane wave runs the xor butterfly of `wave_sum`, offsets 32, 16, 8, 4, 2, 1: v[l] = v[l] + v[l ^ o] on all lanes
     at once (float addition commutes, so every lane of a wave ends with the same bits);
  3. thread 0 starts from 0 and adds the four wave results in wave order (`block_sum`).

Every step is one float32 addition -- there is no multiply to contract into an FMA -- so numpy's float32 arithmetic
reproduces the device's bits.  tests/test_reductions_gpu.py holds each reduction's output to this function of the partials
it reads back from the workspace; tests/test_reduce_ref_cpu.py checks the function itself.

The rest of the file mirrors the block count of every entry point (the `red_blocks(n, per_block)` calls of csrc/loss.hip,
`chansum_splits` of csrc/conv.hip, the grids of csrc/optim.hip and of repo_relu_mask): the GPU suite derives each case's
regime from these and pins them by counting the partials a launch wrote.
"""
import numpy as np

BLOCK = 256                 # blockDim.x of every reduction kernel and of the three finishing sums
WAVE = 64
RED_BLOCKS = 1024           # kRedBlocks: the cap on a reduction's grid (= partials per value)
LAST_BLOCK_MAX_GRID = 64    # kLastBlockMaxGrid: up to here the launch's last block finishes the sum (ticket), above a follow-up
RED_HEADER_BYTES = 256      # kRedHeaderBytes: the workspace's header (ticket word first), then the partials [nvals][blocks]


def fixed_order_sum(parts):
    """float32 sum of `parts` in the device's fixed order (module docstring)."""
    p = np.asarray(parts, dtype=np.float32).ravel()
    acc = np.zeros(BLOCK, dtype=np.float32)
    for i0 in range(0, p.size, BLOCK):
        chunk = p[i0:i0 + BLOCK]
        acc[:chunk.size] = acc[:chunk.size] + chunk
    v = acc.reshape(BLOCK // WAVE, WAVE)
    lane = np.arange(WAVE)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lane ^ o]
    r = np.float32(0.0)
    for w in range(BLOCK // WAVE):
        r = np.float32(r + v[w, 0])
    return r


def fixed_order_depth(n):
    """Additions on the longest chain of fixed_order_sum over n values: the strided adds of thread 0, six butterfly steps,
    four wave results (the first add of steps 1 and 3 is to an exact zero; counting them only loosens a bound)."""
    return -(-n // BLOCK) + 6 + BLOCK // WAVE


def red_blocks(n, per_block):
    """csrc/loss.hip red_blocks: ceil(n / per_block) clamped to [1, kRedBlocks]."""
    return max(1, min(RED_BLOCKS, -(-n // per_block)))


def finishes_in_launch(blocks):
    """True: the ticket path (no follow-up launch); False: final_sum_kernel runs."""
    return blocks <= LAST_BLOCK_MAX_GRID


# elements per block of each loss.hip entry point (its red_blocks call), in the entry point's own unit
def kl_blocks(rows):                       # repo_kl_balance: rows, one wave per row, 40 rows per block
    return red_blocks(rows, 40)


def scalar_nll_blocks(n):                  # repo_scalar_nll
    return red_blocks(n, 1024)


def normal_entropy_blocks(n):              # repo_normal_entropy
    return red_blocks(n, 1024)


def tanh_normal_entropy_blocks(rows, A):   # repo_tanh_normal_entropy: one thread per element
    return red_blocks(rows * A, 256)


def lambda_return_blocks(N):               # repo_lambda_return: one thread per column
    return red_blocks(N, 256)


def tia_blend_blocks(nimg, pixels):        # repo_tia_blend_nll: one thread per 4 pixels
    return red_blocks(nimg * pixels // 4, 512)


def sqnorm_blocks(n):                      # repo_grad_sqnorm: always two launches
    return min(1024, -(-n // 4096))


def clip_adam_blocks(n):                   # repo_clip_adam: grid-stride above 2048 blocks
    return min(2048, -(-n // 256))


def relu_mask_blocks(n):                   # repo_relu_mask: grid-stride above 4096 blocks
    return min(4096, -(-n // 256))


def chansum_splits(nimg, C, P):
    """csrc/conv.hip chansum_splits: the image chunks of repo_channel_sum (grid (C, splits), then one wave per channel)."""
    want = -(-4096 // C)
    min_imgs = -(-8192 // P)
    want = max(1, min(want, -(-nimg // min_imgs)))
    ips = -(-nimg // want)
    return -(-nimg // ips)
