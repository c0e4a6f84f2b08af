"""tests/reduce_ref.py on its own (no GPU): the float32 emulation of the reductions' fixed summation order against an exact
sum, its sensitivity to the order, and the mirrored block counts at the boundary sizes tests/test_reductions_gpu.py uses."""
import math

import numpy as np
import pytest

from tests import reduce_ref as rr


@pytest.mark.parametrize("n", [1, 63, 64, 65, 256, 257, 1024])
@pytest.mark.parametrize("signed", [False, True])
def test_fixed_order_sum_is_within_the_rounding_bound_of_the_exact_sum(n, signed):
    """|s - exact| <= depth * 2^-24 * sum|x|: every value passes through at most `depth` float32 additions, each within
    2^-24 relative of its exact result, so the error is at most ((1 + 2^-24)^d - 1) sum|x| with d the ROUNDING additions
    on the longest chain.  `fixed_order_depth` also counts the two additions to an exact zero, which round nothing:
    d <= depth - 2, and (1 + u)^(depth - 2) - 1 < depth * u for every depth here (<= 14)."""
    rs = np.random.RandomState(n + 1000 * signed)
    x = rs.standard_normal(n).astype(np.float32) * np.float32(3.0)
    if not signed:
        x = np.abs(x)
    x[rs.randint(n)] *= np.float32(1000.0)      # one dominant term: the partial sums then round on a coarser grid
    got = rr.fixed_order_sum(x)
    assert got.dtype == np.float32
    exact = math.fsum(float(v) for v in x)
    depth = rr.fixed_order_depth(n)
    assert depth == {1: 11, 63: 11, 64: 11, 65: 11, 256: 11, 257: 12, 1024: 14}[n]
    bound = depth * 2.0 ** -24 * math.fsum(abs(float(v)) for v in x)
    assert abs(float(got) - exact) <= bound, (n, float(got), exact, bound)


def test_fixed_order_sum_of_a_single_value_and_of_exact_integers():
    assert rr.fixed_order_sum([np.float32(0.1)]) == np.float32(0.1)
    assert rr.fixed_order_sum(np.arange(1024, dtype=np.float32)) == np.float32(1023 * 1024 // 2)


def test_fixed_order_sum_is_order_sensitive():
    """Hand-worked: x = [2^24, 1, 1, 1]; above 2^24 float32 is spaced by 2 and ties round to even.
    Left to right: 2^24 + 1 -> 2^24 (tie, even), three times: 16777216.
    Fixed order: threads 0..3 hold the values, every other lane 0; the butterfly's offsets 32 .. 4 add zeros; offset 2 makes
    lane 0 = 2^24 + 1 -> 2^24 and lane 1 = 1 + 1 = 2; offset 1 makes lane 0 = 2^24 + 2 = 16777218 (exact).
    The exact sum is 16777219."""
    x = np.array([2.0 ** 24, 1.0, 1.0, 1.0], dtype=np.float32)
    ltr = np.float32(0.0)
    for v in x:
        ltr = np.float32(ltr + v)
    assert float(ltr) == 16777216.0
    assert float(rr.fixed_order_sum(x)) == 16777218.0
    # the strided first stage is part of the order: parts[256] is added by thread 0 BEFORE the butterfly.
    # thread 0: 2^24 + 1 -> 2^24; offset 2: lane 0 + lane 2 = 2^24 + 1 -> 2^24.  Both ones are lost.
    y = np.zeros(258, dtype=np.float32)
    y[0], y[2], y[256] = 2.0 ** 24, 1.0, 1.0
    assert float(rr.fixed_order_sum(y)) == 16777216.0
    # the same three values with the ones on thread 1 (its second value) and thread 3: lanes 1 and 3 meet at offset 2
    # (1 + 1 = 2), and offset 1 adds that 2 to 2^24 exactly
    y = np.zeros(258, dtype=np.float32)
    y[0], y[3], y[257] = 2.0 ** 24, 1.0, 1.0
    assert float(rr.fixed_order_sum(y)) == 16777218.0


def test_mirrored_block_counts_at_the_boundary_sizes():
    """(blocks, finishes in its own launch) at every size of the GPU suite's case tables."""
    def regime(b):
        return b, rr.finishes_in_launch(b)

    assert [regime(rr.kl_blocks(r)) for r in (1, 2560, 2561, 41000)] == [(1, True), (64, True), (65, False), (1024, False)]
    for f in (rr.scalar_nll_blocks, rr.normal_entropy_blocks):
        assert [regime(f(n)) for n in (1, 1023, 65536, 65537, 1048577)] == \
            [(1, True), (1, True), (64, True), (65, False), (1024, False)]
    assert -(-1048577 // 1024) == 1025          # the cap is reached by one block: every block strides twice at most
    assert [regime(rr.lambda_return_blocks(n)) for n in (1, 255, 16384, 16385, 262145)] == \
        [(1, True), (1, True), (64, True), (65, False), (1024, False)]
    assert [regime(rr.tanh_normal_entropy_blocks(r, a)) for r, a in ((1, 1), (2730, 6), (2731, 6), (43691, 6), (37, 7))] == \
        [(1, True), (64, True), (65, False), (1024, False), (2, True)]
    assert [regime(rr.tia_blend_blocks(n, p)) for n, p in ((3, 4), (5, 36), (32, 4096), (33, 4096), (513, 4096))] == \
        [(1, True), (1, True), (64, True), (66, False), (1024, False)]
    assert [rr.sqnorm_blocks(n) for n in (1, 2, 3, 4, 5, 4095, 4097, 4194307)] == [1, 1, 1, 1, 1, 1, 2, 1024]
    assert -(-4194307 // 4096) == 1025 and 4194307 % 4 == 3
    assert [rr.clip_adam_blocks(n) for n in (1, 257, 524547)] == [1, 2, 2048]
    assert -(-524547 // 256) == 2050            # more blocks' worth than the grid: the grid-stride loop runs
    assert [rr.relu_mask_blocks(n) for n in (1, 255, 1048589)] == [1, 1, 4096]
    assert -(-1048589 // 256) == 4097
    assert rr.red_blocks(0, 40) == 1            # the lower clamp
    cs = [(1, 1, 1), (300, 5, 1), (7, 3, 255), (7, 3, 256), (7, 3, 257), (9, 32, 900), (1001, 128, 25), (200, 3, 4096)]
    assert [rr.chansum_splits(*c) for c in cs] == [1, 1, 1, 1, 1, 1, 4, 100]
    assert 1001 - 3 * -(-1001 // 4) == 248      # the ragged last split of (1001, 128, 25): 251, 251, 251, 248 images
