"""Which rows a workgroup of the persistent head chains takes, restated in plain Python from csrc/mlp16.hip
(`grid_for`, `my_blocks`, the pair / single loop of `mlp_fwd_kernel` and `mlp_bwd_kernel`) and csrc/mlp32.hip (`grid32_for`,
`my_tiles32`), and the row counts at which that loop first does each thing it can do.

Both engines launch min(blocks, 2 x CUs) workgroups; workgroup b owns a contiguous run of R-row blocks (R = 16 / 32).  The
32-row engine executes one block per tile.  The 16-row engine executes its run in PAIRS (32 rows that share every weight
fragment) while two blocks are left, then at most one single: its tiles are (r0, nr, RB) with RB = 2 or 1.

per_row() / worst_row() are the per-row measure of tests/test_mlp_persistent_gpu.py (tensor methods only: any device)."""
R16, R32 = 16, 32


def slots(cus):
    """Workgroups that fit at once: two per CU (LDS)."""
    return 2 * cus


def blocks(rows, R):
    return (rows + R - 1) // R


def grid(rows, R, cus):
    return min(blocks(rows, R), slots(cus))


def owned(rows, R, cus, b):
    """-> (first, count): the R-row blocks of workgroup b (my_blocks / my_tiles32)."""
    nb, g = blocks(rows, R), grid(rows, R, cus)
    base, rem = nb // g, nb % g
    return b * base + min(b, rem), base + (1 if b < rem else 0)


def tiles(rows, R, cus, b):
    """-> [(r0, nr, RB)]: the tiles workgroup b executes, in order.  R = 32: RB = 1 throughout."""
    first, count = owned(rows, R, cus, b)
    out = []
    while count > 0:
        rb = 2 if R == R16 and count >= 2 else 1
        r0 = first * R
        out.append((r0, min(rb * R, rows - r0), rb))
        first, count = first + rb, count - rb
    return out


def all_tiles(rows, R, cus):
    """-> [(workgroup, tile index within it, r0, nr, RB)] of the whole launch."""
    return [(b, i, r0, nr, rb) for b in range(grid(rows, R, cus)) for i, (r0, nr, rb) in enumerate(tiles(rows, R, cus, b))]


def locate(rows, R, cus, row):
    """-> (workgroup, tile index within it, tiles of that workgroup, RB of the tile, block of the row within the tile)."""
    g = grid(rows, R, cus)
    lo, hi = 0, g - 1
    blk = row // R
    while lo < hi:   # the last workgroup whose first block is <= blk
        mid = (lo + hi + 1) // 2
        if owned(rows, R, cus, mid)[0] <= blk:
            lo = mid
        else:
            hi = mid - 1
    ts = tiles(rows, R, cus, lo)
    for i, (r0, nr, rb) in enumerate(ts):
        if r0 <= row < r0 + nr:
            return lo, i, len(ts), rb, (row - r0) // R
    raise AssertionError((rows, R, cus, row))


def where(rows, R, cus, row):
    b, i, n, rb, k = locate(rows, R, cus, row)
    kind = "tile" if R == R32 else ("pair, block %d" % k if rb == 2 else "single")
    return f"row {row}: workgroup {b}, tile {i} of {n} ({kind})"


def shapes(ts):
    """The RBs of a workgroup's tiles: (2, 1) is pair then single."""
    return tuple(rb for _, _, rb in ts)


# (engine's R, name, rows as a function of S = slots): the smallest counts that reach each transition of the tile loops
REGIMES = [
    (R16, "16S+1", lambda S: 16 * S + 1),
    (R16, "32S-14", lambda S: 32 * S - 14),
    (R16, "32S+1", lambda S: 32 * S + 1),
    (R16, "48S+14", lambda S: 48 * S + 14),
    (R32, "32S+1", lambda S: 32 * S + 1),
    (R32, "64S-23", lambda S: 64 * S - 23),
    (R32, "64S+1", lambda S: 64 * S + 1),
]
SHARED = "32S+1"   # the count both engines take


def regime_rows(cus):
    """-> {(R, name): rows}, every entry confirmed against the mirror (asserted, not assumed)."""
    S = slots(cus)
    out = {}
    for R, name, f in REGIMES:
        rows = f(S)
        assert grid(rows, R, cus) == S, (R, name, cus)
        confirm(R, name, rows, cus)
        out[(R, name)] = rows
    return out


def confirm(R, name, rows, cus):
    S = slots(cus)
    per = [tiles(rows, R, cus, b) for b in range(S)]
    sh = [shapes(t) for t in per]
    last = per[-1][-1]
    if R == R16 and name == "16S+1":      # workgroup 0 one pair; every other one single; the last single has 1 row
        assert sh[0] == (2,) and all(s == (1,) for s in sh[1:]) and last[1:] == (1, 1)
    elif R == R16 and name == "32S-14":   # every workgroup one pair; the last pair has 16 + 2 rows
        assert all(s == (2,) for s in sh) and last[1:] == (18, 2)
    elif R == R16 and name == "32S+1":    # workgroup 0 pair then single; the last workgroup's pair has 16 + 1 rows
        assert sh[0] == (2, 1) and all(s == (2,) for s in sh[1:]) and last[1:] == (17, 2)
    elif R == R16 and name == "48S+14":   # workgroup 0 pair, pair; the others pair, single; the last single has 14 rows
        assert sh[0] == (2, 2) and all(s == (2, 1) for s in sh[1:]) and last[1:] == (14, 1)
    elif R == R32 and name == "32S+1":    # workgroup 0 two tiles; the last tile has 1 row
        assert sh[0] == (1, 1) and all(s == (1,) for s in sh[1:]) and last[1] == 1
    elif R == R32 and name == "64S-23":   # every workgroup two tiles; the last workgroup's second tile has 9 rows
        assert all(s == (1, 1) for s in sh) and last[1] == 9
    elif R == R32 and name == "64S+1":    # workgroup 0 three tiles; the last workgroup's second tile has 1 row
        assert sh[0] == (1, 1, 1) and all(s == (1, 1) for s in sh[1:]) and last[1] == 1
    else:
        raise AssertionError((R, name))


def later_tiles(rows, R, cus):
    """The tiles that are not their workgroup's first."""
    return [t for t in all_tiles(rows, R, cus) if t[1] > 0]


def weight_rows(rows, R, cus):
    """rows_w for the two-upstream reverse: a count that is no multiple of 32 and ends INSIDE a tile that is not its
    workgroup's first -- of the workgroups that have such a tile, the middle one's second tile.  Two regimes of the 16-row
    engine have no such tile (16S+1 and 32S-14: every workgroup executes one tile); there the count ends inside the second
    block of the middle pair, or, with workgroup 0's the only pair, inside that pair's second block."""
    later = [t for t in later_tiles(rows, R, cus) if t[1] == 1 and t[3] >= 14]
    if later:
        _, _, r0, nr, _ = later[len(later) // 2]
        w = r0 + 13
    else:
        pairs = [t for t in all_tiles(rows, R, cus) if t[4] == 2 and t[3] >= R + 2]
        assert pairs, (rows, R, cus)
        w = pairs[len(pairs) // 2][2] + R + 1
    assert 0 < w < rows and w % 32 != 0
    return w


def per_row(got, want):
    """Per row r: |got_r - want_r|_2 / max(|want_r|_2, rms over rows of |want_r|_2), in float64."""
    g, w = got.detach().double().flatten(1), want.detach().double().flatten(1)
    assert g.shape == w.shape, (g.shape, w.shape)
    n = w.norm(dim=1)
    floor = n.pow(2).mean().sqrt()
    return (g - w).norm(dim=1) / n.clamp_min(float(floor) + 1e-300)


def worst_row(got, want):
    """-> (the largest per_row figure, its row)."""
    e = per_row(got, want.to(got.device))
    e = e.nan_to_num(nan=float("inf"))   # a NaN anywhere in a row is the worst there is
    i = int(e.argmax())
    return float(e[i]), i
