"""CPU (pure host, test tap pnr_pair_tiles): the launch plan of the pair minimum (pairmin.h pair_tiles) under pnr_point_segment_distance
and pnr_nearest_other / pnr_join_trees -- how the (points x segments) rectangle is cut into launches of a bounded pair count and each
launch into blockIdx.y slices.  Pinned plans, a restatement of the rule in Python, and the properties every plan must have."""
import numpy as np
import pytest
import pnr_amd

TPB, MIN_SPLIT, TARGET_BLOCKS, AUTO_PAIRS, MAX_GRID_Y = 256, 64, 2048, 1 << 34, 65535


def restated(n, m, split_opt, budget_opt):
    """the rule: a launch holds whole block rows of 256 points and at most `budget` pairs (at least one row by one segment) -- as many
    rows over ALL segments as fit, else one row over budget / 256 segments; rows outer, segments inner.  A launch's slices: the option,
    or enough slices of at least 64 segments for 2048 work-groups; never more than 65535 of them."""
    budget = budget_opt if budget_opt > 0 else AUTO_PAIRS
    rows_fit = budget // m // TPB * TPB
    rows = min(max(rows_fit, TPB), -(-n // TPB) * TPB)
    segs = m if rows_fit >= TPB else max(1, budget // TPB)
    out = []
    for p0 in range(0, n, rows):
        for s0 in range(0, m, segs):
            p1, s1 = min(p0 + rows, n), min(s0 + segs, m)
            gx, ms = -(-(p1 - p0) // TPB), s1 - s0
            split = split_opt
            if split <= 0:
                slices = max(1, min(-(-TARGET_BLOCKS // gx), ms // MIN_SPLIT))
                split = -(-ms // slices)
            split = max(split, -(-ms // MAX_GRID_Y))
            out.append((p0, p1, s0, s1, split, gx, -(-ms // split)))
    return np.array(out, np.int64).reshape(-1, 7)


# (n, m, split, budget) -> the number of launches, which launch is pinned, and that launch
PINNED = [
    ((1000, 777, 64, 100000), 8, 0, (0, 256, 0, 390, 64, 1, 7)),
    ((1000, 777, 0, 0), 1, 0, (0, 1000, 0, 777, 65, 4, 12)),
    ((33536, 33536, 0, 0), 1, 0, (0, 33536, 0, 33536, 2096, 131, 16)),  # the bench forest
    ((1, 1, 0, 0), 1, 0, (0, 1, 0, 1, 1, 1, 1)),
    ((4099, 2053, 64, 100000), 102, -1, (4096, 4099, 1950, 2053, 64, 1, 2)),
    ((5, 1 << 22, 1, 0), 1, 0, (0, 5, 0, 1 << 22, 65, 1, 64528)),  # the split raised by the limit of gridDim.y
    ((1000, 100, 64, 100000), 2, 0, (0, 768, 0, 100, 64, 3, 2)),  # several row launches, each over all segments
    ((1000, 100, 64, 100000), 2, 1, (768, 1000, 0, 100, 64, 1, 2)),
]


@pytest.mark.parametrize("args,count,which,tile", PINNED)
def test_pinned_plans(args, count, which, tile):
    t = pnr_amd.pair_tiles(*args)
    assert len(t) == count and tuple(t[which]) == tile, (len(t), t[which])
    assert np.array_equal(t, restated(*args))


@pytest.mark.parametrize("budget", [100, 256])
def test_a_budget_below_one_block_row_gives_one_row_by_one_segment(budget):
    t = pnr_amd.pair_tiles(300, 5000, 0, budget)
    assert len(t) == 10000
    assert np.array_equal(t[:, 1] - t[:, 0], np.repeat([256, 44], 5000)) and np.all(t[:, 3] - t[:, 2] == 1)
    assert np.all(t[:, 4:] == 1)
    assert np.array_equal(t[:5000, 2], np.arange(5000)) and np.array_equal(t[5000:, 2], np.arange(5000))  # rows outer, segments inner


def test_random_plans_partition_the_rectangle_within_budget_and_grid():
    rng = np.random.default_rng(20261018)
    for _ in range(300):
        n, m = int(rng.integers(1, 5001)), int(rng.integers(1, 5001))
        split = int(rng.choice([0, 1, 7, 64, 1000]))
        budget = int(rng.choice([0, 1, 100, 256, 1000, 100000, 10000000]))
        if budget in (1, 100) and n * m > 2000000:  # one row by one segment per launch: keep the count of launches small
            n, m = n % 600 + 1, m % 600 + 1
        t = pnr_amd.pair_tiles(n, m, split, budget)
        what = (n, m, split, budget)
        assert np.array_equal(t, restated(n, m, split, budget)), what
        p0, p1, s0, s1, sp, gx, gy = t.T
        assert np.all((0 <= p0) & (p0 < p1) & (p1 <= n) & (0 <= s0) & (s0 < s1) & (s1 <= m)), what
        # every (point, segment) exactly once: the row ranges partition [0, n), and within one row range the segment ranges partition [0, m)
        rows = sorted(set(zip(p0.tolist(), p1.tolist())))
        assert rows[0][0] == 0 and rows[-1][1] == n and all(a[1] == b[0] for a, b in zip(rows, rows[1:])), what
        for r0, r1 in rows:
            mine = (p0 == r0) & (p1 == r1)
            a, b = s0[mine], s1[mine]
            assert a[0] == 0 and b[-1] == m and np.array_equal(a[1:], b[:-1]), what
        assert len(t) == len(rows) * int(((p0 == 0) & (p1 == rows[0][1])).sum()), what
        ms = s1 - s0
        assert np.all((1 <= gy) & (gy <= MAX_GRID_Y)) and np.all(sp >= 1), what
        assert np.all(gy * sp >= ms) and np.all((gy - 1) * sp < ms), what  # the slices cover the segments and none is empty
        assert np.all(gx * TPB >= p1 - p0) and np.all((gx - 1) * TPB < p1 - p0), what
        assert np.all(gx * TPB * ms <= max(budget if budget > 0 else AUTO_PAIRS, TPB)), what


def test_arguments():
    import ctypes as C
    L = pnr_amd.lib.load()
    k = C.c_int64()
    for bad in ((0, 5, 0, 0), (5, 0, 0, 0), (5, 5, -1, 0), (5, 5, 0, -1)):
        assert L.pnr_pair_tiles(*bad, None, 0, C.byref(k)) == -1, bad
        assert b"pnr_pair_tiles" in L.pnr_last_error()
    assert L.pnr_pair_tiles(5, 5, 0, 0, None, 0, None) == -1
    assert L.pnr_pair_tiles(1000, 777, 64, 100000, None, 0, C.byref(k)) == 0 and k.value == 8  # the count alone
    few = np.zeros((3, 7), np.int64)
    assert L.pnr_pair_tiles(1000, 777, 64, 100000, few.ctypes.data, 3, C.byref(k)) == 0 and k.value == 8
    assert np.array_equal(few, pnr_amd.pair_tiles(1000, 777, 64, 100000)[:3])
