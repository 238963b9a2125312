"""The pass planner of the multi-pass device index build (mpa_dbg_idx_plan_passes, index.cpp: idx_plan_passes) against a
ten-line Python greedy and against the properties the build relies on: the bucket ranges are contiguous and cover every bin of
the key histogram exactly once, no pass exceeds the budget, and no two neighbouring passes would fit in one (so the greedy plan
has the fewest passes a contiguous plan can have).  Host only: the planner needs no device."""
import numpy as np
import pytest
import miniprot_amd as mpa


def greedy(hist, budget):
    """first bin of every pass plus the end, or -1 when a bin alone exceeds the budget"""
    if any(h > budget for h in hist):
        return -1
    first, load = [0], 0
    for b, h in enumerate(hist):
        if load + h > budget:
            first.append(b)
            load = 0
        load += h
    return first + [len(hist)]


def check_plan(hist, budget):
    plan = mpa.idx_plan_passes(hist, budget)
    assert plan == greedy([int(h) for h in hist], budget), (len(hist), budget)
    if plan == -1:
        assert max(int(h) for h in hist) > budget
        return plan
    hist = np.asarray(hist, dtype=np.int64)
    assert plan[0] == 0 and plan[-1] == len(hist)                      # covers every bin ...
    assert all(a < b for a, b in zip(plan[:-1], plan[1:]))             # ... once, in ascending contiguous non-empty ranges
    loads = [int(hist[a:b].sum()) for a, b in zip(plan[:-1], plan[1:])]
    assert all(l <= budget for l in loads), (loads, budget)
    assert all(l0 + l1 > budget for l0, l1 in zip(loads[:-1], loads[1:])), "two neighbouring passes would fit in one"
    return plan


def random_hist(rng, n_bins):
    """counts over orders of magnitude, single empty bins, and runs of empty bins at both ends"""
    hist = (rng.integers(0, 1000, n_bins) * (10 ** rng.integers(0, 4, n_bins))).astype(np.int64)
    hist[rng.random(n_bins) < 0.2] = 0
    lead, trail = int(rng.integers(0, n_bins // 3 + 1)), int(rng.integers(0, n_bins // 3 + 1))
    hist[:lead] = 0
    hist[n_bins - trail:] = 0
    return hist


@pytest.mark.parametrize("n_bins", [1, 2, 3, 7, 64, 1000, 4095, 4096])
def test_plans_equal_the_greedy_and_hold_their_properties(n_bins):
    rng = np.random.default_rng(1000 + n_bins)
    for _ in range(12):
        hist = random_hist(rng, n_bins)
        total, largest = int(hist.sum()), int(hist.max())
        for budget in {total, largest, max(largest, total // 2), max(largest, total // 7), max(largest, total // 64), largest + 1, total + 5}:
            plan = check_plan(hist, budget)
            if budget >= total:
                assert plan == [0, n_bins]                             # a budget that holds everything: one pass
        assert len(check_plan(hist, total)) == 2
        assert check_plan(hist, largest) != -1                         # the largest bin fits: a plan exists
        if largest > 0:
            assert check_plan(hist, largest - 1) == -1                 # one key less: it cannot be planned


def test_random_bin_counts():
    rng = np.random.default_rng(77)
    for _ in range(200):
        n_bins = int(rng.integers(1, 4097))
        hist = random_hist(rng, n_bins)
        largest = int(hist.max())
        check_plan(hist, int(rng.integers(largest, max(largest, int(hist.sum())) + 2)))


def test_all_zero_and_single_bin():
    for n_bins in (1, 5, 4096):
        assert check_plan(np.zeros(n_bins, np.int64), 0) == [0, n_bins]
        assert check_plan(np.zeros(n_bins, np.int64), 100) == [0, n_bins]
    assert check_plan([9], 9) == [0, 1]
    assert check_plan([9], 10 ** 12) == [0, 1]
    assert check_plan([9], 8) == -1
    assert check_plan([0, 0, 9, 0, 0], 9) == [0, 5]                    # empty runs at both ends ride with the one pass
    assert check_plan([4, 4, 4, 4], 4) == [0, 1, 2, 3, 4]
    assert check_plan([0, 4, 0, 4, 0], 4) == [0, 3, 5]                 # an empty bin never opens a pass


def test_counts_beyond_32_bits():
    hist = [3 << 32, 0, 5 << 32, 1 << 32, 7 << 32]
    assert check_plan(hist, 8 << 32) == [0, 3, 5]
    assert check_plan(hist, (7 << 32) - 1) == -1
