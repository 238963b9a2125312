"""CPU model of k_seed_sift<4096, true> (miniprot_amd/csrc/seed_exec.hip), the sift of a run without a pre-chain: the range walk of
tests/test_sift_model.py with the keep rule of the MAIN chain's reach D -- block lo of a range takes the local number D, the anchors
of a range's last D blocks wait for the next range (re-based by the range's width; a range narrower than D carries everything), the
segment-edge probes look D blocks to either side, D = 0 has neither carry nor probes, and beyond the widest filtered reach every
anchor is kept -- step for step as the kernel does them, checked against the definition: sort the query's anchors by (block,
seed), keep those whose predecessor or successor lies at most D blocks away, rank = index in the full sorted list.  The HIP kernel
is checked on the GPU (tests/test_seed_nopre_gpu.py); this model pins the algorithm."""
import numpy as np
import pytest

REACH_MAX = 15


class Overflow(Exception):
    pass


def sift_segment_reach(lists, lo0, hi0, n_block, reach, cap=4096, carry_max=1024, target=2560):
    """One workgroup: blocks [lo0, hi0) of a query whose occurrence lists (ascending block ids) are `lists`.
    Returns [(block, list, rank)] of the kept anchors in output order."""
    nl = len(lists)
    LB = 1
    while (1 << LB) < nl:
        LB += 1
    keep_all = reach > REACH_MAX
    D = 0 if keep_all else reach
    w_max = (1 << (32 - LB)) - 1 - D
    n_anchor = sum(len(x) for x in lists)
    cur = [int(np.searchsorted(x, lo0, "left")) if lo0 > 0 else 0 for x in lists]
    pos_base = sum(cur)
    # the highest block with an anchor in [lo0 - D, lo0)
    left = [int(x[c - 1]) for x, c in zip(lists, cur) if lo0 > 0 and c > 0 and int(x[c - 1]) + D >= lo0]
    prev_blk = max(left) if left and D else None
    lo, carry, emitted, out = lo0, [], pos_base, []
    width = min(max(n_block * target // n_anchor if n_anchor else n_block, 1), w_max)
    while lo < hi0:
        while True:
            hi = lo + width if hi0 - lo > width else hi0
            cur2 = [int(np.searchsorted(x, hi, "left")) for x in lists]
            total = sum(c1 - c0 for c0, c1 in zip(cur, cur2))
            if len(carry) + total <= cap:
                break
            if hi - lo <= 1:
                raise Overflow()
            width = (hi - lo) >> 1
        keys = list(carry)
        for l, (x, c0, c1) in enumerate(zip(lists, cur, cur2)):
            keys += [((int(b) - lo + D) << LB) | l for b in x[c0:c1]]
        assert all(0 <= k < ((hi - lo + D) << LB) < (1 << 32) for k in keys)
        keys.sort()
        cur = cur2
        n = len(keys)
        last = hi == hi0
        right_end = None
        if last and hi0 < n_block and D > 0:                     # the lowest block with an anchor in [hi0, hi0 + D)
            right = [int(x[c]) for x, c in zip(lists, cur) if c < len(x) and int(x[c]) - hi0 < D]
            if right:
                right_end = min(right) - lo + D
        n_emit = n
        if not last:
            bound = (hi - lo) << LB
            n_emit = sum(1 for k in keys if k < bound)
        if n - n_emit > carry_max:
            raise Overflow()
        left0 = None if prev_blk is None else prev_blk - lo + D
        for i in range(n_emit):
            b = keys[i] >> LB
            lf = keys[i - 1] >> LB if i > 0 else left0
            rt = keys[i + 1] >> LB if i + 1 < n else right_end
            if keep_all or (lf is not None and b - lf <= D) or (rt is not None and rt - b <= D):
                out.append((lo + b - D, keys[i] & ((1 << LB) - 1), emitted + i))
        if n_emit > 0:
            prev_blk = lo + (keys[n_emit - 1] >> LB) - D
        carry = [k - ((hi - lo) << LB) for k in keys[n_emit:]]
        assert all(0 <= (k >> LB) < max(D, 1) for k in carry) and (D > 0 or not carry)
        emitted += n_emit
        lo = hi
        if total < target // 2:
            width = w_max if width > w_max // 2 else width * 2
    return out


def definition(lists, reach):
    allk = sorted((int(b), l) for l, x in enumerate(lists) for b in x)
    keep = []
    for i, (b, l) in enumerate(allk):
        near = (i > 0 and b - allk[i - 1][0] <= reach) or (i + 1 < len(allk) and allk[i + 1][0] - b <= reach)
        if reach > REACH_MAX or near:
            keep.append((b, l, i))
    return keep


def densest(lists, n_block, span):
    """most anchors in `span` consecutive blocks"""
    per = np.bincount(np.concatenate(lists + [np.zeros(0, np.int64)]), minlength=n_block + span)
    return int(np.convolve(per, np.ones(span, np.int64)).max())


def random_lists(rng, n_block, nl, dense):
    lists = []
    for _ in range(nl):
        n = int(rng.integers(0, 40))
        blocks = rng.integers(0, n_block, n)
        if dense:                                                # clusters: many lists hitting the same few neighbourhoods
            centre = rng.choice([n_block // 7, n_block // 2, n_block - 3])
            blocks = np.concatenate([blocks, centre + rng.integers(-20, 20, int(rng.integers(0, 30)))])
        lists.append(np.unique(np.clip(blocks, 0, n_block - 1)).astype(np.int64))
    return lists


@pytest.mark.parametrize("reach", [0, 1, 3, 7, 15, 16, 62])
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_model_equals_definition(seed, reach):
    """whole queries and queries cut into 2..9 segments, buffers of 4 096 down to 64 keys (ranges of a few blocks: narrower than D,
    carries spanning several ranges), sparse and clustered lists"""
    rng = np.random.default_rng(100 * seed + reach)
    checked = 0
    for it in range(12):
        n_block = int(rng.choice([50, 600, 20000]))
        lists = random_lists(rng, n_block, int(rng.choice([1, 3, 40, 300])), dense=bool(it & 1))
        want = definition(lists, reach)
        for ns in (1, int(rng.integers(2, 10))):
            for cap, carry_max, target in ((4096, 1024, 2560), (64, 48, 16)):
                got = []
                try:
                    for k in range(ns):
                        lo0, hi0 = n_block * k // ns, n_block * (k + 1) // ns
                        if hi0 > lo0:
                            got += sift_segment_reach(lists, lo0, hi0, n_block, reach, cap, carry_max, target)
                except Overflow:
                    # the kernel flags the query for the host.  Legitimate only where the input is that dense: a range is at least one
                    # block and the carry at most D, so the buffer overflows only with more than cap anchors in D + 1 consecutive
                    # blocks, the carry only with more than carry_max in D
                    assert densest(lists, n_block, (0 if reach > REACH_MAX else reach) + 1) > min(cap, carry_max), (seed, reach, it, ns, cap)
                    continue
                assert got == want, (seed, reach, it, ns, cap)
                checked += 1
    assert checked >= 24


def test_carry_beyond_its_limit_flags_the_query():
    """more than carry_max anchors in the last D blocks of a range: the query is handed to the host, as on the pre-chain route"""
    lists = [np.arange(0, 200, dtype=np.int64) for _ in range(20)]          # 20 anchors in every block: 60 in any three, 48 may wait
    with pytest.raises(Overflow):
        sift_segment_reach(lists, 0, 200, 200, 3, cap=128, carry_max=48, target=80)
    assert len(sift_segment_reach(lists, 0, 200, 200, 2, cap=128, carry_max=48, target=80)) == 4000     # (40 in any two: fine)
