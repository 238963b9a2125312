"""Synthetic chaining problems for the chain extraction (chain_core.h: chain_extract_core; on the device k_chain_extract), shared by
tests/test_host_core.py, tests/test_seed_gpu.py and the two files that drive the extraction through mpa_dbg_chain_extract
(tests/test_chain_extract_cpu.py, tests/test_chain_extract_gpu.py).

A case is the problems of ONE launch -- sizes mixed and shuffled, empty and one-anchor problems in between, so that neighbours in the
kernel's scratch differ in size -- with the parameter sets and views (modes) it is run under.  The families (a) .. (l) each aim at one
branch of the team code; which branch a problem really takes is not claimed here but read from the hook's path record and asserted in
tests/test_chain_extract_cpu.py.

How the shapes come about (block anchors, kmer 6, bbit 8): an anchor is block << 32 | query position.  Two anchors of one block link
with min(6, dq) + 2 for dq <= 85 residues, so a few anchors of one block with rising query positions are a chain (`fragment`); a
collinear run with a query step of 6 residues scores 8 per anchor inside a block and 6 across a block boundary (`collinear`,
`collinear_scores`: 256 is passed at the 33rd anchor, 65 536 after about 8 340).  Units that must not see each other -- lone roots,
copies of a chain -- sit SLOT = 4 000 blocks apart, beyond the reach of the main chain's 200 000 nt as well as the pre-chain's block."""
import functools
import numpy as np

U = np.uint64
PRE = [256, 256, 256, 25, 1000000, 2, 0, 0.75, 1, 6, 8]               # the pre-chain (map.c:188)
MAIN = [200000, 1000, 200000, 25, 1000000, 3, 0, 0.75, 1, 6, 8]       # the main chain with the mapping defaults
DENSE, SPARSE_SET, SPARSE_CHAINS = 0, 1, 2                            # miniprot_amd.CHAIN_*
SLOT, BASE = 4000, 1000


# ---------------------------------------------------------------- the generators of tests/test_host_core.py (unchanged: same output for a given rng)
def _anchors(rng, n, n_block, qlen, n_planted):
    """random background + planted collinear runs + duplicated fragments (equal scores on purpose)"""
    blk = rng.integers(0, n_block, n)
    q = rng.integers(5, qlen, n)
    xs, ys = [blk], [q]
    for _ in range(n_planted):
        b0, q0, m = int(rng.integers(0, n_block)), int(rng.integers(5, qlen // 2)), int(rng.integers(2, 12))
        dq = np.cumsum(rng.integers(1, 9, m))
        for rep in range(int(rng.integers(1, 4))):           # the same fragment again a few blocks away / shifted by one residue
            xs.append(b0 + (dq * 3) // 256 + rep * int(rng.integers(0, 3)))
            ys.append(q0 + dq + (rep if rng.random() < 0.5 else 0))
    a = (np.concatenate(xs).astype(np.uint64) << np.uint64(32)) | (np.concatenate(ys).astype(np.uint64) & np.uint64(0x7fffffff))
    return np.unique(a)


def _long_chains(rng, n_block, n_copies, where):
    """the same long collinear fragment (chain score well above 255) planted several times: equal high scores, placed at
    the start / end / anywhere of the block range so that they fall inside and behind the first bucket's region"""
    m = int(rng.choice([50, 90, 160]))
    dq = np.cumsum(rng.integers(1, 4, m))
    out = []
    for c in range(n_copies):
        b0 = {"start": 3 + 40 * c, "end": n_block - 400 + 40 * c, "any": int(rng.integers(0, n_block - 100))}[where]
        jitter = 0 if rng.random() < 0.6 else int(rng.integers(0, 2))
        x = (b0 + (dq * 3) // 256).astype(np.uint64)
        out.append((x << np.uint64(32)) | (10 + jitter + dq).astype(np.uint64))
    return np.concatenate(out)


def refine_anchors(rng, n):
    """base-resolution anchors of a refinement window (kmer 5, bbit 0): a collinear run with frame shifts and jumps"""
    dq = np.cumsum(rng.integers(1, 9, n))
    x = 1000 + dq * 3 + (rng.choice([0, 0, 1, -1, 300, 5000], n) * (rng.random(n) < 0.1)).cumsum()
    return np.unique((x.astype(np.uint64) << np.uint64(32)) | (20 + dq).astype(np.uint64))


# ---------------------------------------------------------------- building blocks (blocks relative to the unit's slot)
def pack(blk, q):
    return (np.asarray(blk).astype(U) << U(32)) | np.asarray(q).astype(U)


def collinear(n, step=6, q0=10):
    """n anchors with a query step of `step` residues along the diagonal"""
    dq = step * np.arange(1, n + 1)
    return pack((dq * 3) // 256, q0 + dq)


def collinear_scores(n, step=6, kmer=6):
    """chain scores of collinear(n, step): every anchor links to the one before it -- min(kmer, step), + 2 inside a block"""
    blk = (step * np.arange(1, n + 1) * 3) // 256
    gain = min(kmer, step) + 2 * (blk[1:] == blk[:-1])
    return np.concatenate([[kmer], kmer + np.cumsum(gain)]).astype(np.int64)


def fragment(rng, m):
    """m anchors of one block with rising query positions: one chain, m - 1 chain ends"""
    return pack(np.zeros(m, np.int64), int(rng.integers(5, 400)) + np.cumsum(rng.integers(1, 9, m)))


def twin_fragment(rng, m):
    """a fragment and its copy a block away, shifted by three residues: the copy's first anchor hangs on the original"""
    q = int(rng.integers(5, 400)) + np.cumsum(rng.integers(4, 9, m))
    return np.concatenate([pack(np.zeros(m, np.int64), q), pack(np.ones(m, np.int64), q + 3)])


def trunk_tree(n_trunk, n_leaf):
    """ONE predecessor tree with n_trunk - 1 + n_leaf chain ends: a trunk in block 0 (query step 8: 8 points per anchor) and leaves in
    block 1, two residues behind every second trunk anchor (2 points: no block bonus across blocks).  A leaf cannot be anybody's
    predecessor -- the trunk lies in front of it in sorted order, the next leaf prefers the trunk -- and scores between its trunk anchor
    and the next one: near-equal scores in one tree."""
    assert 2 * (n_leaf - 1) <= n_trunk - 1
    return np.concatenate([pack(np.zeros(n_trunk, np.int64), 20 + 8 * np.arange(n_trunk)), pack(np.ones(n_leaf, np.int64), 20 + 16 * np.arange(n_leaf) + 2)])


def drop_chain(n_good, n_bad, n_tail):
    """a collinear chain with n_bad links that cost about 89 points each in the middle (two blocks on for one residue: a gap of 253 nt).
    With a tail long enough to outscore the front, the best chain end is the last anchor, and its walk back crosses the expensive links"""
    bad = np.zeros(n_good + n_bad + n_tail, bool)
    bad[n_good:n_good + n_bad] = True
    dq = np.cumsum(np.where(bad, 1, 6))
    return pack((dq * 3) // 256 + 2 * np.cumsum(bad), 10 + dq)


def at_slot(unit, slot):
    return unit + (U(BASE + slot * SLOT) << U(32))


def roots(rng, k, slot0=0):
    """k lone anchors, one per slot from slot0 on"""
    return pack(BASE + (slot0 + np.arange(k)) * SLOT, rng.integers(5, 900, k))


def mix(rng, units, n_roots, where):
    """the units next to each other at the start / the end / anywhere of a range of n_roots lone anchors"""
    cut = {"start": 0, "end": n_roots, "any": int(rng.integers(0, n_roots + 1))}[where]
    parts = [roots(rng, cut)] + [at_slot(u, cut + i) for i, u in enumerate(units)] + [roots(rng, n_roots - cut, cut + len(units))]
    return np.unique(np.concatenate(parts))


def scatter(rng, units, n_roots):
    """the units spread at random among n_roots lone anchors"""
    slots = rng.permutation(len(units) + n_roots)
    parts = [at_slot(u, int(s)) for u, s in zip(units, slots)] + [pack(BASE + slots[len(units):] * SLOT, rng.integers(5, 900, n_roots))]
    return np.unique(np.concatenate(parts))


def ends_among_roots(rng, n_ends, n_roots):
    """fragments of 2..4 anchors with n_ends chain ends in all, each a tree of its own, among lone roots"""
    units, left = [], n_ends
    while left > 0:
        m = min(int(rng.integers(1, 4)), left)
        units.append(fragment(rng, m + 1))
        left -= m
    return scatter(rng, units, n_roots)


def exactly(rng, n):
    """a problem of exactly n anchors: dense blocks, a sparse background with planted fragments, or in between"""
    kind = int(rng.integers(0, 3))
    a = _anchors(rng, 3 * n + 20, [40, 3000000, 600][kind], 300, 6)
    return np.sort(rng.choice(a, n, replace=False))


def level1_bucket(rng, size, where, n_roots=300):
    """parallel copies of a collinear chain whose ends score in 256..511 -- `size` of them in all, the one level-1 bucket of the problem;
    where = "start": every one of them is found in region 0 and displaces a lone (absent) root from the bucket's slots behind c0"""
    sc = collinear_scores(80)
    full = int((sc <= 511).sum())                             # the longest chain that stays below 512
    per = int(((sc >= 256) & (sc <= 511)).sum())
    units, left = [], size
    while left > 0:
        c = min(per, left)
        units.append(collinear(full - (per - c)))
        left -= c
    return mix(rng, units, n_roots, where)


def filler(rng):
    k = int(rng.integers(0, 6))
    if k == 0:
        return np.zeros(0, U)
    if k == 1:
        return _anchors(rng, 1, 1000, 100, 0)[:1]
    return _anchors(rng, int(rng.choice([30, 70, 150, 400])), int(rng.choice([40, 2000])), 200, 3)


def launch(rng, probs, tags=None, n_fill=6):
    """one launch: the problems and a few fillers (empty, one anchor, small mixes), shuffled; tags follow their problems.  n_fill < 0: empty
    problems only (for parameters under which a sparse view is exact only if it leaves nothing out)"""
    probs = list(probs)
    tags = list(tags) if tags is not None else [None] * len(probs)
    for _ in range(max(n_fill, 0)):
        probs.append(filler(rng)), tags.append(None)
    probs += [np.zeros(0, U), _anchors(rng, 1, 1000, 100, 0)[:1] if n_fill >= 0 else np.zeros(0, U)]
    tags += [None, None]
    order = rng.permutation(len(probs))
    return [np.ascontiguousarray(probs[i], dtype=U) for i in order], [tags[i] for i in order]


N_TOTALS = (0, 1, 2, 63, 64, 65, 66, 127, 128, 129, 130)     # (a)
N_ENDS = (1, 2, 63, 64, 65, 127, 128, 129)                   # (b)
TREE_ENDS = (2, 63, 64, 65)                                  # (c)
BUCKETS = (255, 256, 257, 600)                               # (g)
BOTH = ((PRE, (DENSE, SPARSE_SET, SPARSE_CHAINS)), (MAIN, (DENSE, SPARSE_CHAINS)))


def _with(args, **kw):
    names = ("max_dist_x", "max_dist_y", "bw", "max_skip", "max_iter", "min_cnt", "min_sc", "coef_log", "is_spliced", "kmer", "bbit")
    out = list(args)
    for k, v in kw.items():
        out[names.index(k)] = v
    return out


@functools.lru_cache(maxsize=None)
def cases():
    """[{name, family, probs, tags, runs: ((args, modes), ...)}]; deterministic"""
    out = []

    def add(name, seed, build, runs=BOTH, n_fill=6):
        rng = np.random.default_rng(seed)
        probs, tags = build(rng)
        probs, tags = launch(rng, probs, tags, n_fill)
        out.append({"name": name, "family": name[0], "probs": probs, "tags": tags, "runs": tuple((tuple(a), tuple(m)) for a, m in runs)})

    # (a) n_total at the n <= 64 switch and at the 64-lane group edges
    add("a_n_total", 101, lambda rng: ([exactly(rng, n) for n in N_TOTALS for _ in range(3)], [("n_total", n) for n in N_TOTALS for _ in range(3)]))
    # (b) chain ends, each in a tree of its own, among lone roots: the last group of the extraction loop is partial
    add("b_ends", 102, lambda rng: ([ends_among_roots(rng, k, int(rng.integers(200, 400))) for k in N_ENDS], [("ends", k) for k in N_ENDS]))

    # (c) one tree holding 2 / 63 / 64 / 65 chain ends (lanes of one group contend for owner[root]); the tree again two slots on (equal
    # scores across trees); 64 ends in 64 trees (nobody contends)
    def fam_c(rng):
        probs, tags = [], []
        for k in TREE_ENDS:
            n_leaf = (k + 1) // 3
            tree = trunk_tree(k - n_leaf + 1, n_leaf)
            probs.append(scatter(rng, [tree], 200)), tags.append(("tree", k))
            probs.append(scatter(rng, [tree, tree, twin_fragment(rng, 9)] + [fragment(rng, 3) for _ in range(5)], 260)), tags.append(("tree", k))
        probs.append(scatter(rng, [fragment(rng, 2) for _ in range(64)], 220)), tags.append(("ends", 64))
        probs.append(_anchors(rng, 300, 50, 300, 20)), tags.append(None)          # dense: a few large trees with many ties
        return probs, tags
    add("c_trees", 103, fam_c)

    # (d) equal scores in bulk: one fragment (and its copy a block away) 300 times -- every shift-0 digit it reaches holds 300 ends
    def fam_d(rng):
        one, two = fragment(rng, 10), twin_fragment(rng, 8)
        return [scatter(rng, [one] * 300, 100), scatter(rng, [two] * 300 + [fragment(rng, 12)] * 20, 500), scatter(rng, [fragment(rng, 9)] * 310, 0)], [("bulk", 300)] * 3
    add("d_bulk_ties", 104, fam_d)

    # (e) two digit levels: chains of 40 / 100 / 300 anchors alone and among lone roots, at the start / end / anywhere
    def fam_e(places, sizes):
        def build(rng):
            probs = [mix(rng, [collinear(n)] * int(rng.integers(1, 4)), bg, w) for n in (40, 100, 300) for bg in sizes for w in places]
            return probs, [("two_level", None)] * len(probs)
        return build
    add("e_two_levels_small", 105, fam_e(("start", "end", "any"), (0, 40)))
    add("e_two_levels_3000", 106, fam_e(("start", "end", "any"), (3000,)), n_fill=3)
    add("e_two_levels_20000", 107, fam_e(("start", "end", "any"), (20000,)), n_fill=3)

    # (e, continued) the team merge of the moved and the low list: long chains in FRONT of region 0's end, dense clusters behind it -- the
    # high chain ends found in region 0 displace chained low-score anchors from the bucket heads behind c0 into the holes they leave.  The
    # clusters are large trees full of equal scores: where a moved anchor ends up among its equals decides which chain claims a shared
    # anchor (ends of different trees may change places without a trace)
    def fam_e_moved(rng):
        probs = []
        for k in range(8):
            chains = [collinear(int(rng.choice([100, 150, 300]))) for _ in range(int(rng.integers(2, 6)))]
            hot = [_anchors(rng, int(rng.choice([200, 300, 500])), int(rng.choice([20, 40])), 300, 30) for _ in range(2)]
            n_roots = int(rng.integers(0, 300)) if k % 2 == 0 else 30
            units = chains + ([None, hot[0], hot[1]] if k % 2 == 0 else [hot[0], None, hot[1]] + [twin_fragment(rng, int(rng.integers(4, 12))) for _ in range(50)])
            parts, slot = [], 0
            for u in units:
                parts.append(roots(rng, n_roots, slot) if u is None else at_slot(u, slot))
                slot += n_roots if u is None else 1
            probs.append(np.unique(np.concatenate(parts)))
        return probs, [("moved", None)] * len(probs)
    add("e_moved_lows", 118, fam_e_moved)

    # (f) bucket 0 of 64 slots or fewer with n_total > 64 (insertion-sorted), and c0 = 63 .. 66
    def fam_f(rng):
        probs = [collinear(n) for n in (100, 150, 200, 250, 300)]
        tags = [("c0", None)] * 5
        for c0 in (63, 64, 65, 66):
            n = int(rng.choice([120, 180]))
            low = int((collinear_scores(n) < 256).sum())
            probs.append(mix(rng, [collinear(n)], c0 - low, str(rng.choice(["start", "end", "any"])))), tags.append(("c0", c0))
        return probs, tags
    add("f_short_bucket0", 108, fam_f)

    # (g) one level-1 bucket of exactly 255 / 256 / 257 / 600 ends (the team's LDS staging holds 256), and a few more on either side
    def fam_g(rng):
        sizes = [(s, w) for s in BUCKETS for w in ("start", "end")] + [(300, "any"), (400, "any"), (513, "any"), (1000, "any"), (200, "any"), (100, "start")]
        return [level1_bucket(rng, s, w) for s, w in sizes], [("bucket", s) for s, w in sizes]
    add("g_level1_bucket", 109, fam_g)

    # (h) max_f >= 65536: the full list -- it fits a dense view and a sparse one that leaves out no more than 64 anchors; beyond, the
    # kernel declines the problem (status 1) and its neighbours are unaffected
    def fam_h(rng):
        probs = [mix(rng, [collinear(8500)], 0, "start"), mix(rng, [collinear(8800)], 30, "any"), mix(rng, [collinear(9000)], 70, "end"), mix(rng, [collinear(8600)], 200, "any")]
        tags = [("max_f", "fits"), ("max_f", "fits"), ("max_f", "declined"), ("max_f", "declined")]
        probs += [mix(rng, [collinear(100)], 300, "any"), ends_among_roots(rng, 70, 210), exactly(rng, 65)]
        return probs, tags + [None] * 3
    add("h_max_f", 110, fam_h)

    # (i) the same decline from the parameters: min_cnt 1 and min_sc = kmer + 1 on sparse views that leave out more than 64 anchors; the
    # full list where it fits (min_sc: up to 64 lone roots left out; min_cnt 1: a view that leaves nothing out -- otherwise the sparse
    # view is not exact, chain_core.h); min_cnt x min_sc on dense views
    def fam_i_sparse(rng):
        probs, tags = [], []
        for _ in range(4):
            probs.append(ends_among_roots(rng, int(rng.integers(5, 90)), int(rng.integers(70, 300)))), tags.append(("params", "declined"))
        for _ in range(7):
            blk = np.repeat(np.arange(int(rng.integers(20, 60))), 5)
            probs.append(np.unique(pack(blk, rng.integers(5, 300, len(blk))))), tags.append(("params", "all_in_view"))
        return probs, tags
    add("i_min_cnt_sparse", 111, fam_i_sparse, runs=((_with(PRE, min_cnt=1), (SPARSE_SET, SPARSE_CHAINS, DENSE)),), n_fill=-1)

    def fam_i_min_sc(rng):
        probs, tags = [], []
        for _ in range(4):
            probs.append(ends_among_roots(rng, int(rng.integers(5, 90)), int(rng.integers(70, 300)))), tags.append(("params", "declined"))
        for _ in range(7):
            probs.append(ends_among_roots(rng, int(rng.integers(40, 130)), int(rng.integers(0, 64)))), tags.append(("params", "fits"))
        return probs, tags
    add("i_min_sc_sparse", 112, fam_i_min_sc, runs=((_with(PRE, min_sc=7), (SPARSE_SET, SPARSE_CHAINS, DENSE)), (_with(MAIN, min_sc=7), (SPARSE_CHAINS,))))

    def fam_i_dense(rng):
        probs = [exactly(rng, n) for n in (30, 64, 65, 200)] + [_anchors(rng, 300, 50, 300, 20), mix(rng, [collinear(100), twin_fragment(rng, 10)], 100, "any"),
                                                              ends_among_roots(rng, 70, 100), scatter(rng, [trunk_tree(44, 22), fragment(rng, 4)], 80)]
        return probs, [None] * len(probs)
    add("i_dense_params", 113, fam_i_dense, runs=tuple((_with(base, min_cnt=c, min_sc=s), (DENSE,)) for c in (1, 2, 3, 4) for s in (0, 6, 7, 20) for base in ((PRE, MAIN)[(c + s) % 2],)))

    # (j) no splicing and a band narrower than the drop across four expensive links: the walk back breaks off at best_suffix - sfx > max_drop
    def fam_j(rng):
        probs = [mix(rng, [drop_chain(60, 4, 60)], 100, "any"), mix(rng, [drop_chain(70, 5, 75), collinear(50)], 30, "start"), scatter(rng, [drop_chain(55, 4, 58)] * 3, 150),
                 _anchors(rng, 300, 50, 300, 20), _anchors(rng, 3000, 3000, 300, 20)]
        return probs, [("drop", None)] * 3 + [None, None]
    unspliced = _with(MAIN, bw=300, is_spliced=0)
    add("j_max_drop", 114, fam_j, runs=((unspliced, (DENSE, SPARSE_CHAINS)), (_with(unspliced, is_spliced=1), (DENSE, SPARSE_CHAINS)), (_with(PRE, is_spliced=0), (SPARSE_SET, DENSE))))

    # (k) the refinement's shape: base resolution, kmer 5
    def fam_k(rng):
        probs = [refine_anchors(rng, n) for n in (5, 64, 65, 80, 600) for _ in range(3)]
        return probs, [("refine", None)] * len(probs)
    refine = [200000, 1000, 200000, 25, 1000000, 3, 0, 0.75, 1, 5, 0]
    add("k_refine", 115, fam_k, runs=((refine, (DENSE,)), (_with(refine, max_skip=2, is_spliced=0), (DENSE,))))

    # (l) the random mixes of tests/test_host_core.py, backgrounds capped at 20 000 anchors
    def fam_l(n_kinds, count):
        def build(rng):
            probs = []
            for it in range(count):
                kind = it % n_kinds
                if kind == 0:
                    a = _anchors(rng, int(rng.choice([70, 500, 5000, 20000])), 3000000, 400, int(rng.choice([0, 3, 40])))
                elif kind == 1:
                    a = _anchors(rng, int(rng.choice([65, 300, 3000])), int(rng.choice([50, 400, 3000])), 300, 20)
                elif kind == 2:
                    a = _anchors(rng, 2000, 3000000, 400, 0)
                    hot = _anchors(rng, 300, 40, 300, 30) + (np.uint64(0 if rng.random() < 0.5 else 2999000) << np.uint64(32))
                    a = np.unique(np.concatenate([a, hot]))
                elif kind == 4:
                    bg = _anchors(rng, int(rng.choice([0, 40, 3000, 20000])), 3000000, 900, int(rng.choice([0, 30])))
                    a = np.unique(np.concatenate([bg, _long_chains(rng, 3000000, int(rng.integers(1, 5)), str(rng.choice(["start", "end", "any"])))]))
                elif kind == 5:
                    m = int(rng.choice([60, 150]))
                    dq = np.cumsum(rng.integers(1, 4, m))
                    x = (5000 + (dq * 3) // 256).astype(np.uint64)
                    a = np.unique(np.concatenate([_anchors(rng, 3000, 3000000, 900, 5), (x << np.uint64(32)) | (10 + dq).astype(np.uint64)]))
                else:
                    a = _anchors(rng, int(rng.choice([0, 1, 30, 64, 65, 66])), 2000, 200, 3)
                probs.append(a)
            return probs, [None] * count
        return build
    add("l_mix_chains", 116, fam_l(5, 30), runs=((PRE, (DENSE,)), ([200000, 1000, 200000, 25, 50, 3, 0, 0.75, 0, 6, 8], (DENSE, SPARSE_CHAINS)), (_with(PRE, min_cnt=4, min_sc=20), (DENSE,))), n_fill=2)
    add("l_mix_prechain", 117, fam_l(6, 36), runs=((PRE, (SPARSE_SET, SPARSE_CHAINS)), (_with(PRE, max_iter=20), (SPARSE_SET,))), n_fill=2)
    return out


def case(name):
    return next(c for c in cases() if c["name"] == name)


# ---------------------------------------------------------------- the expected chains: the oracle, once per (case, parameters)
_expected = {}


def expected(c, args):
    """[(u, a)] of the oracle's mp_chain (oracle/chain_oracle.c, which tests/test_oracle.py pins to the reference) for every problem"""
    import ctypes as C
    import refbind
    key = (c["name"], tuple(args))
    if key not in _expected:
        o = refbind.ora()
        res = []
        for p in c["probs"]:
            a = p.copy()
            u = np.zeros(len(a) + 1, U)
            no = C.c_int64(0)
            nu = o.mpo_chain(*args, len(a), a.ctypes.data, u.ctypes.data, C.byref(no))
            res.append((u[:nu].copy(), a[:no.value].copy()))
        _expected[key] = res
    return _expected[key]


def check_against(c, args, mode, got, want, label):
    """the assertions both files make on one launch: chains bit for bit (the set: the chains' anchors, ascending); a problem whose path
    record says DECLINED has status 1 and no output -- that is asserted, and such a problem is neither compared nor counted.  Returns the
    number of problems compared.  The set is compared with the oracle at the run's own parameters: the pre-chain's min_cnt 2, min_sc 0
    everywhere but in (i), which passes its own on to see the full list built from a sparse view, or declined."""
    us, as_, status, rec = got
    n_checked = 0
    for q, (wu, wa) in enumerate(want):
        where = (label, c["name"], q, c["tags"][q], len(c["probs"][q]), list(args), mode, [int(x) for x in rec[q]])
        assert rec[q][0] <= rec[q][1] == len(c["probs"][q]), where
        if rec[q][4] == 3:                                    # DECLINED
            assert status[q] == 1 and len(us[q]) == 0 and len(as_[q]) == 0, where
            continue
        assert status[q] == 0, where
        if mode == SPARSE_SET:
            assert len(us[q]) == 0 and np.array_equal(as_[q], np.sort(wa)), where
        else:
            assert np.array_equal(us[q], wu), where
            assert np.array_equal(as_[q], wa), where
        n_checked += 1
    return n_checked
