"""Helpers of the MPA_DP_HUGE_WG tests (tests/test_ext_huge_wg_cpu.py, tests/test_ext_huge_wg_gpu.py): X_HUGE extension calls swept by
k_ext_huge_wg, one wave per 64-column block and W waves per workgroup (miniprot_amd/csrc/ext_huge_wg_core.h), instead of the one-wave
kernel.  Small X_HUGE calls, the tables of the GPU tests with the block counts the tests name, and what mpa_dbg_dp_last_huge must report
for a table by the rule of the two kernels.

How to get small X_HUGE calls: the planner's int16 guard is al * max_mat + ncol * ge + end_bonus > 32000 (dp_plan_core.h).  The default
matrix with the W:W score raised to 127 ("hot") puts every extension call of al >= 250 on X_HUGE while go / ge stay the defaults, so that
gap runs do cross block boundaries.  250 residues are four blocks already, and no matrix (int8) or end bonus (at most 1 000) the
library accepts lowers that: the guard cannot put a call of one or three blocks on X_HUGE while go / ge stay the defaults.  The calls of
one and three blocks the tests need (the ones that must STAY on the one-wave kernel in the same launch) are therefore X_HUGE by the
other rule of the planner: a frameshift penalty above 255 (fs = 300, go / ge the defaults) puts EVERY extension call on X_HUGE, swept by
the kernels' <true> instantiations.  Every expectation is the oracle's, and tests/test_ext_huge_wg_cpu.py checks oracle == reference on
every call of every table."""
import os
import numpy as np
import miniprot_amd as mpa
import dpplan
import refbind
import splitwide as sw
from dpgen import make_task, back_translate
from dputil import dpopt_from_params, compare

WIDE_KW = dict(p_intron=0.004, max_intron=200, flank=30)            # rows = 3 al + a few short introns
BOTH = ("left", "right")
WIDE_FS = 300               # -F above 255: every extension call is X_HUGE
AA = b"ARNDCQEGHILKMFPSTWYV*X"


def info():
    """(W, R, MIN_BLOCKS) of the kernel's schedule, from the library"""
    return mpa.dbg_dp_huge_wg_info()


def hot_matrix(fs=23):
    m = refbind.mapping_matrix(fs).copy()
    w = AA.index(b"W")
    m[w, w] = 127
    return m


def hot_params(**kw):
    return refbind.DpParams(hot_matrix(min(kw.get("fs", 23), 127)), **kw)


def default_params(**kw):
    return refbind.DpParams(refbind.mapping_matrix(min(kw.get("fs", 23), 127)), **kw)


def n_blocks(al):
    return ((al + 7) // 8 * 8 + 63) // 64


def block_als(nblk, guard=0):
    """a call whose last block is full and one whose last block is partial and has padded columns (64 k - 9; where the guard that makes
    the call X_HUGE admits that many residues, the first al beyond it: under the hot matrix 250 for four blocks, whose eighth column
    group is padded; the 247-residue call is in below_min_table())"""
    return (64 * nblk, max(64 * nblk - 9, guard + 1))


class knob:
    """MPA_DP_HUGE_WG in the environment while a context is created (it is read then); MPA_DP_SPLIT_WIDE is unset meanwhile"""

    def __init__(self, value="1"):
        self.value = value

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in ("MPA_DP_HUGE_WG", "MPA_DP_SPLIT_WIDE")}
        os.environ.pop("MPA_DP_SPLIT_WIDE", None)
        if self.value is None:
            os.environ.pop("MPA_DP_HUGE_WG", None)
        else:
            os.environ["MPA_DP_HUGE_WG"] = self.value

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


class Table(sw.Table):
    """splitwide.Table (pairs under the parameters P as one mpa.dp_run batch, the oracle's and the reference's results computed once)
    with the X_HUGE calls the test names: huge_blocks, the block count of every extension call that must be X_HUGE, in task order"""

    def huge_als(self, knobs=None):
        kn = dict(dpplan.KNOBS)
        kn.update(knobs or {})
        return [al for al in self.ext_als() if sw.expected_class(al, self.opt, kn) == sw.X_HUGE]

    def huge_blocks(self, knobs=None):
        return [n_blocks(al) for al in self.huge_als(knobs)]

    def plan(self, knobs=None):
        """the host planner on this very table (mpa_dbg_dp_plan) -> dpplan.Plan"""
        kn = dict(dpplan.KNOBS)
        kn.update(knobs or {})
        q_off = np.concatenate([[0], np.cumsum([len(aa) for _, aa in self.pairs])]).astype(np.int64)
        r = mpa.dbg_dp_plan(self.opt, [len(c) for c in self.contigs], q_off, self.tasks, kn)
        return r if isinstance(r, tuple) else dpplan.Plan(r)


def expected_last_huge(blocks, knob_on):
    """what mpa_dbg_dp_last_huge reports for X_HUGE calls of these block counts: (on one wave, on workgroups, blocks, passes)"""
    W, _, MIN_BLOCKS = info()
    wg = [b for b in blocks if knob_on and b >= MIN_BLOCKS]
    return (len(blocks) - len(wg), len(wg), sum(wg), sum((b + W - 1) // W for b in wg))


def results(ctx, tab):
    idx = mpa.Index.from_nt4(tab.contigs)
    idx.to_device(ctx)
    try:
        return mpa.dp_run(ctx, idx, tab.opt, tab.queries, tab.tasks)
    finally:
        idx.close()


def fields(rst):
    return [(int(r["nt_len"]), int(r["aa_len"]), int(r["score"])) for r in rst]


def run(ctx, tab, knob_on, want_blocks, what="", knobs=None):
    """the table on the context: the hook's counts against the rule and against the block counts the test names (sorted), then every
    call's values against the oracle and, where it is built, the reference.  -> the result records"""
    rst, cig = results(ctx, tab)
    got = mpa.dbg_dp_last_huge(ctx)
    assert sorted(tab.huge_blocks(knobs)) == sorted(want_blocks), "%s: the test names blocks %s, the table has %s" % (what, sorted(want_blocks), sorted(tab.huge_blocks(knobs)))
    assert got == expected_last_huge(want_blocks, knob_on), "%s: mpa_dbg_dp_last_huge %s, expected %s" % (what, got, expected_last_huge(want_blocks, knob_on))
    for which in ("oracle", "reference") if refbind.have_ref() else ("oracle",):
        bad, msg = compare(rst, cig, tab.expect(which), tab.meta, tab.pairs)
        assert not bad, "%s: %d/%d DP calls differ from the %s (huge calls %s)\n%s" % (what, len(bad), len(tab.tasks), which, got, msg)
    return rst


# ---- the tables of the GPU tests, built once per process
def _once(key, make):
    return sw._once(("hugewg",) + key, make)


def block_count_nblks():
    W, _, MIN_BLOCKS = info()
    return sorted({MIN_BLOCKS, W - 1, W, W + 1, 2 * W, 2 * W + 1})


def block_count_table():
    """test 1: hot matrix, left and right extensions of every block count at and above MIN_BLOCKS, a full and a partial last block each"""
    def make():
        rng = np.random.default_rng(9600)
        als = [al for nb in block_count_nblks() for al in block_als(nb, sw.guard_limit(dpopt_from_params(hot_params())))]
        return Table(hot_params(), [sw.wide_pair(rng, al, **WIDE_KW) for al in als], 9601), [n_blocks(al) for al in als for _ in BOTH]
    return _once(("blocks",), make)


def below_min_table():
    """test 1, the call of MIN_BLOCKS - 1 blocks that stays on one wave, with calls of MIN_BLOCKS blocks in the same launch"""
    def make():
        MIN_BLOCKS = info()[2]
        rng = np.random.default_rng(9610)
        als = list(block_als(MIN_BLOCKS - 1)) + list(block_als(MIN_BLOCKS))
        return Table(hot_params(fs=WIDE_FS), [sw.wide_pair(rng, al, **WIDE_KW) for al in als], 9611), [n_blocks(al) for al in als for _ in BOTH]
    return _once(("below_min",), make)


def row_count_nblks():
    W = info()[0]
    return (4, W + 1, 2 * W + 3)


def row_counts():
    W, R, _ = info()
    return (3, 4, R + 1, R + 2, R + 3, 2 * R + 2, (W - 1) * R + 1, W * R + 3)


def row_count_table(nblk, rows=None):
    """test 2: windows of a call of nblk blocks cut to `rows` rows each (default: row_counts(): a lone DP row, both sides of a chunk
    edge, a pipeline that never fills and one that just does)"""
    rows = tuple(rows if rows is not None else row_counts())

    def make():
        rng = np.random.default_rng(9620 + nblk)
        al = block_als(nblk, sw.guard_limit(dpopt_from_params(hot_params())))[1]
        mode = ("right",) if nblk % 2 else ("left",)
        return Table(hot_params(), [sw.wide_pair(rng, al, rows=r, **WIDE_KW) for r in rows], 9621 + nblk, modes=mode), [nblk] * len(rows)
    return _once(("rows", nblk, rows), make)


def mixed_table():
    """test 3: X_HUGE calls of 4, W + 1 and 2 W + 1 blocks (hot matrix) and 40 ordinary pairs, whose calls are in the packed classes and
    the traceback kernels, in one batch"""
    def make():
        W = info()[0]
        rng = np.random.default_rng(9630)
        nblks = (4, W + 1, 2 * W + 1)
        huge = [sw.wide_pair(rng, 64 * nb - 1, **WIDE_KW) for nb in nblks]
        small = [make_task(rng) for _ in range(40)]
        assert max(len(aa) for _, aa in small) < 250
        tab = Table(hot_params(), huge + small, 9631, pair_modes=[BOTH] * len(huge) + [sw.ALL_MODES] * len(small))
        return tab, [nb for nb in nblks for _ in BOTH]
    return _once(("mixed",), make)


def mixed_wide_fs_table():
    """test 3 with the calls of 1 and 3 blocks: fs = 300, X_HUGE calls of 1, 3, 4, W + 1 and 2 W + 1 blocks and 40 ordinary pairs of at
    most three blocks (their extension calls are X_HUGE too, and stay on one wave) in one batch"""
    def make():
        W = info()[0]
        rng = np.random.default_rng(9635)
        nblks = (1, 3, 4, W + 1, 2 * W + 1)
        huge = [sw.wide_pair(rng, 64 * nb - 1, **WIDE_KW) for nb in nblks]
        small = [make_task(rng, al=int(rng.integers(8, 190))) for _ in range(40)]
        tab = Table(default_params(fs=WIDE_FS), huge + small, 9636, pair_modes=[BOTH] * len(huge) + [sw.ALL_MODES] * len(small))
        return tab, tab.huge_blocks()
    return _once(("mixed_wide_fs",), make)


def gap_pair(rng, al, flank=20, p_sub=0.1):
    """a window that encodes a random protein of al residues with a gap planted at every block boundary: at the even multiples of 64
    the five residues [64 b - 3, 64 b + 2) have no codons in the window (a run of the I state across the boundary: bin.x, bin.y and the
    I fields of the record), at the odd ones four random codons stand in the window in front of column 64 b (a D run at the boundary)"""
    prot = bytes(rng.choice(list(b"ARNDCQEGHILKMFPSTWYV"), al).tolist())
    nt, k = [], 0
    while k < al:
        b = (k + 3) // 64
        if (k + 3) % 64 == 0 and b % 2 == 0 and k + 5 <= al:
            k += 5
            continue
        if k % 64 == 0 and (k // 64) % 2 == 1:
            nt += list(rng.integers(0, 4, 12))
        ch = prot[k:k + 1] if rng.random() >= p_sub else bytes(rng.choice(list(b"ARNDCQEGHILKMFPSTWYV"), 1).tolist())
        nt += list(back_translate(ch, rng))
        k += 1
    nt = list(rng.integers(0, 4, flank)) + nt + list(rng.integers(0, 4, flank))
    return bytes(np.array(nt, dtype=np.uint8)), prot


def gaps_table():
    """gap runs that cross block boundaries, the boundary between two passes (column 64 W, through HBM) among them: a call of
    2 W + 1 blocks, left and right"""
    def make():
        W = info()[0]
        rng = np.random.default_rng(9680)
        al = 64 * (2 * W + 1) - 9
        tab = Table(hot_params(), [gap_pair(rng, al)], 9681)
        return tab, [n_blocks(al) for _ in BOTH]
    return _once(("gaps",), make)


def xdrop_table():
    """test 4: x-drop 30 and end bonus 11 with flanks of 2 000 random bases: the best row lies early, the sweep still runs every row"""
    def make():
        W = info()[0]
        rng = np.random.default_rng(9640)
        als = (64 * (W + 1), 600)
        tab = Table(hot_params(xdrop=30, end_bonus=11), [sw.wide_pair(rng, al, p_intron=0.004, max_intron=200, flank=2000) for al in als], 9641)
        return tab, [n_blocks(al) for al in als for _ in BOTH]
    return _once(("xdrop",), make)


def saturating_table():
    """test 5: the two pairs of test_extension_that_saturates_int16 -- past the default guard (52 blocks), and an identical pair whose
    score runs into the int16 ceiling (107 blocks)"""
    def make():
        rng = np.random.default_rng(17)
        pairs = [make_task(rng, al=3300, p_indel=0.001, flank=50), make_task(rng, al=6800, p_indel=0.0, p_sub=0.0, p_intron=0.0, p_fs=0.0, p_n=0.0, flank=40)]
        tab = Table(default_params(), pairs, 9651, modes=("right", "left"))
        return tab, tab.huge_blocks()
    return _once(("saturating",), make)


def wide_ge_table():
    """test 6: -E 300 (every extension call is X_HUGE, swept by the kernels' <true> instantiations); columns x ge stays below 2^19"""
    def make():
        rng = np.random.default_rng(9660)
        als = (300, 1000, 1600, 40)
        tab = Table(default_params(ge=300), [sw.wide_pair(rng, al, **WIDE_KW) for al in als], 9661)
        return tab, [n_blocks(al) for al in als for _ in BOTH]
    return _once(("wide_ge",), make)


RETRY_ALS = (300, 513, 700, 1000, 40, 90)


def retry_table():
    """test 7: 512- / 1 024-column calls (X_SPLIT2 / X_SPLIT4) that a repeated round (no_split) puts on X_HUGE, and two narrow ones"""
    def make():
        rng = np.random.default_rng(9670)
        tab = Table(default_params(), [sw.wide_pair(rng, al, p_intron=0.004, max_intron=200, flank=600) for al in RETRY_ALS], 9671)
        return tab, [n_blocks(al) for al in RETRY_ALS if al > 256 for _ in BOTH]
    return _once(("retry",), make)


def all_tables():
    """(id, maker -> (Table, block counts of its X_HUGE calls), planner knobs under which they are X_HUGE) of every table the GPU tests run"""
    out = [("blocks", block_count_table, {}), ("below_min", below_min_table, {}), ("mixed", mixed_table, {}), ("mixed_wide_fs", mixed_wide_fs_table, {}), ("xdrop", xdrop_table, {}), ("gaps", gaps_table, {}),
           ("saturating", saturating_table, {}), ("wide_ge", wide_ge_table, {}), ("retry", retry_table, dict(no_split=1))]
    out += [("rows-%d" % nb, lambda nb=nb: row_count_table(nb), {}) for nb in row_count_nblks()]
    out += [("two-rows-%d" % nb, lambda nb=nb: row_count_table(nb, (2,)), {}) for nb in row_count_nblks()]
    return out
