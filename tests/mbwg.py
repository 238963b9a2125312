"""Helpers of the MPA_DP_MB_WG tests (tests/test_glob_mb_wg_cpu.py, tests/test_glob_mb_wg_gpu.py): traceback calls of more than 1 024
columns (class T_MB) swept by k_glob_mb_wg, one wave per 64-column block and W waves per workgroup on the schedule of
miniprot_amd/csrc/ext_huge_wg_core.h, instead of one wave per call (glob_narrow<64, true> in the round kernel or k_glob_narrow).  The
tables of the GPU tests with the block counts the tests name, and what mpa_dbg_dp_last_mb must report for a table by the rule: every
T_MB call on workgroups with the knob on (all have 17 blocks or more), every one on one wave with it off.

Every expectation is the oracle's, score and CIGAR; tests/test_glob_mb_wg_cpu.py checks oracle == reference on every call of every
table, and that the host planner puts exactly the named calls on T_MB."""
import os
import numpy as np
import miniprot_amd as mpa
import dpplan
import refbind
import hugewg as hw
import splitwide as sw
from dpgen import make_task
from dputil import compare

T_W16, T_MB = 6, 7                                                  # DpClass of a traceback call (dp_device.h)
WIDE_GE = 300                                                       # -E above 255: every launch is a <true> instantiation
CIGAR = ("cigar",)
OP_I, OP_U, OP_V = 1, 12, 13                                        # CIGAR operations (refbind.cigar_str)


def info():
    """(W, R, MIN_BLOCKS) of the schedule: mpa_dbg_dp_huge_wg_info's, there is no second copy"""
    return hw.info()


n_blocks = hw.n_blocks


class knob:
    """MPA_DP_MB_WG in the environment while a context is created (it is read then)"""

    def __init__(self, value="1"):
        self.value = value

    def __enter__(self):
        self.old = os.environ.get("MPA_DP_MB_WG")
        if self.value is None:
            os.environ.pop("MPA_DP_MB_WG", None)
        else:
            os.environ["MPA_DP_MB_WG"] = self.value

    def __exit__(self, *a):
        if self.old is None:
            os.environ.pop("MPA_DP_MB_WG", None)
        else:
            os.environ["MPA_DP_MB_WG"] = self.old


class Table(hw.Table):
    """hugewg.Table with the traceback calls the test names: mb_blocks, the block count of every T_MB call in task order"""

    def mb_als(self):
        return [len(self.pairs[k][1]) for k, fl, _ in self.meta if fl == mpa.F_CIGAR and len(self.pairs[k][1]) > 1024]

    def mb_blocks(self):
        return [n_blocks(al) for al in self.mb_als()]

    def plan_bytes(self, knobs=None):
        """the serialised plan of the host planner on this table (mpa_dbg_dp_plan)"""
        kn = dict(dpplan.KNOBS)
        kn.update(knobs or {})
        q_off = np.concatenate([[0], np.cumsum([len(aa) for _, aa in self.pairs])]).astype(np.int64)
        r = mpa.dbg_dp_plan(self.opt, [len(c) for c in self.contigs], q_off, self.tasks, kn)
        assert not isinstance(r, tuple), r
        return bytes(r)


def expected_last_mb(blocks, knob_on):
    """what mpa_dbg_dp_last_mb reports for T_MB calls of these block counts: (on one wave, on workgroups, blocks, passes)"""
    W = info()[0]
    if not knob_on:
        return (len(blocks), 0, 0, 0)
    return (0, len(blocks), sum(blocks), sum((b + W - 1) // W for b in blocks))


def results(ctx, tab):
    return hw.results(ctx, tab)


def records(rst):
    return [(int(r["nt_len"]), int(r["aa_len"]), int(r["score"]), int(r["n_cigar"])) for r in rst]


def cigars(rst, cig):
    return [[int(x) for x in cig[r["cigar_off"]: r["cigar_off"] + r["n_cigar"]]] for r in rst]


def run(ctx, tab, knob_on, want_blocks, what="", against=("oracle",)):
    """the table on the context: the hook's counts against the rule and against the block counts the test names, then every call's
    score and CIGAR against the oracle (and whatever else `against` names).  -> (records, CIGAR pool)"""
    rst, cig = results(ctx, tab)
    got = mpa.dbg_dp_last_mb(ctx)
    assert sorted(tab.mb_blocks()) == sorted(want_blocks), "%s: the test names blocks %s, the table has %s" % (what, sorted(want_blocks), sorted(tab.mb_blocks()))
    assert got == expected_last_mb(want_blocks, knob_on), "%s: mpa_dbg_dp_last_mb %s, expected %s" % (what, got, expected_last_mb(want_blocks, knob_on))
    for which in against:
        bad, msg = compare(rst, cig, tab.expect(which), tab.meta, tab.pairs)
        assert not bad, "%s: %d/%d DP calls differ from the %s (T_MB calls %s)\n%s" % (what, len(bad), len(tab.tasks), which, got, msg)
    return rst, cig


def same_results(a, b, what=""):
    """records and the CIGAR pool of two contexts"""
    (ra, ca), (rb, cb) = a, b
    assert len(ra) == len(rb) and records(ra) == records(rb), what
    assert cigars(ra, ca) == cigars(rb, cb), what
    assert np.array_equal(np.asarray(ca), np.asarray(cb)), what


# ---- the tables of the GPU tests, built once per process
def _once(key, make):
    return sw._once(("mbwg",) + key, make)


BLOCK_ALS = (1025, 1088, 2048, 2049, 2112, 3100)                    # 17 blocks (the last one 8 columns wide), 17 (full), 32, 33, 33, 49
BLOCK_NBLK = (17, 17, 32, 33, 33, 49)
BLOCK_PASSES = (2, 2, 2, 3, 3, 4)


def block_count_table():
    """traceback calls of BLOCK_ALS residues, rows about 3 al with a few short introns"""
    def make():
        rng = np.random.default_rng(9700)
        return Table(hw.default_params(), [sw.wide_pair(rng, al, **hw.WIDE_KW) for al in BLOCK_ALS], 9701, modes=CIGAR), [n_blocks(al) for al in BLOCK_ALS]
    return _once(("blocks",), make)


ROW_NBLK = (17, 33)


def row_counts():
    return hw.row_counts()


def row_count_table(nblk):
    """windows of a call of nblk blocks cut to row_counts() rows each: a lone DP row, both sides of a chunk edge, a pipeline that never
    fills and one that just does"""
    def make():
        rng = np.random.default_rng(9720 + nblk)
        al = 64 * nblk - (9 if nblk % 2 else 55)                    # 17 blocks: a partial last block; 33: 2 057 residues, one column group in block 32
        assert n_blocks(al) == nblk and al > 1024
        rows = row_counts()
        return Table(hw.default_params(), [sw.wide_pair(rng, al, rows=r, **hw.WIDE_KW) for r in rows], 9721 + nblk, modes=CIGAR), [nblk] * len(rows)
    return _once(("rows", nblk), make)


EDGE_ROWS = (0, 1, 2, 3, 4, 5)


def class_edge_table():
    """windows of 0 .. 5 rows at al = 1 024 (T_W16) and al = 1 025 (T_MB) in one table; the calls of fewer than three rows take the
    contract of include/mpamd.h"""
    def make():
        rng = np.random.default_rng(9730)
        pairs = [sw.wide_pair(rng, al, rows=r, **hw.WIDE_KW) for al in (1024, 1025) for r in EDGE_ROWS]
        return Table(hw.default_params(), pairs, 9731, modes=CIGAR), [17] * len(EDGE_ROWS)
    return _once(("edge",), make)


def gap_boundaries(al):
    """the column boundaries hugewg.gap_pair plants an I run across: 64 b - 1 | 64 b for the even b whose five residues fit the call"""
    return [64 * b for b in range(2, (al + 3) // 64 + 1, 2) if 64 * b + 2 <= al]


def gaps_table():
    """hugewg.gap_pair as traceback calls: I runs planted across every second block boundary, 1 023 | 1 024 (the edge between two passes)
    among them; 33 and 17 blocks"""
    def make():
        W = info()[0]
        rng = np.random.default_rng(9741)                           # (a seed under which every planted run stays across its boundary: the CPU test checks it)
        als = (64 * (2 * W + 1) - 9, 64 * (W + 1) - 20)
        return Table(hw.default_params(), [hw.gap_pair(rng, al) for al in als], 9742, modes=CIGAR), [n_blocks(al) for al in als]
    return _once(("gaps",), make)


def i_runs(cig):
    """[first, end) in query residues of every I run of a CIGAR (M and I consume their length, U and V one residue)"""
    out, aa = [], 0
    for c in cig:
        op, n = c & 15, c >> 4
        if op == OP_I:
            out.append((aa, aa + n))
        aa += n if op in (0, OP_I) else 1 if op in (OP_U, OP_V) else 0
    return out, aa


MIXED_ALS = (1080, 2100, 3130)                                      # 17, 33 and 49 blocks


def mixed_table():
    """three T_MB calls (17, 33 and 49 blocks) next to 40 ordinary pairs in all three modes: packed extension classes, the traceback
    classes T_16 .. T_W16 (one pair of every width of splitwide.MIXED_ALS among them) and the checkpointed ones (windows of 384 rows
    and more)"""
    def make():
        from dpgen import long_window
        rng = np.random.default_rng(9750)
        wide = [sw.wide_pair(rng, al, **hw.WIDE_KW) for al in MIXED_ALS]
        small = sw.mixed_pairs(rng) + [long_window(rng, al) for al in (8, 40, 100, 128)]
        small += [make_task(rng, al=al, p_intron=0.0, flank=10, p_indel=0.0) for al in (100, 120)]      # fewer than 384 rows: T_W2, the plain sweep
        small += [make_task(rng) for _ in range(40 - len(small))]
        tab = Table(hw.default_params(), wide + small, 9751, pair_modes=[CIGAR] * len(wide) + [sw.ALL_MODES] * len(small))
        return tab, [n_blocks(al) for al in MIXED_ALS]
    return _once(("mixed",), make)


WIDE_GE_ALS = (1025, 1700, 40)


def wide_ge_table():
    """-E 300: T_MB calls of 1 025 and 1 700 columns on k_glob_mb_wg<true>, a narrow call on k_glob_narrow<true>; columns x ge < 2^19"""
    def make():
        rng = np.random.default_rng(9760)
        tab = Table(hw.default_params(ge=WIDE_GE), [sw.wide_pair(rng, al, **hw.WIDE_KW) for al in WIDE_GE_ALS], 9761, modes=CIGAR)
        return tab, [n_blocks(al) for al in WIDE_GE_ALS if al > 1024]
    return _once(("wide_ge",), make)


SATURATING_AL = 2100                                                # 33 blocks, three passes: 2 100 x 127 clamps from the third block on


def saturating_table():
    """one call under hugewg.hot_params whose score runs into the int16 clamp: W x al against TGG x al"""
    def make():
        al = SATURATING_AL
        nt = bytes([3, 2, 2]) * al
        return Table(hw.hot_params(), [(nt, b"W" * al)], 9771, modes=CIGAR), [n_blocks(al)]
    return _once(("saturating",), make)


def no_mb_table():
    """a table without a T_MB call, which the device planner still takes with the knob on"""
    def make():
        rng = np.random.default_rng(9780)
        return Table(hw.default_params(), [make_task(rng) for _ in range(12)], 9781), []
    return _once(("no_mb",), make)


def all_tables():
    """(id, maker -> (Table, block counts of its T_MB calls)) of every table the GPU tests run"""
    out = [("blocks", block_count_table), ("edge", class_edge_table), ("gaps", gaps_table), ("mixed", mixed_table), ("wide_ge", wide_ge_table),
           ("saturating", saturating_table), ("no_mb", no_mb_table)]
    out += [("rows-%d" % nb, lambda nb=nb: row_count_table(nb)) for nb in ROW_NBLK]
    return out
