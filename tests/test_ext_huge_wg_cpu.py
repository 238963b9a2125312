"""MPA_DP_HUGE_WG without a device: the schedule of k_ext_huge_wg (miniprot_amd/csrc/ext_huge_wg_core.h) walked step by step by a
stand-alone program under AddressSanitizer and UBSan (tests/hugewg_check.cpp); the tables of tests/test_ext_huge_wg_gpu.py -- their
X_HUGE calls as the host planner classifies them, with the block counts the tests name, and oracle == reference on every call; and the
two hooks in the hooks library."""
import os
import subprocess
import pytest
import miniprot_amd as mpa
import refbind
import hugewg as hw
import splitwide as sw

TABLES = hw.all_tables()


def test_schedule_under_sanitizers(tmp_path):
    """every (block, row) swept once; every LDS read finds the left neighbour's records of the step before, every HBM read at a pass's
    left edge the rows of the pass before; the same number of barriers for every wave; ring slots inside a heap block of the kernel's
    LDS size -- over the shapes around W, R and MIN_BLOCKS, 107 blocks, 5 000 rows and 200 random shapes"""
    root = refbind.ROOT
    csrc = os.path.join(root, "miniprot_amd", "csrc")
    exe = str(tmp_path / "hugewg_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-I" + csrc,
                    os.path.join(root, "tests", "hugewg_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "270 shapes, 0 mismatches" in out.stdout and "ERROR" not in out.stderr, out.stdout + out.stderr
    W, R, MIN_BLOCKS = hw.info()
    assert ("W %d R %d MIN_BLOCKS %d " % (W, R, MIN_BLOCKS)) in out.stdout                 # the program and the library compiled the same constants


def test_constants():
    W, R, MIN_BLOCKS = hw.info()
    assert W >= 2 and R >= 3 and R % 3 == 0 and 1 <= MIN_BLOCKS
    assert W * (22 * 64 * 2 + 4 * 32 * 4 + 2 * R * 16) <= 64 * 1024                        # the wave areas and the double-buffered rings
    assert hw.expected_last_huge([1, MIN_BLOCKS - 1, MIN_BLOCKS, W, W + 1, 2 * W + 1], True) == (2, 4, MIN_BLOCKS + 4 * W + 2, 1 + 1 + 2 + 3)
    assert hw.expected_last_huge([1, MIN_BLOCKS, 2 * W + 1], False) == (3, 0, 0, 0)


def test_small_huge_calls_come_from_the_guard():
    """the hot matrix puts al >= 250 on X_HUGE and no accepted end bonus lowers that below four blocks; fs = 300 puts every call there"""
    from dputil import dpopt_from_params
    o = dpopt_from_params(hw.hot_params())
    assert int(hw.hot_matrix().max()) == 127 and (o.go, o.ge, o.end_bonus) == (11, 1, 5)
    assert sw.guard_limit(o) == 249
    assert sw.guard_limit(dpopt_from_params(hw.hot_params(end_bonus=1000))) == 242 and hw.n_blocks(243) == 4
    assert all(sw.expected_class(al, dpopt_from_params(hw.default_params(fs=hw.WIDE_FS)), hw.dpplan.KNOBS) == sw.X_HUGE for al in (1, 40, 64, 192, 3000))
    assert sw.guard_limit(dpopt_from_params(hw.default_params())) == 2665


@pytest.mark.parametrize("name,make,knobs", TABLES, ids=[t[0] for t in TABLES])
def test_tables_are_huge_calls_of_the_named_blocks(name, make, knobs):
    """the host planner (mpa_dbg_dp_plan) puts exactly the calls the test names on X_HUGE, and their column blocks are the named ones"""
    tab, want = make()
    p = tab.plan(knobs)
    assert not isinstance(p, tuple), p
    T = p.sec["tasks"]
    if name.startswith("two-rows-"):
        # a window of two rows has no row to sweep: whatever its columns, the call is of class X_NONE (11), in no descriptor and behind no
        # unit, and the result rule answers it (include/mpamd.h); with three rows it is the X_HUGE call of `want` blocks ("rows-" tables)
        assert len(T) == 1 and int(T["nl"][0]) == 2 and (int(T["ncol"][0]) + 63) // 64 == want[0] and int(T["flag"][0]) & (mpa.F_EXT_LEFT | mpa.F_EXT_RIGHT)
        assert int(T["cls"][0]) == 11 and p.header["n_huge"] == p.header["n_units"] == p.header["n_ewaves"] == 0
        return
    huge = T[(T["cls"] == sw.X_HUGE) & ((T["flag"] & (mpa.F_EXT_LEFT | mpa.F_EXT_RIGHT)) != 0)]
    assert p.header["n_huge"] == len(huge) == len(want) > 0
    assert sorted((int(c) + 63) // 64 for c in huge["ncol"]) == sorted(want) == sorted(tab.huge_blocks(knobs))
    W, R, MIN_BLOCKS = hw.info()
    if name == "blocks":
        assert sorted(set(want)) == sorted({MIN_BLOCKS, W - 1, W, W + 1, 2 * W, 2 * W + 1}) and all(want.count(b) == 4 for b in set(want))
        als = sorted(set(tab.huge_als()))
        assert all(al % 64 in (0, 55) or al == 250 for al in als) and len(als) == 2 * len(set(want))
        assert all(3 * al <= nl < 4 * al + 300 for al, nl in zip(huge["al"], huge["nl"]))
    if name == "below_min":
        assert sorted(set(want)) == [MIN_BLOCKS - 1, MIN_BLOCKS] and p.header["wide_ge"] == 1
        assert sorted(set(tab.huge_als())) == sorted({64 * b - d for b in (MIN_BLOCKS - 1, MIN_BLOCKS) for d in (0, 9)})
    if name == "mixed":
        assert sorted(want) == sorted(2 * [4, W + 1, 2 * W + 1]) and len(T) - len(huge) == 120 and p.header["wide_ge"] == 0
    if name == "mixed_wide_fs":
        assert {1, 3, 4, W + 1, 2 * W + 1} <= set(want) and max(set(want) - {W + 1, 2 * W + 1}) == 4 and len(want) == 90 and p.header["wide_ge"] == 1
        assert want.count(4) == want.count(W + 1) == want.count(2 * W + 1) == 2
    if name == "saturating":
        assert sorted(want) == [52, 52, 107, 107]
    if name == "wide_ge":
        assert p.header["wide_ge"] == 1 and sorted(set(want)) == [1, 5, 16, 25] and all(int(t["ncol"]) * 300 < 1 << 19 for t in huge)
    if name == "retry":
        assert sorted(set(want)) == [5, 9, 11, 16] and tab.plan().header["n_huge"] == 0        # (X_HUGE only in the repeated round)
    if name.startswith("rows-"):
        assert sorted(int(x) for x in huge["nl"]) == sorted(hw.row_counts())
        assert set(hw.row_counts()) == {3, 4, R + 1, R + 2, R + 3, 2 * R + 2, (W - 1) * R + 1, W * R + 3}
    assert hw.expected_last_huge(want, True)[1] == sum(b >= MIN_BLOCKS for b in want)


@pytest.mark.skipif(not refbind.have_ref(), reason="the reference is not built")
@pytest.mark.parametrize("name,make,knobs", [t for t in TABLES if not t[0].startswith("two-rows-")], ids=[t[0] for t in TABLES if not t[0].startswith("two-rows-")])
def test_expected_values_are_the_references(oracle_built, name, make, knobs):
    """oracle == reference (ns_global_gs16b) on every call of every table of the GPU tests (not the two-row windows, on which the
    reference fails its own assertion: tests/test_dp_edges_cpu.py)"""
    tab, _ = make()
    e, r = tab.expect("oracle"), tab.expect("reference")
    assert len(e) == len(tab.tasks)
    bad = [(k, tab.meta[k], e[k][:3], r[k][:3]) for k in range(len(e)) if e[k] != r[k]]
    assert not bad, bad[:5]


def test_planted_gaps_are_taken(oracle_built):
    """the pair of hugewg.gaps_table(): the oracle's global alignment of it takes the planted gaps -- a run of the I state of four or
    more residues for (nearly) every even block boundary and a D run for (nearly) every odd one.  Where they lie follows from the
    construction (gap_pair: the residues [64 b - 3, 64 b + 2) have no codons), the CIGAR's frameshift operations make its own residue
    count drift by a few columns."""
    tab, want = hw.gaps_table()
    W = hw.info()[0]
    assert want == [2 * W + 1] * 2
    nt, aa = tab.pairs[0]
    assert len(aa) == 64 * (2 * W + 1) - 9 and len(nt) == 40 + 3 * (len(aa) - 5 * W + 4 * W)
    cig = refbind.ora_nasw(nt, aa, tab.P, mpa.F_CIGAR)[3]
    i_runs = sum(1 for c in cig if c & 15 == 1 and c >> 4 >= 4)
    d_runs = sum(1 for c in cig if c & 15 == 2 and c >> 4 >= 3)
    assert i_runs >= W - 2 and d_runs >= W - 2, (i_runs, d_runs)


def test_hooks_are_in_the_hooks_library():
    for name in ("mpa_dbg_dp_last_huge", "mpa_dbg_dp_huge_wg_info"):
        assert hasattr(mpa.dbg_lib(), name) and not hasattr(mpa.lib(), name)
