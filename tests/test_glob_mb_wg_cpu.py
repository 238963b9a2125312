"""MPA_DP_MB_WG without a device: the tables of tests/test_glob_mb_wg_gpu.py (tests/mbwg.py) -- oracle == reference on every call, score
and CIGAR; the host planner puts exactly the named calls on T_MB (and the 1 024-column ones on T_W16); the plan's bytes do not depend
on the knob; the planted gaps are taken across the boundaries they were planted across; and the hook is in the hooks library.  The
schedule itself (miniprot_amd/csrc/ext_huge_wg_core.h) is walked by tests/test_ext_huge_wg_cpu.py."""
import pytest
import miniprot_amd as mpa
import refbind
import mbwg

TABLES = mbwg.all_tables()
IDS = [t[0] for t in TABLES]


@pytest.mark.skipif(not refbind.have_ref(), reason="the reference is not built")
@pytest.mark.parametrize("name,make", TABLES, ids=IDS)
def test_expected_values_are_the_references(oracle_built, name, make):
    """oracle == reference (ns_global_gs16b) on every call of every table of the GPU tests, score and CIGAR"""
    tab, _ = make()
    e, r = tab.expect("oracle"), tab.expect("reference")
    assert len(e) == len(r) == len(tab.tasks)
    bad = [(k, tab.meta[k], e[k][:3], r[k][:3]) for k in range(len(e)) if e[k] != r[k]]
    assert not bad, bad[:5]


@pytest.mark.parametrize("name,make", TABLES, ids=IDS)
def test_tables_are_block_major_calls_of_the_named_blocks(name, make):
    """the host planner (mpa_dbg_dp_plan) puts exactly the calls the test names on T_MB, with the named column blocks, and the
    1 024-column traceback calls on T_W16"""
    tab, want = make()
    p = tab.plan()
    assert not isinstance(p, tuple), p
    T = p.sec["tasks"]
    glob = T[(T["flag"] & (mpa.F_EXT_LEFT | mpa.F_EXT_RIGHT)) == 0]
    mb = glob[glob["cls"] == mbwg.T_MB]
    assert sorted((int(c) + 63) // 64 for c in mb["ncol"]) == sorted(want) == sorted(tab.mb_blocks())
    assert sorted(int(a) for a in mb["al"]) == sorted(tab.mb_als()) and all(int(a) > 1024 for a in mb["al"])
    assert not ((glob["cls"] != mbwg.T_MB) & (glob["al"] > 1024)).any()
    W, R, MIN_BLOCKS = mbwg.info()
    assert all(b > W and b >= MIN_BLOCKS for b in want)                   # more than 1 024 columns: 17 blocks at least, so every call takes the workgroup kernel
    assert mbwg.expected_last_mb(want, True) == (0, len(want), sum(want), sum(-(-b // W) for b in want))
    assert mbwg.expected_last_mb(want, False) == (len(want), 0, 0, 0)
    if name == "blocks":
        assert want == list(mbwg.BLOCK_NBLK) and [-(-b // W) for b in want] == list(mbwg.BLOCK_PASSES)
        assert sorted(int(c) for c in mb["ncol"])[0] == 1032                # 17 blocks, the last one 8 columns wide
        assert all(3 * al <= nl < 4 * al + 300 for al, nl in zip(mb["al"], mb["nl"]))
    if name == "edge":
        w16 = glob[glob["cls"] == mbwg.T_W16]
        assert sorted(int(x) for x in w16["nl"]) == sorted(int(x) for x in mb["nl"]) == list(mbwg.EDGE_ROWS)
        assert set(int(a) for a in w16["al"]) == {1024} and set(int(a) for a in mb["al"]) == {1025}
    if name.startswith("rows-"):
        assert sorted(int(x) for x in mb["nl"]) == sorted(mbwg.row_counts()) and len(set(want)) == 1 and want[0] in mbwg.ROW_NBLK
        assert set(mbwg.row_counts()) == {3, 4, R + 1, R + 2, R + 3, 2 * R + 2, (W - 1) * R + 1, W * R + 3}
    if name == "gaps":
        assert sorted(want) == [W + 1, 2 * W + 1]
    if name == "mixed":
        assert sorted(want) == [17, 33, 49] and len(tab.pairs) == 43
        cls_glob = set(int(c) for c in glob["cls"])
        assert set(range(0, 8)) <= cls_glob and any(c >= 8 for c in cls_glob)        # T_16 .. T_MB and checkpointed classes
        assert len(T) - len(glob) == 80
    if name == "wide_ge":
        assert p.header["wide_ge"] == 1 and sorted(want) == [17, 27] and all(int(t["ncol"]) * mbwg.WIDE_GE < 1 << 19 for t in glob)
    if name == "saturating":
        assert want == [33] and -(-want[0] // W) >= 3
    if name == "no_mb":
        assert want == [] and len(mb) == 0


@pytest.mark.parametrize("name,make", TABLES, ids=IDS)
def test_plan_bytes_do_not_depend_on_the_knob(monkeypatch, name, make):
    """the serialised plan is the same bytes with MPA_DP_MB_WG set and unset, in a single chunk and under a 1 MB traceback budget"""
    tab, _ = make()
    for kn in ({}, dict(tb_budget=1 << 20)):
        monkeypatch.delenv("MPA_DP_MB_WG", raising=False)
        unset = tab.plan_bytes(kn)
        monkeypatch.setenv("MPA_DP_MB_WG", "1")
        assert tab.plan_bytes(kn) == unset
        monkeypatch.setenv("MPA_DP_MB_WG", "0")
        assert tab.plan_bytes(kn) == unset


def test_planted_gaps_are_taken_across_their_boundaries(oracle_built):
    """the pairs of mbwg.gaps_table(): for every boundary 64 b - 1 | 64 b the construction plants an I run across (hugewg.gap_pair: the
    residues [64 b - 3, 64 b + 2) have no codons), the oracle's CIGAR holds an I run that covers both columns; 1 023 | 1 024, the edge
    between two passes, is one of them"""
    tab, want = mbwg.gaps_table()
    seen = set()
    for (nt, aa), e in zip(tab.pairs, tab.expect("oracle")):
        runs, n_aa = mbwg.i_runs(e[3])
        assert n_aa == len(aa)                                            # (a global alignment: the CIGAR consumes the query)
        bounds = mbwg.gap_boundaries(len(aa))
        assert len(bounds) >= 8
        for c in bounds:
            assert any(s <= c - 1 and c + 1 <= t for s, t in runs), (len(aa), c, runs)
        seen |= set(bounds)
    assert 1024 in seen and 64 * mbwg.info()[0] == 1024


def test_saturating_call_reaches_the_clamp(oracle_built):
    tab, _ = mbwg.saturating_table()
    assert tab.expect("oracle")[0][2] >= 32000


def test_hook_is_in_the_hooks_library():
    assert hasattr(mpa.dbg_lib(), "mpa_dbg_dp_last_mb") and not hasattr(mpa.lib(), "mpa_dbg_dp_last_mb")
