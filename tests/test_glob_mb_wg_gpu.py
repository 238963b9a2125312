"""MPA_DP_MB_WG on the GPU: traceback calls of more than 1 024 columns (class T_MB) swept by k_glob_mb_wg (one wave per 64-column block,
W waves per workgroup, boundary records through LDS) against the oracle, bit-exact on the score and the CIGAR; the same tables on a
context without the knob (one wave per call, in the round kernel or k_glob_narrow), with equal records and CIGAR pools.
mpa_dbg_dp_last_mb says which path swept how many calls, blocks and passes: a call that quietly took the other kernel fails on the
counts.  The tables are tests/mbwg.py's; tests/test_glob_mb_wg_cpu.py checks them without a device."""
import os
import re
import subprocess
import sys
import threading
import pytest
import miniprot_amd as mpa
import refbind
import mbwg

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MB_NOTE = "block-major traceback calls"


@pytest.fixture(scope="module")
def ctx_on():
    with mbwg.knob("1"):
        c = mpa.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx_off():
    with mbwg.knob(None):
        c = mpa.Context(0)
    yield c
    c.close()


def both(ctx_on, ctx_off, tab, want, what, against=("oracle",)):
    """the table on both contexts: counts by the rule, the oracle's values with the knob on, equal records and CIGAR pools"""
    on = mbwg.run(ctx_on, tab, True, want, what + ", knob on", against)
    got_on = mpa.dbg_dp_last_mb(ctx_on)
    off = mbwg.results(ctx_off, tab)
    assert mpa.dbg_dp_last_mb(ctx_off) == (len(want), 0, 0, 0), what
    mbwg.same_results(on, off, what)
    return got_on


def test_block_counts(ctx_on, ctx_off, oracle_built):
    """1 025 (17 blocks, the last one 8 columns wide), 1 088 (17, full), 2 048 (32: two full passes), 2 049 and 2 112 (33: a third pass of
    one block) and 3 100 residues (49): 2, 2, 2, 3, 3 and 4 passes"""
    W = mbwg.info()[0]
    tab, want = mbwg.block_count_table()
    assert want == [17, 17, 32, 33, 33, 49] and [(b + W - 1) // W for b in want] == [2, 2, 2, 3, 3, 4]
    assert both(ctx_on, ctx_off, tab, want, "block counts") == (0, 6, 181, 16)


@pytest.mark.parametrize("nblk", mbwg.ROW_NBLK)
def test_row_counts(ctx_on, ctx_off, oracle_built, nblk):
    """windows of 3, 4, R + 1, R + 2, R + 3, 2 R + 2, (W - 1) R + 1 and W R + 3 rows under calls of 17 and 33 blocks"""
    W = mbwg.info()[0]
    tab, want = mbwg.row_count_table(nblk)
    assert want == [nblk] * 8
    assert both(ctx_on, ctx_off, tab, want, "row counts, %d blocks" % nblk) == (0, 8, 8 * nblk, 8 * ((nblk + W - 1) // W))


def test_class_edge_and_short_windows(ctx_on, ctx_off, oracle_built):
    """windows of 0 .. 5 rows at 1 024 residues (T_W16, not counted) and at 1 025 (T_MB) in one table: the calls of fewer than three
    rows meet no barrier and take the contract of include/mpamd.h, which the oracle states"""
    tab, want = mbwg.class_edge_table()
    assert len(tab.tasks) == 12 and want == [17] * 6
    assert both(ctx_on, ctx_off, tab, want, "class edge") == (0, 6, 6 * 17, 6 * 2)


def test_gap_runs_across_block_and_pass_boundaries(ctx_on, ctx_off, oracle_built):
    """I runs planted across every second block boundary, 1 023 | 1 024 (two passes, through HBM) among them (tests/mbwg.py, gaps_table;
    tests/test_glob_mb_wg_cpu.py checks that the optimal alignment takes them there)"""
    tab, want = mbwg.gaps_table()
    both(ctx_on, ctx_off, tab, want, "gaps")


def test_mixed_round(ctx_on, ctx_off, oracle_built):
    """T_MB calls of 17, 33 and 49 blocks next to 40 ordinary pairs (packed extension classes, T_16 .. T_W16, checkpointed calls): the
    split between the kernels is the rule's, every record and CIGAR the knob-off context's"""
    tab, want = mbwg.mixed_table()
    assert both(ctx_on, ctx_off, tab, want, "mixed") == (0, 3, 17 + 33 + 49, 2 + 3 + 4)


def test_later_chunks(ctx_off, oracle_built, monkeypatch):
    """MPA_TB_BUDGET_MB=1: the mixed table's T_MB calls fall into traceback chunks after the first, which the stand-alone launch serves"""
    tab, want = mbwg.mixed_table()
    monkeypatch.setenv("MPA_TB_BUDGET_MB", "1")
    with mbwg.knob("1"):
        c = mpa.Context(0)
    try:
        on = mbwg.run(c, tab, True, want, "chunks, knob on")
        assert mpa.dbg_dp_last_mb(c) == (0, 3, 17 + 33 + 49, 2 + 3 + 4)
    finally:
        c.close()
    mbwg.same_results(on, mbwg.results(ctx_off, tab), "chunks")


def test_gap_extension_above_255(ctx_on, ctx_off, oracle_built):
    """ge = 300: T_MB calls of 1 025 and 1 700 columns on k_glob_mb_wg<true>, the narrow call on k_glob_narrow<true>"""
    tab, want = mbwg.wide_ge_table()
    assert want == [17, 27]
    against = ("oracle", "reference") if refbind.have_ref() else ("oracle",)
    assert both(ctx_on, ctx_off, tab, want, "ge 300", against) == (0, 2, 44, 4)


def test_saturation(ctx_on, ctx_off, oracle_built):
    """a call whose score runs into the int16 clamp, across three passes"""
    tab, want = mbwg.saturating_table()
    assert tab.expect("oracle")[0][2] >= 32000
    assert both(ctx_on, ctx_off, tab, want, "saturation") == (0, 1, 33, 3)


CHILD = ("import sys; sys.path.insert(0, 'tests'); import conftest, miniprot_amd as mpa, mbwg\n"
         "ctx = mpa.Context(0)\n"
         "for name, make, knob_on in ((%r, lambda: mbwg.row_count_table(17), %r), ('no_mb', mbwg.no_mb_table, %r)):\n"
         "    tab, want = make()\n"
         "    print('=== ' + name, file=sys.stderr, flush=True)\n"
         "    mbwg.run(ctx, tab, knob_on, want, name)\n"
         "    print(name, 'last_mb', mpa.dbg_dp_last_mb(ctx), flush=True)\n")


def child(code, **env):
    e = dict(os.environ, **env)
    for k in ("MPA_DP_POOL", "MPA_GPU_DPPLAN", "MPA_GPU_ROUND2", "MPA_TB_BUDGET_MB"):
        if k not in env:
            e.pop(k, None)
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=e, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    return out


def test_device_planner_declines_a_round_with_a_block_major_call(oracle_built):
    """MPA_GPU_DPPLAN=1 with the knob on: a table with T_MB calls is declined to the host planner with a note (MPA_TIMING=1) and swept on
    workgroups; a table without one is still planned on the device.  The results are the oracle's (mbwg.run)."""
    out = child(CHILD % ("rows-17", True, True), MPA_GPU_DPPLAN="1", MPA_DP_MB_WG="1", MPA_TIMING="1")
    assert "rows-17 last_mb (0, 8, 136, 16)" in out.stdout and "no_mb last_mb (0, 0, 0, 0)" in out.stdout, out.stdout + out.stderr
    first, second = out.stderr.split("=== no_mb")
    assert re.search(r"device DP plan declined \(device DP plan: a block-major traceback call", first) and "plan on device:" not in first, first
    assert MB_NOTE in first and "0 on one wave, 8 on workgroups (136 blocks, 16 passes)" in first
    assert "declined" not in second and "plan on device:" in second and MB_NOTE not in second, second


def test_worker_pool_keeps_one_wave(oracle_built):
    """MPA_DP_POOL=1 with the knob on: the knob stays off, every T_MB call is swept on one wave by the pool's workers"""
    out = child(CHILD % ("rows-17", False, False), MPA_DP_POOL="1", MPA_DP_MB_WG="1")
    assert "rows-17 last_mb (8, 0, 0, 0)" in out.stdout, out.stdout + out.stderr


def test_two_contexts_at_once(ctx_on, oracle_built):
    tab, want = mbwg.block_count_table()
    tab.expect("oracle")                                             # (computed before the threads start)
    with mbwg.knob("1"):
        second = mpa.Context(0)
    errs = []

    def worker(c):
        try:
            mbwg.run(c, tab, True, want, "two contexts")
        except BaseException as e:                                   # noqa: BLE001 (reported in the main thread)
            errs.append(repr(e))

    th = [threading.Thread(target=worker, args=(c,)) for c in (ctx_on, second)]
    [t.start() for t in th]
    [t.join() for t in th]
    second.close()
    assert not errs, errs


@pytest.mark.parametrize("name", ["long_u", "syn_a"])
def test_whole_path(ctx_on, name, tmp_path, monkeypatch, capfd):
    """the committed bytes of the reference with the knob on.  Whether the run held a T_MB call is reported, not asserted."""
    import alnstats
    from hostpipe import map_batch_gpu
    idx, mo, q, ref = alnstats.case_inputs(name, tmp_path)
    idx.to_device(ctx_on)
    monkeypatch.setenv("MPA_TIMING", "1")
    capfd.readouterr()
    try:
        ours = map_batch_gpu(ctx_on, idx, mo, q, 4)
    finally:
        idx.close()
    notes = [l for l in capfd.readouterr().err.split("\n") if MB_NOTE in l]
    print("%s with MPA_DP_MB_WG=1: %d DP rounds with T_MB calls%s" % (name, len(notes), "".join("\n  " + l.strip() for l in notes[:4])))
    assert ours == ref, "%s: output differs from the reference with MPA_DP_MB_WG=1" % name
