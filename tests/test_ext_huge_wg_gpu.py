"""MPA_DP_HUGE_WG on the GPU: X_HUGE extension calls swept by k_ext_huge_wg (one wave per 64-column block, W waves per workgroup, boundary
records through LDS) against the oracle, bit-exact on (nt_len, aa_len, score); the same tables on a context without the knob (the
one-wave k_ext_huge).  mpa_dbg_dp_last_huge says which kernel swept how many calls, blocks and passes: a call that quietly took the other
kernel fails on the counts.  The tables are tests/hugewg.py's; tests/test_ext_huge_wg_cpu.py checks them without a device."""
import os
import subprocess
import sys
import threading
import pytest
import miniprot_amd as mpa
import hugewg as hw

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx_on():
    with hw.knob("1"):
        c = mpa.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx_off():
    with hw.knob(None):
        c = mpa.Context(0)
    yield c
    c.close()


def same_records(a, b):
    assert len(a) == len(b) and hw.fields(a) == hw.fields(b)


# ---- 1. block counts
def test_block_counts(ctx_on, ctx_off, oracle_built):
    """left and right extensions of MIN_BLOCKS, W - 1, W, W + 1, 2 W and 2 W + 1 blocks, the last block full and partial: all on the
    workgroup kernel, in one, one, one, two, two and three passes; identical records from the one-wave kernel"""
    W, R, MIN_BLOCKS = hw.info()
    tab, want = hw.block_count_table()
    assert sorted(set(want)) == sorted({MIN_BLOCKS, W - 1, W, W + 1, 2 * W, 2 * W + 1})
    on = hw.run(ctx_on, tab, True, want, "block counts, knob on")
    assert mpa.dbg_dp_last_huge(ctx_on)[:2] == (0, len(want))
    off = hw.run(ctx_off, tab, False, want, "block counts, knob off")
    assert mpa.dbg_dp_last_huge(ctx_off) == (len(want), 0, 0, 0)
    same_records(on, off)


def test_a_call_below_min_blocks_stays_on_one_wave(ctx_on, ctx_off, oracle_built):
    """calls of MIN_BLOCKS - 1 and of MIN_BLOCKS blocks in the same launch: the narrower ones on k_ext_huge, the others on k_ext_huge_wg"""
    W, R, MIN_BLOCKS = hw.info()
    tab, want = hw.below_min_table()
    assert sorted(want) == 4 * [MIN_BLOCKS - 1] + 4 * [MIN_BLOCKS]
    on = hw.run(ctx_on, tab, True, want, "below MIN_BLOCKS, knob on")
    assert mpa.dbg_dp_last_huge(ctx_on) == (4, 4, 4 * MIN_BLOCKS, 4)
    same_records(on, hw.run(ctx_off, tab, False, want, "below MIN_BLOCKS, knob off"))


# ---- 2. row counts
@pytest.mark.parametrize("k", [0, 1, 2])
def test_row_counts(ctx_on, oracle_built, k):
    """windows of 3, 4, R + 1, R + 2, R + 3, 2 R + 2, (W - 1) R + 1 and W R + 3 rows under calls of 4, W + 1 and 2 W + 3 blocks: a lone
    DP row, both sides of a chunk edge, a pipeline that never fills and one that just does"""
    W, R, _ = hw.info()
    nblk = hw.row_count_nblks()[k]
    assert nblk == (4, W + 1, 2 * W + 3)[k]
    tab, want = hw.row_count_table(nblk)
    assert want == [nblk] * 8
    hw.run(ctx_on, tab, True, want, "row counts, %d blocks" % nblk)
    assert mpa.dbg_dp_last_huge(ctx_on) == (0, 8, 8 * nblk, 8 * ((nblk + W - 1) // W))


@pytest.mark.parametrize("k", [0, 1, 2])
def test_two_row_windows(ctx_on, ctx_off, oracle_built, k):
    """A window of two rows has no DP row at all and the reference fails its own assertion on it (nasw-sse.c:441).  The contract
    (include/mpamd.h) is the oracle's (0, al + 1, INT32_MIN): the planner gives the call no unit, so neither sweep is launched for it
    with the knob on or off, and the result rule writes the triple."""
    nblk = hw.row_count_nblks()[k]
    tab, want = hw.row_count_table(nblk, (2,))
    on, _ = hw.results(ctx_on, tab)
    assert mpa.dbg_dp_last_huge(ctx_on) == (0, 0, 0, 0) and mpa.dbg_dp_last_classes(ctx_on)[mpa.X_NONE] == 1
    off, _ = hw.results(ctx_off, tab)
    assert mpa.dbg_dp_last_huge(ctx_off) == (0, 0, 0, 0) and mpa.dbg_dp_last_classes(ctx_off)[mpa.X_NONE] == 1
    e = tab.expect("oracle")[0]
    assert e[:3] == (0, int(tab.tasks["al"][0]) + 1, -2 ** 31)
    assert hw.fields(on)[0] == e[:3] and hw.fields(off)[0] == e[:3], (hw.fields(on), hw.fields(off), e[:3])
    same_records(on, off)


# ---- 3. mixed launch
def test_mixed_launch(ctx_on, ctx_off, oracle_built):
    """X_HUGE calls of 4, W + 1 and 2 W + 1 blocks next to 40 ordinary pairs (packed extension classes, traceback calls): the split
    between the two kernels is the rule's, and every record equals the one of the context without the knob"""
    W, R, MIN_BLOCKS = hw.info()
    tab, want = hw.mixed_table()
    on = hw.run(ctx_on, tab, True, want, "mixed, knob on")
    assert mpa.dbg_dp_last_huge(ctx_on) == (0, 6, 2 * (4 + W + 1 + 2 * W + 1), 2 * (1 + 2 + 3))
    off, cig_off = hw.results(ctx_off, tab)
    assert mpa.dbg_dp_last_huge(ctx_off) == (6, 0, 0, 0)
    same_records(on, off)


def test_mixed_launch_with_calls_of_one_and_three_blocks(ctx_on, ctx_off, oracle_built):
    """fs = 300: X_HUGE calls of 1, 3, 4, W + 1 and 2 W + 1 blocks and the extension calls of 40 ordinary pairs of at most three blocks
    in one launch of each kernel"""
    W, R, MIN_BLOCKS = hw.info()
    tab, want = hw.mixed_wide_fs_table()
    on = hw.run(ctx_on, tab, True, want, "mixed, fs 300, knob on")
    assert mpa.dbg_dp_last_huge(ctx_on) == (len(want) - 6, 6, 2 * (4 + W + 1 + 2 * W + 1), 2 * (1 + 2 + 3))
    same_records(on, hw.run(ctx_off, tab, False, want, "mixed, fs 300, knob off"))


# ---- 4. x-drop and end bonus
def test_xdrop_and_end_bonus(ctx_on, oracle_built):
    """the best row lies early while the sweep still runs every row: the key's column must come from the right block"""
    tab, want = hw.xdrop_table()
    W = hw.info()[0]
    assert sorted(want) == [10, 10, W + 1, W + 1]
    hw.run(ctx_on, tab, True, want, "xdrop 30, end bonus 11")


def test_gap_runs_across_block_boundaries(ctx_on, ctx_off, oracle_built):
    """runs of the I state planted across every second block boundary, the one between two passes among them (tests/hugewg.py, gap_pair;
    tests/test_ext_huge_wg_cpu.py checks that the optimal alignment takes them)"""
    tab, want = hw.gaps_table()
    on = hw.run(ctx_on, tab, True, want, "gaps, knob on")
    same_records(on, hw.run(ctx_off, tab, False, want, "gaps, knob off"))


# ---- 5. past the default guard and into saturation
def test_past_the_guard_and_into_saturation(ctx_on, ctx_off, oracle_built):
    """52 and 107 blocks (four and seven passes), int16 clamping across passes"""
    W = hw.info()[0]
    tab, want = hw.saturating_table()
    assert sorted(want) == [52, 52, 107, 107]
    on = hw.run(ctx_on, tab, True, want, "saturation, knob on")
    assert mpa.dbg_dp_last_huge(ctx_on) == (0, 4, 318, 2 * ((52 + W - 1) // W + (107 + W - 1) // W))
    assert max(x[2] for x in tab.expect("oracle")) >= 32000
    off, _ = hw.results(ctx_off, tab)
    first = [k for k, (p, _, _) in enumerate(tab.meta) if p == 0]
    assert [hw.fields(on)[k] for k in first] == [hw.fields(off)[k] for k in first]


# ---- 6. -E above 255
def test_gap_extension_above_255(ctx_on, oracle_built):
    """ge = 300: calls of 300, 1 000 and 1 600 columns on k_ext_huge_wg<true>, the call of 40 columns on one wave"""
    tab, want = hw.wide_ge_table()
    assert sorted(set(want)) == [1, 5, 16, 25]
    hw.run(ctx_on, tab, True, want, "ge 300")
    assert mpa.dbg_dp_last_huge(ctx_on)[:2] == (2, 6)


# ---- 7. a repeated round
def test_repeated_round(oracle_built):
    """MPA_TEST_HANDOFF_FAIL=1 (read once per process: a child): the repeated round's 512- / 1 024-column calls run on the workgroup
    kernel and return the oracle's values"""
    code = ("import sys; sys.path.insert(0, 'tests'); import conftest, miniprot_amd as mpa, hugewg as hw\n"
            "tab, want = hw.retry_table()\n"
            "ctx = mpa.Context(0)\n"
            "hw.run(ctx, tab, True, want, 'repeated round', knobs=dict(no_split=1))\n"
            "print('retries', ctx.handoff_retries(), 'huge', mpa.dbg_dp_last_huge(ctx))\n")
    env = dict(os.environ, MPA_TEST_HANDOFF_FAIL="1", MPA_DP_HUGE_WG="1")
    env.pop("MPA_DP_SPLIT_WIDE", None)
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "retries 1 huge (0, 8, 82, 8)" in out.stdout, out.stdout + out.stderr


# ---- 8. two contexts at once
def test_two_contexts_at_once(ctx_on, oracle_built):
    tab, want = hw.block_count_table()
    tab.expect("oracle")                                             # (computed before the threads start)
    with hw.knob("1"):
        second = mpa.Context(0)
    errs = []

    def worker(c):
        try:
            hw.run(c, tab, True, want, "two contexts")
        except BaseException as e:                                   # noqa: BLE001 (reported in the main thread)
            errs.append(repr(e))

    th = [threading.Thread(target=worker, args=(c,)) for c in (ctx_on, second)]
    [t.start() for t in th]
    [t.join() for t in th]
    second.close()
    assert not errs, errs
