"""The 2 048- / 3 072-column extension classes (MPA_DP_SPLIT_WIDE=1: X_SPLIT8 / X_SPLIT12) over the accepted penalty range, on the GPU:
all twelve column blocks live under a matrix capped at 4, the group shapes at full width, short windows at 3 072 columns, an x-drop that
stops, every entry of dpgen.PENALTY_POINTS whose guard admits the classes, and both sides of every int16 bound of dpgen.WIDE_BOUND_CASES
with the hottest pair the matrix allows.  (nt_len, aa_len, score, CIGAR) of every call against the oracle and, where it is built, the
reference's ns_global_gs16b; and the class that swept the wide calls (mpa_dbg_dp_last_classes): a call that quietly took the one-wave
sweep fails on its class count.  The tables are tests/splitwide.py's; tests/test_dp_split_wide_cpu.py checks them without a device.

Measured on the MI355X: see CHANGELOG.md ("The 2 048- / 3 072-column extension classes tested over the penalty range")."""
import os
import subprocess
import sys
import pytest
import miniprot_amd as mpa
import refbind
import splitwide as sw
from dpgen import WIDE_BOUND_CASES
from dputil import compare

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ctx_on():
    with sw.knob("1"):
        c = mpa.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx_off():
    with sw.knob(None):
        c = mpa.Context(0)
    yield c
    c.close()


def run(ctx, tab, split_wide, want, what=""):
    """the table on the context: every call's values against the oracle and the reference, then the classes that swept the wide calls"""
    idx = mpa.Index.from_nt4(tab.contigs)
    idx.to_device(ctx)
    try:
        rst, cig = mpa.dp_run(ctx, idx, tab.opt, tab.queries, tab.tasks)
    finally:
        idx.close()
    cls = mpa.dbg_dp_last_classes(ctx)
    for which in ("oracle", "reference") if refbind.have_ref() else ("oracle",):
        bad, msg = compare(rst, cig, tab.expect(which), tab.meta, tab.pairs)
        assert not bad, "%s: %d/%d DP calls differ from the %s (classes %s)\n%s" % (what, len(bad), len(tab.tasks), which, cls, msg)
    sw.check_classes(cls, tab, split_wide, want)
    assert ctx.handoff_retries() == 0
    return cls


def all_on_the_one_wave_sweep(tab):
    return {sw.X_HUGE: tab.n_wide()}


# ---- 1. all twelve column blocks (matrix capped at 4, default penalties)
def test_all_twelve_blocks(ctx_on, oracle_built):
    """left and right extensions past the default guard, on both sides of block 11's first column, with a padded and a full last group"""
    tab, want = sw.range_tables()["twelve_blocks"]
    assert want == {sw.X_SPLIT12: 14}
    run(ctx_on, tab, 1, want, "twelve blocks")


def test_group_shapes_at_full_width(ctx_on, oracle_built):
    """(3 072, 2 049) in one group, a lone 3 072-column call, and 3 073 residues on the one-wave sweep, in one batch"""
    tab, want = sw.range_tables()["group_shapes"]
    assert want == {sw.X_SPLIT12: 3, sw.X_HUGE: 1}
    run(ctx_on, tab, 1, want, "group shapes")


def test_short_windows_at_3072_columns(ctx_on, oracle_built):
    """windows that end while the last blocks have hardly begun"""
    tab, want = sw.range_tables()["short_windows"]
    assert want == {sw.X_SPLIT12: 10}
    run(ctx_on, tab, 1, want, "short windows")


def test_xdrop_stops_a_2900_column_extension(ctx_on, oracle_built):
    tab, want = sw.range_tables()["xdrop_stops"]
    assert want == {sw.X_SPLIT12: 4}
    run(ctx_on, tab, 1, want, "xdrop 30")


# ---- 2. the penalty points whose guard admits the classes
@pytest.mark.parametrize("point", sw.wide_penalty_points(), ids=lambda p: ",".join("%s=%s" % x for x in p[0].items()))
def test_penalty_point(ctx_on, oracle_built, point):
    """left and right extensions at 1 032, min(limit, 2 048) and the guard limit in the new classes, at limit + 1 on the one-wave sweep,
    in a round with every narrower class and traceback calls"""
    kw, lim = point
    tab, want = sw.penalty_table(kw, lim)
    assert want[sw.X_HUGE] == 2 and want[sw.X_SPLIT8] + want[sw.X_SPLIT12] == tab.n_wide() - 2 >= 4
    run(ctx_on, tab, 1, want, str(kw))


# ---- 3. the int16 bound
@pytest.mark.parametrize("over", [0, 1], ids=["at32000", "at32001"])
@pytest.mark.parametrize("case", WIDE_BOUND_CASES, ids=lambda c: "al%d-%s" % (c[0], c[2]))
def test_int16_bound(ctx_on, oracle_built, case, over):
    """the larger sum of may_saturate exactly 32 000 (the case's class) or 32 001 (the one-wave sweep): a random and a hot pair at al,
    random pairs 8 columns narrower and wider; the class of every call from the predicate"""
    tab, want = sw.bound_table(case, over)
    al = case[0]
    mine = sw.X_HUGE if over else (sw.X_SPLIT8 if al <= 2048 else sw.X_SPLIT12)
    assert want.get(mine, 0) >= 4 and sw.may_saturate(al, tab.opt) == (over == 1)
    run(ctx_on, tab, 1, want, "al %d %s" % (al, case[1]))


# ---- 4. knob off: the same tables on k_ext_huge (its first runs at 2 666..3 072 columns under a non-default matrix)
@pytest.mark.parametrize("name", ["twelve_blocks", "group_shapes", "hot_bound_2664"])
def test_knob_off(ctx_off, oracle_built, name):
    tab = sw.bound_table(WIDE_BOUND_CASES[4], 0)[0] if name == "hot_bound_2664" else sw.range_tables()[name][0]
    assert WIDE_BOUND_CASES[4][0] == 2664
    want = all_on_the_one_wave_sweep(tab)
    assert want[sw.X_HUGE] == {"twelve_blocks": 14, "group_shapes": 4, "hot_bound_2664": 8}[name]
    run(ctx_off, tab, 0, want, name + ", knob off")


# ---- 5. planned on the device
def test_twelve_blocks_planned_on_the_device(oracle_built):
    code = ("import sys; sys.path.insert(0, 'tests'); import conftest, miniprot_amd as mpa\n"
            "import test_dp_split_wide_range_gpu as t, splitwide as sw\n"
            "tab, want = sw.range_tables()['twelve_blocks']\n"
            "ctx = mpa.Context(0)\n"
            "cls = t.run(ctx, tab, 1, want, 'planned on the device')\n"
            "print('huge', cls[sw.X_HUGE], 'split12', cls[sw.X_SPLIT12])\n")
    env = dict(os.environ, MPA_GPU_DPPLAN="1", MPA_DP_SPLIT_WIDE="1", MPA_TIMING="1")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "huge 0 split12 14" in out.stdout and "plan on device" in out.stderr and "declined" not in out.stderr, out.stdout + out.stderr
