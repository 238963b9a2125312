"""MPA_DP_SPLIT_WIDE without a device: extension calls of 1 025..3 072 columns classified as X_SPLIT8 / X_SPLIT12 (8 / 12 workgroups per
pair of calls) by the host planner (mpa_dbg_dp_plan_wide) and by the model of the device planner (mpa_dbg_dp_plan_device_wide, ctx None),
what the plan promises the executor (groups, boundaries, units, bytes of the granule pool), and the knob's absence: with split_wide = 0 the
plan is mpa_dbg_dp_plan's, byte for byte.  A stand-alone program (tests/dpsplit_check.cpp, compiled here with AddressSanitizer and UBSan)
runs random tables through both planners with every pool at exactly the executor's bound.  And the batches of
tests/test_dp_split_wide_range_gpu.py (capped matrix, penalty points, int16 bound): their sums, their routing by both planners, the
classes their tests expect, the teeth of the class assertion, and oracle == reference on every call."""
import os
import subprocess
import numpy as np
import pytest
import miniprot_amd as mpa
import dpplan
import refbind
import splitwide as sw
from dpgen import WIDE_BOUND_CASES, PENALTY_POINTS, bound_params
from dputil import dpopt_from_params
from dpplan import EXT, GLOB


def ext_classes(p):
    """al -> set of classes of the plan's extension calls"""
    out = {}
    for t in p.sec["tasks"]:
        if t["flag"] & (mpa.F_EXT_LEFT | mpa.F_EXT_RIGHT):
            out.setdefault(int(t["al"]), set()).add(int(t["cls"]))
    return out


@pytest.mark.parametrize("opts", ["default", "low_matrix"])
def test_classes_by_width(opts):
    """the class edges 1 024 / 1 025, 2 048 / 2 049, 3 072 / 3 073, the guard's last admitted al and the next one (computed from the
    predicate), and the edges the existing plan tests use.  With the default matrix the guard ends inside X_SPLIT12; with every matrix
    entry capped at 4 it lies beyond 3 072 columns, so that the class's own edge is reached."""
    over = {} if opts == "default" else sw.low_matrix()
    o = dpplan.dpopt(**over)
    g = sw.guard_limit(o)
    assert (2049 < g < 3072) if opts == "default" else g > 3073
    assert not sw.may_saturate(g, o) and sw.may_saturate(g + 1, o)
    als = sorted(set(dpplan.EDGES + [1024, 1025, 2048, 2049, 3072, 3073, min(g, 3200), min(g + 1, 3200)]))
    r = np.random.default_rng(9300)
    p = sw.plan(sw.table(r, [(EXT, al, 300 + k) for k, al in enumerate(als)]), over)
    assert isinstance(p, sw.WidePlan), p
    got = ext_classes(p)
    for al in als:
        assert got[al] == {sw.expected_class(al, o, sw.KNOBS)}, (al, got[al])
    # the edges themselves, spelled out
    want = {1024: sw.X_SPLIT4, 1025: sw.X_SPLIT8, 2048: sw.X_SPLIT8, 2049: sw.X_SPLIT12}
    want.update({g: sw.X_SPLIT12, g + 1: sw.X_HUGE} if opts == "default" else {3072: sw.X_SPLIT12, 3073: sw.X_HUGE})
    for al, cls in want.items():
        assert got[al] == {cls}, (al, got[al])
    for t in p.sec["tasks"]:
        if t["cls"] in (sw.X_SPLIT8, sw.X_SPLIT12):
            assert t["pw"] == (2048 if t["cls"] == sw.X_SPLIT8 else 3072)


@pytest.mark.parametrize("name,over,knobs", [("wide_ge", dict(ge=300), {}), ("may_saturate", dict(ge=30), {}), ("no_split", {}, dict(no_split=1)),
                                             ("pool", {}, dict(pool=1)), ("knob_off", {}, dict(split_wide=0))])
def test_what_keeps_the_one_wave_sweep(name, over, knobs):
    """penalties above 255, calls the int16 guard refuses, a repeated round, the worker pool -- and the knob's absence"""
    r = np.random.default_rng(9310)
    als = [40, 1100, 1500] + ([] if name == "wide_ge" else [2100, 2600])          # (ge = 300: columns x ge must stay below 2^19)
    p = sw.plan(sw.table(r, [(EXT, al, 400) for al in als] + [(GLOB, 30, 100)]), over, knobs)
    assert isinstance(p, sw.WidePlan), p
    got = ext_classes(p)
    for al in als:
        if al > 1024:
            assert got[al] == {sw.X_HUGE}, (al, got[al])
    assert p.s8[1] == 0 and p.s12[1] == 0 and p.header["n_huge"] == len([a for a in als if a > 1024 or name == "wide_ge"])


def test_groups_boundaries_units_and_bytes():
    p = sw.plan(*sw.planner_tables()["odd_counts"])
    assert isinstance(p, sw.WidePlan), p
    h, T, W, U = p.header, p.sec["tasks"], p.sec["ewaves"], p.sec["units"]
    n_call = {c: int(np.sum((T["cls"] == c) & ((T["flag"] & mpa.F_CIGAR) == 0))) for c in sw.N_BLK}
    assert n_call[sw.X_SPLIT8] == 5 and n_call[sw.X_SPLIT12] == 3
    n8, n12, n4, n2 = p.s8[1], p.s12[1], h["ewave_cnt6"], h["ewave_cnt5"]
    assert (n8, n12) == (3, 2)                                                 # pairs, rows descending; the last group of each has an empty half
    assert h["n_split"] == n8 + n12 + n4 + n2 and h["n_bound"] == p.n_bound == 7 * n8 + 11 * n12 + 3 * n4 + n2
    assert h["xg_bytes"] == h["n_bound"] * h["key_stride"] * 16 and h["xg_tail"] == (2 * h["n_split"] + 1) * 4 and h["sz_xg"] == h["xg_bytes"] + h["xg_tail"] + 64
    # the descriptors follow X_SPLIT4's and lie before X_128's: the wide groups are neighbours (row keys by descriptor)
    assert p.s8[0] == h["ewave_first6"] + n4 and p.s12[0] == p.s8[0] + n8 and h["dwave_first"] == p.s12[0] + n12
    assert h["n_wide_groups"] == p.s12[0] + n12 - h["ewave_first3"]
    assert h["sz_rowkey"] == h["n_wide_groups"] * 2 * h["key_stride"] * 4 + 64
    for first, cnt, cls in ((p.s8[0], n8, sw.X_SPLIT8), (p.s12[0], n12, sw.X_SPLIT12)):
        nls = []
        for d in range(first, first + cnt):
            ids = [int(x) for x in W[d]["task"][:2] if x >= 0]
            assert all(T[i]["cls"] == cls for i in ids) and all(x == -1 for x in W[d]["task"][2:])
            assert W[d]["max_nl"] == max(T[i]["nl"] for i in ids)
            nls += [int(T[i]["nl"]) for i in ids]
            units = U[(U["kind"] == sw.U_EXT_SPLIT) & (U["first"] == d)]
            assert sorted(units["blk"]) == list(range(sw.N_BLK[cls])) and set(units["n_blk"]) == {sw.N_BLK[cls]}
            assert len(set(units["sgroup"])) == 1 and len(set(units["xg_first"])) == 1
        assert nls == sorted(nls, reverse=True)
        assert len([x for x in W[first + cnt - 1]["task"] if x >= 0]) == 1
    split = U[U["kind"] == sw.U_EXT_SPLIT]
    groups = {(int(u["sgroup"]), int(u["xg_first"]), int(u["n_blk"])) for u in split}
    assert sorted(g[0] for g in groups) == list(range(h["n_split"]))
    bounds = sorted(b for g in groups for b in range(g[1], g[1] + g[2] - 1))
    assert bounds == list(range(h["n_bound"]))
    assert len(U) * 32 <= h["up_off"] - h["up_units"]


def test_knob_off_is_the_plan_of_today():
    """the ten byte-fixed tables of tests/test_dp_plan_cpu.py: with split_wide = 0 the common part is mpa_dbg_dp_plan's, and so are its digests"""
    gold = dpplan.golden()["cases"]
    for name, (tasks, over, knobs) in dpplan.cases().items():
        kn = dict(dpplan.KNOBS, split_wide=0)
        kn.update(knobs)
        wide = mpa.dbg_dp_plan_wide(dpplan.dpopt(**over), dpplan.CTG_LEN, dpplan.q_off(), tasks, kn)
        old = mpa.dbg_dp_plan(dpplan.dpopt(**over), dpplan.CTG_LEN, dpplan.q_off(), tasks, kn)
        assert isinstance(wide, bytes) and wide[:-mpa.DP_PLAN_WIDE_TAIL] == old, name
        p = sw.WidePlan(wide)
        assert p.s8[1] == 0 and p.s12[1] == 0 and p.n_bound == p.header["n_bound"], name
        assert p.digests() == gold[name]["digest"], name


@pytest.mark.parametrize("name", ["a_ext_to_the_guard", "odd_counts", "mixed_3000"])
def test_device_planner_model_equals_the_host_planner(name):
    tasks, over = sw.planner_tables()[name]
    want, got = sw.plan(tasks, over), sw.device_plan(None, tasks, over)
    assert isinstance(want, sw.WidePlan), want
    assert isinstance(got, sw.WidePlan), got
    assert want.s8[1] + want.s12[1] > 0
    assert got.buf == want.buf


def test_device_planner_model_still_declines_the_one_wave_class():
    """with the knob, a table whose wide calls all fit the new classes is planned; one call past the guard and it is declined as before"""
    g = sw.guard_limit(dpplan.dpopt())
    r = np.random.default_rng(9320)
    ok = sw.table(r, [(EXT, 1100, 300), (EXT, g, 500), (EXT, 50, 90), (GLOB, 40, 400)])
    assert isinstance(sw.device_plan(None, ok), sw.WidePlan)
    assert sw.device_plan(None, ok, knobs=dict(split_wide=0))[0] == mpa.DP_PLAN_DECLINED
    bad = sw.table(r, [(EXT, 1100, 300), (EXT, g + 1, 500), (EXT, 50, 90)])
    code, why = sw.device_plan(None, bad)
    assert code == mpa.DP_PLAN_DECLINED and "one-wave int32" in why


# ---- the classes over the penalty range: the case lists and tables of tests/test_dp_split_wide_range_gpu.py, without a device
BOUND_IDS = ["al%d-%s" % (c[0], c[2]) for c in WIDE_BOUND_CASES]
TABLE_CLASS = {1032: sw.X_SPLIT8, 1600: sw.X_SPLIT8, 2000: sw.X_SPLIT8, 2048: sw.X_SPLIT8, 2128: sw.X_SPLIT12, 2600: sw.X_SPLIT12, 2664: sw.X_SPLIT12,
               2904: sw.X_SPLIT12, 3072: sw.X_SPLIT12}                           # the class each bound case names at 32 000


def test_capped_matrix():
    full = refbind.mapping_matrix(23)
    for cap in (4, 10):
        m = sw.capped_matrix(cap)
        assert m.dtype == np.int8 and m.shape == (22, 22) and int(m.max()) == cap
        assert np.array_equal(m[full <= cap], full[full <= cap]) and np.all(m[full > cap] == cap)
        assert list(dpplan.dpopt(**sw.opt_overrides(sw.wide_params(cap=cap))).mat) == list(dpplan.dpopt(**sw.low_matrix(cap)).mat)
    assert int(full.max()) == 11 and np.array_equal(sw.capped_matrix(11), full)


@pytest.mark.parametrize("over", [0, 1], ids=["at32000", "at32001"])
@pytest.mark.parametrize("case", WIDE_BOUND_CASES, ids=BOUND_IDS)
def test_wide_bound_sums_and_routing(case, over):
    """the decisive sum of every dpgen.WIDE_BOUND_CASES entry is 32 000, and 32 001 with its key raised; both planners put the call in
    the class the case names at 32 000 and on the one-wave sweep at 32 001 (the device planner's model by declining the table); the
    capped cases need their cap: under the full matrix they are on the one-wave sweep on both sides"""
    al, _, key, cap = case
    P = sw.wide_params(bound_params(case, over), cap)
    ncol = (al + 7) // 8 * 8
    sums = (al * int(P.mat.max()) + ncol * P.ge + max(0, P.end_bonus), P.go + ncol * P.ge)
    assert max(sums) == 32000 + over and (sums[0] > sums[1]) == (key == "end_bonus")
    assert int(P.mat.max()) == (11 if cap is None else cap)
    over_opt = sw.opt_overrides(P)
    o = dpplan.dpopt(**over_opt)
    assert bytes(o.mat) == bytes(dpopt_from_params(P).mat) and (o.go, o.ge, o.end_bonus) == (P.go, P.ge, P.end_bonus)      # what mpa.dp_run is given
    assert sw.may_saturate(al, o) == (over == 1)
    want = TABLE_CLASS[al] if over == 0 else sw.X_HUGE
    assert sw.expected_class(al, o, sw.KNOBS) == want
    r = np.random.default_rng(9330 + al)
    tasks = sw.table(r, [(EXT, al, 900), (EXT, 40, 100), (GLOB, 30, 500)])
    p = sw.plan(tasks, over_opt)
    assert isinstance(p, sw.WidePlan), p
    assert ext_classes(p)[al] == {want}
    d = sw.device_plan(None, tasks, over_opt)
    if over == 0:
        assert isinstance(d, sw.WidePlan) and d.buf == p.buf
    else:
        assert d[0] == mpa.DP_PLAN_DECLINED and "one-wave int32" in d[1]
    if cap is not None:
        full = sw.plan(tasks, sw.opt_overrides(sw.wide_params(bound_params(case, over))))
        assert ext_classes(full)[al] == {sw.X_HUGE}


def test_wide_penalty_points_are_selected_by_the_guard():
    pts = sw.wide_penalty_points()
    assert [kw for kw, _ in pts] == [kw for kw in PENALTY_POINTS if sw.guard_limit(dpopt_from_params(sw.wide_params(kw))) > 1024]
    lim = {repr(kw): l for kw, l in pts}
    assert len(pts) == 16 and lim[repr(dict(ge=4))] == 2131 and lim[repr(dict(end_bonus=100))] == 2657 and lim[repr(dict(end_bonus=1000))] == 2583
    assert sorted(set(lim.values())) == [2131, 2583, 2657, 2665]
    assert all(any(k in kw for kw, _ in pts) for k in ("ge", "go", "io", "xdrop", "end_bonus", "fs", "sp"))


def plan_counts(p):
    """extension calls of X_SPLIT8, X_SPLIT12 and X_HUGE in a plan"""
    T = p.sec["tasks"]
    ext = (T["flag"] & (mpa.F_EXT_LEFT | mpa.F_EXT_RIGHT)) != 0
    return {c: int(np.sum(ext & (T["cls"] == c))) for c in (sw.X_SPLIT8, sw.X_SPLIT12, sw.X_HUGE) if np.any(ext & (T["cls"] == c))}


def check_table(tab, want):
    """the host planner on the very table the GPU test runs: the calls the test expects per class, with the knob and without it; and
    the assertion helper of the GPU tests has teeth -- the class vector of a context without the knob fails it, and so does one call
    that took the one-wave sweep"""
    on, off = tab.plan(1), tab.plan(0)
    assert isinstance(on, sw.WidePlan) and isinstance(off, sw.WidePlan), (on, off)
    assert plan_counts(on) == {c: n for c, n in want.items() if n} and plan_counts(off) == {sw.X_HUGE: tab.n_wide()}
    assert want.get(sw.X_SPLIT8, 0) + want.get(sw.X_SPLIT12, 0) + want.get(sw.X_HUGE, 0) == tab.n_wide()
    good = tab.class_counts(1)
    sw.check_classes(good, tab, 1, want)
    sw.check_classes(tab.class_counts(0), tab, 0, {sw.X_HUGE: tab.n_wide()})
    if want.get(sw.X_SPLIT8, 0) + want.get(sw.X_SPLIT12, 0):
        with pytest.raises(AssertionError, match="swept"):
            sw.check_classes(tab.class_counts(0), tab, 1, want)                  # the knob-off context in the knob-on one's place
        c = sw.X_SPLIT8 if want.get(sw.X_SPLIT8, 0) else sw.X_SPLIT12
        one = list(good)
        one[c] -= 1
        one[sw.X_HUGE] += 1
        with pytest.raises(AssertionError, match="swept"):
            sw.check_classes(one, tab, 1, want)
        with pytest.raises(AssertionError, match="rules of the classes"):
            sw.check_classes(good, tab, 1, {sw.X_HUGE: tab.n_wide()})            # a test that expects the wrong classes
    return on


def ora_equals_ref(tab):
    """the expected values are the reference's own, not only the restatement's"""
    e, r = tab.expect("oracle"), tab.expect("reference")
    assert len(e) == len(tab.tasks)
    bad = [(k, tab.meta[k], e[k][:3], r[k][:3]) for k in range(len(e)) if e[k] != r[k]]
    assert not bad, bad[:5]


@pytest.mark.parametrize("name", ["twelve_blocks", "group_shapes", "short_windows", "xdrop_stops"])
def test_range_tables(oracle_built, name):
    tab, want = sw.range_tables()[name]
    p = check_table(tab, want)
    T, W = p.sec["tasks"], p.sec["ewaves"]
    assert p.s8[1] == 0
    groups = [[(int(T[i]["al"]), int(T[i]["nl"])) for i in W[d]["task"][:2] if i >= 0] for d in range(p.s12[0], p.s12[0] + p.s12[1])]
    if name == "twelve_blocks":
        assert sorted(al for g in groups for al, _ in g) == sorted(2 * sw.TWELVE_BLOCK_ALS) and all(len(g) == 2 for g in groups)
        assert all(8000 < nl < 10600 for g in groups for _, nl in g)
    if name == "group_shapes":                                                   # (3 072, 2 049) share a group, the second 3 072 call has an empty half
        assert [[al for al, _ in g] for g in groups] == [[3072, 2049], [3072]] and groups[1][0][1] == 5000 and p.header["n_huge"] == 1
    if name == "short_windows":
        assert sorted(nl for g in groups for al, nl in g if al == 3072) == sorted(2 * sw.SHORT_ROWS_3072)
    if name == "xdrop_stops":                                                    # the x-drop does stop: far from the end of the protein, on both sides
        stop = {(len(tab.pairs[k][0]), fl): e[1] for (k, fl, _), e in zip(tab.meta, tab.expect("oracle"))}
        assert all(n < 2900 for n in stop.values()) and sorted(stop.values())[-2] > 900, stop


@pytest.mark.parametrize("point", sw.wide_penalty_points(), ids=lambda p: ",".join("%s=%s" % x for x in p[0].items()))
def test_penalty_point_tables(oracle_built, point):
    kw, lim = point
    tab, want = sw.penalty_table(kw, lim)
    als = sorted(set(a for a in tab.ext_als() if a > 1024))
    assert als == sorted({1032, min(lim, 2048), lim, lim + 1}) and want[sw.X_HUGE] == 2
    assert not sw.may_saturate(lim, tab.opt) and sw.may_saturate(lim + 1, tab.opt)
    assert max(a for a in tab.ext_als() if a <= 1024) == 1000 and sum(fl == mpa.F_CIGAR for _, fl, _ in tab.meta) == len(sw.MIXED_ALS)
    assert len({io for _, _, io in tab.meta}) == 2                               # io and io_alt, as build_workload deals them
    p = check_table(tab, want)
    assert p.header["n_huge"] == 2


@pytest.mark.parametrize("over", [0, 1], ids=["at32000", "at32001"])
@pytest.mark.parametrize("case", WIDE_BOUND_CASES, ids=BOUND_IDS)
def test_bound_tables(oracle_built, case, over):
    """the GPU test's batch of a bound case: the calls at al in the case's class at 32 000 and on the one-wave sweep at 32 001, the
    hot pairs at the highest score the matrix gives, oracle == reference on every call"""
    al, cap = case[0], case[3]
    tab, want = sw.bound_table(case, over)
    assert sorted(set(tab.ext_als())) == [al - 8, al, al + 8] and tab.ext_als().count(al) == 4
    at = want.get(TABLE_CLASS[al], 0) if over == 0 else want.get(sw.X_HUGE, 0)
    assert at >= 4 and (over == 0 or want.get(TABLE_CLASS[al], 0) <= 2)
    if case[2] == "end_bonus" or al == 3072:
        assert sw.expected_class(al + 8, tab.opt, sw.KNOBS) == sw.X_HUGE
    check_table(tab, want)
    hot = [e for (k, fl, _), e in zip(tab.meta, tab.expect("oracle")) if tab.pairs[k][1] == b"W" * al]
    assert len(hot) == 2 and all(e[:3] == (3 * al, al, al * int(tab.P.mat.max()) + tab.P.end_bonus) for e in hot), hot


def all_tables():
    """(id, maker) of every table the GPU tests run"""
    out = [("range-" + name, lambda name=name: sw.range_tables()[name][0]) for name in ("twelve_blocks", "group_shapes", "short_windows", "xdrop_stops")]
    out += [("point-" + ",".join("%s=%s" % x for x in kw.items()), lambda kw=kw, lim=lim: sw.penalty_table(kw, lim)[0]) for kw, lim in sw.wide_penalty_points()]
    out += [("bound-al%d-%s-%d" % (c[0], c[2], 32000 + over), lambda c=c, over=over: sw.bound_table(c, over)[0]) for c in WIDE_BOUND_CASES for over in (0, 1)]
    return out


@pytest.mark.skipif(not refbind.have_ref(), reason="the reference is not built")
@pytest.mark.parametrize("make", [m for _, m in all_tables()], ids=[i for i, _ in all_tables()])
def test_expected_values_are_the_references(oracle_built, make):
    """oracle == reference (ns_global_gs16b) on every call of every table of the GPU tests: random and hot pairs on both sides of every
    bound, full 3 072-column calls under the capped matrix, the penalty points"""
    ora_equals_ref(make())


def test_hooks_are_in_the_hooks_library():
    for name in ("mpa_dbg_dp_plan_wide", "mpa_dbg_dp_plan_device_wide", "mpa_dbg_dp_last_classes"):
        assert hasattr(mpa.dbg_lib(), name) and not hasattr(mpa.lib(), name)


def test_planners_under_sanitizers(tmp_path):
    """tests/dpsplit_check.cpp: random tables through the host planner and the planner core with teams of 1 and 256, every output section
    in a heap block of exactly the executor's bound"""
    root = refbind.ROOT
    csrc = os.path.join(root, "miniprot_amd", "csrc")
    exe = str(tmp_path / "dpsplit_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-I" + csrc,
                    os.path.join(root, "tests", "dpsplit_check.cpp"), os.path.join(csrc, "dp_plan.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 mismatches" in out.stdout and "ERROR" not in out.stderr
