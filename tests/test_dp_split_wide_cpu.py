"""MPA_DP_SPLIT_WIDE without a device: extension calls of 1 025..3 072 columns classified as X_SPLIT8 / X_SPLIT12 (8 / 12 workgroups per
pair of calls) by the host planner (mpa_dbg_dp_plan_wide) and by the model of the device planner (mpa_dbg_dp_plan_device_wide, ctx None),
what the plan promises the executor (groups, boundaries, units, bytes of the granule pool), and the knob's absence: with split_wide = 0 the
plan is mpa_dbg_dp_plan's, byte for byte.  A stand-alone program (tests/dpsplit_check.cpp, compiled here with AddressSanitizer and UBSan)
runs random tables through both planners with every pool at exactly the executor's bound."""
import os
import subprocess
import numpy as np
import pytest
import miniprot_amd as mpa
import dpplan
import refbind
import splitwide as sw
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
