"""The device planner of a DP round (MPA_GPU_DPPLAN) as its model: mpa_dbg_dp_plan_device without a context runs
the planner's stages (miniprot_amd/csrc/dp_plan_core.h) on the host with a team of one.  What it leaves must be the host planner's plan
(mpa_dbg_dp_plan), every section and every header field, byte for byte; tables the device planner declines must say so.  A stand-alone
program (tests/dpplan_check.cpp, compiled here with AddressSanitizer and UBSan) runs the same stages on random tables with every output
in a buffer of exactly the driver's bound.  No sanitizer goes near code loaded into python."""
import os
import subprocess
import pytest
import miniprot_amd as mpa
import dpplan
import dpplan_device as dd
import refbind

PLANNED = dd.planned()
DECLINED = dd.declined()


@pytest.mark.parametrize("name", sorted(PLANNED))
def test_the_model_leaves_the_host_planners_plan(name):
    tasks, over, knobs = PLANNED[name]
    want = dpplan.plan(tasks, over, knobs)
    dd.assert_same_plan(dd.device_plan(None, tasks, over, knobs), want)


def test_the_tables_reach_what_they_are_for():
    """T_MB, every extension class up to X_SPLIT4, the checkpointed classes and T_LITE_W4 occur; the class runs have the lengths their
    names say; the ties table has four row counts"""
    h = dpplan.plan(*PLANNED["spread_c_wide"]).header
    assert all(h["ewave_cnt%d" % k] > 0 for k in range(7) if k != 3) and h["ewave_cnt3"] == 0 and h["dwave_cnt"] > 0 and all(h["lwave_cnt%d" % k] > 0 for k in range(4)) and h["l12_cnt"] > 0
    assert h["n_split"] > 0 and h["bnd_total"] > 0 and h["n_huge"] == 0
    h = dpplan.plan(*PLANNED["spread_k_no_dual_no_prio"]).header                      # (MPA_DP_EXT_DUAL=0: the two-wave groups instead of X_128)
    assert h["ewave_cnt3"] > 0 and h["dwave_cnt"] == 0
    for n in (1, 7, 8, 9):
        t = dpplan.plan(*PLANNED["x16_run_%d" % n]).sec["tasks"]
        assert int(((t["cls"] == 0) & (t["flag"] & (mpa.F_EXT_LEFT | mpa.F_EXT_RIGHT) != 0)).sum()) == n
    for n in (1, 3):
        assert int((dpplan.plan(*PLANNED["lite_w4_run_%d" % n]).sec["tasks"]["cls"] == 12).sum()) == n
    t = PLANNED["ties_3000"][0]
    assert len(t) == 3000 and len(set(t["nl"].tolist())) == 4
    assert sorted(set(PLANNED["prep_chunk_edge"][0]["nl"].tolist())) == [3, 1023, 1024, 1025]
    p = dpplan.plan(*PLANNED["only_ext"])
    assert p.header["n_glob"] == 0 and p.header["n_ext"] == p.header["n"]
    p = dpplan.plan(*PLANNED["only_glob"])
    assert p.header["n_ext"] == 0 and p.header["n_tb_chunks"] == 1


@pytest.mark.parametrize("name", sorted(DECLINED))
def test_the_model_declines(name):
    tasks, over, knobs = DECLINED[name]
    r = dd.device_plan(None, tasks, over, knobs)
    assert isinstance(r, tuple) and r[0] == mpa.DP_PLAN_DECLINED, r


def test_why_the_cases_decline():
    """a_ext and f_saturate have calls of class X_HUGE (7, among the extension calls), d_budget more than one traceback chunk"""
    c = dpplan.cases()
    for name in ("a_ext", "f_saturate"):
        p = dpplan.plan(*c[name])
        assert p.header["n_huge"] > 0, name
    assert dpplan.plan(*c["d_budget"]).header["n_tb_chunks"] > 1
    assert "X_HUGE" in dd.device_plan(None, *c["a_ext"])[1] or "one-wave" in dd.device_plan(None, *c["a_ext"])[1]
    assert "chunk" in dd.device_plan(None, *c["d_budget"])[1]


def test_the_hook_is_in_the_hooks_library():
    """libmpamd.so's C ABI (tests/test_abi_symbols.py) is what it was"""
    assert hasattr(mpa.dbg_lib(), "mpa_dbg_dp_plan_device") and not hasattr(mpa.lib(), "mpa_dbg_dp_plan_device")


def test_stages_under_sanitizers(tmp_path):
    """tests/dpplan_check.cpp: random tables of up to 5 000 calls through the stages with a team of one, every output in a guarded slot
    sized exactly by the driver's bounds, compared with the host planner"""
    root = refbind.ROOT
    csrc = os.path.join(root, "miniprot_amd", "csrc")
    exe = str(tmp_path / "dpplan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-I" + csrc,
                    os.path.join(root, "tests", "dpplan_check.cpp"), os.path.join(csrc, "dp_plan.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 mismatches" in out.stdout and "ERROR" not in out.stderr
