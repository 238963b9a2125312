"""The result stages of a DP round (miniprot_amd/csrc/dp_results_core.h; MPA_GPU_ROUND2) without a device.
mpa_dbg_dp_run_resident without a context runs the stages with a team of one on made-up kernel outputs: the records and the dense pool's
offsets must be those of dp_assemble()'s host loop (tests/dpresults.py restates it), byte for byte; the bounds reduction's shared code must
give what dp_plan_prep_bound gives.  A stand-alone program (tests/dpresults_check.cpp, compiled here with AddressSanitizer and UBSan) runs
the stages with teams of one and of 256 threads, every output in a heap block of exactly the driver's bound.  No sanitizer goes near code
loaded into python."""
import os
import subprocess
import numpy as np
import pytest
import miniprot_amd as mpa
import dpplan_device as dd
import dpresults as dr
import refbind

PLANNED = dd.planned()


def _check(tasks, seed, **kw):
    eo, sc, nc, gids = dr.made_up(tasks, np.random.default_rng(seed), **kw)
    want, pool_n = dr.host_loop(tasks, eo, sc, nc, gids)
    got = mpa.dbg_dp_run_resident(None, None, None, None, tasks, (eo, sc, nc, gids))
    assert len(got) == 3, got
    rst, pool, rec = got
    assert rst.tobytes() == want.tobytes()
    assert rec["n_pool"] == pool_n and len(pool) == 0
    assert (rec["prep_bound"], rec["max_nl"], rec["max_al"]) == dr.bounds_of(tasks)
    return rst, rec


@pytest.mark.parametrize("n_ext,n_glob", [(1, 0), (0, 1), (40, 0), (0, 40), (30, 50), (3, 255), (3, 256), (3, 257), (5, 513)],
                         ids=["one_ext", "one_glob", "only_ext", "only_glob", "mixed", "tb255", "tb256", "tb257", "tb513"])
def test_team_of_one_against_the_host_loop(n_ext, n_glob):
    rst, rec = _check(dr.table(9400 + n_ext + n_glob, n_ext, n_glob), 9401)
    assert int((rst["n_cigar"] > 0).sum()) == n_glob


@pytest.mark.parametrize("name", ["spread_default", "ties_3000", "only_ext", "only_glob", "prep_chunk_edge"])
def test_planner_tables(name):
    _check(PLANNED[name][0], 9402)


def test_traceback_calls_without_words():
    tasks = dr.table(9410, 20, 300)
    rst, rec = _check(tasks, 9411, zero_every=3)
    tb = rst[~dr.is_ext(tasks)]
    assert int((tb["n_cigar"] == 0).sum()) >= 100 and rec["n_pool"] == int(tb["n_cigar"].sum())


def test_a_pool_of_more_than_2_31_words():
    """few calls with large counts: the offsets are int64"""
    tasks = dr.table(9420, 2, 5)
    nc = np.full(len(tasks), (1 << 30) - 7, dtype=np.int32)
    rst, rec = _check(tasks, 9421, nc=nc)
    assert rec["n_pool"] == 5 * ((1 << 30) - 7) > 1 << 31 and int(rst["cigar_off"].max()) == 4 * ((1 << 30) - 7)


def test_bounds_at_the_prep_chunk_edges():
    """nl of 0, 1, 1023, 1024 and 1025: 0 + 1 + 1 + 1 + 2 chunks"""
    r = np.random.default_rng(9430)
    tasks = dr._table(r, [(dr.GLOB, 30, nl) for nl in (0, 1, 1023, 1024, 1025)] + [(dr.EXT, 200, 1)])
    rst, rec = _check(tasks, 9431)
    assert (rec["prep_bound"], rec["max_nl"], rec["max_al"]) == (6, 1025, 200)
    for nl, want in ((0, 0), (1, 1), (1023, 1), (1024, 1), (1025, 2)):
        assert _check(dr._table(r, [(dr.GLOB, 9, nl)]), 9432)[1]["prep_bound"] == want


def test_the_hook_is_in_the_hooks_library():
    """libmpamd.so's C ABI (tests/test_abi_symbols.py) is what it was"""
    assert hasattr(mpa.dbg_lib(), "mpa_dbg_dp_run_resident") and not hasattr(mpa.lib(), "mpa_dbg_dp_run_resident")


def test_the_hook_refuses_a_list_that_names_an_extension_call():
    tasks = dr.table(9440, 3, 3)
    eo, sc, nc, gids = dr.made_up(tasks, np.random.default_rng(9441))
    gids[0] = int(np.flatnonzero(dr.is_ext(tasks))[0])
    r = mpa.dbg_dp_run_resident(None, None, None, None, tasks, (eo, sc, nc, gids))
    assert len(r) == 2 and r[0] < 0, r


def test_stages_under_sanitizers(tmp_path):
    """tests/dpresults_check.cpp: random tables through the stages with a team of one and a team of 256 threads, every output in a heap
    block of exactly the driver's bound, compared with the host loop; the bounds against dp_plan_prep_bound"""
    root = refbind.ROOT
    csrc = os.path.join(root, "miniprot_amd", "csrc")
    exe = str(tmp_path / "dpresults_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-I" + csrc,
                    os.path.join(root, "tests", "dpresults_check.cpp"), os.path.join(csrc, "dp_plan.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 mismatches" in out.stdout and "ERROR" not in out.stderr
