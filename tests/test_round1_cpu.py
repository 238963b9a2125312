"""MPA_GPU_ROUND1 without a device.  The knob belongs to run_dp_rounds(), the driver of a batch that has a DP
context: a caller that drives the mpa_batch_* stage machine itself (tests/hostpipe.py, with the oracle as DP executor) never reaches it and
keeps today's path silently -- same text, same MPA_SPANS_DUMP, no note; MPA_GPU_SPANS=model keeps the model path; and the hook, which has
no host model of a DP round, returns the argument error without a context.  The cases' round-1 tables hold no call the device planner
declines: that is what the GPU tests' note counts rest on, and it is checked here by classifying the stage machine's own tasks."""
import ctypes as C
import numpy as np
import pytest
import miniprot_amd as mpa
import alnstats
import dpplan
import regioncases
import round1cases as r1
import spanscases
import spansdump
from spanscases import MODEL_NOTE
from hostpipe import map_batch_result, oracle_executor


def _memo(executor):
    seen = {}

    def run(idx, queries, dpopt, tasks):
        key = tasks.tobytes()
        if key not in seen:
            seen[key] = executor(idx, queries, dpopt, tasks)
        return seen[key]
    return run


def _run(idx, mo, q, ex, knobs, tmp_path, monkeypatch, capfd, tag):
    for k in ("MPA_GPU_ROUND1", "MPA_GPU_SPANS", "MPA_GPU_ROUND2"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("MPA_TIMING", "1")
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    capfd.readouterr()
    res, dump = spanscases.with_dump(monkeypatch, str(tmp_path / (tag + ".dump")), lambda: map_batch_result(idx, mo, q, ex, n_threads=4))
    return mpa.format_output(idx, mo, q, res)[0], dump, capfd.readouterr().err


def test_the_stage_machine_without_a_context_keeps_todays_path(oracle_built, tmp_path, monkeypatch, capfd):
    idx, mo, q, ref = spanscases.case_inputs("syn_a", tmp_path)
    ex = _memo(oracle_executor)
    plain = _run(idx, mo, q, ex, {}, tmp_path, monkeypatch, capfd, "plain")
    knob = _run(idx, mo, q, ex, {"MPA_GPU_ROUND1": "1"}, tmp_path, monkeypatch, capfd, "knob")
    both = _run(idx, mo, q, ex, {"MPA_GPU_ROUND1": "1", "MPA_GPU_SPANS": "1"}, tmp_path, monkeypatch, capfd, "both")
    idx.close()
    assert plain[0] == ref and len(plain[1]) > 0
    for run in (knob, both):
        assert run[0] == ref and run[1] == plain[1], spansdump.first_difference(run[1], plain[1])
        assert "round 1 resident" not in run[2] and "resident" not in run[2]


def test_the_model_path_stays(oracle_built, tmp_path, monkeypatch, capfd):
    idx, q, mo = spanscases.short_gene()
    ex = _memo(oracle_executor)
    plain = _run(idx, mo, q, ex, {}, tmp_path, monkeypatch, capfd, "plain")
    model = _run(idx, mo, q, ex, {"MPA_GPU_SPANS": "model", "MPA_GPU_ROUND1": "1"}, tmp_path, monkeypatch, capfd, "model")
    idx.close()
    assert model[0] == plain[0] and len(plain[1]) > 0 and model[1] == plain[1], spansdump.first_difference(model[1], plain[1])
    assert MODEL_NOTE in model[2] and MODEL_NOTE not in plain[2] and "round 1 resident" not in model[2]


def test_the_hook_is_exported_and_needs_a_context():
    """by the hooks' own library: libmpamd.so's C ABI (tests/test_abi_symbols.py) is what it was"""
    assert hasattr(mpa.dbg_lib(), "mpa_dbg_round1_chain") and not hasattr(mpa.lib(), "mpa_dbg_round1_chain")
    idx, q, mo = spanscases.world()
    P = spanscases.Plans(q)
    P.add(left=(30, 10), right=(12, 4))
    plans, segs, rst1, _ = P.arrays()
    tasks = np.zeros(len(rst1), dtype=mpa.DP_TASK)
    r = mpa.dbg_round1_chain(None, idx, mo, mpa.dpopt_from(mo), q, plans, segs, tasks)
    idx.close()
    assert len(r) == 2 and r[0] == -5 and "missing arguments" in r[1], r     # MPA_ERR_ARG


def _round1_tasks(idx, mo, q):
    """the round-1 task table of a batch, from the stage machine"""
    L = mpa.lib()
    b = L.mpa_batch_begin(idx.h, C.byref(mo), C.byref(q.c), 4)
    assert b
    dpopt, ptr = mpa.DpOpt(), C.c_void_p()
    n = L.mpa_batch_dp_tasks(b, C.byref(ptr), C.byref(dpopt))
    tasks = np.frombuffer((C.c_char * (max(n, 0) * mpa.DP_TASK.itemsize)).from_address(ptr.value), dtype=mpa.DP_TASK).copy() if n > 0 else np.zeros(0, mpa.DP_TASK)
    mpa.Result(L.mpa_batch_finish(b)).close()              # (destroys the batch, whatever round it is in)
    return tasks, dpopt


@pytest.mark.parametrize("name", ["syn_a", "syn_m", "edge", "syn_b"])
def test_the_device_planner_takes_round_1_of_the_gpu_tests_cases(name, tmp_path):
    """no extension call of more than 1 024 columns (class X_HUGE) and one traceback chunk: what dp_plan_from_head declines.  This is an
    approximation of the device planner's own predicate (dp_plan_device_declines and the header's status bits, which need a device): the
    host planner must take the table, and the chunk count is bounded by hand from the rows of the plain traceback calls at the widest
    class.  The GPU tests' note counts assert the real thing"""
    if name == "edge":
        contigs, prots, names, mo = regioncases.edge_genome()
        idx, q = regioncases.edge_index(contigs), mpa.Queries(prots, names)
    else:
        idx, mo, q, _ = alnstats.case_inputs(name, tmp_path) if name == "syn_m" else spanscases.case_inputs(name, tmp_path)
    tasks, dpopt = _round1_tasks(idx, mo, q)
    ctg_len = [idx.ctg_len(c) for c in range(idx.n_ctg())]
    idx.close()
    assert len(tasks) > 0
    ext = (tasks["flag"] & r1.EXT_BITS) != 0
    assert int(tasks["al"][ext].max(initial=0)) <= 1024, "an extension call of the one-wave int32 class"
    plan = mpa.dbg_dp_plan(dpopt, ctg_len, q.off, tasks, dpplan.KNOBS)
    assert isinstance(plan, bytes), plan                                    # (the host planner takes the table as it is)
    # one traceback chunk: the plain traceback matrices of the calls below the checkpointing threshold fit the budget twice over
    plain_tb = tasks[~ext & (tasks["nl"] < dpplan.KNOBS["lite_min"])]
    assert 2 * int((plain_tb["nl"].astype(np.int64) * 1024 * 2).sum()) < dpplan.KNOBS["tb_budget"]
