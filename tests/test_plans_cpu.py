"""Refinement chains to regions, alignment plans, round-1 DP tasks and gap segments through the code the device runs
(miniprot_amd/csrc/plans_core.h), on the CPU.

MPA_GPU_PLANS=model makes batch_plan_phase() (host_plan.cpp) collect the chains of every refinement window of a query and run the shared
core with a team of one where it otherwise runs refine_region_from_chains / sort_regions / assign_parents / select_secondary /
extension_limits / mark_reliable_anchors / plan_alignment / plan_round1: the stage machine with the oracle as DP executor must still
print the reference's bytes, and the step's own result -- MPA_PLANS_DUMP, tests/plansdump.py -- must equal the dump of the run with the
knob unset, byte for byte.  A stand-alone program (tests/plans_check.cpp, compiled here with AddressSanitizer and UBSan) feeds the core
hand-written and random inputs, with a team of one and a team of 64 threads, and compares them with plain restatements of the host
functions.  No sanitizer goes near code loaded into python."""
import os
import subprocess
import pytest
import miniprot_amd as mpa
import refbind
import regioncases
import planscases
import plansdump
from planscases import MODEL_NOTE, DEVICE_NOTE
from hostpipe import map_batch_result, oracle_executor


def _memo(executor):
    """the DP results of a round, computed once: the two runs of a case hand out the same tasks"""
    seen = {}

    def run(idx, queries, dpopt, tasks):
        key = tasks.tobytes()
        if key not in seen:
            seen[key] = executor(idx, queries, dpopt, tasks)
        return seen[key]
    return run


@pytest.mark.parametrize("name", planscases.CASES)
def test_shared_core_prints_the_reference_and_leaves_the_host_plans(oracle_built, name, tmp_path, monkeypatch, capfd):
    idx, mo, q, ref = planscases.case_inputs(name, tmp_path)
    ex = _memo(oracle_executor)
    monkeypatch.setenv("MPA_TIMING", "1")
    monkeypatch.delenv("MPA_GPU_PLANS", raising=False)
    capfd.readouterr()
    host, dump_host = planscases.with_dump(monkeypatch, str(tmp_path / "host.dump"), lambda: map_batch_result(idx, mo, q, ex, n_threads=4))
    err_host = capfd.readouterr().err
    monkeypatch.setenv("MPA_GPU_PLANS", "model")
    model, dump_model = planscases.with_dump(monkeypatch, str(tmp_path / "model.dump"), lambda: map_batch_result(idx, mo, q, ex, n_threads=4))
    err_model = capfd.readouterr().err
    assert MODEL_NOTE in err_model, "MPA_GPU_PLANS=model did not run the shared core"
    assert MODEL_NOTE not in err_host and DEVICE_NOTE not in err_host and DEVICE_NOTE not in err_model
    text = mpa.format_output(idx, mo, q, model)[0]
    if text != ref:
        for x, y in zip(text.split(b"\n"), ref.split(b"\n")):
            if x != y:
                raise AssertionError("first differing line\n ours %r\n ref  %r" % (x[:300], y[:300]))
    assert text == ref
    assert mpa.format_output(idx, mo, q, host)[0] == ref
    n_q, n_reg, n_plan, n_task, n_seg, n_short, _ = planscases.totals(dump_host)
    assert n_q == len(q.seqs) and n_reg >= len(q.seqs) // 2
    if name == "syn_i":                                        # -A: the step stops behind the selection
        assert n_plan == 0 and n_task == 0 and n_seg == 0
    else:
        assert n_plan >= len(q.seqs) // 2 and n_task > n_plan and n_seg > n_short > 0
    assert dump_model == dump_host, plansdump.first_difference(dump_model, dump_host)
    idx.close()


def test_edge_genome_through_the_shared_core(oracle_built, tmp_path, monkeypatch):
    """the edge genome of the regions tests: regions on reverse strands and at contig ends, a family of 84 copies whose regions share
    a score (the radix passes of the second region order)"""
    contigs, prots, names, mo = regioncases.edge_genome()
    idx, q, ex = regioncases.edge_index(contigs), mpa.Queries(prots, names), _memo(oracle_executor)
    monkeypatch.delenv("MPA_GPU_PLANS", raising=False)
    host, dump_host = planscases.with_dump(monkeypatch, str(tmp_path / "host.dump"), lambda: map_batch_result(idx, mo, q, ex, n_threads=4))
    assert max(len(e[1]) for e in plansdump.parse(dump_host)) > 64
    monkeypatch.setenv("MPA_GPU_PLANS", "model")
    model, dump_model = planscases.with_dump(monkeypatch, str(tmp_path / "model.dump"), lambda: map_batch_result(idx, mo, q, ex, n_threads=4))
    assert dump_model == dump_host, plansdump.first_difference(dump_model, dump_host)
    ref = open(os.path.join(refbind.ROOT, "tests", "golden", regioncases.EDGE_REF), "rb").read()
    assert mpa.format_output(idx, mo, q, model)[0] == ref and mpa.format_output(idx, mo, q, host)[0] == ref
    idx.close()


def test_device_request_without_a_context_is_the_host_path(oracle_built, tmp_path, monkeypatch, capfd):
    """MPA_GPU_PLANS=1 (and 0) where no device refined -- the stage machine driven from outside, mpa_batch_begin -- keeps the host
    functions: no note, the same dump, the same bytes"""
    idx, mo, q, ref = planscases.case_inputs("syn_a", tmp_path)
    q = mpa.Queries(q.seqs[:8], q.names[:8])
    ex = _memo(oracle_executor)
    monkeypatch.setenv("MPA_TIMING", "1")
    monkeypatch.delenv("MPA_GPU_PLANS", raising=False)
    host, dump_host = planscases.with_dump(monkeypatch, str(tmp_path / "host.dump"), lambda: map_batch_result(idx, mo, q, ex, n_threads=2))
    text_host = mpa.format_output(idx, mo, q, host)[0]
    assert text_host and text_host in ref
    for v in ("0", "1"):
        monkeypatch.setenv("MPA_GPU_PLANS", v)
        capfd.readouterr()
        res, dump = planscases.with_dump(monkeypatch, str(tmp_path / "knob.dump"), lambda: map_batch_result(idx, mo, q, ex, n_threads=2))
        err = capfd.readouterr().err
        assert DEVICE_NOTE not in err and MODEL_NOTE not in err and "declined" not in err
        assert dump == dump_host, plansdump.first_difference(dump, dump_host)
        assert mpa.format_output(idx, mo, q, res)[0] == text_host
    idx.close()


def test_core_against_plain_restatements_under_sanitizers(tmp_path):
    """tests/plans_check.cpp: windows without chains, the best chain not first and two chains of one score, more than 64 windows,
    chains of 65 and more than 128 anchors; runs of 2 and 3 anchors, breaks at every threshold, trims that empty a run, a region
    without a marked anchor; windows clamped at both contig ends, the 9 / 10 residue thresholds, neighbour limits, a reverse strand;
    no right extension, io against io_end, left windows on both sides of max_ext; the ungapped shortcut at kmer2 and above, a codon
    with an N, lengths that are no multiple of 3; 400 random inputs; a team of one and a team of 64 threads"""
    root = refbind.ROOT
    exe = str(tmp_path / "plans_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                    "-I" + os.path.join(root, "miniprot_amd", "csrc"), os.path.join(root, "tests", "plans_check.cpp"), "-o", exe, "-lpthread"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 mismatches" in out.stdout and "ERROR" not in out.stderr and "DOES NOT SHOW" not in out.stderr
