"""Main chains to refinement windows through the code the device runs (miniprot_amd/csrc/regions_core.h), on the CPU.

MPA_GPU_REGIONS=model makes stage_windows_from_chains() (host_plan.cpp) run the shared core with a team of one where it otherwise runs
regions_from_chains / sort_regions / assign_parents / select_secondary / extension_limits: the stage machine with the oracle as DP
executor must still print the reference's bytes, and the stage's own result -- MPA_REGIONS_DUMP, tests/regionsdump.py -- must equal the
dump of the run with the knob unset, byte for byte.  A stand-alone program (tests/regions_check.cpp, compiled here with
AddressSanitizer and UBSan) feeds the core hand-written and random chains, with a team of one and a team of 64 threads, and compares
them with plain restatements of the host functions.  No sanitizer goes near code loaded into python."""
import os
import subprocess
import pytest
import miniprot_amd as mpa
import refbind
import regioncases
import regionsdump
from hostpipe import map_batch_result, oracle_executor

MODEL_NOTE = "regions: shared core"
DEVICE_NOTE = "regions on the GPU"


def _memo(executor):
    """the DP results of a round, computed once: the two runs of a case hand out the same tasks"""
    seen = {}

    def run(idx, queries, dpopt, tasks):
        key = tasks.tobytes()
        if key not in seen:
            seen[key] = executor(idx, queries, dpopt, tasks)
        return seen[key]
    return run


@pytest.mark.parametrize("name", ["syn_a", "syn_b", "syn_d", "syn_i", "syn_h", "opt_b12"])
def test_shared_core_prints_the_reference_and_leaves_the_host_regions(oracle_built, name, tmp_path, monkeypatch, capfd):
    idx, mo, q, ref = regioncases.case_inputs(name, tmp_path)
    ex = _memo(oracle_executor)
    monkeypatch.setenv("MPA_TIMING", "1")
    monkeypatch.delenv("MPA_GPU_REGIONS", raising=False)
    capfd.readouterr()
    host, dump_host = regioncases.with_dump(monkeypatch, str(tmp_path / "host.dump"), lambda: map_batch_result(idx, mo, q, ex, n_threads=4))
    err_host = capfd.readouterr().err
    monkeypatch.setenv("MPA_GPU_REGIONS", "model")
    model, dump_model = regioncases.with_dump(monkeypatch, str(tmp_path / "model.dump"), lambda: map_batch_result(idx, mo, q, ex, n_threads=4))
    err_model = capfd.readouterr().err
    assert MODEL_NOTE in err_model, "MPA_GPU_REGIONS=model did not run the shared core"
    assert MODEL_NOTE not in err_host and DEVICE_NOTE not in err_host and DEVICE_NOTE not in err_model
    text = mpa.format_output(idx, mo, q, model)[0]
    if text != ref:
        for x, y in zip(text.split(b"\n"), ref.split(b"\n")):
            if x != y:
                raise AssertionError("first differing line\n ours %r\n ref  %r" % (x[:300], y[:300]))
    assert text == ref
    assert mpa.format_output(idx, mo, q, host)[0] == ref
    parsed = regionsdump.parse(dump_host)
    assert [p[0] for p in parsed] == list(range(len(q.seqs))) and sum(len(p[2]) for p in parsed) >= len(q.seqs) // 2
    assert dump_model == dump_host, regionsdump.first_difference(dump_model, dump_host)
    idx.close()


def test_edge_genome_through_the_shared_core(oracle_built, tmp_path, monkeypatch):
    """the edge genome of the GPU tests on the CPU: chains across strand and contig boundaries in both majority directions, 84 chains
    of which 79 share a score (the radix passes of the region order)"""
    contigs, prots, names, mo = regioncases.edge_genome()
    idx, q, ex = regioncases.edge_index(contigs), mpa.Queries(prots, names), _memo(oracle_executor)
    monkeypatch.delenv("MPA_GPU_REGIONS", raising=False)
    host, dump_host = regioncases.with_dump(monkeypatch, str(tmp_path / "host.dump"), lambda: map_batch_result(idx, mo, q, ex, n_threads=4))
    flags, most, ties = regioncases.edge_findings(dump_host)
    assert flags == {1, 2} and most > 64 and ties > 64, (flags, most, ties)
    monkeypatch.setenv("MPA_GPU_REGIONS", "model")
    model, dump_model = regioncases.with_dump(monkeypatch, str(tmp_path / "model.dump"), lambda: map_batch_result(idx, mo, q, ex, n_threads=4))
    assert dump_model == dump_host, regionsdump.first_difference(dump_model, dump_host)
    ref = open(os.path.join(refbind.ROOT, "tests", "golden", regioncases.EDGE_REF), "rb").read()
    assert mpa.format_output(idx, mo, q, model)[0] == ref and mpa.format_output(idx, mo, q, host)[0] == ref
    idx.close()


def test_device_request_without_a_context_is_the_host_path(oracle_built, tmp_path, monkeypatch, capfd):
    """MPA_GPU_REGIONS=1 (and 0) where no device seeded -- the stage machine driven from outside, mpa_batch_begin -- keeps the host
    functions: no note, the same dump, the same bytes"""
    idx, mo, q, ref = regioncases.case_inputs("syn_a", tmp_path)
    q = mpa.Queries(q.seqs[:8], q.names[:8])
    ex = _memo(oracle_executor)
    monkeypatch.setenv("MPA_TIMING", "1")
    monkeypatch.delenv("MPA_GPU_REGIONS", raising=False)
    host, dump_host = regioncases.with_dump(monkeypatch, str(tmp_path / "host.dump"), lambda: map_batch_result(idx, mo, q, ex, n_threads=2))
    text_host = mpa.format_output(idx, mo, q, host)[0]
    assert text_host and text_host in ref
    for v in ("0", "1"):
        monkeypatch.setenv("MPA_GPU_REGIONS", v)
        capfd.readouterr()
        res, dump = regioncases.with_dump(monkeypatch, str(tmp_path / "knob.dump"), lambda: map_batch_result(idx, mo, q, ex, n_threads=2))
        err = capfd.readouterr().err
        assert DEVICE_NOTE not in err and MODEL_NOTE not in err and "declined" not in err
        assert dump == dump_host, regionsdump.first_difference(dump, dump_host)
        assert mpa.format_output(idx, mo, q, res)[0] == text_host
    idx.close()


def test_core_against_plain_restatements_under_sanitizers(tmp_path):
    """tests/regions_check.cpp: chains across two strands (head larger, tail larger, equal), a strand without blocks in front of a
    chain, 65 and 300 regions of one score and runs of at most 64, a region secondary to the second of two overlapping primaries,
    uncovered at mask_len and one above, best_n reached, two regions at one place, neighbours closer than max_ext and closer than
    100, chains of more than 128 anchors, zero chains and one chain, 400 random inputs; a team of one and a team of 64 threads"""
    root = refbind.ROOT
    exe = str(tmp_path / "regions_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                    "-I" + os.path.join(root, "miniprot_amd", "csrc"), os.path.join(root, "tests", "regions_check.cpp"), "-o", exe, "-lpthread"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 mismatches" in out.stdout and "ERROR" not in out.stderr and "DOES NOT SHOW" not in out.stderr
