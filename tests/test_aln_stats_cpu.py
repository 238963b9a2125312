"""The alignment statistics through the code the device runs (miniprot_amd/csrc/aln_stats_core.h), on the CPU.

MPA_GPU_STATS=model makes take_round3() (host_align.cpp) run the shared core with a team of one where it otherwise runs dist_to_stop /
dist_to_start / summarize_alignment: the stage machine with the oracle as DP executor must still print the reference's bytes, and every
field of every hit, feature and CIGAR must equal the run with the knob unset.  A stand-alone program (tests/alnstats_check.cpp,
compiled here with AddressSanitizer and UBSan) feeds the core hand-written CIGARs, with a team of one and a team of 64 threads, and
compares them with a plain walk.  No sanitizer goes near code loaded into python."""
import os
import subprocess
import pytest
import miniprot_amd as mpa
import refbind
import alnstats
from hostpipe import map_batch_result, oracle_executor

MODEL_NOTE = "alignment statistics: shared core"


def _memo(executor):
    """the DP results of a round, computed once: the two runs of a case hand out the same tasks"""
    seen = {}

    def run(idx, queries, dpopt, tasks):
        key = tasks.tobytes()
        if key not in seen:
            seen[key] = executor(idx, queries, dpopt, tasks)
        return seen[key]
    return run


@pytest.mark.parametrize("name", ["syn_a", "syn_b", "syn_h", "syn_m"])
def test_shared_core_prints_the_reference_and_equals_the_host_walk(oracle_built, name, tmp_path, monkeypatch, capfd):
    idx, mo, q, ref = alnstats.case_inputs(name, tmp_path)
    ex = _memo(oracle_executor)
    monkeypatch.setenv("MPA_TIMING", "1")
    monkeypatch.delenv("MPA_GPU_STATS", raising=False)
    capfd.readouterr()
    host = map_batch_result(idx, mo, q, ex, n_threads=4)
    err_host = capfd.readouterr().err
    monkeypatch.setenv("MPA_GPU_STATS", "model")
    model = map_batch_result(idx, mo, q, ex, n_threads=4)
    err_model = capfd.readouterr().err
    assert MODEL_NOTE in err_model, "MPA_GPU_STATS=model did not run the shared core"
    assert MODEL_NOTE not in err_host and "alignment statistics" not in err_host
    text = mpa.format_output(idx, mo, q, model)[0]
    if text != ref:
        for x, y in zip(text.split(b"\n"), ref.split(b"\n")):
            if x != y:
                raise AssertionError("first differing line\n ours %r\n ref  %r" % (x[:300], y[:300]))
    assert text == ref
    a, b = alnstats.result_arrays(model), alnstats.result_arrays(host)
    assert len(b[0]) > 0 and len(b[1]) > 0
    assert alnstats.first_difference(a, b) is None, alnstats.first_difference(a, b)
    idx.close()


def test_knob_zero_is_the_host_walk(oracle_built, monkeypatch, capfd):
    """MPA_GPU_STATS=0 and a device request without a context (the stage machine driven from outside: mpa_batch_begin) keep the host path"""
    idx, mo, q, ref = alnstats.case_inputs("syn_a")
    q = mpa.Queries(q.seqs[:6], q.names[:6])
    ex = _memo(oracle_executor)
    monkeypatch.setenv("MPA_TIMING", "1")
    for v in ("0", "1"):
        monkeypatch.setenv("MPA_GPU_STATS", v)
        capfd.readouterr()
        res = map_batch_result(idx, mo, q, ex, n_threads=2)
        assert "alignment statistics" not in capfd.readouterr().err
        text = mpa.format_output(idx, mo, q, res)[0]
        assert text and text in ref
    idx.close()


@pytest.mark.parametrize("d,e", [(0, 0), (1, 3), (2, 1), (3, 2)])
def test_edge_genome_through_the_shared_core(oracle_built, d, e, monkeypatch):
    """the edge genome of the GPU tests (contigs cut d bases before their first gene and e bases behind their last) on the CPU: the
    shared core against the host walk, field by field"""
    contigs, prots, names = alnstats.edge_genome(d, e)
    idx = mpa.Index.from_nt4(contigs, ["chr1", "chr2"])
    mpa._check(mpa.lib().mpa_idx_build_kmers(idx.h, 4))
    mo = mpa.default_mapopt()
    mo.flag |= 4
    q, ex = mpa.Queries(prots, names), _memo(oracle_executor)
    monkeypatch.delenv("MPA_GPU_STATS", raising=False)
    host = alnstats.result_arrays(map_batch_result(idx, mo, q, ex, n_threads=4))
    monkeypatch.setenv("MPA_GPU_STATS", "model")
    model = alnstats.result_arrays(map_batch_result(idx, mo, q, ex, n_threads=4))
    assert len(host[0]) >= len(prots) // 2 and (d > 0 or host[0]["vs"].min() == 0)
    assert alnstats.first_difference(model, host) is None, alnstats.first_difference(model, host)
    idx.close()


def test_core_against_a_plain_walk_under_sanitizers(tmp_path):
    """tests/alnstats_check.cpp: M runs of 1, 63, 64, 65 and 129 codons; U and V first, last and back to back; F of 1 and 2 bases, G;
    a D across a stop codon; 70 and 100 operations; a codon with N; windows [vs, ve + 1) and [vs, ve); both strands of two contigs"""
    root = refbind.ROOT
    exe = str(tmp_path / "alnstats_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                    "-I" + os.path.join(root, "miniprot_amd", "csrc"), os.path.join(root, "tests", "alnstats_check.cpp"), "-o", exe, "-lpthread"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 mismatches" in out.stdout and "ERROR" not in out.stderr
