"""The accepted spans between the DP rounds and the region CIGARs behind them through the code the device runs
(miniprot_amd/csrc/spans_core.h), on the CPU.

MPA_GPU_SPANS=model makes the stage machine (host_align.cpp) run the shared core with a team of one where it otherwise runs
take_round1_emit_round2 / assemble_alignment / count_exons: with the oracle as DP executor it must still print the reference's bytes,
and what the two steps leave -- MPA_SPANS_DUMP, tests/spansdump.py -- must equal the dump of the run with the knob unset, byte for
byte.  A stand-alone program (tests/spans_check.cpp, compiled here with AddressSanitizer and UBSan) feeds the core hand-written and
random inputs, with a team of one and a team of 64 threads, and compares them with plain restatements of the host functions.  No
sanitizer goes near code loaded into python."""
import os
import subprocess
import numpy as np
import pytest
import miniprot_amd as mpa
import refbind
import regioncases
import spanscases
import spansdump
from spanscases import MODEL_NOTE, DEVICE_NOTE
from hostpipe import map_batch_result, oracle_executor

_dumps = {}                                           # the host dump of every golden case run so far


def _memo(executor):
    """the DP results of a round, computed once: the two runs of a case hand out the same tasks"""
    seen = {}

    def run(idx, queries, dpopt, tasks):
        key = tasks.tobytes()
        if key not in seen:
            seen[key] = executor(idx, queries, dpopt, tasks)
        return seen[key]
    return run


@pytest.mark.parametrize("name", spanscases.CASES)
def test_shared_core_prints_the_reference_and_leaves_the_host_spans(oracle_built, name, tmp_path, monkeypatch, capfd):
    idx, mo, q, ref = spanscases.case_inputs(name, tmp_path)
    ex = _memo(oracle_executor)
    monkeypatch.setenv("MPA_TIMING", "1")
    monkeypatch.delenv("MPA_GPU_SPANS", raising=False)
    capfd.readouterr()
    host, dump_host = spanscases.with_dump(monkeypatch, str(tmp_path / "host.dump"), lambda: map_batch_result(idx, mo, q, ex, n_threads=4))
    err_host = capfd.readouterr().err
    monkeypatch.setenv("MPA_GPU_SPANS", "model")
    model, dump_model = spanscases.with_dump(monkeypatch, str(tmp_path / "model.dump"), lambda: map_batch_result(idx, mo, q, ex, n_threads=4))
    err_model = capfd.readouterr().err
    n_plan = sum(len(p) for _, p in spansdump.parse(dump_host))
    if name == "syn_i":                                        # -A: no plans, nothing for the step to do
        assert n_plan == 0 and MODEL_NOTE not in err_model
    else:
        assert n_plan >= len(q.seqs) // 2
        assert MODEL_NOTE in err_model, "MPA_GPU_SPANS=model did not run the shared core"
    assert MODEL_NOTE not in err_host and DEVICE_NOTE not in err_host and DEVICE_NOTE not in err_model
    text = mpa.format_output(idx, mo, q, model)[0]
    if text != ref:
        for x, y in zip(text.split(b"\n"), ref.split(b"\n")):
            if x != y:
                raise AssertionError("first differing line\n ours %r\n ref  %r" % (x[:300], y[:300]))
    assert text == ref
    assert mpa.format_output(idx, mo, q, host)[0] == ref
    assert dump_model == dump_host, spansdump.first_difference(dump_model, dump_host)
    _dumps[name] = dump_host
    idx.close()


# the branch no golden case reaches (measured with the knob unset: 0 of 344 plans): every planned region of these genomes has a right
# extension that is accepted.  tests/spans_check.cpp makes it by hand, three ways: has_right == 0, r_nt == 0 and r_aa == 0
NOT_IN_THE_GOLDEN_CASES = ("a plan without a right span",)


def test_the_golden_cases_reach_every_branch(oracle_built, tmp_path, monkeypatch):
    """over the union of the golden cases (knob unset; the dumps of the parametrised test above, or fresh ones): both terminal-exon
    repeats taken, a shortcut span, a DP span and a merged boundary each occur.  NOT reached by any golden case: a plan without a
    right span -- tests/spans_check.cpp and the hand-made inputs of the GPU test cover it (has_right == 0, r_nt == 0, r_aa == 0)."""
    monkeypatch.delenv("MPA_GPU_SPANS", raising=False)
    seen = dict.fromkeys(spanscases.BRANCHES, 0)
    for name in spanscases.CASES:
        if name not in _dumps:
            idx, mo, q, _ = spanscases.case_inputs(name, tmp_path)
            _dumps[name] = spanscases.with_dump(monkeypatch, str(tmp_path / (name + ".dump")), lambda: map_batch_result(idx, mo, q, oracle_executor, n_threads=4))[1]
            idx.close()
        for k, v in spanscases.branches(_dumps[name]).items():
            seen[k] += v
    print(seen)
    assert all(v > 0 for k, v in seen.items() if k not in NOT_IN_THE_GOLDEN_CASES), seen
    assert all(seen[k] == 0 for k in NOT_IN_THE_GOLDEN_CASES), "a golden case reaches it now: take it off the list"


def test_edge_genome_through_the_shared_core(oracle_built, tmp_path, monkeypatch):
    """the edge genome of the regions tests: regions on reverse strands and at contig ends"""
    contigs, prots, names, mo = regioncases.edge_genome()
    idx, q, ex = regioncases.edge_index(contigs), mpa.Queries(prots, names), _memo(oracle_executor)
    monkeypatch.delenv("MPA_GPU_SPANS", raising=False)
    host, dump_host = spanscases.with_dump(monkeypatch, str(tmp_path / "host.dump"), lambda: map_batch_result(idx, mo, q, ex, n_threads=4))
    assert sum(len(p) for _, p in spansdump.parse(dump_host)) > 64
    monkeypatch.setenv("MPA_GPU_SPANS", "model")
    model, dump_model = spanscases.with_dump(monkeypatch, str(tmp_path / "model.dump"), lambda: map_batch_result(idx, mo, q, ex, n_threads=4))
    assert dump_model == dump_host, spansdump.first_difference(dump_model, dump_host)
    ref = open(os.path.join(refbind.ROOT, "tests", "golden", regioncases.EDGE_REF), "rb").read()
    assert mpa.format_output(idx, mo, q, model)[0] == ref and mpa.format_output(idx, mo, q, host)[0] == ref
    idx.close()


def test_device_request_without_a_context_is_the_host_path(oracle_built, tmp_path, monkeypatch, capfd):
    """MPA_GPU_SPANS=1 (and 0) where no context runs the DP rounds -- the stage machine driven from outside, mpa_batch_begin -- keeps
    the host functions: no note, the same dump, the same bytes"""
    idx, mo, q, ref = spanscases.case_inputs("syn_a", tmp_path)
    q = mpa.Queries(q.seqs[:8], q.names[:8])
    ex = _memo(oracle_executor)
    monkeypatch.setenv("MPA_TIMING", "1")
    monkeypatch.delenv("MPA_GPU_SPANS", raising=False)
    host, dump_host = spanscases.with_dump(monkeypatch, str(tmp_path / "host.dump"), lambda: map_batch_result(idx, mo, q, ex, n_threads=2))
    text_host = mpa.format_output(idx, mo, q, host)[0]
    assert text_host and text_host in ref and len(dump_host) > 0
    for v in ("0", "1"):
        monkeypatch.setenv("MPA_GPU_SPANS", v)
        capfd.readouterr()
        res, dump = spanscases.with_dump(monkeypatch, str(tmp_path / "knob.dump"), lambda: map_batch_result(idx, mo, q, ex, n_threads=2))
        err = capfd.readouterr().err
        assert DEVICE_NOTE not in err and MODEL_NOTE not in err and "declined" not in err
        assert dump == dump_host, spansdump.first_difference(dump, dump_host)
        assert mpa.format_output(idx, mo, q, res)[0] == text_host
    idx.close()


def test_a_gap_free_gene_still_needs_round_2(oracle_built, tmp_path, monkeypatch):
    """why no batch of the pipeline has a round 2 without tasks: the reference trims a run of anchors so that kmer2 + 1 residues remain on
    either side of the kept ones (mp_filter_seed, align.c:6-31), one more than the ungapped shortcut takes -- a protein that aligns end to
    end without a gap sends both spans to the DP.  (Plans whose spans all take the shortcut run through mpa_dbg_spans on the device and
    through tests/spans_check.cpp.)  The model leaves the host's dump here too."""
    idx, q, mo = spanscases.short_gene()
    monkeypatch.delenv("MPA_GPU_SPANS", raising=False)
    _, host = spanscases.with_dump(monkeypatch, str(tmp_path / "host.dump"), lambda: map_batch_result(idx, mo, q, oracle_executor, n_threads=1))
    monkeypatch.setenv("MPA_GPU_SPANS", "model")
    _, model = spanscases.with_dump(monkeypatch, str(tmp_path / "model.dump"), lambda: map_batch_result(idx, mo, q, oracle_executor, n_threads=1))
    idx.close()
    assert model == host, spansdump.first_difference(model, host)
    (_, plans), = spansdump.parse(host)
    (p, cigar), = plans
    assert p["qs"] == 0 and p["qe"] == len(q.seqs[0]) and list(cigar) == [len(q.seqs[0]) << 4]
    for side in ("left", "right"):
        assert p[side]["ae1"] - p[side]["ae0"] == mo.kmer2 + 1 and p[side]["ne1"] - p[side]["ne0"] == 3 * (mo.kmer2 + 1) and p[side]["task"] >= 0


def test_the_test_hook_is_exported():
    """by the hook's own library, next to the product: libmpamd.so's C ABI (tests/test_abi_symbols.py) is what it was"""
    assert hasattr(mpa.dbg_lib(), "mpa_dbg_spans")


def test_core_against_plain_restatements_under_sanitizers(tmp_path):
    """tests/spans_check.cpp: an empty left span followed by an M that merges into its zero-length word; the repeat conditions at each
    threshold; the right span with r_nt == 0, r_aa == 0 and has_right == 0; the shortcut at kmer2 and kmer2 + 1, nlen != 3 alen, a codon
    with an N; the boundaries M|M, M|I, 10|10, 11|11 and N|N; seven single-word M segments in a row; plans with 0, 1, 63, 64, 65 and
    200 gap segments; segments of 1, 64, 65 and 300 words; 400 random plans; a team of one and a team of 64 threads"""
    root = refbind.ROOT
    exe = str(tmp_path / "spans_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                    "-I" + os.path.join(root, "miniprot_amd", "csrc"), os.path.join(root, "tests", "spans_check.cpp"), "-o", exe, "-lpthread"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 mismatches" in out.stdout and "ERROR" not in out.stderr and "DOES NOT SHOW" not in out.stderr
