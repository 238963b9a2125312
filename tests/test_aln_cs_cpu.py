"""The cs:Z: difference strings through the code the device runs (miniprot_amd/csrc/aln_cs_core.h), on the CPU.

MPA_GPU_CS=model makes take_round3() (host_align.cpp) build the body of every aligned region's cs string with the shared core and a
team of one; the region carries it to the result and the formatter pastes it in where it otherwise walks the alignment itself
(put_cs_body, host_format.cpp).  The stage machine with the oracle as DP executor must still print the reference's bytes, the format
note must say that every string was carried and none built, and MPA_CS_DUMP must hold the same bodies as the run with the knob unset.
A stand-alone program (tests/alncs_check.cpp, compiled here with AddressSanitizer and UBSan) feeds the core hand-written CIGARs, with
a team of one and a team of 64 threads, into guarded slots and compares them with a plain walk.  No sanitizer goes near code loaded
into python."""
import os
import subprocess
import pytest
import miniprot_amd as mpa
import refbind
import alnstats
import csdump
import golden
from hostpipe import map_batch_result, oracle_executor

MODEL_NOTE = "cs strings: shared core"
GOLDEN = ["syn_a", "syn_b", "syn_h", "syn_e", "long_u"]


def _memo(executor):
    """the DP results of a round, computed once: the two runs of a case hand out the same tasks"""
    seen = {}

    def run(idx, queries, dpopt, tasks):
        key = tasks.tobytes()
        if key not in seen:
            seen[key] = executor(idx, queries, dpopt, tasks)
        return seen[key]
    return run


def _run(idx, mo, q, ex, knob, dump, monkeypatch, capfd, n_threads=4):
    """one batch through the stage machine and the formatter with MPA_GPU_CS = knob (None: unset): (text, stderr, parsed dump)"""
    monkeypatch.setenv("MPA_TIMING", "1")
    monkeypatch.setenv("MPA_CS_DUMP", str(dump))
    if knob is None:
        monkeypatch.delenv("MPA_GPU_CS", raising=False)
    else:
        monkeypatch.setenv("MPA_GPU_CS", knob)
    if os.path.exists(str(dump)):
        os.remove(str(dump))
    capfd.readouterr()
    res = map_batch_result(idx, mo, q, ex, n_threads=n_threads)
    text = mpa.format_output(idx, mo, q, res)[0]
    err = capfd.readouterr().err
    monkeypatch.delenv("MPA_CS_DUMP")
    return text, err, csdump.parse(csdump.read(str(dump))) if os.path.exists(str(dump)) else []


_host_bodies = {}


@pytest.mark.parametrize("name", GOLDEN)
def test_shared_core_prints_the_reference_and_equals_the_host_walk(oracle_built, name, tmp_path, monkeypatch, capfd):
    idx, mo, q, ref = alnstats.case_inputs(name, tmp_path)
    ex = _memo(oracle_executor)
    t_host, err_host, d_host = _run(idx, mo, q, ex, None, tmp_path / "host.cs", monkeypatch, capfd)
    t_model, err_model, d_model = _run(idx, mo, q, ex, "model", tmp_path / "model.cs", monkeypatch, capfd)
    idx.close()
    assert MODEL_NOTE in err_model, "MPA_GPU_CS=model did not run the shared core"
    assert "cs strings" not in err_host
    if t_model != ref:
        for x, y in zip(t_model.split(b"\n"), ref.split(b"\n")):
            if x != y:
                raise AssertionError("first differing line\n ours %r\n ref  %r" % (x[-300:], y[-300:]))
    assert t_model == ref and t_host == ref
    n_cs = ref.count(b"cs:Z:")
    assert n_cs > 0
    assert csdump.format_counts(err_model) == (n_cs, 0)
    assert csdump.format_counts(err_host) == (0, n_cs)
    assert len(d_host) >= n_cs
    assert csdump.first_difference(d_model, d_host, 1, 0) is None, csdump.first_difference(d_model, d_host, 1, 0)
    _host_bodies[name] = [b for _, b in d_host]


def _regions_edge():
    """the edge genome of the regions tests (tests/regioncases.py): genes planted without a mutation, so its alignments are match
    runs of 120 to 300 codons -- the ':n' with n >= 100 that the five synthetic cases above lack (their longest run is 51)"""
    import regioncases
    contigs, prots, names, mo = regioncases.edge_genome()
    return regioncases.edge_index(contigs), mo, mpa.Queries(prots, names), open(golden.path(regioncases.EDGE_REF), "rb").read()


def test_long_match_runs_through_the_shared_core(oracle_built, tmp_path, monkeypatch, capfd):
    idx, mo, q, ref = _regions_edge()
    ex = _memo(oracle_executor)
    t_host, err_host, d_host = _run(idx, mo, q, ex, None, tmp_path / "host.cs", monkeypatch, capfd)
    t_model, err_model, d_model = _run(idx, mo, q, ex, "model", tmp_path / "model.cs", monkeypatch, capfd)
    idx.close()
    assert t_model == ref and t_host == ref
    assert MODEL_NOTE in err_model and csdump.format_counts(err_model) == (ref.count(b"cs:Z:"), 0)
    assert csdump.first_difference(d_model, d_host, 1, 0) is None, csdump.first_difference(d_model, d_host, 1, 0)
    _host_bodies["regions_edge"] = [b for _, b in d_host]


def test_cases_cover_what_the_walk_distinguishes(oracle_built, tmp_path, monkeypatch, capfd):
    """over the union of the cases above the unset run's dump holds thousands of mismatches, insertions, deletions, introns, the one-
    and two-base '*' forms (G, and the heads of U and V) and ':n' runs with n >= 100 (or the comparisons above would test less than
    they say).  None of them holds an 'n' (nor does the edge genome below): the ambiguous-base branch rests on the planted genome and the checker."""
    for name in GOLDEN + ["regions_edge"]:
        if name not in _host_bodies:                           # (run alone: map the case here)
            idx, mo, q, _ = _regions_edge() if name == "regions_edge" else alnstats.case_inputs(name, tmp_path)
            _host_bodies[name] = [b for _, b in _run(idx, mo, q, _memo(oracle_executor), None, tmp_path / (name + ".cs"), monkeypatch, capfd)[2]]
            idx.close()
    c = csdump.kinds([b for name in GOLDEN + ["regions_edge"] for b in _host_bodies[name]])
    assert c["mismatch"] >= 2000, c
    for k in ("insertion", "deletion", "intron", "star1", "star2", "run100"):
        assert c[k] > 0, c
    assert c["n"] == 0, c


@pytest.mark.parametrize("d,e", [(0, 0), (1, 3), (2, 1), (3, 2)])
def test_edge_genome_through_the_shared_core(oracle_built, d, e, tmp_path, monkeypatch, capfd):
    """the edge genome of the GPU tests (contigs cut d bases before their first gene and e bases behind their last; 5 % N): the shared
    core against the formatter's walk, dump and text"""
    contigs, prots, names = alnstats.edge_genome(d, e)
    idx = mpa.Index.from_nt4(contigs, ["chr1", "chr2"])
    mpa._check(mpa.lib().mpa_idx_build_kmers(idx.h, 4))
    mo = mpa.default_mapopt()
    mo.flag |= 4
    q, ex = mpa.Queries(prots, names), _memo(oracle_executor)
    t_host, err_host, d_host = _run(idx, mo, q, ex, None, tmp_path / "host.cs", monkeypatch, capfd)
    t_model, err_model, d_model = _run(idx, mo, q, ex, "model", tmp_path / "model.cs", monkeypatch, capfd)
    idx.close()
    assert len(d_host) >= len(prots) // 2
    assert MODEL_NOTE in err_model and csdump.format_counts(err_model)[1] == 0 and csdump.format_counts(err_model)[0] > 0
    assert csdump.first_difference(d_model, d_host, 1, 0) is None, csdump.first_difference(d_model, d_host, 1, 0)
    assert t_model == t_host and t_host.count(b"cs:Z:") > 0


def test_planted_ambiguous_bases_through_the_shared_core(oracle_built, tmp_path, monkeypatch, capfd):
    """neither the golden cases nor the edge genome put an N under an alignment; csdump.planted_n_genome() does: eight codons with an
    ambiguous base print as mismatches with an 'n'"""
    contigs, prots, names = csdump.planted_n_genome()
    idx = mpa.Index.from_nt4(contigs, ["chr1"])
    mpa._check(mpa.lib().mpa_idx_build_kmers(idx.h, 4))
    mo = mpa.default_mapopt()
    mo.flag |= 4
    q, ex = mpa.Queries(prots, names), _memo(oracle_executor)
    t_host, _, d_host = _run(idx, mo, q, ex, None, tmp_path / "host.cs", monkeypatch, capfd)
    t_model, err_model, d_model = _run(idx, mo, q, ex, "model", tmp_path / "model.cs", monkeypatch, capfd)
    idx.close()
    assert csdump.kinds([b for _, b in d_host])["n"] == 8
    assert csdump.first_difference(d_model, d_host, 1, 0) is None, csdump.first_difference(d_model, d_host, 1, 0)
    assert t_model == t_host and csdump.format_counts(err_model) == (2, 0)


@pytest.mark.parametrize("name", ["syn_g", "syn_f"])
def test_cases_that_print_no_cs_string_skip_the_step(oracle_built, name, tmp_path, monkeypatch, capfd):
    """--no-cs (syn_g) and --gtf (syn_f): nothing to carry, so nothing is built -- no note, the reference's bytes"""
    idx, mo, q, ref = alnstats.case_inputs(name, tmp_path)
    text, err, _ = _run(idx, mo, q, _memo(oracle_executor), "model", tmp_path / "m.cs", monkeypatch, capfd)
    idx.close()
    assert "cs strings" not in err
    assert csdump.format_counts(err) == (0, 0)
    assert text == ref and b"cs:Z:" not in text


def test_knob_zero_is_the_host_walk(oracle_built, tmp_path, monkeypatch, capfd):
    """MPA_GPU_CS=0 and a device request without a context (the stage machine driven from outside: mpa_batch_begin) keep the host path"""
    idx, mo, q, ref = alnstats.case_inputs("syn_a")
    q = mpa.Queries(q.seqs[:6], q.names[:6])
    ex = _memo(oracle_executor)
    for v in ("0", "1"):
        text, err, dump = _run(idx, mo, q, ex, v, tmp_path / ("k%s.cs" % v), monkeypatch, capfd, n_threads=2)
        assert "cs strings" not in err
        carried, built = csdump.format_counts(err)
        assert carried == 0 and built == text.count(b"cs:Z:") and built > 0
        assert all(h["src"] == 0 for h, _ in dump) and len(dump) >= built
        assert text and text in ref
    idx.close()


def test_core_against_a_plain_walk_under_sanitizers(tmp_path):
    """tests/alncs_check.cpp: M runs of 1, 63, 64, 65, 129 and 1 000 codons (all-match, all-mismatch = the bound, alternating, one mismatch
    at codon 0 / 63 / 64 / last); match runs of 9, 10, 99, 100 and 1 000; a run over three steps; two M operations back to back; I, D, F
    of 1 and 2, G; N, U, V first, last and back to back with intron lengths of 1 to 7 digits; 70 and 100 words; codons with N; a
    lower-case query; both strands of two contigs -- in guarded slots sized by aln_cs_bound"""
    root = refbind.ROOT
    exe = str(tmp_path / "alncs_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                    "-I" + os.path.join(root, "miniprot_amd", "csrc"), os.path.join(root, "tests", "alncs_check.cpp"), "-o", exe, "-lpthread"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 mismatches" in out.stdout and "ERROR" not in out.stderr
