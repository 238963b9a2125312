"""The residue rows of --aln / --trans through the code the device runs (miniprot_amd/csrc/aln_rows_core.h), on the CPU.

MPA_GPU_ROWS=model makes take_round3() (host_align.cpp) build the four rows (##ATN, ##ATA, ##AAS, ##AQA) and the translated target (##STA)
of every aligned region with the shared core and a team of one; the region carries them to the result and the formatter pastes them
in behind the five prefixes where it otherwise walks the alignment itself (put_residues, host_format.cpp).  The stage machine with the
oracle as DP executor must still print the reference's bytes, and the format note must say that every row set was carried and none
built.  A stand-alone program (tests/alnrows_check.cpp, compiled here with AddressSanitizer and UBSan) feeds the core hand-written
CIGARs, with a team of one and a team of 64 threads, into guarded slots and compares them with a plain walk.  No sanitizer goes near
code loaded into python."""
import os
import subprocess
import pytest
import miniprot_amd as mpa
import refbind
import alnstats
import alnrows
from hostpipe import map_batch_result, oracle_executor

MODEL_NOTE = "residue rows: shared core"
GOLDEN = ["syn_k", "syn_l", "syn_m"]                       # -u --aln; --trans --gff; --aln --trans --gtf
EDGES = [(0, 0), (1, 3), (2, 1), (3, 2)]


def _memo(executor):
    """the DP results of a round, computed once: the two runs of a case hand out the same tasks"""
    seen = {}

    def run(idx, queries, dpopt, tasks):
        key = tasks.tobytes()
        if key not in seen:
            seen[key] = executor(idx, queries, dpopt, tasks)
        return seen[key]
    return run


def _run(idx, mo, q, ex, knob, monkeypatch, capfd, n_threads=4):
    """one batch through the stage machine and the formatter with MPA_GPU_ROWS = knob (None: unset): (text, stderr)"""
    monkeypatch.setenv("MPA_TIMING", "1")
    if knob is None:
        monkeypatch.delenv("MPA_GPU_ROWS", raising=False)
    else:
        monkeypatch.setenv("MPA_GPU_ROWS", knob)
    capfd.readouterr()
    res = map_batch_result(idx, mo, q, ex, n_threads=n_threads)
    text = mpa.format_output(idx, mo, q, res)[0]
    return text, capfd.readouterr().err


def _pair(idx, mo, q, monkeypatch, capfd):
    """(host text, host stderr, model text, model stderr); closes the index"""
    ex = _memo(oracle_executor)
    t_host, err_host = _run(idx, mo, q, ex, None, monkeypatch, capfd)
    t_model, err_model = _run(idx, mo, q, ex, "model", monkeypatch, capfd)
    idx.close()
    return t_host, err_host, t_model, err_model


def _check_pair(t_host, err_host, t_model, err_model):
    """model against host: the same bytes, every row set carried in the model run and built in the host run"""
    assert MODEL_NOTE in err_model, "MPA_GPU_ROWS=model did not run the shared core"
    assert "residue rows" not in err_host
    if t_model != t_host:
        for x, y in zip(t_model.split(b"\n"), t_host.split(b"\n")):
            if x != y:
                raise AssertionError("first differing line\n model %r\n host  %r" % (x[-300:], y[-300:]))
    assert t_model == t_host
    n = alnrows.row_sets(t_host)
    assert n > 0
    assert alnrows.format_counts(err_model) == (n, 0)
    assert alnrows.format_counts(err_host) == (0, n)


_host_texts = {}


@pytest.mark.parametrize("name", GOLDEN)
def test_shared_core_prints_the_reference(oracle_built, name, tmp_path, monkeypatch, capfd):
    idx, mo, q, ref = alnstats.case_inputs(name, tmp_path)
    t_host, err_host, t_model, err_model = _pair(idx, mo, q, monkeypatch, capfd)
    _check_pair(t_host, err_host, t_model, err_model)
    assert t_model == ref and t_host == ref
    _host_texts[name] = t_host


def test_case_that_prints_no_rows_skips_the_step(oracle_built, tmp_path, monkeypatch, capfd):
    """syn_a (-u): nothing to carry, so nothing is built -- no note, no row counts, the reference's bytes"""
    idx, mo, q, ref = alnstats.case_inputs("syn_a", tmp_path)
    text, err = _run(idx, mo, q, _memo(oracle_executor), "model", monkeypatch, capfd)
    idx.close()
    assert "residue rows" not in err and alnrows.format_counts(err) is None
    assert text == ref and alnrows.row_sets(text) == 0


def test_knob_zero_and_a_device_request_without_a_context_keep_the_host_walk(oracle_built, tmp_path, monkeypatch, capfd):
    """MPA_GPU_ROWS=0, and =1 in the stage machine driven from outside (mpa_batch_begin: no context): built = all, carried = 0"""
    idx, mo, q, ref = alnstats.case_inputs("syn_m", tmp_path)
    q = mpa.Queries(q.seqs[:8], q.names[:8])
    ex = _memo(oracle_executor)
    for v in ("0", "1"):
        text, err = _run(idx, mo, q, ex, v, monkeypatch, capfd, n_threads=2)
        assert "residue rows" not in err
        n = alnrows.row_sets(text)
        assert n > 0 and alnrows.format_counts(err) == (0, n)
        assert text and text in ref
    idx.close()


@pytest.mark.parametrize("d,e", EDGES)
def test_edge_genome_through_the_shared_core(oracle_built, d, e, monkeypatch, capfd):
    """the edge genome of the statistics tests (contigs cut d bases before their first gene and e bases behind their last; 5 % N) with
    --aln --trans"""
    out = _pair(*alnrows.edge(d, e), monkeypatch, capfd)
    _check_pair(*out)
    _host_texts["edge%d%d" % (d, e)] = out[0]


@pytest.mark.parametrize("cut", [1, 2])
def test_alignments_that_end_at_the_contig_end_print_no_trailing_codon(oracle_built, cut, monkeypatch, capfd):
    """alnstats.edge_genome(d, e) keeps every gene's stop codon inside its contig, so ve + 3 never lies beyond it; trimmed `cut` bases
    further (alnrows.trimmed_edge) the outermost alignments end fewer than three bases before their strand's end: no trailing codon"""
    out = _pair(*alnrows.trimmed_edge(cut), monkeypatch, capfd)
    _check_pair(*out)
    assert alnrows.near_end(out[0]) >= 1
    assert alnrows.kinds(out[0])["sta_open"] >= alnrows.near_end(out[0])
    _host_texts["trimmed%d" % cut] = out[0]


def test_planted_ambiguous_bases_through_the_shared_core(oracle_built, monkeypatch, capfd):
    """csdump.planted_n_genome(): eight codons with an ambiguous base -- N in the ##ATN rows, X in ##ATA and ##STA"""
    out = _pair(*alnrows.planted_n(), monkeypatch, capfd)
    _check_pair(*out)
    assert alnrows.kinds(out[0])["N"] == 8
    assert sum(x.count(b"X") for x in alnrows.rows(out[0])[b"STA"]) == 8
    _host_texts["planted_n"] = out[0]


def test_lowered_frameshift_penalty_prints_frameshift_matches(oracle_built, monkeypatch, capfd):
    """the golden cases hold no '$' (a frameshift match, operation G) and one '!': syn_k's input with the frameshift penalty lowered to
    6 holds dozens of both"""
    out = _pair(*alnrows.low_frameshift(alnstats.case_inputs, "syn_k", 6), monkeypatch, capfd)
    _check_pair(*out)
    k = alnrows.kinds(out[0])
    assert k["$"] > 0 and k["!"] > 0, k
    _host_texts["low_fs"] = out[0]


def test_cases_cover_what_the_walk_distinguishes(oracle_built, tmp_path, monkeypatch, capfd):
    """over the cases above the unset run's text holds abridged introns, whole introns, '!', '$', STA rows that end in '*' and STA rows
    that do not, and an N in an ATN row (or the comparisons above would test less than they say)"""
    makers = {"planted_n": alnrows.planted_n, "low_fs": lambda: alnrows.low_frameshift(alnstats.case_inputs, "syn_k", 6), "trimmed1": lambda: alnrows.trimmed_edge(1)}
    makers.update({name: (lambda name=name: alnstats.case_inputs(name, tmp_path)[:3]) for name in GOLDEN})
    for name, make in makers.items():
        if name not in _host_texts:                            # (run alone: map the case here)
            idx, mo, q = make()
            _host_texts[name] = _run(idx, mo, q, _memo(oracle_executor), None, monkeypatch, capfd)[0]
            idx.close()
    total = {}
    for name in makers:
        for k, v in alnrows.kinds(_host_texts[name]).items():
            total[k] = total.get(k, 0) + v
    for k in ("abridged", "whole", "!", "$", "sta_stop", "sta_open", "N"):
        assert total[k] > 0, total


WALK_KNOBS = (("MPA_GPU_STATS", "alignment statistics: shared core"), ("MPA_GPU_CS", "cs strings: shared core"), ("MPA_GPU_ROWS", MODEL_NOTE))


def test_every_combination_of_the_three_walks_through_their_models(oracle_built, tmp_path, monkeypatch, capfd):
    """take_round3() decides for each of the three walks behind the last DP round on its own.  syn_a's input with --aln --trans (its
    options are -u: the row lines are all that --aln --trans add, so the text without them is the golden file) under all eight
    settings of (MPA_GPU_STATS, MPA_GPU_CS, MPA_GPU_ROWS) in {unset, model}: the bytes of the all-unset run, each walk's note exactly
    when its knob is `model`, and MPA_CS_DUMP records of source 1 exactly when MPA_GPU_CS=model (0 otherwise)"""
    import csdump
    idx, mo, q, ref = alnstats.case_inputs("syn_a", tmp_path)
    mo.flag |= alnrows.ALN | alnrows.TRANS
    ex = _memo(oracle_executor)
    dump = str(tmp_path / "walks.cs")
    monkeypatch.setenv("MPA_TIMING", "1")
    monkeypatch.setenv("MPA_CS_DUMP", dump)
    base = None
    for k in range(8):
        on = [bool(k >> i & 1) for i in range(3)]
        for (knob, _), v in zip(WALK_KNOBS, on):
            if v:
                monkeypatch.setenv(knob, "model")
            else:
                monkeypatch.delenv(knob, raising=False)
        if os.path.exists(dump):
            os.remove(dump)
        capfd.readouterr()
        res = map_batch_result(idx, mo, q, ex, n_threads=4)
        text = mpa.format_output(idx, mo, q, res)[0]
        err = capfd.readouterr().err
        recs = csdump.parse(csdump.read(dump))
        if base is None:
            base = text
            assert alnrows.row_sets(text) > 0 and len(recs) > 0
            assert b"".join(l + b"\n" for l in text.split(b"\n")[:-1] if not (l[:2] == b"##" and l[2:5] in alnrows.KINDS)) == ref
        assert text == base, on
        for (knob, note), v in zip(WALK_KNOBS, on):
            assert (note in err) == v, (on, knob)
        assert all(int(h["src"]) == (1 if on[1] else 0) for h, _ in recs), on
    idx.close()


def test_core_against_a_plain_walk_under_sanitizers(tmp_path):
    """tests/alnrows_check.cpp: M runs of 1, 21, 22, 63, 64, 65 and 1 000 codons; I, D, F of 1 and 2, G of 1 and 2 bases; N, U, V first,
    last and back to back with intron lengths of 2 flank - 1, 2 flank, 2 flank + 1 and 1 to 7 digits at flanks of 0, 1 and 200; 70 and
    100 words; codons and introns with N; a lower-case query; alignments that end 0 to 3 bases before their strand's end, whose last
    codon is a stop, and with no codon at all; each of the three flag combinations; both strands of two contigs -- in guarded slots
    sized by aln_rows_slot"""
    root = refbind.ROOT
    exe = str(tmp_path / "alnrows_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                    "-I" + os.path.join(root, "miniprot_amd", "csrc"), os.path.join(root, "tests", "alnrows_check.cpp"), "-o", exe, "-lpthread"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 mismatches" in out.stdout and "ERROR" not in out.stderr
