"""The output text of a batch through the code the device runs (miniprot_amd/csrc/format_core.h), on the CPU.
All comparisons are byte for byte.

1. mpa_dbg_format(NULL, ...) -- the shared core with a team of one -- on the hand-made tables of tests/formatcases.py against
   mpa_format_output(), the host formatter, for every id0 of formatcases.ID0S; the printed hits equal mpa_result_n_output().
2. MPA_GPU_FORMAT=model against the knob unset on results of the stage machine with the oracle as DP executor: all fifteen
   tests/golden/syn_*.ref.paf cases and golden.OPTION_CASES, also with the walk models on; the note is printed with the knob and only then.
3. tests/format_check.cpp under the sanitizers: teams of one and of 64 threads against plain restatements, the ratio helper against
   snprintf("%.4f"), the id patch at its width edge."""
import os
import subprocess
import pytest
import miniprot_amd as mpa
import refbind
import alnstats
import formatcases
import golden
from hostpipe import map_batch_result, oracle_executor

MODEL_NOTE = "format: shared core"
TABLES = [t["name"] for t in formatcases.tables()]


def first_difference(a, b):
    if a == b:
        return None
    la, lb = a.split(b"\n"), b.split(b"\n")
    for k, (x, y) in enumerate(zip(la, lb)):
        if x != y:
            return "line %d\n got  %r\n want %r" % (k, x[:400], y[:400])
    return "%d lines, want %d" % (len(la), len(lb))


@pytest.mark.parametrize("k", range(len(TABLES)), ids=TABLES)
def test_shared_core_prints_what_the_host_formatter_prints(k):
    t = formatcases.tables()[k]
    idx, mo, q, res = formatcases.objects(t)
    try:
        n_out = res.n_output(mo, q)
        assert n_out == formatcases.n_printed_expected(t), "the table's filters, restated"
        for id0 in formatcases.ID0S:
            want, id_after = mpa.format_output(idx, mo, q, res, id0)
            got, n, declined = mpa.dbg_format(None, idx, mo, q, res, id0)
            d = first_difference(got, want)
            assert d is None, "%s, id0 %d: %s" % (t["name"], id0, d)
            assert n == n_out and id_after == id0 + n_out
            # the one decline these tables hold: a GFF3 / GTF id that reaches seven digits (the delimiter form prints no running id)
            ids = b"\tminiprot\t" in want and bool(mo.flag & 0x20 or (mo.flag & 0x8 and not 33 <= mo.gff_delim <= 126))
            assert declined == bool(ids and id0 + n_out > 999999), (t["name"], id0)
    finally:
        res.close()
        idx.close()


def test_tables_cover_what_the_formatter_distinguishes():
    seen = dict(unmapped=0, no_aln=0, reverse=0, big_pos=0, negative=0, ten_digits=0, stop_feature=0, has_stop=0, odd_splice=0, frameshift=0, filtered=0, cut_by_n=0, cs_5000=0,
                rows_4097=0, cig_1000=0, feats_65=0, queries_3000=0)
    for t in formatcases.tables():
        h, f, off = t["hits"], t["feats"], t["hit_off"]
        seen["unmapped"] += bool((off[1:] == off[:-1]).any())
        seen["no_aln"] += bool((h["has_aln"] == 0).any())
        seen["reverse"] += bool((h["vid"] & 1).any())
        seen["big_pos"] += bool((h["ve"] > 2 ** 31).any())
        seen["negative"] += bool((h["dp_score"] < 0).any())
        seen["ten_digits"] += bool((h["blen"] >= 10 ** 9).any())
        seen["stop_feature"] += bool((f["type"] == 1).any())
        seen["has_stop"] += bool((h["dist_stop"] == 0).any())
        seen["odd_splice"] += bool(((f["donor"] != b"GT") & (f["donor"] != b"")).any())
        seen["frameshift"] += bool((f["n_fs"] > 0).any())
        n = formatcases.n_printed_expected(t)
        seen["filtered"] += 0 < n < len(h)
        seen["cut_by_n"] += t["opt"]["out_n"] in (0, 1)
        seen["cs_5000"] += t["cs"] is not None and bool((t["cs"]["len"] == 5000).any())
        seen["rows_4097"] += t["rows"] is not None and bool((t["rows"]["width"] == 4097).any())
        seen["cig_1000"] += bool((h["n_cigar"] == 1000).any())
        seen["feats_65"] += bool((h["n_feat"] == 65).any())
        seen["queries_3000"] += len(off) == 3001
    assert all(v > 0 for v in seen.values()), seen


def test_the_hook_refuses_hits_that_point_outside_their_arrays():
    t = dict(formatcases.tables()[0])
    hits = t["hits"].copy()
    k = int((hits["has_aln"] != 0).nonzero()[0][0])
    hits["cigar_off"][k] = len(t["cigars"])
    t["hits"] = hits
    idx, mo, q, res = formatcases.objects(t)
    with pytest.raises(mpa.MpaError):
        mpa.dbg_format(None, idx, mo, q, res)
    res.close()
    idx.close()


def test_a_prefix_longer_than_64_bytes_declines_and_prints_the_hosts_bytes(monkeypatch, capfd):
    t = dict(formatcases.tables()[2])
    t["opt"] = dict(t["opt"], prefix=b"x" * 65)
    idx, mo, q, res = formatcases.objects(t)
    monkeypatch.setenv("MPA_TIMING", "1")
    capfd.readouterr()
    got, n, declined = mpa.dbg_format(None, idx, mo, q, res, 3)
    err = capfd.readouterr().err
    assert declined and "format declined (a gff_prefix longer than 64 bytes)" in err
    assert got == mpa.format_output(idx, mo, q, res, 3)[0] and n == res.n_output(mo, q)
    res.close()
    idx.close()


def test_core_against_plain_restatements_under_sanitizers(tmp_path):
    """tests/format_check.cpp: random batches (every flag combination, filters, strands, hits without alignment, rows whose slots are
    wider than their width) through the three stages with a team of one and a team of 64 threads against a plain restatement of the
    host formatter, output buffers of exactly the sized bytes; the same hits as the records the finish step leaves on the device; fmt_ratio against snprintf("%.4f") for every n <= blen <= 3 000 and random
    31-bit pairs; format_patch_ids at 999 999"""
    root = refbind.ROOT
    exe = str(tmp_path / "format_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                    "-I" + os.path.join(root, "miniprot_amd", "csrc"), os.path.join(root, "tests", "format_check.cpp"), "-o", exe, "-lpthread"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 mismatches" in out.stdout and "ERROR" not in out.stderr


# ---- the whole path: results of the stage machine, formatted with the knob unset and with the model
WALK_MODELS = {"MPA_GPU_STATS": "model", "MPA_GPU_CS": "model", "MPA_GPU_ROWS": "model"}
KNOBS = ("MPA_GPU_FORMAT", "MPA_GPU_FINISH", "MPA_GPU_STATS", "MPA_GPU_CS", "MPA_GPU_ROWS", "MPA_GPU_SPANS")


def _both_texts(idx, mo, q, others, monkeypatch, capfd):
    monkeypatch.setenv("MPA_TIMING", "1")
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in others.items():
        monkeypatch.setenv(k, v)
    res = map_batch_result(idx, mo, q, oracle_executor, n_threads=4)
    capfd.readouterr()
    t_host, id_host = mpa.format_output(idx, mo, q, res, 5)
    err_host = capfd.readouterr().err
    monkeypatch.setenv("MPA_GPU_FORMAT", "model")
    t_model, id_model = mpa.format_output(idx, mo, q, res, 5)
    err_model = capfd.readouterr().err
    assert MODEL_NOTE in err_model, "MPA_GPU_FORMAT=model did not run the shared core"
    assert "declined" not in err_model
    assert MODEL_NOTE not in err_host and "format output" in err_host
    assert id_model == id_host == 5 + res.n_output(mo, q)
    d = first_difference(t_model, t_host)
    assert d is None, d
    monkeypatch.delenv("MPA_GPU_FORMAT")
    return mpa.format_output(idx, mo, q, res, 0)[0], res


SYN = [c["name"] for c in golden.SYNTH_CASES]


@pytest.mark.parametrize("name,others", [(n, {}) for n in SYN] + [(n, WALK_MODELS) for n in ("syn_e", "syn_k", "syn_m")],
                         ids=SYN + [n + "_models" for n in ("syn_e", "syn_k", "syn_m")])
def test_model_prints_the_golden_text(oracle_built, name, others, tmp_path, monkeypatch, capfd):
    idx, mo, q, ref = alnstats.case_inputs(name, tmp_path)
    text, res = _both_texts(idx, mo, q, others, monkeypatch, capfd)
    if others and not mo.flag & 0x200:
        assert len(mpa.result_flat(res)["cs"]) > 0             # (the cs bodies came with the hits: the model pasted them)
    res.close()
    idx.close()
    assert text == ref


@pytest.mark.parametrize("case", golden.OPTION_CASES, ids=[c["name"] for c in golden.OPTION_CASES])
def test_model_prints_the_option_cases(oracle_built, case, tmp_path, monkeypatch, capfd):
    import seedopts
    contigs, prots, names = golden.synth_inputs(case)
    idx = mpa.Index.read_fasta(seedopts.write_genome(tmp_path, contigs), case["idx"])
    assert idx.build_kmers(4) == "host"
    mo, q = golden.mapopt_for(case), mpa.Queries(prots, names)
    text, res = _both_texts(idx, mo, q, {}, monkeypatch, capfd)
    res.close()
    idx.close()
    assert text == open(golden.path(case["name"] + ".ref.paf"), "rb").read()


def test_format_paf_takes_the_model_too(oracle_built, tmp_path, monkeypatch, capfd):
    import ctypes as C
    idx, mo, q, ref = alnstats.case_inputs("syn_e", tmp_path)
    res = map_batch_result(idx, mo, q, oracle_executor, n_threads=4)
    names = (C.c_char_p * len(q.names))(*[n.encode() for n in q.names])
    texts = []
    for knob in (None, "model"):
        monkeypatch.setenv("MPA_TIMING", "1")
        if knob:
            monkeypatch.setenv("MPA_GPU_FORMAT", knob)
        capfd.readouterr()
        out = C.c_void_p()
        n = mpa.lib().mpa_format_paf(idx.h, C.byref(mo), C.byref(q.c), names, res.h, C.byref(out))
        assert n > 0
        texts.append(C.string_at(out.value, n))
        mpa.lib().mpa_free(out)
        assert (MODEL_NOTE in capfd.readouterr().err) == bool(knob)
    res.close()
    idx.close()
    assert texts[0] == texts[1] and b"##PAF" not in texts[0] and b"\tminiprot\t" not in texts[0]
