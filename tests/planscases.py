"""Inputs of the plans tests (tests/test_plans_cpu.py, tests/test_plans_gpu.py; MPA_GPU_PLANS): the golden cases by name -- with the
index options and the splice-score track of the cases that have them --, runs with the dump of tests/plansdump.py switched on, and the
step's notes."""
import os
import miniprot_amd as mpa
import golden
import seedopts
import plansdump

MODEL_NOTE = "plans: shared core"
DEVICE_NOTE = "plans on the GPU"
NO_ANCHORS = "refinement anchors downloaded 0 B"
# what each case is here for: baseline runs; -G 500000; -p 0.3 -N 50; -S (io == io_end: no repeats); -A (stops after the selection);
# -J 35 -e 5000 -n 2; a splice-score track (the SS_SKIP0 flags); the index option -b 12
CASES = ["syn_a", "syn_b", "syn_c", "syn_d", "syn_h", "syn_i", "syn_j", "syn_n", "opt_b12"]


def case_inputs(name, tmp_path):
    """(index, map options, queries, golden text) of a golden case of golden.SYNTH_CASES or golden.OPTION_CASES"""
    case = [c for c in golden.SYNTH_CASES + golden.OPTION_CASES if c["name"] == name][0]
    contigs, prots, names = golden.synth_inputs(case)
    if "idx" in case:
        idx = mpa.Index.read_fasta(seedopts.write_genome(tmp_path, contigs, name + ".fa"), case["idx"])
    else:
        idx = mpa.Index.from_nt4(contigs, ["chr%d" % (i + 1) for i in range(len(contigs))])
    mpa._check(mpa.lib().mpa_idx_build_kmers(idx.h, 4))
    mo = golden.mapopt_for(case)
    if "spsc" in case:
        idx.set_spsc(golden.write_spsc(case, contigs, str(tmp_path / "spsc.tsv")), mo)
    ref, header = open(golden.path(name + ".ref.paf"), "rb").read(), golden.file_header(case)
    assert ref.startswith(header)
    return idx, mo, mpa.Queries(prots, names), ref[len(header):]


def with_dump(monkeypatch, path, run):
    """run() with MPA_PLANS_DUMP=path (a fresh file); returns (what run() returned, the dump's bytes)"""
    if os.path.exists(path):
        os.remove(path)
    monkeypatch.setenv("MPA_PLANS_DUMP", path)
    try:
        out = run()
    finally:
        monkeypatch.delenv("MPA_PLANS_DUMP")
    return out, plansdump.read(path)


def totals(dump):
    """(queries, regions, plans, tasks, segments, shortcut segments, regions left without a plan) of a dump"""
    p = plansdump.parse(dump)
    return (len(p), sum(len(e[1]) for e in p), sum(len(e[2]) for e in p), sum(len(e[3]) for e in p), sum(len(e[4]) for e in p),
            sum(int((e[4]["task"] < 0).sum()) for e in p), sum(int((e[1]["cnt"] == 0).sum()) for e in p))
