"""MPA_GPU_SPANS=1: the host step between the two DP rounds (the accepted spans and the round-2 tasks) and step (a) behind them (the
region CIGARs) run on the batch's DP context -- k_spans, k_spans_emit and k_assemble (span_kernels.hip; the code is spans_core.h, which
tests/test_spans_cpu.py pins on the CPU).  What the two steps leave is visible in MPA_SPANS_DUMP (tests/spansdump.py) and in the text:
both must equal the run with the knob unset on the same context, byte for byte, and the text the reference's bytes.

A round 2 without tasks cannot be made through the pipeline: the reference's trimming of a run of anchors (mp_filter_seed, align.c:6-31)
leaves kmer2 + 1 residues on either side of the kept anchors, one more than the ungapped shortcut takes, so a protein that aligns end
to end without a gap still sends both spans to the DP (tests/test_spans_cpu.py::test_a_gap_free_gene_still_needs_round_2 shows it).  The
case runs through mpa_dbg_spans instead: plans whose spans all take the shortcut, k_assemble without round-2 results."""
import os
import numpy as np
import pytest
import miniprot_amd as mpa
import golden
import regioncases
import alnstats
import spanscases
import spansdump
from spanscases import DEVICE_NOTE, NO_WORDS

pytestmark = pytest.mark.gpu

WALK_KNOBS = {"MPA_GPU_STATS": "1", "MPA_GPU_CS": "1", "MPA_GPU_ROWS": "1"}
ALL_KNOBS = dict(WALK_KNOBS, MPA_GPU_SEED="1", MPA_GPU_SKETCH="1", MPA_GPU_REGIONS="1", MPA_GPU_REFINE="1", MPA_GPU_PLANS="1")


@pytest.fixture(scope="module")
def ctx():
    c = mpa.Context(0)
    yield c
    c.close()


def _run(ctx, idx, mo, q, knob, monkeypatch, capfd, path, more=None, n_threads=4):
    """one blocking batch with MPA_GPU_SPANS = knob (None: unset) and the knobs of `more`: (text, dump, stderr)"""
    monkeypatch.setenv("MPA_TIMING", "1")
    for k, v in (more or {}).items():
        monkeypatch.setenv(k, v)
    if knob is None:
        monkeypatch.delenv("MPA_GPU_SPANS", raising=False)
    else:
        monkeypatch.setenv("MPA_GPU_SPANS", knob)
    capfd.readouterr()
    res, dump = spanscases.with_dump(monkeypatch, path, lambda: mpa.map_batch(ctx, idx, mo, q, n_threads))
    err = capfd.readouterr().err
    return mpa.format_output(idx, mo, q, res)[0], dump, err


def _check_pair(host, dev, n_steps=2):
    assert dev[2].count(DEVICE_NOTE) == n_steps, "MPA_GPU_SPANS=1 did not run both steps on the device"
    assert "spans declined" not in dev[2], [l for l in dev[2].split("\n") if "declined" in l][:3]
    assert DEVICE_NOTE not in host[2]
    assert len(host[1]) > 0 and dev[1] == host[1], spansdump.first_difference(dev[1], host[1])
    assert dev[0] == host[0]


@pytest.mark.parametrize("name", spanscases.CASES)
def test_golden_cases(ctx, name, tmp_path, monkeypatch, capfd):
    idx, mo, q, ref = spanscases.case_inputs(name, tmp_path)
    idx.to_device(ctx)
    host = _run(ctx, idx, mo, q, None, monkeypatch, capfd, str(tmp_path / "host.dump"))
    dev = _run(ctx, idx, mo, q, "1", monkeypatch, capfd, str(tmp_path / "dev.dump"))
    idx.close()
    if name == "syn_i":                                        # -A: no DP rounds, nothing for the step to do
        assert DEVICE_NOTE not in dev[2] and dev[1] == host[1] == b"" and dev[0] == host[0] == ref
        return
    _check_pair(host, dev)
    assert dev[0] == ref, "text differs from the reference"
    assert sum(len(p) for _, p in spansdump.parse(dev[1])) >= len(q.seqs) // 2


@pytest.mark.parametrize("name,knobs", [("syn_a", WALK_KNOBS), ("syn_m", WALK_KNOBS), ("syn_a", ALL_KNOBS)], ids=["syn_a-walks", "syn_m-walks", "syn_a-every-knob"])
def test_with_the_walk_knobs(ctx, name, knobs, tmp_path, monkeypatch, capfd):
    """the statistics, cs strings and residue rows read the pool k_assemble wrote: no CIGAR word is staged or uploaded"""
    idx, mo, q, ref = alnstats.case_inputs(name, tmp_path) if name == "syn_m" else spanscases.case_inputs(name, tmp_path)
    idx.to_device(ctx)
    host = _run(ctx, idx, mo, q, None, monkeypatch, capfd, str(tmp_path / "host.dump"), knobs)
    dev = _run(ctx, idx, mo, q, "1", monkeypatch, capfd, str(tmp_path / "dev.dump"), knobs)
    idx.close()
    _check_pair(host, dev)
    assert dev[0] == ref, "text differs from the reference"
    upload = [l for l in dev[2].split("\n") if "walks upload:" in l]
    assert len(upload) == 1 and NO_WORDS in upload[0], upload
    assert "walks upload:" not in host[2]
    assert "alignment statistics on the GPU" in dev[2] and "alignment statistics on the GPU" in host[2]
    assert not [l for l in dev[2].split("\n") if "declined" in l]


def test_edge_genome(ctx, tmp_path, monkeypatch, capfd):
    """regions on reverse strands and at contig ends"""
    contigs, prots, names, mo = regioncases.edge_genome()
    idx, q = regioncases.edge_index(contigs), mpa.Queries(prots, names)
    idx.to_device(ctx)
    host = _run(ctx, idx, mo, q, None, monkeypatch, capfd, str(tmp_path / "host.dump"))
    dev = _run(ctx, idx, mo, q, "1", monkeypatch, capfd, str(tmp_path / "dev.dump"))
    idx.close()
    _check_pair(host, dev)
    assert dev[0] == open(golden.path(regioncases.EDGE_REF), "rb").read()


def test_stream_of_three_batches(ctx, tmp_path, monkeypatch, capfd):
    """mpa_map_batches(): the steps run on the lanes' contexts -- same bytes, both notes of every batch, the host's dump"""
    idx, mo, q, ref = spanscases.case_inputs("syn_b", tmp_path)
    idx.to_device(ctx)
    n = len(q.seqs)
    batches = [mpa.Queries(q.seqs[a:b], q.names[a:b]) for a, b in ((0, n // 3), (n // 3, 2 * n // 3), (2 * n // 3, n))]
    monkeypatch.setenv("MPA_TIMING", "1")
    out = []
    for knob in (None, "1"):
        if knob:
            monkeypatch.setenv("MPA_GPU_SPANS", knob)
        else:
            monkeypatch.delenv("MPA_GPU_SPANS", raising=False)
        capfd.readouterr()
        texts, dump = spanscases.with_dump(monkeypatch, str(tmp_path / "stream.dump"), lambda: mpa.map_batches(ctx, idx, mo, batches, 4))
        out.append((b"".join(texts), dump, capfd.readouterr().err))
    idx.close()
    host, dev = out
    assert dev[0] == ref and host[0] == ref
    assert dev[2].count(DEVICE_NOTE) == 6 and "spans declined" not in dev[2] and DEVICE_NOTE not in host[2]
    # (the batches of a stream finish in any order: the dump's queries are compared as a set of records)
    key = lambda d: sorted((qid, [(p.tobytes(), c.tobytes()) for p, c in plans]) for qid, plans in spansdump.parse(d))
    assert len(host[1]) > 0 and key(dev[1]) == key(host[1])


@pytest.fixture(scope="module")
def world():
    idx, q, mo = spanscases.world()
    yield idx, q, mo
    idx.close()


def _both(ctx, world, P):
    """hand-made plans through the shared core on the host (ctx NULL) and through the kernels: the two results"""
    idx, q, mo = world
    idx.to_device(ctx)
    plans, segs, rst1, pool1 = P.arrays()
    rec, tasks = spanscases.dbg_spans(None, idx, mo, q, plans, segs, rst1, pool1)
    rst2, pool2 = P.round2(rec)
    host = spanscases.dbg_spans(None, idx, mo, q, plans, segs, rst1, pool1, rst2, pool2)
    dev = spanscases.dbg_spans(ctx, idx, mo, q, plans, segs, rst1, pool1, rst2, pool2)
    assert dev[0].tobytes() == host[0].tobytes(), "span records differ"
    assert dev[1].tobytes() == host[1].tobytes(), "round-2 tasks differ"
    assert dev[2].tobytes() == host[2].tobytes(), "assemble records differ"
    for j, (a, b) in enumerate(zip(dev[3], host[3])):
        assert a.tobytes() == b.tobytes(), "plan %d: cigar %r against %r" % (j, a[:20], b[:20])
    assert not host[2]["bad"].any()
    return host


def test_handmade_plans_on_the_device_against_the_shared_core(ctx, world):
    """the inputs of tests/spans_check.cpp (spanscases.handmade): thresholds of both repeats, the right span's three ways not to be
    made, the shortcut's limits, the boundaries that merge and those that never do, 0 - 200 gap segments, segments of 1 - 300 words"""
    T, P = spanscases.handmade(world[1])
    rec, tasks, arec, cig = _both(ctx, world, P)
    d = dict(T)
    W = spanscases.W
    assert list(cig[d["seven single-word M segments"]]) == [W(0, 48)]
    assert [len(cig[d[k]]) for k in ("M|M", "M|I", "10|10", "11|11", "N|N")] == [4, 5, 5, 5, 4]
    assert rec[d["left repeat: l_nt == max_ext - 1"]]["flags"] & spansdump.LEFT_REPEAT and not rec[d["left repeat: l_nt == max_ext"]]["flags"] & spansdump.LEFT_REPEAT
    assert rec[d["right repeat: r_nt == max_ext - 1"]]["flags"] & spansdump.RIGHT_REPEAT and not rec[d["right repeat: r_nt == max_ext"]]["flags"] & spansdump.RIGHT_REPEAT
    for k in ("right span: r_nt == 0", "right span: r_aa == 0", "right span: has_right == 0"):
        assert not rec[d[k]]["flags"] & spansdump.RIGHT
    assert rec[d["right span: made"]]["flags"] & spansdump.RIGHT
    assert rec[d["shortcut: alen == kmer2"]]["left"]["task"] < 0 and rec[d["shortcut: alen == kmer2 + 1"]]["left"]["task"] >= 0
    assert rec[d["shortcut: nlen != 3 alen"]]["left"]["task"] >= 0
    assert arec[d["200 gap segments"]]["n_cigar"] > 200 and arec[d["a segment of 300 words"]]["n_cigar"] >= 598   # (two segments of 300 words, two single words, at most four merges)
    # the task numbers are the host's running count: query-major, plans in order, left before right
    want = 0
    for r in rec:
        for seg in (r["left"], r["right"]):
            if seg["task"] >= 0:
                assert seg["task"] == want
                want += 1
    assert want == len(tasks) > 0


def test_a_thousand_plans_number_their_tasks_across_workgroups(ctx, world):
    """1 000 plans of 0 - 2 tasks each: k_spans runs four workgroups of 256 plans, and the numbers carry over at plans 255, 256, 257"""
    P = spanscases.many_plans(world[1])
    rec, tasks, arec, cig = _both(ctx, world, P)
    n_of = [int(r["left"]["task"] >= 0) + int(r["right"]["task"] >= 0) for r in rec]
    assert len(rec) == 1000 and set(n_of) == {0, 1, 2} and sum(n_of) == len(tasks)
    first = np.concatenate([[0], np.cumsum(n_of)])
    for j in (255, 256, 257, 511, 512, 767, 768, 999):
        got = [int(s["task"]) for s in (rec[j]["left"], rec[j]["right"]) if s["task"] >= 0]
        assert got == list(range(int(first[j]), int(first[j + 1]))), j
    assert sum(n_of[255:258]) > 0


def test_round_2_without_tasks(ctx, world):
    """every span takes the shortcut: no round-2 task, k_assemble runs without round-2 results or pool"""
    P = spanscases.Plans(world[1])
    for j in range(70):
        P.add(left=(3 * (j % 6), j % 6), right=None if j % 3 == 0 else (3 * (1 + j % 5), 1 + j % 5), qid=j % 4, vid=j % 4, vs0=900 + 31 * j,
              gaps=[spanscases.short_gap(2), spanscases.dp_gap([spanscases.W(0, 9)])][:j % 3])
    rec, tasks, arec, cig = _both(ctx, world, P)
    assert len(tasks) == 0 and all(r["left"]["task"] < 0 and r["right"]["task"] < 0 for r in rec)
    assert all(len(c) == 1 for c in cig) and (arec["n_merged"] > 0).any()


def test_knob_unset_is_the_host_path(ctx, tmp_path, monkeypatch, capfd):
    """(shows nothing on its own) no note, the dump of the first run again"""
    idx, mo, q, ref = spanscases.case_inputs("syn_a", tmp_path)
    idx.to_device(ctx)
    a = _run(ctx, idx, mo, q, None, monkeypatch, capfd, str(tmp_path / "a.dump"))
    b = _run(ctx, idx, mo, q, "0", monkeypatch, capfd, str(tmp_path / "b.dump"))
    idx.close()
    assert DEVICE_NOTE not in a[2] + b[2] and spanscases.MODEL_NOTE not in a[2] + b[2]
    assert a[1] == b[1] and a[0] == b[0] == ref
