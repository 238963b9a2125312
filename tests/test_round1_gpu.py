"""MPA_GPU_ROUND1=1: a batch's DP round 1 planned on the device, its result records and dense CIGAR pool assembled there, and the step between
the rounds (k_spans, k_spans_emit, k_task_bounds) chained behind them inside the round's one wait.
(a) mpa_dbg_round1_chain on a context against today's path on the same context -- mpa_dp_run, then mpa_dbg_spans on its results: result
    records, span records, round-2 tasks and their count, the three bounds and the fetched pool byte for byte, a subset against the oracle;
    the hook's record says one wait, no pool bytes down before the fetch, no result record among the bytes up; a table the device planner
    declines comes back as declined; the device guard with a non-zero word (mpa_dbg_spans_guard) stops the step.  The tables are the plans, gap segments and round-1 tasks of syn_b (tests/round1cases.py), tiled.
(b) the whole path with MPA_GPU_SPANS=1 MPA_GPU_ROUND1=1, with MPA_GPU_ROUND2=1 added and with every device knob: the golden bytes,
    MPA_SPANS_DUMP equal to the run without knobs, exactly one timing line per batch; the declined note without the spans knob; the
    repeated round (MPA_TEST_HANDOFF_FAIL); both late pool fetches behind the forced decline (MPA_TEST_ROUND2_DECLINE).
    The cases' round 1 holds no call the device planner declines (no extension call above 1 024 columns, one traceback chunk): checked
    without a device by classifying the tasks of tests/hostpipe.py's stage machine -- syn_a, syn_m, the edge genome and syn_b as they are."""
import os
import re
import subprocess
import sys
import numpy as np
import pytest
import miniprot_amd as mpa
import alnstats
import dpresults as dr
import golden
import planscases
import regioncases
import round1cases as r1
import spanscases
import spansdump
from hostpipe import oracle_executor

pytestmark = pytest.mark.gpu

R1_KNOBS = {"MPA_GPU_SPANS": "1", "MPA_GPU_ROUND1": "1"}
R1R2_KNOBS = dict(R1_KNOBS, MPA_GPU_ROUND2="1")
EVERY_KNOB = dict(R1R2_KNOBS, MPA_GPU_DPPLAN="1", MPA_GPU_PLANS="1", MPA_GPU_REGIONS="1", MPA_GPU_STATS="1", MPA_GPU_CS="1", MPA_GPU_ROWS="1", MPA_GPU_SKETCH="1", MPA_GPU_SEED="1",
                  MPA_GPU_REFINE="1", MPA_GPU_FINISH="1", MPA_GPU_FORMAT="1")
ALL_NAMES = sorted(set(EVERY_KNOB) | {"MPA_TEST_ROUND2_DECLINE", "MPA_PLANS_DUMP"})
RESIDENT_NOTE = re.compile(r"dp: round 1 resident: (\d+) up, (\d+) down, (\d+) wait")
DECLINE_NOTE = "round 1 resident declined"
LATE1_NOTE, LATE2_NOTE = "round 1 resident: pool fetched late", "round 2 resident: pool fetched late"


def _unset(monkeypatch):
    for k in ALL_NAMES:
        monkeypatch.delenv(k, raising=False)


# ---- (a)
@pytest.fixture(scope="module", params=[(384, 0), (120, 1)], ids=["lite384", "lite120-wide"])
def lane(request, tmp_path_factory):
    """a context per checkpointing threshold (MPA_DP_LITE_MIN / MPA_DP_LITE_WIDE are read when a context is created) with syn_b on it, and
    the units of syn_b's plans dump from a run without knobs on that context"""
    lite_min, wide = request.param
    tmp = tmp_path_factory.mktemp("round1")
    dump_path = str(tmp / "plans.dump")
    old = {k: os.environ.get(k) for k in ["MPA_DP_LITE_MIN", "MPA_DP_LITE_WIDE"] + ALL_NAMES}
    for k in ALL_NAMES:
        os.environ.pop(k, None)
    os.environ["MPA_DP_LITE_MIN"], os.environ["MPA_DP_LITE_WIDE"] = str(lite_min), str(wide)
    try:
        ctx = mpa.Context(0)
        idx, mo, q, _ = planscases.case_inputs("syn_b", tmp)
        idx.to_device(ctx)
        os.environ["MPA_PLANS_DUMP"] = dump_path
        mpa.map_batch(ctx, idx, mo, q, 4).close()
    finally:
        os.environ.pop("MPA_PLANS_DUMP", None)
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    us = r1.units(open(dump_path, "rb").read(), q)
    assert len(us) > 10
    yield ctx, idx, mo, q, us
    idx.close()
    ctx.close()


def _both_paths(lane, table):
    """(today's path, the hook) on one table: ((rst, pool, span records, round-2 tasks), the hook's tuple)"""
    ctx, idx, mo, q, _ = lane
    plans, tasks, segs = table
    dpopt = mpa.dpopt_from(mo)
    want_rst, want_pool = mpa.dp_run(ctx, idx, dpopt, q, tasks)
    want_rec, want_t2 = mpa.dbg_spans(ctx, idx, mo, q, plans, segs, want_rst, want_pool)
    got = mpa.dbg_round1_chain(ctx, idx, mo, dpopt, q, plans, segs, tasks)
    return (want_rst, want_pool, want_rec, want_t2), got


def _check_hook(lane, table):
    ctx, idx, mo, q, _ = lane
    plans, tasks, segs = table
    (want_rst, want_pool, want_rec, want_t2), got = _both_paths(lane, table)
    assert len(got) == 6, got
    rst, pool, rec, t2, bounds, info = got
    assert rst.tobytes() == want_rst.tobytes(), "result records differ"
    assert rec == want_rec, "span records differ"
    assert len(t2) == len(want_t2) and t2 == want_t2, "round-2 tasks differ (%d against %d)" % (len(t2) // 40, len(want_t2) // 40)
    assert bounds == dr.bounds_of(np.frombuffer(want_t2, mpa.DP_TASK)), bounds
    assert pool.tobytes() == want_pool.tobytes(), "dense pools differ"
    # the record: one wait behind the planner's, no pool words down before the explicit fetch, the step's kernels inside the wait, and an
    # upload that holds the planner's block, the residues and the step's block without its record section -- no result record (24 n bytes)
    n, text = len(tasks), sum(len(s) for s in q.seqs)
    assert info["plan_waits"] == 1 and info["round_waits"] == 1, info
    assert info["pool_bytes_down"] == 0 and info["pool_bytes_fetched"] == 4 * len(want_pool), info
    assert info["chained_launches"] >= 2, info
    assert info["plan_bytes_up"] == r1.planner_upload_bytes(n, len(q.seqs)) and info["residue_bytes"] == text, info
    assert info["spans_bytes_up"] == r1.spans_block_bytes(len(plans), len(segs), text) and info["rst1_bytes_skipped"] >= 24 * n, info
    assert info["bytes_up"] == info["plan_bytes_up"] + info["residue_bytes"] + info["spans_bytes_up"], info
    assert info["task_bytes_up"] >= 40 * n and info["bytes_down"] >= 24 * n + 80 * len(plans), info
    return rst, pool


@pytest.mark.parametrize("n_plan", [1, 255, 256, 257, 1000])
def test_the_hook_against_todays_path_by_plans(lane, n_plan, monkeypatch, oracle_built):
    """1 plan; the SPANS_BLOCK edge; about 1 000 plans, whose round-2 task numbers cross workgroups"""
    _unset(monkeypatch)
    table = r1.tile_plans(lane[4], n_plan)
    assert len(table[0]) == n_plan and not r1.only_extension_calls(table[1])
    rst, pool = _check_hook(lane, table)
    if n_plan == 1:                                                  # the subset that also goes to the oracle
        ctx, idx, mo, q, _ = lane
        tasks = table[1]
        per = lambda r, p: [(int(x["nt_len"]), int(x["aa_len"]), int(x["score"]), [int(w) for w in p[x["cigar_off"]: x["cigar_off"] + x["n_cigar"]]]) for x in r]
        want, have = per(*oracle_executor(idx, q, mpa.dpopt_from(mo), tasks)), per(rst, pool)
        bad = [k for k in range(len(tasks)) if have[k] != want[k]]
        assert not bad, "%d/%d DP calls differ from the oracle, first %d" % (len(bad), len(tasks), bad[0])


@pytest.mark.parametrize("n_task", [255, 256, 257])
def test_the_hook_against_todays_path_by_calls(lane, n_task, monkeypatch):
    """the TeamWG::W edge of the results kernels"""
    _unset(monkeypatch)
    table = r1.tile_tasks(lane[4], n_task)
    assert len(table[1]) == n_task
    _check_hook(lane, table)


def test_a_table_without_a_gap_segment(lane, tmp_path, monkeypatch):
    """a protein aligned end to end to a gene without an intron: round 1 holds extension calls only -- no scan, no gather, a pool of 0 words"""
    _unset(monkeypatch)
    ctx = lane[0]
    idx, q, mo = spanscases.short_gene()
    idx.to_device(ctx)
    _, dump = planscases.with_dump(monkeypatch, str(tmp_path / "plans.dump"), lambda: mpa.map_batch(ctx, idx, mo, q, 1).close())
    us = r1.units(dump, q)
    table = r1.tile_plans(us, 1)
    assert r1.only_extension_calls(table[1]) and int((table[2]["task"] >= 0).sum()) == 0
    rst, pool = _check_hook((ctx, idx, mo, q, us), table)
    idx.close()
    assert len(pool) == 0 and int(rst["n_cigar"].sum()) == 0


@pytest.mark.parametrize("err,bad", [(1, 0), (0, 1), (7, 1 << 40)], ids=["hand-off-error", "bad-call", "both"])
def test_the_device_guard_stops_the_step(lane, err, bad, monkeypatch):
    """the words a chained step is guarded by, set non-zero on the device (mpa_dbg_spans_guard): k_spans, k_spans_emit and k_task_bounds
    leave a task count of 0 and bounds of 0 on a table whose unguarded step makes round-2 tasks (257 plans: two workgroups, the second
    with one plan).  The records handed in are a real round's: the guard is observed by its outputs, nothing is provoked"""
    ctx, idx, mo, q, us = lane
    _unset(monkeypatch)
    plans, tasks, segs = r1.tile_plans(us, 257)
    rst, pool = mpa.dp_run(ctx, idx, mpa.dpopt_from(mo), q, tasks)
    _, t2 = mpa.dbg_spans(ctx, idx, mo, q, plans, segs, rst, pool)
    assert len(t2) >= 40 * 64                                        # (unguarded: the step makes round-2 tasks)
    assert mpa.dbg_spans_guard(ctx, idx, mo, q, plans, segs, rst, err, bad) == (0, (0, 0, 0))
    # ... and the step behind it on the same context is what it was
    assert mpa.dbg_spans(ctx, idx, mo, q, plans, segs, rst, pool)[1] == t2
    r = mpa.dbg_spans_guard(ctx, idx, mo, q, plans, segs, rst, 0, 0)
    assert len(r) == 2 and r[0] == -5 and "both guard words are zero" in r[1], r


def test_a_declined_table_says_so(lane, monkeypatch):
    """one extension call of 1 100 columns (a call no plan names, behind the table): the device planner leaves the round to mpa_dp_run, and
    today's path on the same table still agrees with the core"""
    ctx, idx, mo, q, us = lane
    _unset(monkeypatch)
    plans, tasks, segs = r1.tile_plans(us, 3)
    # (no protein of the case has 1 100 residues: one more query behind the others, which keep their numbers and offsets)
    rng = np.random.default_rng(9610)
    long_q = np.frombuffer(b"ARNDCQEGHILKMFPSTWYV", dtype=np.uint8)[rng.integers(0, 20, 1200)].tobytes()
    q = mpa.Queries(list(q.seqs) + [long_q], list(q.names) + ["long"])
    extra = tasks[:1].copy()
    extra["flag"], extra["qid"], extra["aa_off"], extra["al"] = mpa.F_EXT_RIGHT, len(q.seqs) - 1, 0, 1100
    tasks = np.concatenate([tasks, extra])
    (want_rst, want_pool, want_rec, want_t2), got = _both_paths((ctx, idx, mo, q, us), (plans, tasks, segs))
    assert len(got) == 2 and got[0] == mpa.ROUND1_DECLINED and "device DP plan" in got[1], got
    core = mpa.dbg_spans(None, idx, mo, q, plans, segs, want_rst, want_pool)
    assert (want_rec, want_t2) == core


# ---- (b)
@pytest.fixture(scope="module")
def ctx():
    c = mpa.Context(0)
    yield c
    c.close()


def _run(ctx, idx, mo, q, knobs, monkeypatch, capfd, path):
    """one blocking batch with the given knobs: (text, dump, stderr)"""
    _unset(monkeypatch)
    monkeypatch.setenv("MPA_TIMING", "1")
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    capfd.readouterr()
    res, dump = spanscases.with_dump(monkeypatch, path, lambda: mpa.map_batch(ctx, idx, mo, q, 4))
    err = capfd.readouterr().err
    return mpa.format_output(idx, mo, q, res)[0], dump, err


def _check_resident(plain, dev, ref, n_batches=1):
    assert dev[0] == plain[0] == ref, "text differs from the reference"
    assert len(plain[1]) > 0 and dev[1] == plain[1], spansdump.first_difference(dev[1], plain[1])
    notes = RESIDENT_NOTE.findall(dev[2])
    assert len(notes) == n_batches and all(w == "1" for _, _, w in notes), [l for l in dev[2].split("\n") if "round 1" in l or "declined" in l][:6]
    assert DECLINE_NOTE not in dev[2] and LATE1_NOTE not in dev[2]
    assert "round 1 resident" not in plain[2]
    return [(int(u), int(d)) for u, d, _ in notes]


def _case(name, tmp_path):
    if name == "edge":
        contigs, prots, names, mo = regioncases.edge_genome()
        return regioncases.edge_index(contigs), mo, mpa.Queries(prots, names), open(golden.path(regioncases.EDGE_REF), "rb").read()
    return alnstats.case_inputs(name, tmp_path) if name == "syn_m" else spanscases.case_inputs(name, tmp_path)


@pytest.mark.parametrize("knobs", [R1_KNOBS, R1R2_KNOBS, EVERY_KNOB], ids=["spans-round1", "spans-round1-round2", "every-knob"])
@pytest.mark.parametrize("name", ["syn_a", "syn_m", "edge"])
def test_golden_cases(ctx, name, knobs, tmp_path, monkeypatch, capfd):
    idx, mo, q, ref = _case(name, tmp_path)
    idx.to_device(ctx)
    plain = _run(ctx, idx, mo, q, {}, monkeypatch, capfd, str(tmp_path / "plain.dump"))
    dev = _run(ctx, idx, mo, q, knobs, monkeypatch, capfd, str(tmp_path / "dev.dump"))
    idx.close()
    (up, down), = _check_resident(plain, dev, ref)
    # (the byte counts are checked exactly through the hook; here: the span records, 80 bytes a plan, are among what comes down)
    n_plan = sum(len(plans) for _, plans in spansdump.parse(dev[1]))
    assert n_plan > 0 and down >= 80 * n_plan and up > 0
    if "MPA_GPU_ROUND2" in knobs:
        assert len(re.findall(r"dp: round 2 resident: \d+ up, \d+ down, 1 wait", dev[2])) == 1 and "round 2 resident declined" not in dev[2]


@pytest.mark.parametrize("knobs", [R1_KNOBS, R1R2_KNOBS, EVERY_KNOB], ids=["spans-round1", "spans-round1-round2", "every-knob"])
def test_stream_of_three_batches(ctx, knobs, tmp_path, monkeypatch, capfd):
    idx, mo, q, ref = spanscases.case_inputs("syn_b", tmp_path)
    idx.to_device(ctx)
    n = len(q.seqs)
    batches = [mpa.Queries(q.seqs[a:b], q.names[a:b]) for a, b in ((0, n // 3), (n // 3, 2 * n // 3), (2 * n // 3, n))]
    out = []
    for kn in ({}, knobs):
        _unset(monkeypatch)
        monkeypatch.setenv("MPA_TIMING", "1")
        for k, v in kn.items():
            monkeypatch.setenv(k, v)
        capfd.readouterr()
        texts, dump = spanscases.with_dump(monkeypatch, str(tmp_path / "stream.dump"), lambda: mpa.map_batches(ctx, idx, mo, batches, 4))
        out.append((b"".join(texts), dump, capfd.readouterr().err))
    idx.close()
    plain, dev = out
    assert dev[0] == ref and plain[0] == ref
    notes = RESIDENT_NOTE.findall(dev[2])
    assert len(notes) == 3 and all(w == "1" for _, _, w in notes) and DECLINE_NOTE not in dev[2], [l for l in dev[2].split("\n") if "declined" in l][:6]
    # (the batches of a stream finish in any order: the dump's queries are compared as a set of records)
    key = lambda d: sorted((qid, [(p.tobytes(), c.tobytes()) for p, c in plans]) for qid, plans in spansdump.parse(d))
    assert len(plain[1]) > 0 and key(dev[1]) == key(plain[1])


def test_without_the_spans_knob_the_round_declines(ctx, tmp_path, monkeypatch, capfd):
    idx, mo, q, ref = spanscases.case_inputs("syn_a", tmp_path)
    idx.to_device(ctx)
    plain = _run(ctx, idx, mo, q, {}, monkeypatch, capfd, str(tmp_path / "plain.dump"))
    dev = _run(ctx, idx, mo, q, {"MPA_GPU_ROUND1": "1"}, monkeypatch, capfd, str(tmp_path / "dev.dump"))
    idx.close()
    assert dev[0] == plain[0] == ref and dev[1] == plain[1]
    assert dev[2].count(DECLINE_NOTE) == 1 and "MPA_GPU_SPANS is not 1" in dev[2] and not RESIDENT_NOTE.findall(dev[2])


def test_a_repeated_round_declines_and_is_repeated_once():
    """MPA_TEST_HANDOFF_FAIL=1 (read once per process: a child): syn_b's round 1 has split extension calls (257 .. 1 024 columns); their
    hand-off is reported as timed out behind the round's wait, the chained outputs are discarded, the round declines with the hand-off
    reason and mpa_dp_run repeats it once.  The host-side test switch reports the time-out: no kernel fails"""
    code = ("import sys, os, tempfile, pathlib; sys.path.insert(0, 'tests'); import conftest, miniprot_amd as mpa, spanscases\n"
            "tmp = pathlib.Path(tempfile.mkdtemp())\n"
            "idx, mo, q, ref = spanscases.case_inputs('syn_b', tmp)\n"
            "ctx = mpa.Context(0); idx.to_device(ctx)\n"
            "text = mpa.format_output(idx, mo, q, mpa.map_batch(ctx, idx, mo, q, 4))[0]\n"
            "print('retries', ctx.handoff_retries(), 'golden', text == ref)\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ALL_NAMES}
    env.update(R1_KNOBS, MPA_TIMING="1")
    out = {}
    for fail in ("1", "0"):
        r = subprocess.run([sys.executable, "-c", code], cwd=root, env=dict(env, MPA_TEST_HANDOFF_FAIL=fail), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        out[fail] = (r.stdout, r.stderr)
    so, se = out["1"]
    assert "retries 1 golden True" in so, so
    assert se.count(DECLINE_NOTE) == 1 and "round 1 resident declined (round 1 resident: a column-block hand-off timed out, the round is repeated by mpa_dp_run)" in se, \
        [l for l in se.split("\n") if "round 1" in l]
    assert not RESIDENT_NOTE.findall(se)
    so, se = out["0"]
    assert "retries 0 golden True" in so and len(RESIDENT_NOTE.findall(se)) == 1 and DECLINE_NOTE not in se, so


def test_the_forced_decline_takes_both_late_pool_fetches(ctx, tmp_path, monkeypatch, capfd):
    """MPA_TEST_ROUND2_DECLINE=1 with the three knobs: the step behind the resident round 2 declines and the host joins the words itself --
    round 1's from the spans step's pool and round 2's from the round's, each in a wait of its own"""
    idx, mo, q, ref = spanscases.case_inputs("syn_a", tmp_path)
    idx.to_device(ctx)
    plain = _run(ctx, idx, mo, q, {}, monkeypatch, capfd, str(tmp_path / "plain.dump"))
    dev = _run(ctx, idx, mo, q, dict(R1R2_KNOBS, MPA_TEST_ROUND2_DECLINE="1"), monkeypatch, capfd, str(tmp_path / "dev.dump"))
    idx.close()
    assert dev[0] == plain[0] == ref and dev[1] == plain[1], spansdump.first_difference(dev[1], plain[1])
    assert len(RESIDENT_NOTE.findall(dev[2])) == 1 and dev[2].count(LATE1_NOTE) == 1 and dev[2].count(LATE2_NOTE) == 1 and "device spans declined (MPA_TEST_ROUND2_DECLINE)" in dev[2]
    for note in (LATE1_NOTE, LATE2_NOTE):
        m = re.search(re.escape(note) + r", (\d+) bytes down", dev[2])
        assert m and int(m.group(1)) > 0
