"""MPA_GPU_ROUND2=1: a batch's DP round 2 planned from the tasks the device step between the rounds left in place, its result records and
dense CIGAR pool assembled on the device in front of the round's one wait (dp_results_kernels.hip).
(a) mpa_dbg_dp_run_resident on a context against mpa_dp_run on the same context with the knobs unset: records and dense pool byte for
    byte, a subset against the oracle; the hook's record says one wait, no task bytes up, no pool bytes down before the explicit fetch; a
    table the device planner declines and a repeated round come back as declined.
(b) the whole path with MPA_GPU_SPANS=1 MPA_GPU_DPPLAN=1 MPA_GPU_ROUND2=1 and with every device knob: the golden bytes, MPA_SPANS_DUMP
    equal to the run with the knob unset, the timing line; the declined note without the spans knob; the late pool fetch behind the
    forced decline (MPA_TEST_ROUND2_DECLINE)."""
import os
import re
import subprocess
import sys
import numpy as np
import pytest
import miniprot_amd as mpa
import alnstats
import dpplan
import dpresults as dr
import golden
import regioncases
import spanscases
import spansdump
from dpplan import EXT, GLOB
from hostpipe import oracle_executor

pytestmark = pytest.mark.gpu

R2_KNOBS = {"MPA_GPU_SPANS": "1", "MPA_GPU_DPPLAN": "1", "MPA_GPU_ROUND2": "1"}
EVERY_KNOB = dict(R2_KNOBS, MPA_GPU_PLANS="1", MPA_GPU_REGIONS="1", MPA_GPU_STATS="1", MPA_GPU_CS="1", MPA_GPU_ROWS="1", MPA_GPU_SKETCH="1", MPA_GPU_SEED="1", MPA_GPU_REFINE="1")
ALL_NAMES = sorted(set(EVERY_KNOB) | {"MPA_TEST_ROUND2_DECLINE"})
RESIDENT_NOTE = re.compile(r"dp: round 2 resident: (\d+) up, (\d+) down, 1 wait")
DECLINE_NOTE, LATE_NOTE = "round 2 resident declined", "round 2 resident: pool fetched late"


# ---- (a)
def _world():
    """a three-contig random genome of dpplan.CTG_LEN and four random proteins of dpplan.Q_LEN"""
    rng = np.random.default_rng(9500)
    contigs = [rng.integers(0, 4, n).astype(np.uint8) for n in dpplan.CTG_LEN]
    aa = np.frombuffer(b"ARNDCQEGHILKMFPSTWYV", dtype=np.uint8)
    return mpa.Index.from_nt4(contigs), mpa.Queries([aa[rng.integers(0, 20, n)].tobytes() for n in dpplan.Q_LEN])


def _mixed(n, lite_min, seed):
    """n calls that cycle through extension calls and traceback calls of at most 64, 65..128, 129..256 and more than 256 columns, with row
    counts below and above the checkpointing threshold"""
    r = np.random.default_rng(seed)
    kinds = [(EXT, 1, 200), (GLOB, 1, 64), (GLOB, 65, 128), (GLOB, 129, 256), (GLOB, 257, 330), (EXT, 201, 600)]
    rows = [max(3, lite_min // 3), max(3, lite_min - 1), lite_min, lite_min + 150]
    spec = []
    for k in range(n):
        mode, lo, hi = kinds[k % len(kinds)]
        spec.append((mode, int(r.integers(lo, hi + 1)), rows[int(r.integers(0, 4))] if mode == GLOB else int(r.integers(3, 700))))
    return dpplan._table(r, spec)


@pytest.fixture(scope="module", params=[(384, 0), (120, 1)], ids=["lite384", "lite120-wide"])
def lane(request):
    """a context per checkpointing threshold (MPA_DP_LITE_MIN / MPA_DP_LITE_WIDE are read when a context is created) with the world on it"""
    lite_min, wide = request.param
    old = {k: os.environ.get(k) for k in ("MPA_DP_LITE_MIN", "MPA_DP_LITE_WIDE")}
    os.environ["MPA_DP_LITE_MIN"], os.environ["MPA_DP_LITE_WIDE"] = str(lite_min), str(wide)
    try:
        ctx = mpa.Context(0)
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    idx, q = _world()
    idx.to_device(ctx)
    yield ctx, idx, q, lite_min
    idx.close()
    ctx.close()


def _unset(monkeypatch):
    for k in ALL_NAMES:
        monkeypatch.delenv(k, raising=False)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 3000])
def test_the_hook_against_mpa_dp_run(lane, n, monkeypatch, oracle_built):
    ctx, idx, q, lite_min = lane
    _unset(monkeypatch)
    tasks = _mixed(n, lite_min, 9510 + n)
    if n == 1:
        tasks = _mixed(2, lite_min, 9510)[1:]                        # (one traceback call)
    want_rst, want_pool = mpa.dp_run(ctx, idx, dpplan.dpopt(), q, tasks)
    got = mpa.dbg_dp_run_resident(ctx, idx, dpplan.dpopt(), q, tasks)
    assert len(got) == 3, got
    rst, pool, rec = got
    assert rst.tobytes() == want_rst.tobytes(), "result records differ"
    assert pool.tobytes() == want_pool.tobytes(), "dense pools differ"
    assert rec["round_waits"] == 1 and rec["plan_waits"] == 1, rec
    assert rec["task_bytes_up"] == 0 and rec["pool_bytes_down"] == 0 and rec["pool_bytes_fetched"] == 4 * len(want_pool), rec
    assert rec["bytes_down"] >= 24 * n and rec["n_pool"] == len(want_pool), rec
    assert (rec["prep_bound"], rec["max_nl"], rec["max_al"]) == dr.bounds_of(tasks), rec
    if n == 257:                                                     # the subset that also goes to the oracle
        per = lambda r, p: [(int(x["nt_len"]), int(x["aa_len"]), int(x["score"]), [int(w) for w in p[x["cigar_off"]: x["cigar_off"] + x["n_cigar"]]]) for x in r]
        want, have = per(*oracle_executor(idx, q, dpplan.dpopt(), tasks)), per(rst, pool)
        bad = [k for k in range(n) if have[k] != want[k]]
        assert not bad, "%d/%d DP calls differ from the oracle, first %d" % (len(bad), n, bad[0])


def test_only_extension_calls(lane, monkeypatch):
    """no traceback id exists: no scan, no gather, an empty pool"""
    ctx, idx, q, lite_min = lane
    _unset(monkeypatch)
    tasks = _mixed(600, lite_min, 9520)
    tasks = tasks[dr.is_ext(tasks)]
    want_rst, want_pool = mpa.dp_run(ctx, idx, dpplan.dpopt(), q, tasks)
    rst, pool, rec = mpa.dbg_dp_run_resident(ctx, idx, dpplan.dpopt(), q, tasks)
    assert rst.tobytes() == want_rst.tobytes() and len(pool) == len(want_pool) == 0 and rec["round_waits"] == 1


def test_a_declined_table_says_so(lane, monkeypatch):
    """gap extension above 255: the device planner leaves the round to mpa_dp_run"""
    ctx, idx, q, _ = lane
    _unset(monkeypatch)
    tasks, over, _ = dpplan.cases()["e_wide_ge"]
    r = mpa.dbg_dp_run_resident(ctx, idx, dpplan.dpopt(**over), q, tasks)
    assert len(r) == 2 and r[0] == mpa.ROUND2_DECLINED, r


def test_a_repeated_round_declines():
    """MPA_TEST_HANDOFF_FAIL=1 (read once per process: a child): the hand-off of a split extension call is reported as timed out behind the
    round's wait, and the resident round comes back as declined -- mpa_dp_run repeats it"""
    code = ("import sys; sys.path.insert(0, 'tests'); import conftest, miniprot_amd as mpa, dpplan, dpplan_device as dd\n"
            "import test_round2_gpu as t\n"
            "tasks, over, _ = dd.planned()['spread_default']\n"
            "idx, q = t._world(); ctx = mpa.Context(0); idx.to_device(ctx)\n"
            "r = mpa.dbg_dp_run_resident(ctx, idx, dpplan.dpopt(), q, tasks)\n"
            "print('result', len(r), r[0] if len(r) == 2 else '', r[1] if len(r) == 2 else '')\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = {}
    for fail in ("1", "0"):
        r = subprocess.run([sys.executable, "-c", code], cwd=root, env=dict(os.environ, MPA_TEST_HANDOFF_FAIL=fail), capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout + r.stderr
        out[fail] = r.stdout
    assert "result 2 %d" % mpa.ROUND2_DECLINED in out["1"] and "hand-off" in out["1"], out["1"]
    assert "result 3" in out["0"], out["0"]


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


def _check_resident(plain, dev, ref):
    assert dev[0] == plain[0] == ref, "text differs from the reference"
    assert len(plain[1]) > 0 and dev[1] == plain[1], spansdump.first_difference(dev[1], plain[1])
    notes = RESIDENT_NOTE.findall(dev[2])
    assert len(notes) == 1 and DECLINE_NOTE not in dev[2] and LATE_NOTE not in dev[2], [l for l in dev[2].split("\n") if "round 2" in l or "declined" in l][:6]
    assert "resident" not in plain[2]
    return int(notes[0][0]), int(notes[0][1])


@pytest.mark.parametrize("name,knobs", [("syn_a", R2_KNOBS), ("syn_m", R2_KNOBS), ("syn_a", EVERY_KNOB), ("syn_m", EVERY_KNOB)], ids=["syn_a", "syn_m", "syn_a-every-knob", "syn_m-every-knob"])
def test_golden_cases(ctx, name, knobs, tmp_path, monkeypatch, capfd):
    idx, mo, q, ref = alnstats.case_inputs(name, tmp_path) if name == "syn_m" else spanscases.case_inputs(name, tmp_path)
    idx.to_device(ctx)
    plain = _run(ctx, idx, mo, q, {}, monkeypatch, capfd, str(tmp_path / "plain.dump"))
    dev = _run(ctx, idx, mo, q, knobs, monkeypatch, capfd, str(tmp_path / "dev.dump"))
    idx.close()
    up, down = _check_resident(plain, dev, ref)
    # round 2's uploads are the query offsets and residues, its downloads header, records and traceback ids: no task record (40 bytes a
    # task) goes up, and the records that come down are 24 bytes a task
    n_task2 = sum(int(p["left"]["task"] >= 0) + int(p["right"]["task"] >= 0) for _, plans in spansdump.parse(dev[1]) for p, _ in plans)
    total_aa = sum(len(s) for s in q.seqs)
    assert n_task2 > 0 and up <= total_aa + 8 * (len(q.seqs) + 1) + 1024, (up, total_aa, n_task2)
    assert 24 * n_task2 <= down <= 28 * n_task2 + 8192, (down, n_task2)


def test_edge_genome(ctx, tmp_path, monkeypatch, capfd):
    """regions on reverse strands and at contig ends"""
    contigs, prots, names, mo = regioncases.edge_genome()
    idx, q = regioncases.edge_index(contigs), mpa.Queries(prots, names)
    idx.to_device(ctx)
    plain = _run(ctx, idx, mo, q, {}, monkeypatch, capfd, str(tmp_path / "plain.dump"))
    dev = _run(ctx, idx, mo, q, R2_KNOBS, monkeypatch, capfd, str(tmp_path / "dev.dump"))
    every = _run(ctx, idx, mo, q, EVERY_KNOB, monkeypatch, capfd, str(tmp_path / "every.dump"))
    idx.close()
    ref = open(golden.path(regioncases.EDGE_REF), "rb").read()
    _check_resident(plain, dev, ref)
    _check_resident(plain, every, ref)


@pytest.mark.parametrize("knobs", [R2_KNOBS, EVERY_KNOB], ids=["three-knobs", "every-knob"])
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
    assert len(RESIDENT_NOTE.findall(dev[2])) == 3 and DECLINE_NOTE not in dev[2], [l for l in dev[2].split("\n") if "declined" in l][:6]
    # (the batches of a stream finish in any order: the dump's queries are compared as a set of records)
    key = lambda d: sorted((qid, [(p.tobytes(), c.tobytes()) for p, c in plans]) for qid, plans in spansdump.parse(d))
    assert len(plain[1]) > 0 and key(dev[1]) == key(plain[1])


def test_without_the_spans_knob_the_round_declines(ctx, tmp_path, monkeypatch, capfd):
    idx, mo, q, ref = spanscases.case_inputs("syn_a", tmp_path)
    idx.to_device(ctx)
    plain = _run(ctx, idx, mo, q, {}, monkeypatch, capfd, str(tmp_path / "plain.dump"))
    dev = _run(ctx, idx, mo, q, {"MPA_GPU_ROUND2": "1"}, monkeypatch, capfd, str(tmp_path / "dev.dump"))
    idx.close()
    assert dev[0] == plain[0] == ref and dev[1] == plain[1]
    assert dev[2].count(DECLINE_NOTE) == 1 and "did not run on the device" in dev[2] and not RESIDENT_NOTE.findall(dev[2])


def test_the_forced_decline_takes_the_late_pool_fetch(ctx, tmp_path, monkeypatch, capfd):
    """MPA_TEST_ROUND2_DECLINE=1: the step behind the resident round 2 declines, the host fetches the dense pool from the context in a second
    wait and joins the words itself"""
    idx, mo, q, ref = spanscases.case_inputs("syn_a", tmp_path)
    idx.to_device(ctx)
    plain = _run(ctx, idx, mo, q, {}, monkeypatch, capfd, str(tmp_path / "plain.dump"))
    dev = _run(ctx, idx, mo, q, dict(R2_KNOBS, MPA_TEST_ROUND2_DECLINE="1"), monkeypatch, capfd, str(tmp_path / "dev.dump"))
    idx.close()
    assert dev[0] == plain[0] == ref and dev[1] == plain[1], spansdump.first_difference(dev[1], plain[1])
    assert len(RESIDENT_NOTE.findall(dev[2])) == 1 and dev[2].count(LATE_NOTE) == 1 and "device spans declined (MPA_TEST_ROUND2_DECLINE)" in dev[2]
    m = re.search(r"pool fetched late, (\d+) bytes down", dev[2])
    assert m and int(m.group(1)) > 0
