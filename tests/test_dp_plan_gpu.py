"""MPA_GPU_DPPLAN=1: the planner of a DP round on the device (dp_plan_kernels.hip).
(a) mpa_dbg_dp_plan_device on a context: what the kernels leave in the pools and in the header is the host planner's serialised plan
    (mpa_dbg_dp_plan), byte for byte, for the tables of tests/dpplan_device.py; tables the device planner declines report that.
(b) mpa_dp_run on a random genome for two of the tables: results and CIGARs equal with the knob set and unset and equal the oracle's; the
    MPA_TIMING note says who planned.
(c) the whole path: golden cases, every device knob together, a stream of three batches -- the golden bytes."""
import os
import subprocess
import sys
import numpy as np
import pytest
import miniprot_amd as mpa
import alnstats
import dpplan
import dpplan_device as dd
import spanscases
from hostpipe import oracle_executor

pytestmark = pytest.mark.gpu

PLANNED = dd.planned()
DECLINED = dd.declined()
DEVICE_NOTE, DECLINE_NOTE, HOST_NOTE = "dp: plan on device", "device DP plan declined", "dp: classify/sort/layout"
EVERY_KNOB = {"MPA_GPU_SPANS": "1", "MPA_GPU_PLANS": "1", "MPA_GPU_REGIONS": "1", "MPA_GPU_STATS": "1", "MPA_GPU_CS": "1", "MPA_GPU_ROWS": "1", "MPA_GPU_SKETCH": "1",
              "MPA_GPU_SEED": "1", "MPA_GPU_REFINE": "1"}


@pytest.fixture(scope="module")
def ctx():
    c = mpa.Context(0)
    yield c
    c.close()


# ---- (a)
@pytest.mark.parametrize("name", sorted(PLANNED))
def test_the_kernels_leave_the_host_planners_plan(ctx, name):
    tasks, over, knobs = PLANNED[name]
    dd.assert_same_plan(dd.device_plan(ctx, tasks, over, knobs), dpplan.plan(tasks, over, knobs))


def test_twenty_thousand_calls(ctx):
    """79 workgroups of calls, every call of at most 64 rows: ties in most keys, the unit sort over 80 064 padded keys"""
    tasks, over, knobs = dd.big()
    assert len(tasks) == 20000 and int(tasks["nl"].max()) <= 64
    dd.assert_same_plan(dd.device_plan(ctx, tasks, over, knobs), dpplan.plan(tasks, over, knobs))


@pytest.mark.parametrize("name", sorted(DECLINED))
def test_declined_tables_say_so(ctx, name):
    tasks, over, knobs = DECLINED[name]
    r = dd.device_plan(ctx, tasks, over, knobs)
    assert isinstance(r, tuple) and r[0] == mpa.DP_PLAN_DECLINED, r


# ---- (b)
def _world():
    """a three-contig random genome of dpplan.CTG_LEN and four random proteins of dpplan.Q_LEN"""
    rng = np.random.default_rng(9300)
    contigs = [rng.integers(0, 4, n).astype(np.uint8) for n in dpplan.CTG_LEN]
    aa = np.frombuffer(b"ARNDCQEGHILKMFPSTWYV", dtype=np.uint8)
    return mpa.Index.from_nt4(contigs), mpa.Queries([aa[rng.integers(0, 20, n)].tobytes() for n in dpplan.Q_LEN])


def _per_call(rst, pool):
    return [(int(r["nt_len"]), int(r["aa_len"]), int(r["score"]), [int(x) for x in pool[r["cigar_off"]: r["cigar_off"] + r["n_cigar"]]]) for r in rst]


def _dp_run(ctx, idx, q, tasks, over, knob, monkeypatch, capfd):
    monkeypatch.setenv("MPA_TIMING", "1")
    if knob is None:
        monkeypatch.delenv("MPA_GPU_DPPLAN", raising=False)
    else:
        monkeypatch.setenv("MPA_GPU_DPPLAN", knob)
    capfd.readouterr()
    rst, pool = mpa.dp_run(ctx, idx, dpplan.dpopt(**over), q, tasks)
    return rst, pool, capfd.readouterr().err


@pytest.fixture(scope="module")
def world(ctx):
    idx, q = _world()
    idx.to_device(ctx)
    yield idx, q
    idx.close()


@pytest.mark.parametrize("name", ["spread_default", "prep_chunk_edge", "tiny_ext"])     # (tiny_ext: extension calls of fewer than three rows, answered without a unit)
def test_dp_run_with_the_device_plan(ctx, world, oracle_built, name, monkeypatch, capfd):
    """the executor's knobs are the context's (lite_min 384, lite_wide 0): the tables' calls, not their knob sets"""
    idx, q = world
    tasks, over, _ = PLANNED[name]
    host = _dp_run(ctx, idx, q, tasks, over, None, monkeypatch, capfd)
    dev = _dp_run(ctx, idx, q, tasks, over, "1", monkeypatch, capfd)
    assert DEVICE_NOTE in dev[2] and DECLINE_NOTE not in dev[2] and HOST_NOTE not in dev[2], dev[2]
    assert "bytes up" in dev[2] and HOST_NOTE in host[2] and DEVICE_NOTE not in host[2]
    assert dev[0].tobytes() == host[0].tobytes() and dev[1].tobytes() == host[1].tobytes()
    want = _per_call(*oracle_executor(idx, q, dpplan.dpopt(**over), tasks))
    got = _per_call(dev[0], dev[1])
    bad = [k for k in range(len(tasks)) if got[k] != want[k]]
    assert not bad, "%d/%d DP calls differ from the oracle, first %d: %r != %r" % (len(bad), len(tasks), bad[0], got[bad[0]][:3], want[bad[0]][:3])


def test_dp_run_declines_wide_ge(ctx, world, monkeypatch, capfd):
    idx, q = world
    tasks, over, _ = dpplan.cases()["e_wide_ge"]
    host = _dp_run(ctx, idx, q, tasks, over, None, monkeypatch, capfd)
    dev = _dp_run(ctx, idx, q, tasks, over, "1", monkeypatch, capfd)
    assert DECLINE_NOTE in dev[2] and HOST_NOTE in dev[2] and DEVICE_NOTE not in dev[2], dev[2]
    assert dev[0].tobytes() == host[0].tobytes() and dev[1].tobytes() == host[1].tobytes()


def test_a_repeated_round_declines():
    """MPA_TEST_HANDOFF_FAIL=1 (read once per process: a child): the first attempt is planned on the device, the repeated round (no_split)
    on the host, and the results are those of the run without either knob"""
    code = ("import sys, os; sys.path.insert(0, 'tests'); import conftest, numpy as np, miniprot_amd as mpa, dpplan, dpplan_device as dd\n"
            "import test_dp_plan_gpu as t\n"
            "tasks, over, _ = dd.planned()['spread_default']\n"
            "idx, q = t._world(); ctx = mpa.Context(0); idx.to_device(ctx)\n"
            "os.environ['MPA_GPU_DPPLAN'] = '1'\n"
            "rst, pool = mpa.dp_run(ctx, idx, dpplan.dpopt(), q, tasks)\n"
            "print('retries', ctx.handoff_retries())\n"
            "np.save(sys.argv[1], rst); np.save(sys.argv[2], pool)\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        out = []
        for k, fail in enumerate(("1", "0")):
            a, b = os.path.join(tmp, "rst%d.npy" % k), os.path.join(tmp, "pool%d.npy" % k)
            env = dict(os.environ, MPA_TEST_HANDOFF_FAIL=fail, MPA_TIMING="1")
            r = subprocess.run([sys.executable, "-c", code, a, b], cwd=root, env=env, capture_output=True, text=True, timeout=300)
            assert r.returncode == 0, r.stdout + r.stderr
            out.append((np.load(a), np.load(b), r.stdout, r.stderr))
    failed, plain = out
    assert "retries 1" in failed[2] and "retries 0" in plain[2]
    assert failed[3].count(DEVICE_NOTE + " ") == 1 and "a repeated round" in failed[3] and HOST_NOTE in failed[3], failed[3]
    assert DECLINE_NOTE not in plain[3]
    assert failed[0].tobytes() == plain[0].tobytes() and failed[1].tobytes() == plain[1].tobytes()


# ---- (c)
def _map(ctx, idx, mo, q, knobs, monkeypatch, capfd):
    monkeypatch.setenv("MPA_TIMING", "1")
    for k in list(EVERY_KNOB) + ["MPA_GPU_DPPLAN"]:
        monkeypatch.delenv(k, raising=False)
    for k, v in knobs.items():
        monkeypatch.setenv(k, v)
    capfd.readouterr()
    res = mpa.map_batch(ctx, idx, mo, q, 4)
    return mpa.format_output(idx, mo, q, res)[0], capfd.readouterr().err


@pytest.mark.parametrize("name,knobs", [("syn_a", {}), ("syn_m", {}), ("syn_a", EVERY_KNOB)], ids=["syn_a", "syn_m", "syn_a-every-knob"])
def test_golden_cases(ctx, name, knobs, tmp_path, monkeypatch, capfd):
    idx, mo, q, ref = alnstats.case_inputs(name, tmp_path) if name == "syn_m" else spanscases.case_inputs(name, tmp_path)
    idx.to_device(ctx)
    text, err = _map(ctx, idx, mo, q, dict(knobs, MPA_GPU_DPPLAN="1"), monkeypatch, capfd)
    idx.close()
    assert text == ref, "text differs from the reference"
    assert err.count(DEVICE_NOTE + " ") >= 1, [l for l in err.split("\n") if "dp:" in l and "plan" in l or "declined" in l][:6]


def test_stream_of_three_batches(ctx, tmp_path, monkeypatch, capfd):
    idx, mo, q, ref = spanscases.case_inputs("syn_b", tmp_path)
    idx.to_device(ctx)
    n = len(q.seqs)
    batches = [mpa.Queries(q.seqs[a:b], q.names[a:b]) for a, b in ((0, n // 3), (n // 3, 2 * n // 3), (2 * n // 3, n))]
    monkeypatch.setenv("MPA_TIMING", "1")
    monkeypatch.setenv("MPA_GPU_DPPLAN", "1")
    capfd.readouterr()
    texts = mpa.map_batches(ctx, idx, mo, batches, 4)
    err = capfd.readouterr().err
    idx.close()
    assert b"".join(texts) == ref
    assert err.count(DEVICE_NOTE + " ") >= 3, [l for l in err.split("\n") if "declined" in l][:6]
