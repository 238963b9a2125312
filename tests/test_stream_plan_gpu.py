"""The stream plan on the device (miniprot_amd/csrc/stream_plan.h): a stream of six mini-batches of a small synthetic
genome with the plan on, with MPA_STREAM_PLAN=0 (the legacy layout) and through the blocking mpa_map_batch give the same bytes, and the
plan in force on the context (mpa_dbg_stream_plan) is the module's plan for the hardware queues of this process.  No timing here: what
the layouts do to the stream's throughput is profiles/hw_queues_ab.txt."""
import os

import pytest

import miniprot_amd as mpa
import golden
from hostpipe import map_batch_gpu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = mpa.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def work(ctx):
    case = [c for c in golden.SYNTH_CASES if c["name"] == "syn_b"][0]
    contigs, prots, names = golden.synth_inputs(case)
    idx = mpa.Index.from_nt4(contigs, ["chr%d" % (i + 1) for i in range(len(contigs))])
    mpa._check(mpa.lib().mpa_idx_build_kmers(idx.h, 4))
    idx.to_device(ctx)
    mo = golden.mapopt_for(case)
    n = len(prots)
    cuts = [0, n // 6, n // 3, n // 3, n // 2, (3 * n) // 4, n]        # six mini-batches, one of them empty
    batches = [mpa.Queries(prots[a:b], names[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    blocking = map_batch_gpu(ctx, idx, mo, mpa.Queries(prots, names), 4)
    assert golden.file_header(case) + blocking == open(golden.path(case["name"] + ".ref.paf"), "rb").read()
    yield idx, mo, batches, blocking
    idx.close()


def _env_q():
    return int(os.environ.get("GPU_MAX_HW_QUEUES") or 4)


@pytest.mark.parametrize("knob", [None, "0", "A", "B", "C"])
def test_same_bytes_under_every_layout(ctx, work, monkeypatch, knob):
    """MPA_STREAM_PLAN unset (the default layout), 0 (legacy) and each candidate: the bytes of the blocking call, and the hook reports
    the module's plan for this process's hardware queues -- also when the layout changes between two streams on one context"""
    idx, mo, batches, blocking = work
    for name in ("MPA_STREAM_PLAN", "MPA_PRIO_MAIN", "MPA_PRIO_SEED", "MPA_DP_LANES", "MPA_SEEDERS", "MPA_PLANNERS"):
        monkeypatch.delenv(name, raising=False)
    if knob is not None:
        monkeypatch.setenv("MPA_STREAM_PLAN", knob)
    assert b"".join(mpa.map_batches(ctx, idx, mo, batches, 4)) == blocking
    plan = mpa.dbg_stream_plan(ctx)
    assert plan == mpa.dbg_stream_plan_for(_env_q(), 5, 3, 4, knob) and plan == mpa.dbg_stream_plan_for(0, 5, 3, 4, knob)
    assert plan["q"] == _env_q()
    if knob == "0" or _env_q() >= 12:
        assert plan["layout"] == "legacy"
    else:
        assert plan["layout"] == (knob or mpa.dbg_stream_plan_for(_env_q())["layout"]) and plan["n_streams"] == 12


def test_other_stage_counts_replace_the_siblings(ctx, work, monkeypatch):
    """eight lanes, four seeders, six planners after the default counts, and one of each after that: same bytes, the plan follows"""
    idx, mo, batches, blocking = work
    monkeypatch.delenv("MPA_STREAM_PLAN", raising=False)
    for lanes, seeders, planners in ((8, 4, 6), (1, 1, 1)):
        monkeypatch.setenv("MPA_DP_LANES", str(lanes))
        monkeypatch.setenv("MPA_SEEDERS", str(seeders))
        monkeypatch.setenv("MPA_PLANNERS", str(planners))
        assert b"".join(mpa.map_batches(ctx, idx, mo, batches, 4)) == blocking
        assert mpa.dbg_stream_plan(ctx) == mpa.dbg_stream_plan_for(_env_q(), lanes, seeders, planners)
