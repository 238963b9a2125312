"""MPA_GPU_PLANS=1: where the whole refinement ran on the device (dev_refine_chains), the call ends in k_plans (plan_kernels.hip; the
code is plans_core.h, which tests/test_plans_cpu.py pins on the CPU) instead of k_chain_pack -- the regions, alignment plans, round-1
DP tasks and gap segments of every query come back, the refinement chains' anchors stay on the device.  What the step leaves is
visible in MPA_PLANS_DUMP (tests/plansdump.py) and in the text: both must equal the run with the knob unset on the same context, byte
for byte, and the text the reference's bytes.  Every run here has MPA_GPU_SEED=1 and MPA_GPU_REFINE=1, so that the device chains exist."""
import pytest
import miniprot_amd as mpa
import golden
import longprot
import regioncases
import planscases
import plansdump
from planscases import DEVICE_NOTE, NO_ANCHORS

pytestmark = pytest.mark.gpu

REFINE_NOTE = "refinement on the GPU"
WAIT_NOTE = "refine: plans + pack (wait)"


@pytest.fixture(scope="module")
def ctx():
    c = mpa.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def knobs(monkeypatch):
    monkeypatch.setenv("MPA_GPU_SEED", "1")
    monkeypatch.setenv("MPA_GPU_REFINE", "1")
    monkeypatch.setenv("MPA_TIMING", "1")


def _run(ctx, idx, mo, q, knob, monkeypatch, capfd, path, n_threads=4):
    """one blocking batch with MPA_GPU_PLANS = knob (None: unset): (text, dump, stderr)"""
    if knob is None:
        monkeypatch.delenv("MPA_GPU_PLANS", raising=False)
    else:
        monkeypatch.setenv("MPA_GPU_PLANS", knob)
    capfd.readouterr()
    res, dump = planscases.with_dump(monkeypatch, path, lambda: mpa.map_batch(ctx, idx, mo, q, n_threads))
    err = capfd.readouterr().err
    return mpa.format_output(idx, mo, q, res)[0], dump, err


def _check_pair(host, dev):
    assert REFINE_NOTE in host[2] and REFINE_NOTE in dev[2], "the device did not refine"
    assert DEVICE_NOTE in dev[2], "MPA_GPU_PLANS=1 did not run the plans on the device"
    assert dev[2].count(DEVICE_NOTE) == 1 and NO_ANCHORS in dev[2] and WAIT_NOTE in dev[2]
    assert "declined" not in dev[2], [l for l in dev[2].split("\n") if "declined" in l][:3]
    assert DEVICE_NOTE not in host[2] and WAIT_NOTE not in host[2]
    assert dev[1] == host[1], plansdump.first_difference(dev[1], host[1])
    assert dev[0] == host[0]


@pytest.mark.parametrize("name", planscases.CASES)
def test_golden_cases(ctx, name, tmp_path, monkeypatch, capfd):
    idx, mo, q, ref = planscases.case_inputs(name, tmp_path)
    idx.to_device(ctx)
    host = _run(ctx, idx, mo, q, None, monkeypatch, capfd, str(tmp_path / "host.dump"))
    dev = _run(ctx, idx, mo, q, "1", monkeypatch, capfd, str(tmp_path / "dev.dump"))
    idx.close()
    _check_pair(host, dev)
    assert dev[0] == ref, "text differs from the reference"
    n_q, n_reg, n_plan, n_task, n_seg, n_short, _ = planscases.totals(dev[1])
    assert n_q == len(q.seqs) and n_reg >= len(q.seqs) // 2
    if name == "syn_i":
        assert n_plan == 0 and n_task == 0
    else:
        assert n_plan >= len(q.seqs) // 2 and n_task > n_plan and n_seg > n_short > 0


def test_long_proteins(ctx, tmp_path, monkeypatch, capfd):
    """tests/longprot.py: queries whose k-mer map lives in HBM, refinement chains of thousands of anchors"""
    c = longprot.case()
    idx = mpa.Index.from_nt4(c["contigs"], ["chr1"])
    mpa._check(mpa.lib().mpa_idx_build_kmers(idx.h, 4))
    idx.to_device(ctx)
    q, mo = mpa.Queries(c["prots"], c["names"]), longprot.mapopt()
    monkeypatch.delenv("MPA_REFINE_GMAP_MIN", raising=False)
    host = _run(ctx, idx, mo, q, None, monkeypatch, capfd, str(tmp_path / "host.dump"))
    dev = _run(ctx, idx, mo, q, "1", monkeypatch, capfd, str(tmp_path / "dev.dump"))
    idx.close()
    _check_pair(host, dev)
    assert "refine: global-map class" in dev[2]
    assert dev[0] == open(golden.path("long_u.ref.paf"), "rb").read()
    assert max(int(e[2]["n_gap"].max()) for e in plansdump.parse(dev[1]) if len(e[2])) > 1000


def test_all_device_stages_together(ctx, tmp_path, monkeypatch, capfd):
    """MPA_GPU_REGIONS, MPA_GPU_STATS and MPA_GPU_SKETCH next to the new knob: same bytes, every stage's note"""
    idx, mo, q, ref = planscases.case_inputs("syn_b", tmp_path)
    idx.to_device(ctx)
    host = _run(ctx, idx, mo, q, None, monkeypatch, capfd, str(tmp_path / "host.dump"))
    for k in ("MPA_GPU_REGIONS", "MPA_GPU_STATS", "MPA_GPU_SKETCH"):
        monkeypatch.setenv(k, "1")
    dev = _run(ctx, idx, mo, q, "1", monkeypatch, capfd, str(tmp_path / "dev.dump"))
    idx.close()
    _check_pair(host, dev)
    assert dev[0] == ref
    for note in ("regions on the GPU", "alignment statistics on the GPU", "sketch on the GPU"):
        assert note in dev[2] and note not in host[2], note


def test_edge_genome(ctx, tmp_path, monkeypatch, capfd):
    """regions on reverse strands and at contig ends, 84 regions of one query of which most share a score (the radix passes of the
    second region order), mapped with -N 100 --outn=100 -p 0.1"""
    contigs, prots, names, mo = regioncases.edge_genome()
    idx, q = regioncases.edge_index(contigs), mpa.Queries(prots, names)
    idx.to_device(ctx)
    host = _run(ctx, idx, mo, q, None, monkeypatch, capfd, str(tmp_path / "host.dump"))
    assert max(len(e[1]) for e in plansdump.parse(host[1])) > 64
    dev = _run(ctx, idx, mo, q, "1", monkeypatch, capfd, str(tmp_path / "dev.dump"))
    idx.close()
    _check_pair(host, dev)
    assert dev[0] == open(golden.path(regioncases.EDGE_REF), "rb").read()


def test_stream_of_three_batches(ctx, tmp_path, monkeypatch, capfd):
    """mpa_map_batches(): the planners end their refinement call in k_plans and take the records -- same bytes, one note per batch"""
    idx, mo, q, ref = planscases.case_inputs("syn_b", tmp_path)
    idx.to_device(ctx)
    n = len(q.seqs)
    batches = [mpa.Queries(q.seqs[a:b], q.names[a:b]) for a, b in ((0, n // 3), (n // 3, 2 * n // 3), (2 * n // 3, n))]
    monkeypatch.setenv("MPA_GPU_PLANS", "1")
    capfd.readouterr()
    texts = mpa.map_batches(ctx, idx, mo, batches, 4)
    err = capfd.readouterr().err
    idx.close()
    assert b"".join(texts) == ref
    assert err.count(DEVICE_NOTE) == 3 and err.count(NO_ANCHORS) == 3 and "declined" not in err
