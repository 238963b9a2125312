"""MPA_GPU_REGIONS=1: where device seeding ran both chaining rounds, the main round ends in k_regions (region_kernels.hip; the code is
regions_core.h, which tests/test_regions_cpu.py pins on the CPU) instead of k_chain_pack -- the selected regions of every query and
their refinement limits come back, the main chains' anchors stay on the device.  What the stage leaves is visible in MPA_REGIONS_DUMP
(tests/regionsdump.py) and in the text: both must equal the run with the knob unset on the same context, byte for byte, and the text
the reference's bytes.  Every run here has MPA_GPU_SEED=1, so that the device chains exist."""
import pytest
import miniprot_amd as mpa
import golden
import regioncases
import regionsdump
from test_seed_gpu import main_chains

pytestmark = pytest.mark.gpu

GPU_NOTE = "regions on the GPU"
SEED_NOTE = "seeding on the GPU"
NO_ANCHORS = "anchors downloaded 0 B"
# (case, extra knobs): the pre-chain route; the direct route (no pre-chain: MPA_GPU_SEED_NOPRE); the device sketch in front
CASES = [("syn_a", {}), ("syn_b", {}), ("syn_c", {}), ("syn_d", {}), ("syn_i", {}), ("opt_b12", {}), ("opt_k5M0b6L20", {}),
         ("syn_h", {"MPA_GPU_SEED_NOPRE": "1"}), ("opt_noprechain", {"MPA_GPU_SEED_NOPRE": "1"}), ("syn_a", {"MPA_GPU_SKETCH": "1"})]


@pytest.fixture(scope="module")
def ctx():
    c = mpa.Context(0)
    yield c
    c.close()


@pytest.fixture(autouse=True)
def knobs(monkeypatch):
    monkeypatch.setenv("MPA_GPU_SEED", "1")
    monkeypatch.setenv("MPA_TIMING", "1")


def _run(ctx, idx, mo, q, knob, monkeypatch, capfd, path, n_threads=4):
    """one blocking batch with MPA_GPU_REGIONS = knob (None: unset): (text, dump, stderr)"""
    if knob is None:
        monkeypatch.delenv("MPA_GPU_REGIONS", raising=False)
    else:
        monkeypatch.setenv("MPA_GPU_REGIONS", knob)
    capfd.readouterr()
    res, dump = regioncases.with_dump(monkeypatch, path, lambda: mpa.map_batch(ctx, idx, mo, q, n_threads))
    err = capfd.readouterr().err
    return mpa.format_output(idx, mo, q, res)[0], dump, err


def _check_pair(host, dev):
    assert SEED_NOTE in host[2] and SEED_NOTE in dev[2], "the device did not seed"
    assert GPU_NOTE in dev[2], "MPA_GPU_REGIONS=1 did not run the regions on the device"
    assert dev[2].count(GPU_NOTE) == 1 and NO_ANCHORS in dev[2]
    assert "declined" not in dev[2], [l for l in dev[2].split("\n") if "declined" in l][:3]
    assert GPU_NOTE not in host[2] and "seed: regions" not in host[2]
    assert dev[1] == host[1], regionsdump.first_difference(dev[1], host[1])
    assert dev[0] == host[0]


@pytest.mark.parametrize("name,extra", CASES, ids=["%s%s" % (n, "".join("-" + k[4:].lower() for k in e)) for n, e in CASES])
def test_golden_cases(ctx, name, extra, tmp_path, monkeypatch, capfd):
    for k, v in extra.items():
        monkeypatch.setenv(k, v)
    idx, mo, q, ref = regioncases.case_inputs(name, tmp_path)
    idx.to_device(ctx)
    host = _run(ctx, idx, mo, q, None, monkeypatch, capfd, str(tmp_path / "host.dump"))
    dev = _run(ctx, idx, mo, q, "1", monkeypatch, capfd, str(tmp_path / "dev.dump"))
    idx.close()
    _check_pair(host, dev)
    assert dev[0] == ref, "text differs from the reference"
    parsed = regionsdump.parse(dev[1])
    assert [p[0] for p in parsed] == list(range(len(q.seqs))) and sum(len(p[2]) for p in parsed) >= len(q.seqs) // 2
    if "MPA_GPU_SKETCH" in extra:
        assert "sketch on the GPU" in dev[2]


def test_edge_genome(ctx, tmp_path, monkeypatch, capfd):
    """chains across strand and contig boundaries in both majority directions and 84 chains of which 79 share a score (the radix passes
    of the region order: runs of more than 64 equal keys), mapped with -N 100 --outn=100 -p 0.1"""
    contigs, prots, names, mo = regioncases.edge_genome()
    idx, q = regioncases.edge_index(contigs), mpa.Queries(prots, names)
    idx.to_device(ctx)
    host = _run(ctx, idx, mo, q, None, monkeypatch, capfd, str(tmp_path / "host.dump"))
    flags, most, ties = regioncases.edge_findings(host[1])
    assert flags == {1, 2}, "the split flag does not occur in both directions on the host path"
    assert most > 64 and ties > 64, (most, ties)
    dev = _run(ctx, idx, mo, q, "1", monkeypatch, capfd, str(tmp_path / "dev.dump"))
    idx.close()
    _check_pair(host, dev)
    assert dev[0] == open(golden.path(regioncases.EDGE_REF), "rb").read()


def test_stream_of_three_batches(ctx, tmp_path, monkeypatch, capfd):
    """mpa_map_batches(): the seeders end their main round in k_regions, the planners take the records -- same bytes, one note per batch"""
    idx, mo, q, ref = regioncases.case_inputs("syn_b", tmp_path)
    idx.to_device(ctx)
    n = len(q.seqs)
    batches = [mpa.Queries(q.seqs[a:b], q.names[a:b]) for a, b in ((0, n // 3), (n // 3, 2 * n // 3), (2 * n // 3, n))]
    monkeypatch.setenv("MPA_GPU_REGIONS", "1")
    capfd.readouterr()
    texts = mpa.map_batches(ctx, idx, mo, batches, 4)
    err = capfd.readouterr().err
    idx.close()
    assert b"".join(texts) == ref
    assert err.count(GPU_NOTE) == 3 and err.count(NO_ANCHORS) == 3 and "declined" not in err


def test_queries_handed_back_take_the_host_regions(ctx, tmp_path, monkeypatch, capfd):
    """A batch of which the sift hands one query to the host: a protein of 140 copies of an 80-residue unit whose coding sequence
    fills one 256-base block of the genome, so that this block holds more anchors of the query (140 per kept k-mer of the unit) than
    a sift range takes (4 096) however small the segments (MPA_SIFT_SEG=256) and the ranges get.  That query takes the host's regions
    from the host's chains, the others the device's records.  Same dump, same bytes (-A: chains only, the long query is not aligned)."""
    import numpy as np
    import gen_synth
    monkeypatch.setenv("MPA_SIFT_SEG", "256")
    contigs, prots, names = gen_synth.generate(1500000, 2, 24, 91)
    rng = np.random.default_rng(77)
    unit = regioncases._protein(rng, 80)
    contigs[0][256 * 1000:256 * 1000 + 240] = regioncases._coding(unit)
    prots, names = [bytes(p) for p in prots] + [unit * 140], list(names) + ["repeat"]
    idx = mpa.Index.from_nt4(contigs, ["chr1", "chr2"])
    mpa._check(mpa.lib().mpa_idx_build_kmers(idx.h, 4))
    idx.to_device(ctx)
    q = mpa.Queries(prots, names)
    mo = golden.apply_flags(mpa.default_mapopt(), ["-A", "-u"])
    monkeypatch.delenv("MPA_GPU_REGIONS", raising=False)
    n_back = main_chains(ctx, idx, mo, q, 4)[0]
    assert 0 < n_back < len(q.seqs) // 2, "the batch does not mix queries handed back with queries the device chained: %d of %d" % (n_back, len(q.seqs))
    host = _run(ctx, idx, mo, q, None, monkeypatch, capfd, str(tmp_path / "host.dump"))
    dev = _run(ctx, idx, mo, q, "1", monkeypatch, capfd, str(tmp_path / "dev.dump"))
    idx.close()
    _check_pair(host, dev)
    last = regionsdump.parse(host[1])[-1]
    assert last[1] >= 1 and len(last[2]) >= 1, "the query handed back has no regions"
    assert host[0].count(b"\n") >= len(q.seqs) // 2
