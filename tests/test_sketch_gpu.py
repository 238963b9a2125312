"""The sketch stage on the device (MPA_GPU_SKETCH=1: k_sketch_count, k_offsets2, k_sketch_emit in sketch_exec.hip) against the host
stage it mirrors (stage_seeds, pinned to the oracle's sketch and a restated cut-off by tests/test_sketch_host.py).  Every comparison
is exact: the kept seeds of every query as (position, bucket, occurrences) in job order, the offsets, the cut-off in force; and,
through the whole path, the reference's bytes.  mpa_dbg_seed_jobs also checks the kb_off / dst / qid fields of the device's jobs
against ki[] and the prefix arrays, so a pass here covers everything k_seed_sift reads."""
import os
import numpy as np
import pytest
import miniprot_amd as mpa
import golden
import seedopts
import sketchcases as sc
from hostpipe import map_batch_gpu
from test_seed_options_gpu import HOST_SEEDING, SEED_NOTE, _check_stage_notes

pytestmark = pytest.mark.gpu
SKETCH_NOTE = "sketch on the GPU"


@pytest.fixture(scope="module")
def ctx():
    c = mpa.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def genome(tmp_path_factory):
    contigs, _ = seedopts.tandem_genome(5, 35)
    return seedopts.write_genome(tmp_path_factory.mktemp("sketch"), contigs)


def _same_jobs(host, dev, what):
    _, h_off, h_t, h_mo = host
    _, d_off, d_t, d_mo = dev
    assert np.array_equal(h_off, d_off), (what, "offsets")
    assert np.array_equal(h_mo, d_mo), (what, "cut-offs", np.flatnonzero(h_mo != d_mo)[:5])
    assert np.array_equal(h_t, d_t), (what, "triples")


@pytest.mark.parametrize("point", seedopts.INDEX_POINTS, ids=seedopts.index_name)
def test_device_seed_jobs_equal_host_seed_jobs(ctx, genome, point):
    """the grid and the branch queries of tests/test_sketch_host.py: same triples, offsets and cut-offs, and NO query handed to the
    host -- every protein here is at most 8 192 residues, so an implementation cannot pass by handing everything back"""
    _, _, kmer, _ = point
    _, seqs = sc.all_queries(kmer)
    assert max(len(s) for s in seqs) <= 8192
    idx = mpa.Index.read_fasta(genome, point)
    assert idx.build_kmers(sc.NCPU) == "host"
    idx.to_device(ctx)
    q = mpa.Queries(seqs)
    for max_occ in sc.MAX_OCC:
        mo = sc.mapopt(max_occ)
        host = sc.seed_jobs(None, idx, mo, q)
        dev = sc.seed_jobs(ctx, idx, mo, q)
        _same_jobs(host, dev, (point, max_occ))
        assert dev[0] == 0, ("queries handed to the host", dev[0])
        assert host[1][-1] > 300
    idx.close()


def test_a_protein_of_40000_residues_with_every_kmer_kept(ctx, genome):
    """-M0 (every k-mer is a seed) and one protein of 40 000 residues among the others: results equal whatever the kernel's capacity
    (this implementation has none -- the counts stay in global memory -- so nothing is handed back; were it, the lazily built
    host seeds would be what is compared)"""
    point = (6, 20, 5, 0)
    _, seqs = sc.all_queries(point[2])
    rng = np.random.default_rng(11)
    long = b"".join(seqs[int(k)] for k in rng.integers(0, 50, 400))[:40000]
    assert len(long) == 40000
    seqs = seqs[:20] + [long] + seqs[20:]
    idx = mpa.Index.read_fasta(genome, point)
    assert idx.build_kmers(sc.NCPU) == "host"
    idx.to_device(ctx)
    q = mpa.Queries(seqs)
    for max_occ in sc.MAX_OCC:
        mo = sc.mapopt(max_occ)
        host = sc.seed_jobs(None, idx, mo, q)
        dev = sc.seed_jobs(ctx, idx, mo, q)
        _same_jobs(host, dev, max_occ)
        assert dev[0] <= 1                                       # (the long one at most)
    assert host[1][21] - host[1][20] > 10000                     # the long protein does keep seeds
    idx.close()


def test_restored_index_and_device_built_index_give_the_same_jobs(ctx, genome, tmp_path):
    """ki[] is uploaded byte-wise from whatever holds it: owned memory of a host build, a (possibly misaligned) view into a mapped
    .mpi, or the table dev_index_build brought back -- the same jobs from all three"""
    point = seedopts.INDEX_POINTS[0]
    _, seqs = sc.all_queries(point[2])
    q, mo = mpa.Queries(seqs), sc.mapopt(None)
    a = mpa.Index.read_fasta(genome, point)
    assert a.build_kmers(sc.NCPU) == "host"
    want = sc.seed_jobs(None, a, mo, q)
    mpi = str(tmp_path / "g.mpi")
    a.dump(mpi)
    a.close()
    r = mpa.Index.restore(mpi)
    r.to_device(ctx)
    dev = sc.seed_jobs(ctx, r, mo, q)
    _same_jobs(want, dev, "restored .mpi")
    assert dev[0] == 0
    # the sketch alone has brought ki up next to the genome (2^23 buckets of 8 bytes at -k6 -M1; the packed genome is 1.5 MB); it is
    # counted in mpa_device_bytes() and goes when the index does
    held = mpa.Context.device_bytes()
    r.close()
    assert (1 << 26) <= held - mpa.Context.device_bytes() < (1 << 26) + (4 << 20)
    os.remove(mpi)
    b = mpa.Index.read_fasta(genome, point)
    assert b.build_kmers(4, ctx) == "gpu"
    b.to_device(ctx)
    dev = sc.seed_jobs(ctx, b, mo, q)
    _same_jobs(want, dev, "device-built index")
    assert dev[0] == 0
    b.close()


@pytest.mark.parametrize("case", golden.OPTION_CASES, ids=[c["name"] for c in golden.OPTION_CASES])
def test_option_cases_paf_identical_with_the_device_sketch(ctx, case, tmp_path, monkeypatch, capfd):
    """The whole path at golden.OPTION_CASES with the device sketch and every other optional device stage forced on: the reference's
    bytes from the blocking call and from a 3-batch stream; the sketch ran on the device exactly where device seeding did, and
    nothing declined."""
    monkeypatch.setenv("MPA_GPU_SKETCH", "1")
    monkeypatch.setenv("MPA_GPU_SEED", "1")
    monkeypatch.setenv("MPA_GPU_REFINE", "1")
    monkeypatch.setenv("MPA_TIMING", "1")
    contigs, prots, names = golden.synth_inputs(case)
    idx = mpa.Index.read_fasta(seedopts.write_genome(tmp_path, contigs), case["idx"])
    assert idx.build_kmers(4, ctx) == "gpu"
    idx.to_device(ctx)
    mo = golden.mapopt_for(case)
    ref = open(golden.path(case["name"] + ".ref.paf"), "rb").read()
    n = len(prots)
    runs = [("blocking call", lambda: map_batch_gpu(ctx, idx, mo, mpa.Queries(prots, names), 4)),
            ("stream", lambda: b"".join(mpa.map_batches(ctx, idx, mo, [mpa.Queries(prots[a:b], names[a:b]) for a, b in ((0, n // 3), (n // 3, 2 * n // 3), (2 * n // 3, n))], 4)))]
    for what, run in runs:
        capfd.readouterr()
        ours = run()
        notes = capfd.readouterr().err
        _check_stage_notes(case, notes, what)                        # (`declined` absent, seeding and refinement where they belong)
        assert (SKETCH_NOTE in notes) == (SEED_NOTE in notes) == (case["name"] not in HOST_SEEDING), what
        if SKETCH_NOTE in notes:
            assert "A1: seeds of all queries" not in notes, what     # the host stage did not run as well
        assert ours == ref, "%s: output differs from the reference for %s" % (what, case["name"])
    idx.close()


def test_under_the_anchor_threshold_the_host_seeds_from_lazily_built_seeds(ctx, monkeypatch, capfd):
    """MPA_GPU_SKETCH=1 with MPA_GPU_SEED unset on a small batch: the device sketch finds the batch under the anchor threshold, the
    host seeds it from seeds it builds when the anchor stage asks for them -- the bytes of the knob unset"""
    case = golden.OPTION_CASES[4]
    contigs, prots, names = golden.synth_inputs(case)
    idx = mpa.Index.from_nt4(contigs, ["chr1", "chr2"])
    assert idx.build_kmers(4, ctx) == "gpu"
    idx.to_device(ctx)
    mo = golden.mapopt_for(case)
    q = mpa.Queries(prots, names)
    monkeypatch.delenv("MPA_GPU_SEED", raising=False)
    monkeypatch.delenv("MPA_GPU_SKETCH", raising=False)
    monkeypatch.setenv("MPA_TIMING", "1")
    capfd.readouterr()
    plain = map_batch_gpu(ctx, idx, mo, q, 4)
    notes = capfd.readouterr().err
    assert SKETCH_NOTE not in notes and SEED_NOTE not in notes
    monkeypatch.setenv("MPA_GPU_SKETCH", "1")
    ours = map_batch_gpu(ctx, idx, mo, q, 4)
    notes = capfd.readouterr().err
    assert SKETCH_NOTE in notes and SEED_NOTE not in notes and "declined" not in notes
    assert ours == plain
    assert ours == open(golden.path(case["name"] + ".ref.paf"), "rb").read()
    streamed = b"".join(mpa.map_batches(ctx, idx, mo, [mpa.Queries(prots[:10], names[:10]), mpa.Queries(prots[10:], names[10:])], 4))
    assert streamed == plain
    idx.close()


def test_two_pipelines_on_one_device_with_the_device_sketch(monkeypatch):
    """mpa.map_batches_multi with two root contexts on device 0 and the knob on: every seeder context of both pipelines sketches
    against the ONE copy of ki[] the index holds for the device -- the reference's bytes"""
    monkeypatch.setenv("MPA_GPU_SKETCH", "1")
    monkeypatch.setenv("MPA_GPU_SEED", "1")
    case = golden.SYNTH_CASES[1]
    contigs, prots, names = golden.synth_inputs(case)
    idx = mpa.Index.from_nt4(contigs, ["chr%d" % (i + 1) for i in range(len(contigs))])
    mpa._check(mpa.lib().mpa_idx_build_kmers(idx.h, 2))
    n = len(prots)
    cuts = [0, n // 7, n // 7, n // 3, n // 2, n - 3, n]               # six uneven mini-batches, one of them empty
    batches = [mpa.Queries(prots[a:b], names[a:b]) for a, b in zip(cuts[:-1], cuts[1:])]
    c0, c1 = mpa.Context(0), mpa.Context(0)
    try:
        mo = golden.mapopt_for(case)
        idx.to_device(c0)
        multi = b"".join(mpa.map_batches_multi([c0, c1], idx, mo, batches, 4))
        assert golden.file_header(case) + multi == open(golden.path(case["name"] + ".ref.paf"), "rb").read()
    finally:
        c1.close()
        c0.close()
    idx.close()
