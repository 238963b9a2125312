"""MPA_GPU_STATS=1: the statistics pass behind the last DP round -- dist_stop / dist_start, the CIGAR walk's counts and scores, the
exon and stop-codon features -- on the device (k_aln_stats, stats_kernels.hip; the code is aln_stats_core.h, which
tests/test_aln_stats_cpu.py pins on the CPU).  Everything it computes is visible in the result arrays and in the text: both must equal
the run with the knob unset on the same context, and the text the reference's bytes."""
import os
import subprocess
import pytest
import miniprot_amd as mpa
import refbind
import golden
import gen_synth
import alnstats

pytestmark = pytest.mark.gpu

GPU_NOTE = "alignment statistics on the GPU"
CASES = ["syn_a", "syn_b", "syn_c", "syn_e", "syn_h", "syn_n", "long_u"]


@pytest.fixture(scope="module")
def ctx():
    c = mpa.Context(0)
    yield c
    c.close()


def _run(ctx, idx, mo, q, knob, capfd, n_threads=4):
    """one blocking batch with MPA_GPU_STATS = knob (None: unset): (text, result arrays, stderr)"""
    keep = {k: os.environ.get(k) for k in ("MPA_GPU_STATS", "MPA_TIMING")}
    os.environ["MPA_TIMING"] = "1"
    if knob is None:
        os.environ.pop("MPA_GPU_STATS", None)
    else:
        os.environ["MPA_GPU_STATS"] = knob
    try:
        capfd.readouterr()
        res = mpa.map_batch(ctx, idx, mo, q, n_threads)
        err = capfd.readouterr().err
    finally:
        for k, v in keep.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return mpa.format_output(idx, mo, q, res)[0], alnstats.result_arrays(res), err


_done = {}


def _case(ctx, name, capfd, tmp_path_factory):
    """a golden case mapped once with the knob unset and once with MPA_GPU_STATS=1, shared by the tests below"""
    if name not in _done:
        idx, mo, q, ref = alnstats.case_inputs(name, tmp_path_factory.mktemp(name))
        idx.to_device(ctx)
        host = _run(ctx, idx, mo, q, None, capfd)
        dev = _run(ctx, idx, mo, q, "1", capfd)
        idx.close()
        _done[name] = (host, dev, ref)
    return _done[name]


@pytest.mark.parametrize("name", CASES)
def test_golden_cases(ctx, name, capfd, tmp_path_factory):
    host, dev, ref = _case(ctx, name, capfd, tmp_path_factory)
    assert GPU_NOTE in dev[2], "MPA_GPU_STATS=1 did not run the statistics on the device"
    assert "declined" not in dev[2], [l for l in dev[2].split("\n") if "declined" in l][:3]
    assert "alignment statistics" not in host[2]
    assert dev[0] == ref, "text differs from the reference"
    assert host[0] == ref
    assert len(host[1][0]) > 0 and len(host[1][1]) > 0
    assert alnstats.first_difference(dev[1], host[1]) is None, alnstats.first_difference(dev[1], host[1])


def test_cases_cover_what_the_walk_distinguishes(ctx, capfd, tmp_path_factory):
    """over the union of the golden cases the host results hold every operation kind, an in-frame stop, a reverse-strand hit and a
    stop-codon feature; long_u holds a CIGAR of more than 64 words and an M run of more than 64 codons"""
    ops, flags = set(), {"n_stop": False, "reverse": False, "stop_feature": False}
    for name in CASES:
        c = alnstats.coverage(_case(ctx, name, capfd, tmp_path_factory)[0][1])
        ops |= c["ops"]
        for k in flags:
            flags[k] = flags[k] or c[k]
    assert ops == set("MIDNUVFG"), sorted(ops)
    assert all(flags.values()), flags
    hits, _, cigars = _case(ctx, "long_u", capfd, tmp_path_factory)[0][1]
    assert hits["n_cigar"].max() > 64
    assert ((cigars & 0xf) == 0).any() and (cigars[(cigars & 0xf) == 0] >> 4).max() > 64


def test_stream_of_three_batches(ctx, capfd, monkeypatch):
    """mpa_map_batches(): the statistics run on the lanes' contexts -- same bytes, the note of every batch that aligned anything"""
    idx, mo, q, ref = alnstats.case_inputs("syn_b")
    idx.to_device(ctx)
    n = len(q.seqs)
    batches = [mpa.Queries(q.seqs[a:b], q.names[a:b]) for a, b in ((0, n // 3), (n // 3, 2 * n // 3), (2 * n // 3, n))]
    monkeypatch.setenv("MPA_TIMING", "1")
    monkeypatch.setenv("MPA_GPU_STATS", "1")
    capfd.readouterr()
    texts = mpa.map_batches(ctx, idx, mo, batches, 4)
    err = capfd.readouterr().err
    assert b"".join(texts) == ref
    assert err.count(GPU_NOTE) == 3 and "declined" not in err
    idx.close()


# ---- the edge genome ---------------------------------------------------------------------------------
def _edge_index(d, e):
    contigs, prots, names = alnstats.edge_genome(d, e)
    idx = mpa.Index.from_nt4(contigs, ["chr%d" % (i + 1) for i in range(len(contigs))])
    mpa._check(mpa.lib().mpa_idx_build_kmers(idx.h, 4))
    mo = mpa.default_mapopt()
    mo.flag |= 4
    return idx, mo, mpa.Queries(prots, names)


_edge_done = {}


def _edge(ctx, d, e, capfd, tmp_path_factory):
    """the edge genome of (d, e) mapped with the knob unset and set, and by the reference where its binary is present: once per pair"""
    if (d, e) not in _edge_done:
        idx, mo, q = _edge_index(d, e)
        idx.to_device(ctx)
        host = _run(ctx, idx, mo, q, None, capfd)
        dev = _run(ctx, idx, mo, q, "1", capfd)
        ref = None
        if os.path.exists(refbind.REF_BIN):
            tmp = tmp_path_factory.mktemp("edge%d%d" % (d, e))
            mpi, faa = str(tmp / "g.mpi"), str(tmp / "p.fa")
            idx.dump(mpi)
            gen_synth.write_fasta_aa(faa, q.seqs, q.names)
            ref = subprocess.run([refbind.REF_BIN, "-t4", "-u", mpi, faa], capture_output=True).stdout
        idx.close()
        _edge_done[(d, e)] = (host, dev, ref, len(q.seqs))
    return _edge_done[(d, e)]


@pytest.mark.parametrize("d", [0, 1, 2, 3])
@pytest.mark.parametrize("e", [0, 1, 2, 3])
def test_edge_genome_device_equals_host(ctx, d, e, capfd, tmp_path_factory):
    """contigs that begin d bases before their first gene and end e bases behind their last: dist_start at the window's first codon,
    dist_stop at the contig end, '.' donors and acceptors, ambiguous codons -- field by field against the host walk"""
    host, dev, _, n = _edge(ctx, d, e, capfd, tmp_path_factory)
    assert GPU_NOTE in dev[2] and "declined" not in dev[2]
    assert len(host[1][0]) >= n // 2
    assert alnstats.first_difference(dev[1], host[1]) is None, alnstats.first_difference(dev[1], host[1])
    assert dev[0] == host[0]


@pytest.mark.parametrize("d", [0, 1, 2, 3])
@pytest.mark.parametrize("e", [0, 1, 2, 3])
def test_edge_genome_text_equals_the_live_reference(ctx, d, e, capfd, tmp_path_factory):
    if not os.path.exists(refbind.REF_BIN):
        pytest.skip("oracle/_ref/miniprot not present")
    _, dev, ref, n = _edge(ctx, d, e, capfd, tmp_path_factory)
    assert dev[0] == ref and ref.count(b"\n") >= n // 2


def test_edge_genome_reaches_the_edges(ctx, capfd, tmp_path_factory):
    """the d = e = 0 genome does put an alignment on a contig's first base, and stop-codon features, in-frame stops and both strands are
    among its hits (or the cases above would test less than they say)"""
    hits, feats, _ = _edge(ctx, 0, 0, capfd, tmp_path_factory)[0][1]
    assert ((hits["has_aln"] != 0) & (hits["vs"] == 0)).any(), hits["vs"].min()
    c = alnstats.coverage((hits, feats, _))
    assert c["stop_feature"] and c["reverse"] and c["n_stop"], c


# ---- the knob unset -----------------------------------------------------------------------------------
def test_knob_unset_launches_nothing_and_holds_no_memory(capfd):
    """k_aln_stats has one launch site, dev_aln_walks(), which sizes its two device pools first.  On a fresh context: runs with the knob
    unset (or 0) leave mpa_device_bytes() where it was and print no note; the first run with the knob set then grows it -- so the runs
    before it had allocated no pool, i.e. had not been there -- and going back to unset changes nothing again."""
    c = mpa.Context(0)
    idx = mpa.Index.from_fasta(golden.path("DPP3-hs.gen.fa.gz"))
    idx.to_device(c)
    from hostpipe import read_fasta
    names, seqs = read_fasta(golden.path("DPP3-mm.pep.fa.gz"))
    q, mo = mpa.Queries(seqs, names), mpa.default_mapopt()
    ref = open(golden.path("dpp3.ref.paf"), "rb").read()
    t0, _, err0 = _run(c, idx, mo, q, None, capfd, 2)
    b0 = mpa.Context.device_bytes()
    t1, _, err1 = _run(c, idx, mo, q, None, capfd, 2)
    t2, _, err2 = _run(c, idx, mo, q, "0", capfd, 2)
    assert mpa.Context.device_bytes() == b0
    assert "alignment statistics" not in err0 + err1 + err2
    t3, _, err3 = _run(c, idx, mo, q, "1", capfd, 2)
    b1 = mpa.Context.device_bytes()
    assert GPU_NOTE in err3 and b1 > b0
    t4, _, err4 = _run(c, idx, mo, q, None, capfd, 2)
    assert mpa.Context.device_bytes() == b1 and "alignment statistics" not in err4
    assert t0 == t1 == t2 == t3 == t4 == ref
    idx.close()
    c.close()
