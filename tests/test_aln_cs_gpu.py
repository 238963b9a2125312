"""MPA_GPU_CS=1: the body of every aligned region's cs:Z: string behind the last DP round on the device (k_aln_cs, stats_kernels.hip; the
code is aln_cs_core.h, which tests/test_aln_cs_cpu.py pins on the CPU).  The strings travel in the result and the formatter pastes them
in: the text must equal the run with the knob unset on the same context and the reference's bytes, the format note must say that none
was built on the host, and MPA_CS_DUMP must hold the same bodies as the unset run, with source 2 against 0."""
import itertools
import os
import subprocess
import pytest
import miniprot_amd as mpa
import refbind
import golden
import gen_synth
import alnstats
import csdump
from csdump import format_counts

pytestmark = pytest.mark.gpu

GPU_NOTE = "cs strings on the GPU"
CASES = ["syn_a", "syn_b", "syn_c", "syn_e", "syn_h", "syn_n", "long_u"]
ALL_KNOBS = {"MPA_GPU_SEED": "1", "MPA_GPU_SKETCH": "1", "MPA_GPU_REGIONS": "1", "MPA_GPU_REFINE": "1", "MPA_GPU_PLANS": "1", "MPA_GPU_STATS": "1"}


@pytest.fixture(scope="module")
def ctx():
    c = mpa.Context(0)
    yield c
    c.close()


def _run(ctx, idx, mo, q, knob, capfd, tmp, n_threads=4, more=None):
    """one blocking batch with MPA_GPU_CS = knob (None: unset) and the knobs of `more`: (text, parsed dump, stderr)"""
    env = {"MPA_GPU_CS": knob, "MPA_TIMING": "1", "MPA_CS_DUMP": str(tmp / ("cs_%d.dump" % next(_serial)))}
    env.update(more or {})
    keep = {k: os.environ.get(k) for k in env}
    for k, v in env.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = v
    try:
        capfd.readouterr()
        res = mpa.map_batch(ctx, idx, mo, q, n_threads)
        os.environ.pop("MPA_CS_DUMP")
        text = mpa.format_output(idx, mo, q, res)[0]
        err = capfd.readouterr().err
    finally:
        for k, v in keep.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    dump = csdump.parse(csdump.read(env["MPA_CS_DUMP"])) if os.path.exists(env["MPA_CS_DUMP"]) else []
    return text, dump, err


_done = {}
_serial = itertools.count()


def _case(ctx, name, capfd, tmp_path_factory, more=None):
    """a golden case mapped once with the knob unset and once with MPA_GPU_CS=1 (both with the knobs of `more`), shared by the tests below"""
    key = (name, tuple(sorted((more or {}).items())))
    if key not in _done:
        tmp = tmp_path_factory.mktemp(name)
        idx, mo, q, ref = alnstats.case_inputs(name, tmp)
        idx.to_device(ctx)
        host = _run(ctx, idx, mo, q, None, capfd, tmp, more=more)
        dev = _run(ctx, idx, mo, q, "1", capfd, tmp, more=more)
        idx.close()
        _done[key] = (host, dev, ref)
    return _done[key]


def _check(host, dev, ref):
    assert GPU_NOTE in dev[2], "MPA_GPU_CS=1 did not run the cs strings on the device"
    declined = [l for l in dev[2].split("\n") if "declined" in l and ("cs strings" in l or "statistics" in l)]
    assert not declined, declined[:3]
    assert "cs strings" not in host[2]
    if ref is not None:
        assert dev[0] == ref, "text differs from the reference"
        assert host[0] == ref
    assert dev[0] == host[0]
    n_cs = host[0].count(b"cs:Z:")
    assert n_cs > 0 and format_counts(dev[2]) == (n_cs, 0) and format_counts(host[2]) == (0, n_cs)
    assert len(host[1]) >= n_cs
    assert csdump.first_difference(dev[1], host[1], 2, 0) is None, csdump.first_difference(dev[1], host[1], 2, 0)


@pytest.mark.parametrize("name", CASES)
def test_golden_cases(ctx, name, capfd, tmp_path_factory):
    _check(*_case(ctx, name, capfd, tmp_path_factory))


@pytest.mark.parametrize("name", ["syn_b", "long_u"])
def test_with_the_statistics_on_the_device_too(ctx, name, capfd, tmp_path_factory):
    """MPA_GPU_STATS=1 as well: the two kernels share one upload and one wait -- both notes, the same bytes"""
    host, dev, ref = _case(ctx, name, capfd, tmp_path_factory, {"MPA_GPU_STATS": "1"})
    _check(host, dev, ref)
    assert "alignment statistics on the GPU" in dev[2] and "alignment statistics on the GPU" in host[2]


def test_with_every_device_knob(ctx, capfd, tmp_path_factory):
    host, dev, ref = _case(ctx, "syn_b", capfd, tmp_path_factory, ALL_KNOBS)
    _check(host, dev, ref)


def test_stream_of_three_batches(ctx, capfd, monkeypatch):
    """mpa_map_batches(): the strings are built on the lanes' contexts -- same bytes, the note of every batch that aligned anything"""
    idx, mo, q, ref = alnstats.case_inputs("syn_b")
    idx.to_device(ctx)
    n = len(q.seqs)
    batches = [mpa.Queries(q.seqs[a:b], q.names[a:b]) for a, b in ((0, n // 3), (n // 3, 2 * n // 3), (2 * n // 3, n))]
    monkeypatch.setenv("MPA_TIMING", "1")
    monkeypatch.setenv("MPA_GPU_CS", "1")
    capfd.readouterr()
    texts = mpa.map_batches(ctx, idx, mo, batches, 4)
    err = capfd.readouterr().err
    assert b"".join(texts) == ref
    assert err.count(GPU_NOTE) == 3 and "cs strings declined" not in err
    assert format_counts(err) == (ref.count(b"cs:Z:"), 0)
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
        tmp = tmp_path_factory.mktemp("edge%d%d" % (d, e))
        idx, mo, q = _edge_index(d, e)
        idx.to_device(ctx)
        host = _run(ctx, idx, mo, q, None, capfd, tmp)
        dev = _run(ctx, idx, mo, q, "1", capfd, tmp)
        ref = None
        if os.path.exists(refbind.REF_BIN):
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
    """contigs that begin d bases before their first gene and end e bases behind their last, 5 % N: ambiguous codons and bases, strings
    that start on a contig's first base and end on its last -- dump and text against the host walk"""
    host, dev, _, n = _edge(ctx, d, e, capfd, tmp_path_factory)
    assert len(host[1]) >= n // 2
    _check(host, dev, None)


@pytest.mark.parametrize("d", [0, 1, 2, 3])
@pytest.mark.parametrize("e", [0, 1, 2, 3])
def test_edge_genome_text_equals_the_live_reference(ctx, d, e, capfd, tmp_path_factory):
    if not os.path.exists(refbind.REF_BIN):
        pytest.skip("oracle/_ref/miniprot not present")
    _, dev, ref, n = _edge(ctx, d, e, capfd, tmp_path_factory)
    assert dev[0] == ref and ref.count(b"\n") >= n // 2


def test_planted_ambiguous_bases(ctx, capfd, tmp_path):
    """neither the golden cases nor the edge genome put an N under an alignment; csdump.planted_n_genome() does: eight codons with an
    ambiguous base print as mismatches with an 'n' -- device against host and, where present, the live reference"""
    contigs, prots, names = csdump.planted_n_genome()
    idx = mpa.Index.from_nt4(contigs, ["chr1"])
    mpa._check(mpa.lib().mpa_idx_build_kmers(idx.h, 4))
    mo = mpa.default_mapopt()
    mo.flag |= 4
    q = mpa.Queries(prots, names)
    idx.to_device(ctx)
    host = _run(ctx, idx, mo, q, None, capfd, tmp_path)
    dev = _run(ctx, idx, mo, q, "1", capfd, tmp_path)
    if os.path.exists(refbind.REF_BIN):
        mpi, faa = str(tmp_path / "g.mpi"), str(tmp_path / "p.fa")
        idx.dump(mpi)
        gen_synth.write_fasta_aa(faa, q.seqs, q.names)
        assert dev[0] == subprocess.run([refbind.REF_BIN, "-t4", "-u", mpi, faa], capture_output=True).stdout
    idx.close()
    _check(host, dev, None)
    assert csdump.kinds([b for _, b in dev[1]])["n"] == 8


# ---- options that print no cs string -------------------------------------------------------------------
@pytest.mark.parametrize("name", ["syn_g", "syn_f"])
def test_cases_that_print_no_cs_string_skip_the_step(name, capfd, tmp_path_factory):
    """--no-cs (syn_g) and --gtf (syn_f) with the knob set, on a fresh context: no note, no pool -- mpa_device_bytes() stays where the
    unset run left it -- and the reference's bytes"""
    c = mpa.Context(0)
    tmp = tmp_path_factory.mktemp(name)
    idx, mo, q, ref = alnstats.case_inputs(name, tmp)
    idx.to_device(c)
    t0, _, err0 = _run(c, idx, mo, q, None, capfd, tmp)
    b0 = mpa.Context.device_bytes()
    t1, _, err1 = _run(c, idx, mo, q, "1", capfd, tmp)
    assert mpa.Context.device_bytes() == b0
    assert "cs strings" not in err0 + err1 and format_counts(err1) == (0, 0)
    assert t0 == t1 == ref and b"cs:Z:" not in t1
    idx.close()
    c.close()


# ---- the knob unset -----------------------------------------------------------------------------------
def test_knob_unset_launches_nothing_and_holds_no_memory(capfd, tmp_path):
    """k_aln_cs has one launch site, which sizes its device pools first.  On a fresh context: runs with the knob unset (or 0) leave
    mpa_device_bytes() where it was and print no note; the first run with the knob set then grows it -- so the runs before it had
    allocated no pool, i.e. had not been there -- and going back to unset changes nothing again."""
    c = mpa.Context(0)
    idx = mpa.Index.from_fasta(golden.path("DPP3-hs.gen.fa.gz"))
    idx.to_device(c)
    from hostpipe import read_fasta
    names, seqs = read_fasta(golden.path("DPP3-mm.pep.fa.gz"))
    q, mo = mpa.Queries(seqs, names), mpa.default_mapopt()
    ref = open(golden.path("dpp3.ref.paf"), "rb").read()
    t0, _, err0 = _run(c, idx, mo, q, None, capfd, tmp_path, 2)
    b0 = mpa.Context.device_bytes()
    t1, _, err1 = _run(c, idx, mo, q, None, capfd, tmp_path, 2)
    t2, _, err2 = _run(c, idx, mo, q, "0", capfd, tmp_path, 2)
    assert mpa.Context.device_bytes() == b0
    assert "cs strings" not in err0 + err1 + err2
    assert format_counts(err2)[0] == 0
    t3, _, err3 = _run(c, idx, mo, q, "1", capfd, tmp_path, 2)
    b1 = mpa.Context.device_bytes()
    assert GPU_NOTE in err3 and b1 > b0 and format_counts(err3)[1] == 0
    t4, _, err4 = _run(c, idx, mo, q, None, capfd, tmp_path, 2)
    assert mpa.Context.device_bytes() == b1 and "cs strings" not in err4
    assert t0 == t1 == t2 == t3 == t4 == ref
    idx.close()
    c.close()
