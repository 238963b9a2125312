"""MPA_GPU_ROWS=1: the residue rows of --aln / --trans of every aligned region behind the last DP round on the device (k_aln_rows,
stats_kernels.hip; the code is aln_rows_core.h, which tests/test_aln_rows_cpu.py pins on the CPU).  The rows travel in the result and
the formatter pastes them in: the text must equal the run with the knob unset on the same context, the golden file where one exists
and otherwise the live reference where its binary is present, and the format note must say that no row set was built on the host."""
import os
import subprocess
import pytest
import miniprot_amd as mpa
import refbind
import golden                                               # (puts tools/ on the path: gen_synth)
import gen_synth
import alnstats
import alnrows

pytestmark = pytest.mark.gpu

GPU_NOTE = "residue rows on the GPU"
ALL_KNOBS = {"MPA_GPU_SEED": "1", "MPA_GPU_SKETCH": "1", "MPA_GPU_REGIONS": "1", "MPA_GPU_REFINE": "1", "MPA_GPU_PLANS": "1", "MPA_GPU_STATS": "1", "MPA_GPU_CS": "1"}


@pytest.fixture(scope="module")
def ctx():
    c = mpa.Context(0)
    yield c
    c.close()


def _run(ctx, idx, mo, q, knob, capfd, n_threads=4, more=None):
    """one blocking batch with MPA_GPU_ROWS = knob (None: unset) and the knobs of `more`: (text, stderr)"""
    env = {"MPA_GPU_ROWS": knob, "MPA_TIMING": "1"}
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
        text = mpa.format_output(idx, mo, q, res)[0]
        err = capfd.readouterr().err
    finally:
        for k, v in keep.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    return text, err


def _reference(idx, q, flags, tmp):
    """the live reference's output for an index and queries, None where its binary is not present"""
    if not os.path.exists(refbind.REF_BIN):
        return None
    mpi, faa = str(tmp / "g.mpi"), str(tmp / "p.fa")
    idx.dump(mpi)
    gen_synth.write_fasta_aa(faa, q.seqs, q.names)
    return subprocess.run([refbind.REF_BIN, "-t4"] + flags + [mpi, faa], capture_output=True).stdout


def _pair(ctx, idx, mo, q, capfd, more=None):
    idx.to_device(ctx)
    return _run(ctx, idx, mo, q, None, capfd, more=more), _run(ctx, idx, mo, q, "1", capfd, more=more)


def _check(host, dev, ref):
    assert GPU_NOTE in dev[1], "MPA_GPU_ROWS=1 did not run the residue rows on the device"
    declined = [l for l in dev[1].split("\n") if "declined" in l and ("rows" in l or "cs strings" in l or "statistics" in l)]
    assert not declined, declined[:3]
    assert "residue rows" not in host[1]
    if ref is not None:
        assert dev[0] == ref, "text differs from the reference"
        assert host[0] == ref
    assert dev[0] == host[0]
    n = alnrows.row_sets(host[0])
    assert n > 0 and alnrows.format_counts(dev[1]) == (n, 0) and alnrows.format_counts(host[1]) == (0, n)


_done = {}


def _case(ctx, name, capfd, tmp_path_factory, more=None):
    """a golden case mapped once with the knob unset and once with MPA_GPU_ROWS=1 (both with the knobs of `more`)"""
    key = (name, tuple(sorted((more or {}).items())))
    if key not in _done:
        idx, mo, q, ref = alnstats.case_inputs(name, tmp_path_factory.mktemp(name))
        host, dev = _pair(ctx, idx, mo, q, capfd, more)
        idx.close()
        _done[key] = (host, dev, ref)
    return _done[key]


@pytest.mark.parametrize("name", ["syn_k", "syn_l", "syn_m"])
def test_golden_cases(ctx, name, capfd, tmp_path_factory):
    """-u --aln; --trans --gff; --aln --trans --gtf"""
    _check(*_case(ctx, name, capfd, tmp_path_factory))


def test_with_statistics_and_cs_strings_on_the_device_too(ctx, capfd, tmp_path_factory):
    """MPA_GPU_STATS=1 MPA_GPU_CS=1 as well: the three kernels share one upload and one wait -- three notes, and the one call's two
    slot lines, the same bytes"""
    host, dev, ref = _case(ctx, "syn_m", capfd, tmp_path_factory, {"MPA_GPU_STATS": "1", "MPA_GPU_CS": "1"})
    _check(host, dev, ref)
    for note in ("alignment statistics on the GPU", "cs strings on the GPU", GPU_NOTE):
        assert dev[1].count(note) == 1
    assert dev[1].count("cs slots:") == 1 and dev[1].count("rows slots:") == 1
    assert "alignment statistics on the GPU" in host[1] and "cs strings on the GPU" in host[1]


WALKS = (("MPA_GPU_STATS", "alignment statistics on the GPU", None), ("MPA_GPU_CS", "cs strings on the GPU", "cs slots:"), ("MPA_GPU_ROWS", GPU_NOTE, "rows slots:"))


def test_every_combination_of_the_three_walks(ctx, capfd, tmp_path):
    """The walks whose knob is 1 share one device call, whatever the others do.  syn_a's input with --aln --trans (its options are -u:
    the row lines are all that --aln --trans add, so the text without them is the golden file) on one context under all eight
    settings of (MPA_GPU_STATS, MPA_GPU_CS, MPA_GPU_ROWS) in {unset, 1} and two mixed ones (model, 1, 1) and (1, model, unset): the
    bytes and the result arrays of the all-unset run, nothing declined, each walk's note once when its knob is 1 and never otherwise,
    and its slot line with it"""
    idx, mo, q, ref = alnstats.case_inputs("syn_a", tmp_path)
    mo.flag |= alnrows.ALN | alnrows.TRANS
    idx.to_device(ctx)
    settings = [tuple("1" if k >> i & 1 else None for i in range(3)) for k in range(8)] + [("model", "1", "1"), ("1", "model", None)]
    keep = {k: os.environ.get(k) for k in ("MPA_TIMING",) + tuple(w[0] for w in WALKS)}
    base = None
    try:
        os.environ["MPA_TIMING"] = "1"
        for setting in settings:
            for (knob, _, _), v in zip(WALKS, setting):
                if v is None:
                    os.environ.pop(knob, None)
                else:
                    os.environ[knob] = v
            capfd.readouterr()
            res = mpa.map_batch(ctx, idx, mo, q, 4)
            text = mpa.format_output(idx, mo, q, res)[0]
            arrays = alnstats.result_arrays(res)
            err = capfd.readouterr().err
            if base is None:
                base = (text, arrays)
                assert alnrows.row_sets(text) > 0
                assert b"".join(l + b"\n" for l in text.split(b"\n")[:-1] if not (l[:2] == b"##" and l[2:5] in alnrows.KINDS)) == ref
            assert text == base[0], setting
            assert alnstats.first_difference(arrays, base[1]) is None, (setting, alnstats.first_difference(arrays, base[1]))
            assert "declined" not in err, (setting, [l for l in err.split("\n") if "declined" in l][:3])
            for (knob, note, slots), v in zip(WALKS, setting):
                assert err.count(note) == (1 if v == "1" else 0), (setting, knob)
                if slots:
                    assert err.count(slots) == (1 if v == "1" else 0), (setting, knob)
    finally:
        for k, v in keep.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
        idx.close()


def test_with_every_device_knob(ctx, capfd, tmp_path_factory):
    _check(*_case(ctx, "syn_m", capfd, tmp_path_factory, ALL_KNOBS))


def test_stream_of_three_batches(ctx, capfd, monkeypatch):
    """mpa_map_batches(): the rows are built on the lanes' contexts -- same bytes, the note of every batch"""
    idx, mo, q, ref = alnstats.case_inputs("syn_k")
    idx.to_device(ctx)
    n = len(q.seqs)
    batches = [mpa.Queries(q.seqs[a:b], q.names[a:b]) for a, b in ((0, n // 3), (n // 3, 2 * n // 3), (2 * n // 3, n))]
    monkeypatch.setenv("MPA_TIMING", "1")
    monkeypatch.setenv("MPA_GPU_ROWS", "1")
    capfd.readouterr()
    texts = mpa.map_batches(ctx, idx, mo, batches, 4)
    err = capfd.readouterr().err
    assert b"".join(texts) == ref
    assert err.count(GPU_NOTE) == 3 and "declined" not in err
    assert alnrows.format_counts(err) == (alnrows.row_sets(ref), 0)
    idx.close()


# ---- the edge genome ---------------------------------------------------------------------------------
_edge_done = {}


def _edge(ctx, d, e, capfd, tmp_path_factory):
    """the edge genome of (d, e) with --aln --trans mapped with the knob unset and set, and by the reference where its binary is
    present: once per pair"""
    if (d, e) not in _edge_done:
        idx, mo, q = alnrows.edge(d, e)
        host, dev = _pair(ctx, idx, mo, q, capfd)
        ref = _reference(idx, q, ["-u", "--aln", "--trans"], tmp_path_factory.mktemp("edge%d%d" % (d + 4, e + 4)))
        idx.close()
        _edge_done[(d, e)] = (host, dev, ref, len(q.seqs))
    return _edge_done[(d, e)]


@pytest.mark.parametrize("d", [0, 1, 2, 3])
@pytest.mark.parametrize("e", [0, 1, 2, 3])
def test_edge_genome_device_equals_host_and_the_live_reference(ctx, d, e, capfd, tmp_path_factory):
    """contigs that begin d bases before their first gene and end e bases behind their last, 5 % N"""
    host, dev, ref, n = _edge(ctx, d, e, capfd, tmp_path_factory)
    assert alnrows.row_sets(host[0]) >= n // 2
    _check(host, dev, ref)


@pytest.mark.parametrize("cut", [1, 2])
def test_alignments_that_end_at_the_contig_end(ctx, cut, capfd, tmp_path_factory):
    """the edge genome trimmed into its outermost stop codons: ve + 3 lies beyond the contig, no trailing codon"""
    host, dev, ref, _ = _edge(ctx, -cut, -cut, capfd, tmp_path_factory)
    _check(host, dev, ref)
    assert alnrows.near_end(dev[0]) >= 1 and alnrows.kinds(dev[0])["sta_open"] >= alnrows.near_end(dev[0])


def test_planted_ambiguous_bases(ctx, capfd, tmp_path):
    idx, mo, q = alnrows.planted_n()
    host, dev = _pair(ctx, idx, mo, q, capfd)
    ref = _reference(idx, q, ["-u", "--aln", "--trans"], tmp_path)
    idx.close()
    _check(host, dev, ref)
    assert alnrows.kinds(dev[0])["N"] == 8


def test_lowered_frameshift_penalty(ctx, capfd, tmp_path):
    """syn_k's input with -F 6: '$' and '!' columns by the dozen"""
    idx, mo, q = alnrows.low_frameshift(alnstats.case_inputs, "syn_k", 6)
    host, dev = _pair(ctx, idx, mo, q, capfd)
    ref = _reference(idx, q, ["-u", "--aln", "--trans", "-F", "6"], tmp_path)
    idx.close()
    _check(host, dev, ref)
    k = alnrows.kinds(dev[0])
    assert k["$"] > 0 and k["!"] > 0, k


@pytest.mark.parametrize("flank", [0, 1])
def test_intron_flank_of_zero_and_one(ctx, flank, capfd, tmp_path):
    """syn_m with max_intron_flank 0 ("~len~" alone) and 1 (--max-intron-out 0 / 1 of the reference's command line)"""
    idx, mo, q, _ = alnstats.case_inputs("syn_m", tmp_path)
    mo.max_intron_flank = flank
    host, dev = _pair(ctx, idx, mo, q, capfd)
    ref = _reference(idx, q, ["--aln", "--trans", "--gtf", "--max-intron-out", str(flank)], tmp_path)
    idx.close()
    _check(host, dev, ref)
    assert alnrows.kinds(dev[0])["abridged"] > 0


# ---- options that print no rows --------------------------------------------------------------------------
def test_case_that_prints_no_rows_skips_the_step(capfd, tmp_path):
    """syn_a (-u) with the knob set, on a fresh context: no note, no pool -- mpa_device_bytes() stays where the unset run left it"""
    c = mpa.Context(0)
    idx, mo, q, ref = alnstats.case_inputs("syn_a", tmp_path)
    idx.to_device(c)
    t0, err0 = _run(c, idx, mo, q, None, capfd)
    b0 = mpa.Context.device_bytes()
    t1, err1 = _run(c, idx, mo, q, "1", capfd)
    assert mpa.Context.device_bytes() == b0
    assert "residue rows" not in err0 + err1 and alnrows.format_counts(err1) is None
    assert t0 == t1 == ref and alnrows.row_sets(t1) == 0
    idx.close()
    c.close()


# ---- the knob unset -----------------------------------------------------------------------------------
def test_knob_unset_launches_nothing_and_holds_no_memory(capfd, tmp_path):
    """k_aln_rows has one launch site, which sizes its device pools first.  On a fresh context: runs with the knob unset (or 0) leave
    mpa_device_bytes() where it was and print no note; the first run with the knob set then grows it -- so the runs before it had
    allocated no pool, i.e. had not been there -- and going back to unset changes nothing again."""
    c = mpa.Context(0)
    idx, mo, q, ref = alnstats.case_inputs("syn_m", tmp_path)
    idx.to_device(c)
    t0, err0 = _run(c, idx, mo, q, None, capfd, 2)
    b0 = mpa.Context.device_bytes()
    t1, err1 = _run(c, idx, mo, q, None, capfd, 2)
    t2, err2 = _run(c, idx, mo, q, "0", capfd, 2)
    assert mpa.Context.device_bytes() == b0
    assert "residue rows" not in err0 + err1 + err2
    assert alnrows.format_counts(err2)[0] == 0
    t3, err3 = _run(c, idx, mo, q, "1", capfd, 2)
    b1 = mpa.Context.device_bytes()
    assert GPU_NOTE in err3 and b1 > b0 and alnrows.format_counts(err3)[1] == 0
    t4, err4 = _run(c, idx, mo, q, None, capfd, 2)
    assert mpa.Context.device_bytes() == b1 and "residue rows" not in err4
    assert t0 == t1 == t2 == t3 == t4 == ref
    idx.close()
    c.close()
