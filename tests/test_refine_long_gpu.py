"""Device refinement of LONG proteins: past 2 048 groups (distinct k = kmer2 k-mers) a query's k-mer map lives in device memory
(k_refine_gmap_build, k_refine_scan_gmap; for the scan-only fallback k_refine_scan_gset past 4 096 k-mers) instead of LDS, and a
window or a query beyond the sort key's 2^22 goes back to the host alone, not with its whole batch.  The case is tests/longprot.py:
queries on both sides of every limit, ordinary ones in between; the reference's bytes for it are tests/golden/long_u.ref.paf."""
import ctypes as C
import numpy as np
import pytest
import miniprot_amd as mpa
from hostpipe import map_batch_gpu
import golden
import longprot
import seedopts

pytestmark = pytest.mark.gpu

REFINE_NOTE, REFINE_SCAN_NOTE, GMAP_NOTE = "refinement on the GPU", "refinement scan on the GPU", "refine: global-map class"
REFINE_SUPER = 4                                                # chunks of 2 048 positions that one workgroup of the scan sweeps (refine_kernels.hip)
LONG_NAMES = [n for n, _, _ in longprot.LONG]


@pytest.fixture(scope="module")
def ctx():
    c = mpa.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def long_case(ctx):
    c = longprot.case()
    idx = mpa.Index.from_nt4(c["contigs"], ["chr1"])
    mpa._check(mpa.lib().mpa_idx_build_kmers(idx.h, 4))
    idx.to_device(ctx)
    yield c, idx, mpa.Queries(c["prots"], c["names"])
    idx.close()


def _same_chains(dev, host, what):
    for k, name in enumerate(("off_u", "u", "off_a", "a")):
        assert np.array_equal(dev[k], host[k]), (what, name)


def test_whole_path_with_long_proteins(ctx, long_case, monkeypatch, capfd):
    """the bytes of the reference, blocking call and a 3-batch stream, with the whole refinement on the device: no batch declines
    because of its long queries, and the global-map class did run; the same bytes with the class switched off (the batches then
    decline and the host refines, as before this class existed)"""
    c, idx, q = long_case
    monkeypatch.setenv("MPA_GPU_SEED", "1")
    monkeypatch.setenv("MPA_GPU_REFINE", "1")
    monkeypatch.setenv("MPA_TIMING", "1")
    monkeypatch.delenv("MPA_REFINE_GMAP_MIN", raising=False)
    mo = longprot.mapopt()
    ref = open(golden.path("long_u.ref.paf"), "rb").read()
    n = len(c["prots"])
    batches = [mpa.Queries(c["prots"][a:b], c["names"][a:b]) for a, b in ((0, n // 3), (n // 3, 2 * n // 3), (2 * n // 3, n))]

    def check_notes(what):
        notes = capfd.readouterr().err
        assert "declined" not in notes, (what, [l for l in notes.split("\n") if "declined" in l][:3])
        assert REFINE_NOTE in notes and GMAP_NOTE in notes, what
        assert REFINE_SCAN_NOTE not in notes, what

    capfd.readouterr()
    ours = map_batch_gpu(ctx, idx, mo, q, 4)
    check_notes("blocking call")
    assert ours == ref, "blocking call: output differs from the reference"
    ours = b"".join(mpa.map_batches(ctx, idx, mo, batches, 4))
    check_notes("stream")
    assert ours == ref, "stream: output differs from the reference"
    monkeypatch.setenv("MPA_REFINE_GMAP_MIN", "off")
    assert map_batch_gpu(ctx, idx, mo, q, 4) == ref, "MPA_REFINE_GMAP_MIN=off: output differs from the reference"


def _locus_window(c, name, margin=150):
    vid, st, ln = c["loci"][name]
    st0 = max(st - margin, 0)
    return (c["long"][name], vid, st0, min(st + ln + margin, longprot.GENOME) - st0)


def test_chains_of_long_queries_equal_the_host_chains(ctx, long_case, monkeypatch):
    """mpa_dbg_refine_chains, device against host, exact: the planted locus of every long query, windows of awkward lengths (1, shorter
    than a k-mer, the chunk size +-1, what one workgroup sweeps +-1, 20 000) over a long query's locus, and windows of ordinary
    queries, so that ONE call has queries of all four size classes (LDS maps of 1 024 / 2 048 / 4 096 slots, map in device memory)"""
    c, idx, q = long_case
    monkeypatch.delenv("MPA_REFINE_GMAP_MIN", raising=False)
    mo = longprot.mapopt()
    wins = [_locus_window(c, name) for name in LONG_NAMES]
    vid, st, ln = c["loci"]["g9000"]
    for k, wl in enumerate((1, 14, 2047, 2048, 2049, REFINE_SUPER * 2048 - 1, REFINE_SUPER * 2048 + 1, 20000)):
        wins.append((c["long"]["g9000"], vid, st + 1000 * k, wl))
        wins.append((c["long"]["g20000"], c["loci"]["g20000"][0], c["loci"]["g20000"][1] + 777 * k, wl))
    for i in c["ordinary"]:
        wins.append((i,) + longprot.ordinary_locus(c["names"][i]))
    ng = [longprot.groups(c["prots"][w[0]]) for w in wins]
    assert min(ng) <= 512 and any(512 < x <= 1024 for x in ng) and any(1024 < x <= 2048 for x in ng) and max(ng) > 2048
    host = mpa.refine_chains(None, idx, mo, q, wins)
    dev = mpa.refine_chains(ctx, idx, mo, q, wins)
    _same_chains(dev, host, "-l 5")
    assert not dev[4].any()                                      # nothing handed back
    for k, name in enumerate(LONG_NAMES):                        # the planted locus of every long query has a chain
        assert host[0][k + 1] > host[0][k], name
    # the ends of the k-mer range that matter for the width of the word (dev_refine_in_range), for the 9 000-group query
    sub = [w for w in wins if w[0] == c["long"]["g9000"]]
    for kmer2 in (4, 7):
        mo2 = longprot.mapopt(kmer2)
        assert longprot.groups(c["prots"][c["long"]["g9000"]], kmer2) > 2048
        host = mpa.refine_chains(None, idx, mo2, q, sub)
        _same_chains(mpa.refine_chains(ctx, idx, mo2, q, sub), host, "-l %d" % kmer2)
        assert host[0][1] > host[0][0], kmer2


def _refine_hits(c, idx, kmer, prot, wins):
    L = mpa.lib()
    L.mpa_dbg_refine_hits.restype = C.c_int64
    L.mpa_dbg_refine_hits.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_char_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
    vid = np.array([w[0] for w in wins], np.int32)
    as_ = np.array([w[1] for w in wins], np.int64)
    ln_ = np.array([w[2] for w in wins], np.int32)
    first = np.zeros(len(wins) + 1, np.int64)
    out = C.c_void_p()
    n = L.mpa_dbg_refine_hits(c.h if c else None, idx.h, kmer, prot, len(prot), len(wins), vid.ctypes.data, as_.ctypes.data, ln_.ctypes.data, first.ctypes.data, C.byref(out))
    assert n >= 0, (n, mpa.last_error())
    a = np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_uint64)), (max(n, 1),))[:n].copy()
    L.mpa_free(out)
    return first, a


@pytest.mark.parametrize("name", ["k4096", "k4097", "g9000", "g20000"])
def test_scan_only_fallback_for_long_queries(ctx, long_case, monkeypatch, name):
    """mpa_dbg_refine_hits (the scan-only fallback, k_refine_scan / k_refine_scan_gset), device against host, on both sides of the
    4 096 k-mers its LDS set takes and far beyond; window lengths as in test_seed_gpu.py, placed over the query's planted locus"""
    c, idx, _ = long_case
    monkeypatch.delenv("MPA_REFINE_GMAP_MIN", raising=False)
    prot = c["prots"][c["long"][name]]
    assert (len(longprot.kmer_words(prot)) > 4096) == (name != "k4096")
    vid, st, ln = c["loci"][name]
    wins = [(vid, st, ln)]
    for k, wl in enumerate((0, 5, 14, 15, 16, 89, 90, 2047, 2048, 2049, 4096, 6000, 20000)):
        wins.append((vid, st + 500 * k, wl))
        wins.append((vid ^ 1, longprot.GENOME - st - ln + 300 * k, wl))
    fh, ah = _refine_hits(None, idx, longprot.KMER2, prot, wins)
    fd, ad = _refine_hits(ctx, idx, longprot.KMER2, prot, wins)
    assert np.array_equal(fh, fd) and np.array_equal(ah, ad)
    assert fh[1] > 1000                                          # the locus does hit


@pytest.mark.parametrize("case_name", ["syn_a", "syn_e", "opt_L37"])
def test_every_query_through_the_global_map(ctx, case_name, tmp_path, monkeypatch, capfd):
    """MPA_REFINE_GMAP_MIN=1 sends every query of a golden case through the global-map class (small tables, many of them, 1 024
    slots at least): the committed bytes of the reference.  The knob is read per call: for syn_a the class runs with 1 and does not
    run at the default, in one process."""
    case = [x for x in golden.SYNTH_CASES + golden.OPTION_CASES if x["name"] == case_name][0]
    monkeypatch.setenv("MPA_GPU_SEED", "1")
    monkeypatch.setenv("MPA_GPU_REFINE", "1")
    monkeypatch.setenv("MPA_TIMING", "1")
    contigs, prots, names = golden.synth_inputs(case)
    if "idx" in case:
        idx = mpa.Index.read_fasta(seedopts.write_genome(tmp_path, contigs), case["idx"])
        assert idx.build_kmers(4, ctx) == "gpu"
    else:
        idx = mpa.Index.from_nt4(contigs, ["chr%d" % (i + 1) for i in range(len(contigs))])
        mpa._check(mpa.lib().mpa_idx_build_kmers(idx.h, 4))
    idx.to_device(ctx)
    mo = golden.mapopt_for(case)
    ref = open(golden.path(case["name"] + ".ref.paf"), "rb").read()
    q = mpa.Queries(prots, names)
    monkeypatch.setenv("MPA_REFINE_GMAP_MIN", "1")
    capfd.readouterr()
    ours = golden.file_header(case) + map_batch_gpu(ctx, idx, mo, q, 4)
    notes = capfd.readouterr().err
    assert REFINE_NOTE in notes and GMAP_NOTE in notes and "declined" not in notes
    assert ours == ref, "MPA_REFINE_GMAP_MIN=1: output differs from the reference for %s" % case["name"]
    if case_name == "syn_a":
        monkeypatch.delenv("MPA_REFINE_GMAP_MIN")
        ours = golden.file_header(case) + map_batch_gpu(ctx, idx, mo, q, 4)
        notes = capfd.readouterr().err
        assert REFINE_NOTE in notes and GMAP_NOTE not in notes
        assert ours == ref
    idx.close()


def test_a_window_of_2_to_the_22_bases_goes_back_alone(ctx, monkeypatch):
    """a window of 2^22 bases does not fit the sort key of the pairing (window << 44 | position << 22 | query position): it comes back
    flagged for the host, without chains, and the other windows of the call are refined on the device as the host refines them"""
    monkeypatch.delenv("MPA_REFINE_GMAP_MIN", raising=False)
    rng = np.random.default_rng(2222)
    g = rng.integers(0, 4, 5000000).astype(np.uint8)
    from miniprot_amd import synth
    prot, gene = synth.make_gene(rng, 300, 7.5, 1.5, 70, 600, min_exons=3)
    g[100000:100000 + len(gene)] = gene
    idx = mpa.Index.from_nt4([g], ["c1"])
    idx.to_device(ctx)
    q = mpa.Queries([bytes(prot), bytes(synth.AA[rng.integers(0, 20, 250)])])
    mo = longprot.mapopt()
    small = [(0, 0, 99000, len(gene) + 2000), (1, 1, 3000000, 5000)]
    wins = [small[0], (0, 0, 50000, 1 << 22), small[1]]
    dev = mpa.refine_chains(ctx, idx, mo, q, wins)
    assert dev[4].tolist() == [0, 1, 0]
    assert dev[0][2] == dev[0][1] and dev[2][2] == dev[2][1]     # no chains for the window that went back
    host = mpa.refine_chains(None, idx, mo, q, small)
    assert host[0][1] > 0                                        # the planted gene does chain
    for k in (0, 1):                                             # u and anchors of the two ordinary windows (0 and 2 of the device call)
        d = 2 * k
        assert np.array_equal(dev[1][dev[0][d]:dev[0][d + 1]], host[1][host[0][k]:host[0][k + 1]])
        assert np.array_equal(dev[3][dev[2][d]:dev[2][d + 1]], host[3][host[2][k]:host[2][k + 1]])
    idx.close()
