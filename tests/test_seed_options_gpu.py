"""The GPU seeding side away from miniprot's default options (tests/seedopts.py): k_seed_sift, k_prechain_fwd, k_chain_fwd /
k_chain_fwd_wave, k_chain_extract, k_refine_scan, k_refine_scan_map + k_refine_pair_*, k_index_scan take their shape from the
index options (-k -M -b -L) and from the seeding / chaining options of mpa_mapopt_t, and every other GPU test runs them at
`-k6 -M1 -b8 -L30` with default chaining.  Every comparison here is exact (arrays equal, bytes equal); the references are the
host stages (pinned to the reference at these very points by tests/test_host_pipeline.py::test_option_cases_paf_identical), the
reference's own mp_chain() (oracle/_ref/libminiprot_ref.so) and the reference's output (tests/golden/opt_*.ref.paf)."""
import ctypes as C
import os
import subprocess
import sys
import numpy as np
import pytest
import miniprot_amd as mpa
import golden
import gen_synth
import refbind
import seedopts
from hostpipe import map_batch_gpu
from test_seed_gpu import survivors, main_chains, raw_anchors

pytestmark = pytest.mark.gpu
UNSUPPORTED = -3                                       # MPA_ERR_UNSUPPORTED (include/mpamd.h)
NCPU = min(16, os.cpu_count() or 4)


@pytest.fixture(scope="module")
def ctx():
    c = mpa.Context(0)
    yield c
    c.close()


class _Tandem:
    """the tandem-copy genome of tests/test_seed_gpu.py (generate(3000000, 2, 40, 35), copies drawn with default_rng(5)) as a FASTA
    file, its 53 queries, and the index of the point in use (one at a time: the parameters below come grouped by index point)"""

    def __init__(self, tmp):
        contigs, self.seqs = seedopts.tandem_genome(5, 35)
        self.fa = seedopts.write_genome(tmp, contigs)
        self.q = mpa.Queries(self.seqs)
        self.point, self.idx = None, None

    def index(self, point, ctx):
        if self.point != point:
            self.close()
            self.idx = mpa.Index.read_fasta(self.fa, point)
            assert self.idx.build_kmers(NCPU) == "host"          # (the host build is the one the CPU tests pin to `miniprot -d`)
            self.idx.to_device(ctx)
            self.point = point
        return self.idx

    def close(self):
        if self.idx is not None:
            self.idx.close()
        self.point, self.idx = None, None


@pytest.fixture(scope="module")
def tandem(tmp_path_factory):
    t = _Tandem(tmp_path_factory.mktemp("tandem"))
    yield t
    t.close()


K4 = (4, 10, 4, 0)
PRECHAIN_POINTS = [c for c in seedopts.CHAIN_POINTS if c.prechain]
# every index point with every chaining point that runs the pre-chain, and once more with segments of 300 anchors
SIFT_GRID = [(ip, cp, seg) for ip in seedopts.INDEX_POINTS for cp, seg in [(c, None) for c in PRECHAIN_POINTS] + [(PRECHAIN_POINTS[0], "300")]]


def _grid_id(p):
    return "%s-%s%s" % (seedopts.index_name(p[0]), p[1].name, "-seg" + p[2] if p[2] else "")


def check_sift_and_chains(tandem, ctx, ip, cp):
    """device survivors and device main chains of every query == the host's == the reference's mp_chain() at this point's kmer,
    bbit and chaining arguments"""
    bbit, _, kmer, _ = ip
    idx, q = tandem.index(ip, ctx), tandem.q
    mo = cp.apply(mpa.default_mapopt())
    a_off, a_all = raw_anchors(idx, mo, q, NCPU)
    hs_off, hs = survivors(None, idx, mo, q, NCPU)
    ds_off, ds = survivors(ctx, idx, mo, q, NCPU)          # (errors with "device seeding was not used" if the device declined the batch)
    assert np.array_equal(hs_off, ds_off) and np.array_equal(hs, ds), "pre-chain survivors: device != host"
    _, hu_off, hu, ha_off, ha = main_chains(None, idx, mo, q, NCPU)
    n_back, du_off, du, da_off, da = main_chains(ctx, idx, mo, q, NCPU)
    assert np.array_equal(hu_off, du_off) and np.array_equal(hu, du), "main chains, u: device != host"
    assert np.array_equal(ha_off, da_off) and np.array_equal(ha, da), "main chains, anchors: device != host"
    for i in range(len(q.seqs)):
        _, pre = refbind.ref_chain(a_all[a_off[i]:a_off[i + 1]], seedopts.chain_args(mo, kmer, bbit, True))
        pre = np.sort(pre)                                     # radix_sort_mp64, map.c:191
        assert np.array_equal(pre, ds[ds_off[i]:ds_off[i + 1]]), ("pre-chain survivors: device != mp_chain", i)
        u, ca = refbind.ref_chain(pre, seedopts.chain_args(mo, kmer, bbit, False))
        assert np.array_equal(u, du[du_off[i]:du_off[i + 1]]), ("main chains, u: device != mp_chain", i)
        assert np.array_equal(ca, da[da_off[i]:da_off[i + 1]]), ("main chains, anchors: device != mp_chain", i)
    # not passing on nothing (the reference alone gives 637 .. 635 657 survivors and 34 .. 53 673 chains over the grid)
    assert ds_off[-1] >= 500 and du_off[-1] >= 30, (int(ds_off[-1]), int(du_off[-1]))
    if ip == K4 and mo.max_occ > 50:
        # -k4 on 3 Mbp: up to 306 738 anchors per query, every large query on the halved staging of k_seed_sift (above 16 384
        # anchors a query owns half as many staging slots as anchors, and a segment that keeps more than half hands its query back
        # to the host): here the hand-backs may be many -- they matched above like every other query
        assert int(np.diff(a_off).max()) > 16384
    else:                                                      # (-k4 with -c 50: 7 561 anchors at most, the ordinary staging)
        assert n_back < len(q.seqs) // 2, n_back
    return int(ds_off[-1]), int(du_off[-1]), int(n_back)


@pytest.mark.skipif(not refbind.have_ref(), reason="oracle/_ref/libminiprot_ref.so not built")
@pytest.mark.parametrize("ip,cp,seg", SIFT_GRID, ids=[_grid_id(p) for p in SIFT_GRID])
def test_device_sift_and_chaining_rounds_across_the_option_grid(tandem, ctx, ip, cp, seg, monkeypatch):
    """Sift + pre-chain + both chaining rounds on the device at every INDEX_POINTS x CHAIN_POINTS pair that runs the pre-chain:
    what depends on the options there is the sift's key packing ((block - lo + 1) << LB | list, LB from the seeds of a query: twice
    as many with -M0, a sixteenth with -M4), w_max and the segment cuts over genome >> bbit blocks, the halved staging (-k4, -k5),
    (kcur - kprev) << bbit and max_dist_x >> bbit in the forward passes, the 28-bit words of -k7, min_chn_cnt / min_chn_sc in the
    device extraction.  Also with MPA_SIFT_SEG=300 so that segments cut through queries at every block size."""
    if seg:
        monkeypatch.setenv("MPA_SIFT_SEG", seg)
    n_surv, n_chain, n_back = check_sift_and_chains(tandem, ctx, ip, cp)
    print("%s: %d survivors, %d chains, %d queries handed back" % (_grid_id((ip, cp, seg)), n_surv, n_chain, n_back))


@pytest.mark.skipif(not refbind.have_ref(), reason="oracle/_ref/libminiprot_ref.so not built")
@pytest.mark.parametrize("cp", [c for c in seedopts.CHAIN_POINTS if not c.prechain], ids=lambda c: c.name)
@pytest.mark.parametrize("ip", [(8, 30, 6, 1), (6, 20, 5, 0)], ids=seedopts.index_name)
def test_without_a_pre_chain_the_device_stays_out(tandem, ctx, ip, cp):
    """--no-pre-chain and -S: map.c:186 skips the pre-chain, and device seeding exists only with it -- a call with a device context
    must then give the host's chains (= mp_chain() on all anchors), not an error and not a device result"""
    bbit, _, kmer, _ = ip
    idx, q = tandem.index(ip, ctx), tandem.q
    mo = cp.apply(mpa.default_mapopt())
    a_off, a_all = raw_anchors(idx, mo, q, NCPU)
    s_off, s = survivors(ctx, idx, mo, q, NCPU)
    assert np.array_equal(s_off, a_off) and np.array_equal(s, a_all)
    n_back, du_off, du, da_off, da = main_chains(ctx, idx, mo, q, NCPU)
    assert n_back == 0                                          # (counts queries a DEVICE run handed back)
    for i in range(len(q.seqs)):
        u, ca = refbind.ref_chain(a_all[a_off[i]:a_off[i + 1]], seedopts.chain_args(mo, kmer, bbit, False))
        assert np.array_equal(u, du[du_off[i]:du_off[i + 1]]) and np.array_equal(ca, da[da_off[i]:da_off[i + 1]]), i
    assert du_off[-1] >= 30


def test_sift_with_ranges_of_2048(tmp_path):
    """k_seed_sift<2048> (MPA_SIFT_CAP=2048: ranges of half the size, 18 KB of LDS) is compiled into the product: tests/test_seed_gpu.py
    and the default-chaining row of the grid above once more with it, in a process of its own (the variable is read once)"""
    env = dict(os.environ, MPA_SIFT_CAP="2048")
    sel = ["tests/test_seed_gpu.py", "tests/test_seed_options_gpu.py::test_device_sift_and_chaining_rounds_across_the_option_grid", "-k",
           "not test_device_sift_and_chaining_rounds_across_the_option_grid or default"]
    r = subprocess.run([sys.executable, "-m", "pytest", "-x", "-q", "-m", "gpu", "-p", "no:cacheprovider"] + sel, cwd=refbind.ROOT, env=env, capture_output=True, text=True, timeout=1200)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    import re
    m = re.search(r"(\d+) passed", r.stdout)
    # (the 16 tests of tests/test_seed_gpu.py as of this writing, and two per index point of the grid; none skipped)
    assert m and int(m.group(1)) >= 16 + 2 * len(seedopts.INDEX_POINTS) and "skipped" not in r.stdout, r.stdout[-500:]


@pytest.mark.parametrize("serial_run", ["48", "4"])
def test_device_chain_forward_equals_host_forward_off_defaults(serial_run, monkeypatch):
    """k_chain_fwd / k_chain_fwd_wave against the host pass as in tests/test_seed_gpu.py, with the block size, the k-mer, the log
    coefficient and the query-side reach drawn away from the defaults: (kcur - kprev) << bbit, max_dist_x >> bbit and the block
    bonus at bbit 4, 6, 10, 12; kmer 4, 5, 7; coef_log 0.2, 0.75, 2.0; max_dist_y 200, 1000"""
    monkeypatch.setenv("MPA_CHAIN_SERIAL_RUN", serial_run)
    from chaincases import _anchors, _long_chains
    L = mpa.lib()
    L.mpa_dbg_chain_forward.argtypes = [C.c_void_p] + [C.c_int32] * 5 + [C.c_float] + [C.c_int32] * 4 + [C.c_void_p] * 4
    rng = np.random.default_rng(23)
    ctx = mpa.Context(0)

    def both(args, probs):
        first = np.zeros(len(probs) + 1, np.int64)
        np.cumsum([len(p) for p in probs], out=first[1:])
        a = np.ascontiguousarray(np.concatenate(probs + [np.zeros(0, np.uint64)]), dtype=np.uint64)
        res = []
        for c in (None, ctx.h):
            f, pr = np.full(len(a) + 1, -7, np.int32), np.full(len(a) + 1, -7, np.int32)
            rc = L.mpa_dbg_chain_forward(c, *args, len(probs), first.ctypes.data, a.ctypes.data, f.ctypes.data, pr.ctypes.data)
            assert rc == 0, mpa.last_error()
            res.append((f[:len(a)], pr[:len(a)]))
        assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1]), (args, [len(p) for p in probs][:8])
        return int((res[0][1] >= 0).sum())

    for bbit in (4, 6, 10, 12):                                   # main-chain shape, one group per block size
        linked = 0
        n_block = max(6000000 >> bbit, 2000)                      # blocks of both strands of a 3 Mbp genome
        for it in range(9):
            probs = []
            for k in range(int(rng.choice([1, 7, 60]))):
                kind = int(rng.integers(0, 5))
                if kind == 0:
                    probs.append(_anchors(rng, int(rng.choice([70, 500, 9000])), n_block, 400, int(rng.choice([0, 3, 40]))))
                elif kind == 1:
                    probs.append(_anchors(rng, int(rng.choice([65, 300, 3000])), int(rng.choice([50, 400, 3000])), 300, 20))
                elif kind == 2:
                    probs.append(np.unique(np.concatenate([_anchors(rng, 2000, n_block, 900, 10), _long_chains(rng, n_block, 3, "any")])))
                elif kind == 3:
                    probs.append(np.zeros(0, np.uint64))
                else:
                    probs.append(_anchors(rng, 1, 1000, 100, 0)[:1])
            kmer, coef, dist_y = (4, 5, 7)[it % 3], (0.2, 0.75, 2.0)[it // 3], int(rng.choice([200, 1000]))
            args = [int(rng.choice([200000, 20000, 2000])), dist_y, int(rng.choice([200000, 20000, 2000])), int(rng.choice([25, 2, 0])), int(rng.choice([1000000, 20])), coef,
                    int(rng.integers(0, 2)), kmer, bbit]
            linked += both(args, probs)
        assert linked > 5000, bbit
    linked = 0
    for it in range(9):                                           # refinement shape: base resolution (bbit 0), kmer2 3..7
        probs = []
        for k in range(int(rng.choice([1, 30]))):
            n = int(rng.choice([0, 1, 5, 80, 600]))
            dq = np.cumsum(rng.integers(1, 9, n))
            x = 1000 + dq * 3 + (rng.choice([0, 0, 1, -1, 300, 5000], n) * (rng.random(n) < 0.1)).cumsum()
            probs.append(np.unique((x.astype(np.uint64) << np.uint64(32)) | (20 + dq).astype(np.uint64)))
        args = [200000, int(rng.choice([200, 1000])), 200000, int(rng.choice([25, 2])), 1000000, (0.2, 0.75, 2.0)[it % 3], int(rng.integers(0, 2)), (3, 4, 6, 7, 5)[it % 5], 0]
        linked += both(args, probs)
    assert linked > 5000
    ctx.close()


CODON_TAB = "KNKNTTTTRSRSIIMIQHQHPPPPRRRRLLLLEDEDAAAAGGGGVVVV*Y*YSSSS*CWCLFLF"
ORF0 = 3000                                            # first base of the stop-free stretch of the refinement contig
PLANT_LEN = (35, 36, 37, 38, 39)                        # ORF lengths (codons) planted at chunk boundaries


def _refine_contig(rng):
    """the contig of tests/test_seed_gpu.py's refinement test (a stretch without stop codons in frame 0, its reverse complement, N
    islands, random sequence) plus ORFs of exactly 35..39 codons, planted with stop codons, that END or START at a k-mer lying on
    the first or the last positions of a 2048-base chunk of a window: whether such a k-mer counts is decided by walking its reading
    frame into the chunk's 112-base halo, from the chunk's first position exactly 37 codons far.  Returns (contig, sites): a site =
    (window start, window position of the k-mer's last base, ORF length, codon index of the k-mer's last codon)."""
    codons = [c for c in range(64) if c not in (48, 50, 56)]             # all but TAA TAG TGA
    orf = np.array([[c >> 4, c >> 2 & 3, c & 3] for c in rng.choice(codons, 6000)], dtype=np.uint8).reshape(-1)
    g = np.concatenate([rng.integers(0, 4, ORF0).astype(np.uint8), orf, rng.integers(0, 4, 9000).astype(np.uint8), orf[::-1].copy() ^ 3, rng.integers(0, 4, 500).astype(np.uint8)])
    for at in rng.integers(0, len(g) - 40, 25):
        g[at:at + int(rng.integers(1, 30))] = 4
    stop = np.array([3, 0, 0], np.uint8)                                  # TAA
    sites = []
    c = 900                                                               # codon index (in the stretch) of a site's k-mer
    for m in PLANT_LEN:
        for back, delta in ((True, 0), (True, 1), (True, 2), (False, 0), (False, 2)):
            c += 150
            g[ORF0 + 3 * (c - 45):ORF0 + 3 * (c + 45)] = orf[3 * (c - 45):3 * (c + 45)]      # (no N island near the site)
            last = ORF0 + 3 * c + 2                                       # genome position of the last base of codon c
            if back:      # the ORF is codons c - m + 1 .. c; the k-mer ends `delta` positions behind the first position of chunk 1
                g[ORF0 + 3 * (c - m):ORF0 + 3 * (c - m) + 3] = stop
                g[ORF0 + 3 * (c + 1):ORF0 + 3 * (c + 1) + 3] = stop
                wpos = 2048 + delta
            else:         # the ORF is codons c - 7 .. c + m - 8 (a k-mer of up to 7 residues fits before c); the k-mer ends `delta` before the end of chunk 0
                g[ORF0 + 3 * (c - 8):ORF0 + 3 * (c - 8) + 3] = stop
                g[ORF0 + 3 * (c + m - 7):ORF0 + 3 * (c + m - 7) + 3] = stop
                wpos = 2047 - delta
            sites.append((last - wpos, wpos, m, c))
    return g, sites


def _translate(nt):
    return "".join("X" if max(nt[i:i + 3]) > 3 else CODON_TAB[int(nt[i]) << 4 | int(nt[i + 1]) << 2 | int(nt[i + 2])] for i in range(0, len(nt) - 2, 3)).replace("*", "X")


def _refine_world(tmp_path):
    rng = np.random.default_rng(5)
    g, sites = _refine_contig(rng)
    c2 = rng.integers(0, 4, 700).astype(np.uint8)
    fa = seedopts.write_genome(tmp_path, [g, c2], "refine.fa")
    # the query: the translation of a stretch of the contig (many window k-mers are in its k-mer set) and of the 8 codons that end
    # with every site's k-mer
    prot = _translate(g[ORF0:ORF0 + 2400]) + "".join("X" + _translate(g[ORF0 + 3 * (c - 7):ORF0 + 3 * (c + 1)]) for _, _, _, c in sites)
    wins = []
    clen = [len(g), 700]
    for ln in (0, 5, 14, 15, 16, 89, 90, 2047, 2048, 2049, 4096, 6000, 20000):
        for vid in (0, 1):
            st = int(rng.integers(0, max(clen[0] - ln, 1)))
            wins.append((vid, st, min(ln, clen[0] - st)))
    wins += [(0, 0, clen[0]), (1, 0, clen[0]), (0, clen[0] - 3000, 3000), (1, clen[0] - 2100, 2100), (2, 0, 700), (3, 100, 600)]
    n_plain = len(wins)
    wins += [(0, st, 4200) for st, _, _, _ in sites]
    return fa, prot.encode(), wins, n_plain, sites


def _refine_hits(ctx, idx, kmer, prot, wins):
    L = mpa.lib()
    L.mpa_dbg_refine_hits.restype = C.c_int64
    L.mpa_dbg_refine_hits.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_char_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
    vid = np.array([w[0] for w in wins], np.int32)
    as_ = np.array([w[1] for w in wins], np.int64)
    ln_ = np.array([w[2] for w in wins], np.int32)
    first = np.zeros(len(wins) + 1, np.int64)
    out = C.c_void_p()
    n = L.mpa_dbg_refine_hits(ctx.h if ctx else None, idx.h, kmer, prot, len(prot), len(wins), vid.ctypes.data, as_.ctypes.data, ln_.ctypes.data, first.ctypes.data, C.byref(out))
    if n < 0:
        return int(n), None, None
    a = np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_uint64)), (max(n, 1),))[:n].copy()
    L.mpa_free(out)
    return int(n), first, a


@pytest.mark.parametrize("min_aa_len", [10, 30, 36, 37, 38, 40])
def test_device_refinement_scan_across_kmer_and_orf_length(ctx, tmp_path, min_aa_len):
    """k_refine_scan against the host's window scan at kmer2 3..7 and at indexes built with -L 10, 30, 36, 37: the same hits, hit for
    hit.  The kernel decides the minimum ORF length by walking into a fixed 112-base halo, which takes -L up to 37 for every k of
    3..7 (dev_refine_in_range, mpa_internal.h); at -L 38 and 40 the device must DECLINE (MPA_ERR_UNSUPPORTED through this entry
    point) -- a guard one wider would scan with a halo that cannot see the 38th codon, one narrower would send -L37 to the host
    unnoticed.  Planted ORFs of 35..39 codons at chunk boundaries make that 37th codon decide hits."""
    fa, prot, wins, n_plain, sites = _refine_world(tmp_path)
    idx = mpa.Index.read_fasta(fa, (8, min_aa_len, 6, 1))
    idx.to_device(ctx)
    for kmer in seedopts.REFINE_KMERS:
        n_h, fh, ah = _refine_hits(None, idx, kmer, prot, wins)
        assert n_h >= 0, mpa.last_error()
        assert fh[n_plain] > 500, (kmer, int(fh[n_plain]))          # the awkward windows over the stop-free stretch do hit
        # the planted k-mers count exactly when their ORF is long enough: the sites are what they were built to be (host result; the
        # device's is compared with it below)
        for j, (st, wpos, m, c) in enumerate(sites):
            pos = ah[fh[n_plain + j]:fh[n_plain + j + 1]] & np.uint64(0xffffffff)
            assert (wpos in pos) == (m >= min_aa_len), (kmer, j, wpos, m)
        n_d, fd, ad = _refine_hits(ctx, idx, kmer, prot, wins)
        if min_aa_len > 37:
            assert n_d == UNSUPPORTED, (kmer, n_d)
            continue
        assert n_d >= 0, mpa.last_error()
        assert np.array_equal(fh, fd) and np.array_equal(ah, ad), kmer
    idx.close()


INDEX_BUILD_POINTS = [(p, "gpu") for p in seedopts.INDEX_POINTS] + [
    ((8, 30, 7, 3), "gpu"),          # 25 bucket bits (28 is the guard's own edge: a 2 GB table)
    ((8, 1001, 6, 1), "host"),       # -L above 1000: beyond the halo k_index_scan can be given
    ((8, 4, 6, 1), "host"),          # -L below -k
    ((21, 30, 6, 1), "host"),        # -b above 20
]


def _same_file(a, b):
    if os.path.getsize(a) != os.path.getsize(b):
        return False
    with open(a, "rb") as fa, open(b, "rb") as fb:
        while True:
            x, y = fa.read(1 << 24), fb.read(1 << 24)
            if x != y:
                return False
            if not x:
                return True


@pytest.mark.parametrize("point,where", INDEX_BUILD_POINTS, ids=[seedopts.index_name(p) for p, _ in INDEX_BUILD_POINTS])
def test_index_build_across_index_options(tandem, ctx, tmp_path, point, where):
    """k_index_scan + sort + unique against the host build (pinned to `miniprot -d`) on the 3 Mbp tandem genome at every index
    point: the halo computed from -L, the modimizer mask, pos >> bbit, the bucket count 4 k - M up to 25 bits; and three tuples that
    dev_index_build's guard must hand to the host while the host build still works.  The .mpi bytes are equal in every case and the
    build runs where the guard says."""
    a = mpa.Index.read_fasta(tandem.fa, point)
    b = mpa.Index.read_fasta(tandem.fa, point)
    assert a.build_kmers(NCPU, ctx) == where
    assert b.build_kmers(NCPU) == "host"
    fa_, fb_ = str(tmp_path / "a.mpi"), str(tmp_path / "b.mpi")
    a.dump(fa_), b.dump(fb_)
    a.close(), b.close()
    same, size = _same_file(fa_, fb_), os.path.getsize(fa_)
    os.remove(fa_), os.remove(fb_)
    assert same, point
    assert size > 1500000                                            # (the packed genome alone is 1.5 MB)


# which stage must run where with MPA_GPU_SEED=1 MPA_GPU_REFINE=1 (a point may not move from one list to the other unnoticed):
# device seeding exists only with the pre-chain; the device refinement takes -l up to 7 and -L up to 37 (dev_refine_in_range)
HOST_SEEDING = {"opt_noprechain"}
HOST_REFINEMENT = {"opt_L38", "opt_L40", "opt_k7M4b10L40"}
SEED_NOTE, REFINE_NOTE, REFINE_SCAN_NOTE = "seeding on the GPU", "refinement on the GPU", "refinement scan on the GPU"


def _check_stage_notes(case, notes, what):
    assert "declined" not in notes, (what, [l for l in notes.split("\n") if "declined" in l][:3])
    assert (SEED_NOTE in notes) == (case["name"] not in HOST_SEEDING), (what, "seeding")
    assert (REFINE_NOTE in notes) == (case["name"] not in HOST_REFINEMENT), (what, "refinement")
    assert REFINE_SCAN_NOTE not in notes, what                       # (the scan-only fallback of a declined device refinement)


@pytest.mark.parametrize("case", golden.OPTION_CASES, ids=[c["name"] for c in golden.OPTION_CASES])
def test_option_cases_paf_identical_on_the_gpu(ctx, case, tmp_path, monkeypatch, capfd):
    """The whole path at the option points of golden.OPTION_CASES with every optional device stage forced on and the index built on
    the device: the bytes of the reference (which built its own index with the same flags), blocking call and a 3-batch stream,
    and -- from the library's timing notes -- each stage ran where this file says it runs."""
    monkeypatch.setenv("MPA_GPU_SEED", "1")
    monkeypatch.setenv("MPA_GPU_REFINE", "1")
    monkeypatch.setenv("MPA_TIMING", "1")
    contigs, prots, names = golden.synth_inputs(case)
    idx = mpa.Index.read_fasta(seedopts.write_genome(tmp_path, contigs), case["idx"])
    assert idx.build_kmers(4, ctx) == "gpu"
    idx.to_device(ctx)
    mo = golden.mapopt_for(case)
    ref = open(golden.path(case["name"] + ".ref.paf"), "rb").read()
    capfd.readouterr()
    ours = map_batch_gpu(ctx, idx, mo, mpa.Queries(prots, names), 4)
    _check_stage_notes(case, capfd.readouterr().err, "blocking call")
    assert ours == ref, "blocking call: output differs from the reference for %s" % case["name"]
    n = len(prots)
    batches = [mpa.Queries(prots[a:b], names[a:b]) for a, b in ((0, n // 3), (n // 3, 2 * n // 3), (2 * n // 3, n))]
    ours = b"".join(mpa.map_batches(ctx, idx, mo, batches, 4))
    _check_stage_notes(case, capfd.readouterr().err, "stream")
    assert ours == ref, "stream: output differs from the reference for %s" % case["name"]
    idx.close()


def test_max_ava_device_refinement_equals_host_refinement(ctx, monkeypatch):
    """mp_mapopt_t::max_ava (pairs of a k-mer are kept while n1 * n2 <= max_ava, a 32-bit product: k_refine_pair_count) has no
    command-line flag, so the reference binary cannot be driven there: this leg is DEVICE AGAINST HOST ONLY -- the whole path with
    device seeding and refinement against the whole path with both on the host, at max_ava 1, 50, 1000 (default), 2^31 - 1, with
    a low-complexity protein and a repeat-rich one among the queries (large n1 and n2)."""
    case = golden.OPTION_CASES[0]
    contigs, prots, names, planted = gen_synth.generate(case["genome"], case["n_ctg"], case["n_prot"], case["seed"], return_planted=True)
    prots = list(prots) + [bytes(planted[0]) * 3, bytes(planted[1])[:60] + b"Q" * 200 + bytes(planted[1])[60:]]
    names = list(names) + ["tripled", "polyq"]
    idx = mpa.Index.from_nt4(contigs, ["chr1", "chr2"])
    assert idx.build_kmers(4, ctx) == "gpu"
    idx.to_device(ctx)
    q = mpa.Queries(prots, names)
    outs = []
    for p in seedopts.REFINE_POINTS:
        if p.flags is not None:
            continue
        mo = mpa.default_mapopt()
        mo.flag |= 4
        p.apply(mo)
        monkeypatch.setenv("MPA_GPU_SEED", "0"), monkeypatch.setenv("MPA_GPU_REFINE", "0")
        host = map_batch_gpu(ctx, idx, mo, q, 4)
        monkeypatch.setenv("MPA_GPU_SEED", "1"), monkeypatch.setenv("MPA_GPU_REFINE", "1")
        dev = map_batch_gpu(ctx, idx, mo, q, 4)
        assert dev == host, p.name
        assert host.count(b"\n") >= len(prots)
        outs.append(host)
    # (the option does reach the output: with the host stages and the oracle executor max_ava 1 prints two lines fewer here than 50,
    # 1000 and 2^31 - 1, which print the same bytes)
    assert outs[0] != outs[2]
    idx.close()
