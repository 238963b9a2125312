"""The option grid of the seeding side (index build, sift, pre-chain, both chaining rounds, refinement) in one place, as
dpgen.py is for the DP penalties: points away from miniprot's defaults at which the GPU stages are compared with the host
stages and with the reference.  Every point carries the reference's command-line flags (None where miniprot has no flag for
the field) and apply(), which sets the same thing in mpa_mapopt_t; index points are the idxopt tuple of Index.read_fasta().

What was established on the CPU for these points (host stages against the live reference and against its mp_chain()): see
tests/test_host_pipeline.py::test_option_cases_paf_identical and the docstrings of tests/test_seed_options_gpu.py."""
import os
import numpy as np
import golden
import gen_synth

# (bbit, min_aa_len, kmer, mod_bit): mp_idxopt_init (options.c:14-22) first; small blocks + every k-mer kept; the 28-bit hash
# words of k = 7 with one k-mer in 16 kept; -k4 (78 000 anchors per query on a 3 Mbp genome: the sift's halved staging);
# 4 096-base blocks; and the two sides of what the refinement scan's 112-base halo takes (-L 37 / 38)
INDEX_POINTS = [(8, 30, 6, 1), (6, 20, 5, 0), (10, 40, 7, 4), (4, 10, 4, 0), (12, 30, 6, 1), (8, 37, 6, 1), (8, 38, 6, 1)]


def index_flags(p):
    return ["-b", str(p[0]), "-L", str(p[1]), "-k", str(p[2]), "-M", str(p[3])]


def index_name(p):
    return "b%dL%dk%dM%d" % tuple(p)


class Point:
    def __init__(self, name, flags, extra=None, prechain=True):
        self.name, self.flags, self.extra, self.prechain = name, flags, extra, prechain

    def apply(self, mo):
        """the point set in mo (golden.apply_flags is the one translator of the reference's flags)"""
        golden.apply_flags(mo, self.flags or [])
        if self.extra:
            self.extra(mo)
        return mo

    def __repr__(self):
        return self.name


def _few_iterations(mo):
    mo.max_chn_iter = 20                        # (mp_mapopt_t::max_chn_iter has no command-line flag)


# prechain: does map.c:186 run the pre-chain at this point (not with --no-pre-chain, not without splicing) -- device seeding
# exists only where it does
CHAIN_POINTS = [
    Point("default", []),
    Point("skip2-w0.2-g200", ["--max-skip", "2", "-w", "0.2", "-g", "200"]),
    Point("n6-m40-c50", ["-n", "6", "-m", "40", "-c", "50"]),
    Point("G2000", ["-G", "2000"]),
    Point("iter20-skip0", ["--max-skip", "0"], _few_iterations),
    Point("no-pre-chain", ["--no-pre-chain"], prechain=False),
    Point("no-splice", ["-S"], prechain=False),
]


def _max_ava(v):
    def f(mo):
        mo.max_ava = v                          # (mp_mapopt_t::max_ava has no command-line flag)
    return f


REFINE_KMERS = [3, 4, 5, 6, 7]
MAX_AVA = [1, 50, 1000, 2**31 - 1]
REFINE_POINTS = [Point("l%d" % k, ["-l", str(k)]) for k in REFINE_KMERS] + [Point("ava%d" % v, None, _max_ava(v)) for v in MAX_AVA]


def chain_args(mo, kmer, bbit, pre):
    """the argument tuple of refbind.ref_chain for the reference's pre-chain call (map.c:188) or its main-chain call (map.c:194)"""
    spl = 0 if (mo.flag & 0x1) else 1
    if pre:
        w = 1 << bbit
        return (w, w, w, mo.max_chn_max_skip, mo.max_chn_iter, 2, 0, mo.chn_coef_log, spl, kmer, bbit)
    return (mo.max_intron, mo.max_gap, mo.bw, mo.max_chn_max_skip, mo.max_chn_iter, mo.min_chn_cnt, mo.min_chn_sc, mo.chn_coef_log, spl, kmer, bbit)


def write_genome(tmp_path, contigs, name="g.fa"):
    """the genome as FASTA (chr1, chr2, ...): Index.from_nt4() cannot take index options, Index.read_fasta() can"""
    fa = os.path.join(str(tmp_path), name)
    gen_synth.write_fasta_nt(fa, contigs)
    return fa


def tandem_genome(seed, gen_seed, genome=3000000, n_prot=40):
    """the genome of tests/test_seed_gpu.py: planted genes plus loci copied several times back to back (long runs of anchors in
    adjacent blocks, many equal chain scores).  Returns (contigs, queries): the proteins, ten of the planted originals and the odd
    queries (unrelated, tiny, chimeric with a repeated domain)."""
    rng = np.random.default_rng(seed)
    contigs, prots, names, planted = gen_synth.generate(genome, 2, n_prot, gen_seed, return_planted=True)
    g = contigs[0]
    for k in range(6):
        src = int(rng.integers(0, len(g) - 20000))
        seg = g[src:src + int(rng.integers(2000, 9000))].copy()
        at = int(rng.integers(0, len(g) - 10 * len(seg)))
        for r in range(int(rng.integers(2, 6))):
            g[at + r * len(seg):at + (r + 1) * len(seg)] = seg
    extra = [b"M" + bytes(rng.choice(list(b"ACDEFGHIKLMNPQRSTVWY"), 300).tolist()), b"MA", bytes(planted[0]) + bytes(planted[1]) + bytes(planted[0])]
    return contigs, list(prots) + [bytes(p) for p in planted[:10]] + extra
