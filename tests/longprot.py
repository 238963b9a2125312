"""One deterministic case with LONG proteins for the device refinement (tests/test_refine_long_*.py, tools/make_golden.py long).

The refinement keeps a query's distinct k = kmer2 k-mers ("groups", about one per residue) in a map: in LDS up to 2 048 groups (three
size classes), in device memory beyond.  The case puts queries on both sides of every limit into one batch:

  genome     4 Mbp, one contig, gen_synth.generate() with 72 planted genes (introns of at most 3 000 bases).  The first 24 proteins
             (the first third of the contig) are the ORDINARY queries; the rest of the contig takes the long genes, planted with
             make_gene(..., imax=3000) one after the other, so that every locus stays far below the 2^22 bases a refinement window
             may have on the device.
  long ones  group counts at -l 5 of exactly 2 048 (the last LDS class: the control) and 2 049, about 3 000, 9 000 and 20 000; exactly
             4 096 and 4 097 k-mers (the limit of the scan-only fallback's LDS set); one with an internal duplication of 300 residues
             (groups with two query positions); one with X and * inside (the k-mer run starts again behind them).
             Exact counts are reached by trimming residues from the query's end; the counts come from groups() below, a restatement
             of the library's query_groups() over the library's own reduced alphabet (ns_tab_aa13).
  order      ordinary and long queries interleaved, so that a 3-batch stream has long queries in every batch.

Everything derives from fixed seeds; the reference's output for it is tests/golden/long_u.ref.paf."""
import ctypes as C
import functools
import os
import sys
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tools"))
import gen_synth  # noqa: E402
from miniprot_amd import synth  # noqa: E402  (gen_synth is its command-line front; _codons is not among the names it re-exports)

GENOME, N_PLANTED, N_ORDINARY, SEED = 4000000, 72, 24, 611
KMER2 = 5
FLAGS = ["-u"]
# name -> (what is exact, target); "g" = groups at -l 5, "k" = k-mers (all of them, not the distinct ones)
LONG = [("g2048", "g", 2048), ("g2049", "g", 2049), ("g3000", "g", 3000), ("k4096", "k", 4096), ("k4097", "k", 4097), ("g9000", "g", 9000),
        ("g20000", "g", 20000), ("dup300", "g", 2700), ("xstar", "g", 2600)]
EXACT = ("g2048", "g2049", "k4096", "k4097")


def aa13():
    """the library's reduced alphabet (4-bit code per residue letter; 14 = '*', 15 = 'X' and everything unknown)"""
    import miniprot_amd as mpa
    return np.frombuffer(bytes((C.c_uint8 * 256).in_dll(mpa.lib(), "ns_tab_aa13")), np.uint8)


def kmer_words(prot, k=KMER2, tab=None):
    """the packed word of the k-mer ending at every residue that ends one (query_groups(), host_plan.cpp: a residue with a code of 14
    or more starts the run again), in query order"""
    tab = aa13() if tab is None else tab
    mask = (1 << 4 * k) - 1
    out, w, run = [], 0, 0
    for ch in prot:
        c = int(tab[ch])
        if c >= 14:
            w = run = 0
            continue
        w = (w << 4 | c) & mask
        run += 1
        if run >= k:
            out.append(w)
    return out


def groups(prot, k=KMER2, tab=None):
    """distinct k-mers of a query = the groups of the device refinement (its hash is a bijection on the masked words)"""
    return len(set(kmer_words(prot, k, tab)))


def _trim_to(prot, what, target, tab):
    """the longest prefix of prot with exactly `target` groups ("g") or k-mers ("k")"""
    words = kmer_words(prot, KMER2, tab)
    assert len(words) == len(prot) - (KMER2 - 1), "the protein has residues outside the alphabet"
    if what == "k":
        n = target
    else:
        seen, n = set(), 0
        for i, w in enumerate(words):                       # n = k-mers of the longest prefix with `target` distinct words
            seen.add(w)
            if len(seen) > target:
                break
            n = i + 1
        assert len(seen) >= target, "planted protein too short for %d groups" % target
    return prot[:n + KMER2 - 1]


@functools.lru_cache(maxsize=1)
def case():
    """-> dict(contigs, prots, names, long = {name: index into prots}, loci = {name: (vid, strand-local start, length)}, ordinary = [indices])"""
    tab = aa13()
    contigs, prots, names = gen_synth.generate(GENOME, 1, N_PLANTED, SEED, imax=3000)
    g = contigs[0]
    ordinary = [bytes(p) for p in prots[:N_ORDINARY]]
    ord_names = names[:N_ORDINARY]
    rng = np.random.default_rng([SEED, 2049])
    at = GENOME // 3 + 20000                                   # behind the ordinary genes' slots
    long_p, loci = {}, {}
    for li, (name, what, target) in enumerate(LONG):
        if name == "dup300":
            base, _ = gen_synth.make_gene(rng, target - 300, 7.5, 1.5, 70, 3000)
            planted = np.concatenate([base[:900], base[400:700], base[900:]])     # residues 400..700 once more behind residue 900
            # (the gene is re-drawn for the planted protein: single codon draw per residue, introns as make_gene places them)
            planted, gene = _gene_for(rng, planted)
        else:
            n_res = int(target * 1.06) + 80 if what == "g" else target + 40
            planted, gene = gen_synth.make_gene(rng, n_res, 7.5, 1.5, 70, 3000)
        if name == "dup300":                                   # the repeat's two copies mutate together: the QUERY has every k-mer of it twice
            m = [gen_synth.mutate(rng, base[a:b]) for a, b in ((0, 400), (400, 700), (700, 900), (900, len(base)))]
            q = m[0] + m[1] + m[2] + m[1] + m[3]
        else:
            q = gen_synth.mutate(rng, planted)
        if name == "xstar":
            q = bytearray(q)
            for p, ch in ((300, b"X"), (301, b"X"), (1200, b"*"), (1900, b"X"), (2300, b"*")):
                q[p] = ch[0]
            q = bytes(q)
        elif name != "dup300":
            q = _trim_to(q, what, target, tab)
        rev = li % 2 == 1
        seg = gen_synth.COMP[gene[::-1]] if rev else gene
        assert at + len(seg) + 20000 < GENOME, "the long genes do not fit into the contig"
        g[at:at + len(seg)] = seg
        loci[name] = (1 if rev else 0, GENOME - at - len(seg) if rev else at, len(seg))
        long_p[name] = q
        at += len(seg) + 20000
    # interleave: three ordinary queries, one long one, ...; the ordinary ones that are left at the end
    out_p, out_n, where, ord_idx = [], [], {}, []
    longs = list(long_p.items())
    for i in range(N_ORDINARY):
        ord_idx.append(len(out_p))
        out_p.append(ordinary[i]), out_n.append(ord_names[i])
        if i % 2 == 1 and longs:
            name, q = longs.pop(0)
            where[name] = len(out_p)
            out_p.append(q), out_n.append("long_" + name)
    assert not longs
    return {"contigs": contigs, "prots": out_p, "names": out_n, "long": where, "loci": loci, "ordinary": ord_idx}


def _gene_for(rng, prot):
    """a gene for a GIVEN protein, built as make_gene() builds one for a protein it draws: codons, a stop, exons cut by GT..AG introns
    of at most 3 000 bases"""
    length = len(prot)
    cds = np.empty(3 * length + 3, dtype=np.uint8)
    synth._codons(rng, prot, cds)
    cds[3 * length:] = gen_synth.STOPS[rng.integers(len(gen_synth.STOPS))]
    cuts = sorted(rng.choice(np.arange(20, len(cds) - 20), int(rng.integers(4, length // 60)), replace=False).tolist())
    parts, prev = [], 0
    for c in cuts:
        parts.append(cds[prev:c])
        intron = rng.integers(0, 4, int(np.clip(rng.lognormal(7.5, 1.5), 70, 3000))).astype(np.uint8)
        intron[0:2], intron[2], intron[-2:], intron[-3] = (2, 3), rng.choice([0, 2]), (0, 2), rng.choice([1, 3])
        parts.append(intron)
        prev = c
    parts.append(cds[prev:])
    return prot, np.concatenate(parts)


def ordinary_locus(name, span=30000):
    """(vid, strand-local start, length) of a window that covers the planted gene of an ordinary query (its name carries strand and
    start; with introns of at most 3 000 bases a gene of these proteins is shorter than `span`)"""
    _, _, strand, start = name.split("_")
    start = max(int(start) - 200, 0)
    end = min(start + span, GENOME)
    return (1, GENOME - end, end - start) if strand == "-" else (0, start, end - start)


def mapopt(kmer2=KMER2):
    import miniprot_amd as mpa
    mo = mpa.default_mapopt()
    mo.flag |= 0x4                                             # -u
    mo.kmer2 = kmer2
    return mo
