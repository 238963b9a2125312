"""Inputs of the regions tests (tests/test_regions_cpu.py, tests/test_regions_gpu.py; MPA_GPU_REGIONS): the golden cases by name,
runs with the dump of tests/regionsdump.py switched on, and the edge genome.

The edge genome (about 500 kbp, four contigs, built from a seed) holds what the golden genomes do not:
  * chains that span two strands.  In block space the strands follow each other -- contig 0 forward, contig 0 reverse, contig 1
    forward, ... -- so a gene whose first half ends the forward strand of a contig and whose second half starts that contig's reverse
    strand (contig = filler + coding(P1) + revcomp(coding(P2))) chains across the strand boundary; with |P1| > |P2| the head of the
    chain is its larger part, with |P1| < |P2| the tail.  The same across a contig boundary: a contig's reverse strand ends with the
    reverse complement of its start, the next contig's forward strand follows (contig k = revcomp(coding(P1)) + ..., contig k + 1 =
    coding(P2) + ...).
  * a family of FAMILY identical copies of one gene with identical 2 kb flanks: mapped with -N 100 --outn=100 -p 0.1 its query has
    more than 64 chains of equal score, so the order of the regions is the tie order of the reference's radix passes.
"""
import os
import numpy as np
import miniprot_amd as mpa
import golden
import seedopts
import regionsdump

CODON = {"A": "GCT", "C": "TGT", "D": "GAT", "E": "GAA", "F": "TTT", "G": "GGT", "H": "CAT", "I": "ATT", "K": "AAA", "L": "CTG", "M": "ATG",
         "N": "AAT", "P": "CCT", "Q": "CAA", "R": "CGT", "S": "TCT", "T": "ACT", "V": "GTT", "W": "TGG", "Y": "TAT"}
NT = {"A": 0, "C": 1, "G": 2, "T": 3}
FAMILY = 84
EDGE_FLAGS = ["-N", "100", "--outn=100", "-p", "0.1", "-u"]   # the reference's command line for tests/golden/regions_edge.ref.paf
EDGE_REF = "regions_edge.ref.paf"


def case_inputs(name, tmp_path):
    """(index, map options, queries, golden text) of a golden case: golden.SYNTH_CASES or golden.OPTION_CASES (index options through a FASTA)"""
    case = [c for c in golden.SYNTH_CASES + golden.OPTION_CASES if c["name"] == name][0]
    contigs, prots, names = golden.synth_inputs(case)
    if "idx" in case:
        idx = mpa.Index.read_fasta(seedopts.write_genome(tmp_path, contigs, name + ".fa"), case["idx"])
    else:
        idx = mpa.Index.from_nt4(contigs, ["chr%d" % (i + 1) for i in range(len(contigs))])
    mpa._check(mpa.lib().mpa_idx_build_kmers(idx.h, 4))
    ref = open(golden.path(name + ".ref.paf"), "rb").read()
    return idx, golden.mapopt_for(case), mpa.Queries(prots, names), ref


def with_dump(monkeypatch, path, run):
    """run() with MPA_REGIONS_DUMP=path (a fresh file); returns (what run() returned, the dump's bytes)"""
    if os.path.exists(path):
        os.remove(path)
    monkeypatch.setenv("MPA_REGIONS_DUMP", path)
    try:
        out = run()
    finally:
        monkeypatch.delenv("MPA_REGIONS_DUMP")
    return out, regionsdump.read(path)


# ---- the edge genome ----------------------------------------------------------------------------------
def _coding(prot):
    return np.array([NT[c] for a in prot.decode() for c in CODON[a]], np.uint8)


def _revcomp(nt):
    return (3 - nt[::-1]).astype(np.uint8)


def _protein(rng, n):
    return b"M" + bytes(rng.choice(list(b"ACDEFGHIKLMNPQRSTVWY"), n - 1).tolist())


def edge_genome():
    """(contigs, proteins, names, mapopt)"""
    rng = np.random.default_rng(20261)
    fill = lambda n: rng.integers(0, 4, n).astype(np.uint8)
    big, small = 300, 120                                                    # residues of the larger and of the smaller part of a split gene
    s_head, s_tail = _protein(rng, big + small), _protein(rng, big + small)  # across a strand boundary: the head / the tail is the larger part
    b_head, b_tail = _protein(rng, big + small), _protein(rng, big + small)  # across a contig boundary
    fam = _protein(rng, 260)
    unit = np.concatenate([fill(2000), _coding(fam), fill(2000)])           # one copy with its flanks
    singles = [_protein(rng, 300) for _ in range(6)]
    planted = lambda ps: [np.concatenate([_coding(p) if k % 2 == 0 else _revcomp(_coding(p)), fill(3000)]) for k, p in enumerate(ps)]
    # contig 0: its reverse strand ends with the head of b_head, its forward strand with the head of s_head and, reversed, s_head's tail
    c0 = np.concatenate([_revcomp(_coding(b_head[:big])), fill(15000)] + planted(singles[:3]) + [fill(20000), _coding(s_head[:big]), _revcomp(_coding(s_head[big:]))])
    c1 = np.concatenate([_coding(b_head[big:]), fill(12000)] + planted(singles[3:]) + [fill(9000)])
    c2 = np.concatenate([_revcomp(_coding(b_tail[:small])), fill(18000), _coding(s_tail[:small]), _revcomp(_coding(s_tail[small:]))])
    c3 = np.concatenate([_coding(b_tail[small:]), fill(4000)] + [unit] * FAMILY + [fill(3000)])
    prots = [s_head, s_tail, b_head, b_tail, fam] + singles
    names = ["strand_head", "strand_tail", "ctg_head", "ctg_tail", "family"] + ["single%d" % i for i in range(len(singles))]
    mo = golden.apply_flags(mpa.default_mapopt(), ["-N", "100", "-p", "0.1", "-u"])
    mo.out_n = 100                                                           # --outn=100
    return [np.ascontiguousarray(c) for c in (c0, c1, c2, c3)], prots, names, mo


def edge_index(contigs):
    idx = mpa.Index.from_nt4(contigs, ["chr%d" % (i + 1) for i in range(len(contigs))])
    mpa._check(mpa.lib().mpa_idx_build_kmers(idx.h, 4))
    return idx


def edge_findings(dump):
    """what the dump of the edge genome's batch shows of the things it was built for: (split flags seen, the largest number of chains
    of a query before the selection, the largest number of kept regions of one query that share a chn_sc)"""
    flags, most, ties = set(), 0, 0
    for _, n_chains, rec, _ in regionsdump.parse(dump):
        flags |= set(int(x) for x in rec["split"] if x)
        most = max(most, n_chains)
        if len(rec):
            ties = max(ties, int(np.unique(rec["chn_sc"], return_counts=True)[1].max()))
    return flags, most, ties
