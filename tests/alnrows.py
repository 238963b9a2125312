"""Helpers of the residue-row tests (MPA_GPU_ROWS; miniprot_amd/csrc/aln_rows_core.h): a parser that cuts the five row kinds of --aln /
--trans out of an output text, the `rows carried / built` counts of the formatter's note, what a text holds of the things the walk
treats differently, and the extra inputs the golden cases lack."""
import re
import numpy as np
import miniprot_amd as mpa

KINDS = (b"ATN", b"ATA", b"AAS", b"AQA", b"STA")
ALN, TRANS = 0x80, 0x100                                   # MPA_MF_SHOW_RESIDUE, MPA_MF_SHOW_TRANS (include/mpamd.h)


def rows(text):
    """{kind: [row bodies in text order]} for the five kinds"""
    out = {k: [] for k in KINDS}
    for line in text.split(b"\n"):
        if line.startswith(b"##") and line[2:5] in out and line[5:6] == b"\t":
            out[line[2:5]].append(line[6:])
    return out


def row_sets(text):
    """how many alignments of a text print rows (an alignment prints ##ATN, ##STA or both)"""
    r = rows(text)
    n_atn, n_sta = len(r[b"ATN"]), len(r[b"STA"])
    assert n_atn == len(r[b"ATA"]) == len(r[b"AAS"]) == len(r[b"AQA"])
    assert n_atn == 0 or n_sta == 0 or n_atn == n_sta
    for a, b, c, d in zip(r[b"ATN"], r[b"ATA"], r[b"AAS"], r[b"AQA"]):
        assert len(a) == len(b) == len(c) == len(d), "rows of unequal width"
    return max(n_atn, n_sta)


def format_counts(err):
    """(carried, built) summed over the format notes of a stderr text; None when no note counts rows"""
    m = re.findall(r"format output\s+[0-9.]+ ms\s+cs carried \d+, built \d+; rows carried (\d+), built (\d+)", err)
    if not m:
        return None
    return sum(int(a) for a, _ in m), sum(int(b) for _, b in m)


def kinds(text):
    """what a text's rows hold of the things the walk treats differently (counts)"""
    r = rows(text)
    atn, ata, sta = r[b"ATN"], r[b"ATA"], r[b"STA"]
    return {"abridged": sum(len(re.findall(rb"~[0-9]+~", x)) for x in atn),
            "whole": sum(len(re.findall(rb"(?<![a-z~])[a-z]+(?![a-z~])", x)) for x in atn),
            "!": sum(x.count(b"!") for x in ata), "$": sum(x.count(b"$") for x in ata),
            "sta_stop": sum(x.endswith(b"*") for x in sta), "sta_open": sum(not x.endswith(b"*") for x in sta),
            "N": sum(x.count(b"N") for x in atn), "n": sum(x.count(b"n") for x in atn)}


def index_of(contigs):
    idx = mpa.Index.from_nt4(contigs, ["chr%d" % (i + 1) for i in range(len(contigs))])
    mpa._check(mpa.lib().mpa_idx_build_kmers(idx.h, 4))
    return idx


def rows_mapopt(flank=None):
    """the default options with -u --aln --trans"""
    mo = mpa.default_mapopt()
    mo.flag |= 0x4 | ALN | TRANS
    if flank is not None:
        mo.max_intron_flank = flank
    return mo


def planted_n():
    """(index, options, queries): csdump.planted_n_genome() with --aln --trans -- N in ATN rows and X in the translation"""
    import csdump
    contigs, prots, names = csdump.planted_n_genome()
    return index_of(contigs), rows_mapopt(), mpa.Queries(prots, names)


def edge(d, e):
    """(index, options, queries): alnstats.edge_genome(d, e) with --aln --trans"""
    import alnstats
    contigs, prots, names = alnstats.edge_genome(d, e)
    return index_of(contigs), rows_mapopt(), mpa.Queries(prots, names)


def trimmed_edge(cut):
    """(index, options, queries): the edge genome trimmed `cut` bases INTO its contigs' outermost genes (their stop codons on the
    strand that ends there): alignments that end fewer than three bases before their strand's end, so print no trailing codon and an
    ##STA row without a '*'.  alnstats.edge_genome(d, e) with d, e >= 0 puts none there: the stop codon is still inside the contig."""
    return edge(-cut, -cut)


def near_end(text):
    """printed alignments of a text whose end is fewer than three bases before their strand's end (ve + 3 beyond the contig)"""
    n = 0
    for line in text.split(b"\n"):
        f = line.split(b"\t")
        if len(f) > 12 and not line.startswith(b"##") and f[4] in (b"+", b"-") and f[5] != b"*":
            ln, st, en = int(f[6]), int(f[7]), int(f[8])
            n += (ln - en < 3) if f[4] == b"+" else (st < 3)
    return n


def low_frameshift(case_inputs, name="syn_k", fs=4):
    """(index, options, queries) of a golden input with --aln --trans and the frameshift penalty lowered to `fs`, at which the
    aligner opens frameshift matches ('$' rows) as well as frameshift deletions ('!')"""
    import ctypes as C
    idx, mo, q, _ = case_inputs(name)
    mo.flag |= 0x4 | ALN | TRANS
    mpa.lib().mpa_mapopt_set_fs(C.byref(mo), fs)
    return idx, mo, q
