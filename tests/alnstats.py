"""Helpers of the alignment-statistics tests (tests/test_aln_stats_cpu.py, tests/test_aln_stats_gpu.py; MPA_GPU_STATS):
the result arrays of a batch as numpy records with a field-by-field comparison, the inputs of the golden cases, and the edge genome."""
import ctypes as C
import functools
import numpy as np
import miniprot_amd as mpa
from miniprot_amd import synth
import golden

FEAT = np.dtype([("vs", "<i8"), ("ve", "<i8"), ("qs", "<i4"), ("qe", "<i4"), ("type", "<i2"), ("phase", "<i2"), ("n_fs", "<i4"), ("n_stop", "<i4"),
                 ("score", "<i4"), ("n_iden", "<i4"), ("blen", "<i4"), ("donor", "u1", (2,)), ("acceptor", "u1", (2,))], align=True)
assert FEAT.itemsize == 56                                  # sizeof(mpa_feat_t), include/mpamd.h
OPS = "MIDN------FGUV"                                      # CIGAR operation codes (nasw.h)


def result_arrays(res):
    """(hits, feats, cigars) of an mpa.Result, copied out of the library's memory"""
    L = mpa.lib()
    L.mpa_result_feats.restype = C.c_void_p
    L.mpa_result_feats.argtypes = [C.c_void_p]
    n = int(res.n_hit())
    if n == 0:
        return np.zeros(0, mpa.HIT), np.zeros(0, FEAT), np.zeros(0, np.uint32)
    hits = np.frombuffer((C.c_char * (n * mpa.HIT.itemsize)).from_address(L.mpa_result_hits(res.h)), dtype=mpa.HIT).copy()
    n_feat = int((hits["feat_off"] + hits["n_feat"]).max())
    n_cig = int((hits["cigar_off"] + hits["n_cigar"]).max())
    feats = np.frombuffer((C.c_char * (n_feat * FEAT.itemsize)).from_address(L.mpa_result_feats(res.h)), dtype=FEAT).copy() if n_feat else np.zeros(0, FEAT)
    cigars = np.ctypeslib.as_array(L.mpa_result_cigars(res.h), (max(n_cig, 1),))[:n_cig].copy()
    return hits, feats, cigars


def first_difference(a, b):
    """None when two result_arrays() triples are equal field by field; otherwise a sentence that names the first differing hit"""
    ha, fa, ca = a
    hb, fb, cb = b
    if len(ha) != len(hb):
        return "%d hits against %d" % (len(ha), len(hb))
    for k in range(len(ha)):
        x, y = ha[k], hb[k]
        where = "hit %d (query %d, vid %d, vs %d)" % (k, x["qid"], x["vid"], x["vs"])
        for f in mpa.HIT.names:
            if x[f] != y[f]:
                return "%s: %s %d against %d" % (where, f, x[f], y[f])
        if not np.array_equal(ca[x["cigar_off"]:x["cigar_off"] + x["n_cigar"]], cb[y["cigar_off"]:y["cigar_off"] + y["n_cigar"]]):
            return where + ": CIGAR"
        for j in range(int(x["n_feat"])):
            p, q = fa[x["feat_off"] + j], fb[y["feat_off"] + j]
            for f in FEAT.names:
                if not np.array_equal(p[f], q[f]):
                    return "%s: feature %d: %s %s against %s" % (where, j, f, p[f], q[f])
    return None


def coverage(arrays):
    """what a triple holds of the things the statistics pass treats differently: operation kinds, in-frame stops, strands, stop features"""
    hits, feats, cigars = arrays
    ops = set(OPS[int(c) & 0xf] for c in np.unique(cigars & 0xf))
    return {"ops": ops, "n_stop": bool((hits["n_stop"] > 0).any()), "reverse": bool((hits["vid"][hits["has_aln"] != 0] & 1).any()),
            "stop_feature": bool((feats["type"] == 1).any())}


def case_inputs(name, tmp_path=None):
    """(index, map options, queries, golden text) of a golden case: a synthetic case of golden.SYNTH_CASES, or "long_u" (tests/longprot.py)"""
    if name == "long_u":
        import longprot
        c = longprot.case()
        contigs, prots, names, mo, header = c["contigs"], c["prots"], c["names"], longprot.mapopt(), b""
        case = None
    else:
        case = [c for c in golden.SYNTH_CASES if c["name"] == name][0]
        contigs, prots, names = golden.synth_inputs(case)
        mo, header = golden.mapopt_for(case), golden.file_header(case)
    idx = mpa.Index.from_nt4(contigs, ["chr%d" % (i + 1) for i in range(len(contigs))])
    mpa._check(mpa.lib().mpa_idx_build_kmers(idx.h, 4))
    if case is not None and "spsc" in case:
        idx.set_spsc(golden.write_spsc(case, contigs, str(tmp_path / "spsc.tsv")), mo)
    ref = open(golden.path(name + ".ref.paf"), "rb").read()
    assert ref.startswith(header)
    return idx, mo, mpa.Queries(prots, names), ref[len(header):]


# ---- the edge genome: contigs that begin d bases before their first planted gene and end e bases behind their last ------------
EDGE_GENOME, EDGE_CTG, EDGE_PROT, EDGE_SEED = 300000, 2, 12, 4242


@functools.lru_cache(maxsize=1)
def _edge_base():
    """the untrimmed genome (5 % N in runs, 2 % pseudo-paralogs), its proteins, and [start, end) of every planted gene per contig"""
    seen = []
    plain = synth.add_paralogs

    def spy(contigs, genes, slot, frac, seed):                # (the generator hands its list of planted genes to this step only)
        seen.extend(genes)
        return plain(contigs, genes, slot, frac, seed)
    synth.add_paralogs = spy
    try:
        contigs, prots, names, planted = synth.generate(EDGE_GENOME, EDGE_CTG, EDGE_PROT, EDGE_SEED, imax=3000, n_frac=0.05, paralog_frac=0.02, return_planted=True)
    finally:
        synth.add_paralogs = plain
    assert len(seen) == EDGE_PROT
    span = []
    for ci in range(EDGE_CTG):
        mine = [(st, st + ln) for c, st, ln, _ in seen if c == ci]
        span.append((min(s for s, _ in mine), max(e for _, e in mine)))
    return contigs, [bytes(p) for p in prots], list(names), span


def edge_genome(d, e):
    """(contigs, proteins, names): every contig trimmed to d bases before its first planted gene and e bases after its last.  At
    d = 0 a forward gene's start codon is the contig's first codon (dist_start meets the window's first codon) and a reverse gene's
    stop codon its strand's last (dist_stop reaches the contig end); the donor / acceptor bases next to an edge are '.'; the N runs
    and the mutated queries give ambiguous codons."""
    contigs, prots, names, span = _edge_base()
    return [np.ascontiguousarray(c[s - d:t + e]) for c, (s, t) in zip(contigs, span)], prots, names
