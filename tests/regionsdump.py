"""MPA_REGIONS_DUMP=<file>: what the first planning step (main chains -> regions -> refinement windows) left for every query, whichever
path produced it -- the host functions of host_regions.cpp, the shared core on the host (MPA_GPU_REGIONS=model) or k_regions on the
device (MPA_GPU_REGIONS=1).  This is how the tests see the stage without an exported symbol.

Layout (little endian, appended batch after batch, inside a batch in query order):
    per query   int32 qid, int32 chains before the selection, int32 n
                n records of 64 bytes: int32 cnt, id, parent, n_sub, subsc, chn_sc, chn_sc_ungap; uint32 vid; int32 qs, qe;
                                       int64 vs, ve; int32 split (0: the chain lay on one strand, 1: it spanned two strands or contigs
                                       and its head was kept, 2: its tail was kept); int32 0
                n limits: uint64 left << 32 | right (how far the refinement window reaches beyond the region)
"""
import numpy as np

HEAD = np.dtype([("qid", "<i4"), ("n_chains", "<i4"), ("n", "<i4")])
REC = np.dtype([("cnt", "<i4"), ("id", "<i4"), ("parent", "<i4"), ("n_sub", "<i4"), ("subsc", "<i4"), ("chn_sc", "<i4"), ("chn_sc_ungap", "<i4"), ("vid", "<u4"),
                ("qs", "<i4"), ("qe", "<i4"), ("vs", "<i8"), ("ve", "<i8"), ("split", "<i4"), ("pad", "<i4")])
assert HEAD.itemsize == 12 and REC.itemsize == 64


def parse(data):
    """[(qid, chains before the selection, records, limits)] in file order"""
    out, at = [], 0
    while at < len(data):
        h = np.frombuffer(data, HEAD, 1, at)[0]
        at += HEAD.itemsize
        n = int(h["n"])
        rec = np.frombuffer(data, REC, n, at).copy()
        at += n * REC.itemsize
        ext = np.frombuffer(data, "<u8", n, at).copy()
        at += n * 8
        out.append((int(h["qid"]), int(h["n_chains"]), rec, ext))
    assert at == len(data), "a truncated dump"
    return out


def read(path):
    with open(path, "rb") as f:
        return f.read()


def first_difference(a, b):
    """None when two dumps (bytes) are equal; otherwise a sentence that names the first differing query and field"""
    if a == b:
        return None
    pa, pb = parse(a), parse(b)
    if len(pa) != len(pb):
        return "%d queries against %d" % (len(pa), len(pb))
    for k, ((qa, ca, ra, ea), (qb, cb, rb, eb)) in enumerate(zip(pa, pb)):
        if (qa, ca, len(ra)) != (qb, cb, len(rb)):
            return "entry %d: (qid, chains, regions) %s against %s" % (k, (qa, ca, len(ra)), (qb, cb, len(rb)))
        for i in range(len(ra)):
            for f in REC.names:
                if ra[i][f] != rb[i][f]:
                    return "entry %d (query %d), region %d: %s %d against %d" % (k, qa, i, f, ra[i][f], rb[i][f])
            if ea[i] != eb[i]:
                return "entry %d (query %d), region %d: limits %#x against %#x" % (k, qa, i, ea[i], eb[i])
    return "the bytes differ, the parsed fields do not"
