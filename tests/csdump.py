"""MPA_CS_DUMP=<file>: the body of the cs:Z: string (what follows "cs:Z:") of every aligned region a batch keeps, whichever path produced
it -- the formatter's walk (put_cs_body, host_format.cpp; MPA_GPU_CS unset), the shared core on the host (MPA_GPU_CS=model) or k_aln_cs
on the device (MPA_GPU_CS=1).  This is how the tests see the step without an exported symbol.

Layout (little endian, appended batch after batch, inside a batch in query and region order, behind stage_finish):
    per region  40 bytes: int32 query number, vid; int64 vs, ve; int32 qs, qe, source (0 host, 1 shared core, 2 device), length
                then `length` bytes: the body
"""
import re
import numpy as np

HEAD = np.dtype([("qid", "<i4"), ("vid", "<i4"), ("vs", "<i8"), ("ve", "<i8"), ("qs", "<i4"), ("qe", "<i4"), ("src", "<i4"), ("len", "<i4")])
assert HEAD.itemsize == 40


def parse(data):
    """[(head record, body bytes)] in file order"""
    out, at = [], 0
    while at < len(data):
        h = np.frombuffer(data, HEAD, 1, at)[0].copy()
        at += HEAD.itemsize
        n = int(h["len"])
        assert n >= 0 and at + n <= len(data), "a truncated dump"
        out.append((h, bytes(data[at:at + n])))
        at += n
    return out


def read(path):
    with open(path, "rb") as f:
        return f.read()


def first_difference(a, b, src_a=None, src_b=None):
    """None when two parsed dumps name the same regions with the same bodies (and every record of a / b has source src_a / src_b, where
    given); otherwise a sentence that names the first differing record"""
    if len(a) != len(b):
        return "%d records against %d" % (len(a), len(b))
    for k, ((ha, ba), (hb, bb)) in enumerate(zip(a, b)):
        where = "record %d (query %d, vid %d, vs %d)" % (k, ha["qid"], ha["vid"], ha["vs"])
        for f in ("qid", "vid", "vs", "ve", "qs", "qe"):
            if ha[f] != hb[f]:
                return "%s: %s %d against %d" % (where, f, ha[f], hb[f])
        if src_a is not None and ha["src"] != src_a:
            return "%s: source %d, not %d" % (where, ha["src"], src_a)
        if src_b is not None and hb["src"] != src_b:
            return "%s: source %d, not %d" % (where, hb["src"], src_b)
        if ba != bb:
            i = next((i for i, (x, y) in enumerate(zip(ba, bb)) if x != y), min(len(ba), len(bb)))
            return "%s: bodies of %d and %d bytes differ at byte %d: %r against %r" % (where, len(ba), len(bb), i, ba[max(0, i - 12):i + 12], bb[max(0, i - 12):i + 12])
    return None


def kinds(bodies):
    """what a list of bodies holds of the things the walk treats differently (counts)"""
    c = {"mismatch": 0, "insertion": 0, "deletion": 0, "intron": 0, "star1": 0, "star2": 0, "run100": 0, "n": 0}
    for b in bodies:
        c["mismatch"] += len(re.findall(rb"\*[acgtn]{3}[A-Z*]", b))
        c["insertion"] += b.count(b"+")
        c["deletion"] += b.count(b"-")                      # (D and F operations, and the tail of a split codon behind an intron)
        c["intron"] += b.count(b"~")
        c["star1"] += len(re.findall(rb"\*[acgtn][A-Z*]", b))
        c["star2"] += len(re.findall(rb"\*[acgtn]{2}[A-Z*]", b))
        c["run100"] += len(re.findall(rb":[0-9]{3,}", b))
        c["n"] += b.count(b"n")
    return c


def format_counts(err):
    """(carried, built) summed over the format notes of a stderr text"""
    m = re.findall(r"format output\s+[0-9.]+ ms\s+cs carried (\d+), built (\d+)", err)
    assert m, "no format note with cs counts:\n" + err[-400:]
    return sum(int(a) for a, _ in m), sum(int(b) for _, b in m)


def planted_n_genome():
    """(contigs, proteins, names): two exact genes, one per strand, with an N planted into four codons of each -- alignments that run
    across ambiguous bases, which neither the golden cases nor the edge genome of the statistics tests hold: "*nctA" and ":n" around it"""
    import regioncases
    rng = np.random.default_rng(77)
    prots = [regioncases._protein(rng, 180), regioncases._protein(rng, 150)]
    genes = [regioncases._coding(prots[0]), regioncases._revcomp(regioncases._coding(prots[1]))]
    for g in genes:
        for at in (60, 61 + 3 * 20, 62 + 3 * 50, 3 * 100):
            g[at] = 4
    fill = lambda n: rng.integers(0, 4, n).astype(np.uint8)
    contig = np.concatenate([fill(3001), genes[0], fill(4000), genes[1], fill(2502)])
    return [np.ascontiguousarray(contig)], prots, ["fwd", "rev"]
