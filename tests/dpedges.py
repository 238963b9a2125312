"""DP calls at the edges of a call's inputs (tests/test_dp_edges_cpu.py, tests/test_dp_edges_gpu.py): windows of fewer than three rows,
slices of longer queries, windows at contig and buffer ends, query bytes outside the amino-acid alphabet.  Pure numpy, no device.

place() lays windows out by EXPLICIT placements -- contig, strand, where on the strand the window lies, which slices of which query it
is aligned with -- where dputil.build_workload draws all of that.  Every family is a function of its seed alone and returns a Case; a
Case is built once per process (case()) and never modified."""
import ctypes as C
import numpy as np
import miniprot_amd as mpa
import refbind
from dpgen import AA, make_task, long_window
from dputil import COMP

EDGES = (1, 7, 8, 9, 16, 17, 32, 33, 64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 1100)   # al on each side of every class boundary
TINY_EXT_AL = (8, 24, 50, 100, 200, 400, 800, 1100)    # one al per extension class: 16 / 32 / 64 lanes, 128, 256, 512, 1024 columns, the int32 sweep
FLAG = {"cigar": mpa.F_CIGAR, "left": mpa.F_EXT_LEFT, "right": mpa.F_EXT_RIGHT}
MODES = ("cigar", "left", "right")
SS_SKIP0 = 8                                            # MPA_F_SS_SKIP0


class Case:
    """contigs, queries, tasks, meta as build_workload returns them; meta[k] = (pair, flag without MPA_F_SS_SKIP0, io, aa_off, al);
    windows[pair] = the window's bases in strand order; query_seqs[qid] = the whole query"""

    def __init__(self, contigs, query_seqs, tasks, meta, windows):
        self.contigs, self.query_seqs, self.tasks, self.meta, self.windows = contigs, query_seqs, tasks, meta, windows
        self.queries = mpa.Queries(query_seqs)

    def calls(self):
        """per task (window, the slice the expectation is computed on)"""
        return [(self.windows[p], self.query_seqs[int(t["qid"])][a:a + n]) for t, (p, fl, io, a, n) in zip(self.tasks, self.meta)]

    def meta3(self):
        """meta for dputil.compare() over calls(): (task, flag, io)"""
        return [(k, fl, io) for k, (p, fl, io, a, n) in enumerate(self.meta)]

    def tiny_ext(self):
        """the extension calls of fewer than three rows: the reference fails its own assertion on them (nasw-sse.c:441)"""
        return [k for k, t in enumerate(self.tasks) if (int(t["flag"]) & (mpa.F_EXT_LEFT | mpa.F_EXT_RIGHT)) and int(t["nl"]) < 3]

    def ctg_len(self):
        return [len(c) for c in self.contigs]

    def q_off(self):
        return self.queries.off.copy()


class PrefixedQueries:
    """the same batch passed as a slice of a larger buffer: `pad` bytes that belong to no query in front, q_off[0] = pad"""

    def __init__(self, queries, pad=37):
        self.buf = bytes(((7 * k + 3) % 251) + 1 for k in range(pad)) + queries.buf
        self.off = queries.off + pad
        self.c = mpa.QBatch(len(queries.seqs), self.buf, self.off.ctypes.data_as(C.POINTER(C.c_int64)))


def place(pairs, query_seqs, rng, io=29, contigs=None, n_ctg=3):
    """pairs: dicts with
         ctg, rev     the contig and the strand
         where        "start" / "end": the window begins at strand position `shift` / ends `shift` bases before the strand's end
                      (shift 0: it starts / ends the contig); "whole": it is the contig; "inside": anywhere else
         qid, slices  the query and a list of (aa_off, al, mode[, extra flag bits]) slices of it, one task each
       and either nt (the window, in strand order: the contigs are assembled from the windows, with spacers of 1..29 bases around
       the "inside" ones) or, with `contigs` given, nl and shift: the window is cut out of the contig ("inside": at strand position st).
    Returns a Case."""
    if contigs is None:
        head, tail, mid = {}, {}, {}
        for k, p in enumerate(pairs):
            w, c = p["where"], p["ctg"]
            assert p.get("shift", 0) == 0, "assembled contigs: windows start, end or are a contig, or lie inside"
            fwd_first = w == "whole" or (w == "start") != bool(p["rev"])     # first in the forward contig
            if w == "inside":
                mid.setdefault(c, []).append(k)
            if w in ("start", "end", "whole"):
                d = head if fwd_first else tail
                assert c not in d and not (w == "whole" and (c in tail or c in mid)), "two windows claim the same end of contig %d" % c
                d[c] = k
                if w == "whole":
                    tail[c] = k
        parts, pos = [[] for _ in range(n_ctg)], [0] * n_ctg
        fwd_at = {}

        def put(c, k):
            arr = np.frombuffer(pairs[k]["nt"], dtype=np.uint8)
            parts[c].append(COMP[arr[::-1]] if pairs[k]["rev"] else arr)
            fwd_at[k] = pos[c]
            pos[c] += len(arr)

        def spacer(c):
            gap = rng.integers(0, 4, int(rng.integers(1, 30))).astype(np.uint8)
            parts[c].append(gap)
            pos[c] += len(gap)

        for c in range(n_ctg):
            assert not (c in mid and c in head and head[c] == tail.get(c)), "contig %d is one window and holds others" % c
            if c in head:
                put(c, head[c])
            if c in head and c in tail and head[c] == tail[c]:
                continue
            for k in mid.get(c, []):
                spacer(c)
                put(c, k)
            if c in mid or c not in head:
                spacer(c)
            if c in tail:
                put(c, tail[c])
        contigs = [np.concatenate(x) for x in parts]
        st_of = {k: (len(contigs[pairs[k]["ctg"]]) - (f + len(pairs[k]["nt"])) if pairs[k]["rev"] else f) for k, f in fwd_at.items()}
        windows = [p["nt"] for p in pairs]
    else:
        st_of, windows = {}, []
        for k, p in enumerate(pairs):
            L, nl, sh = len(contigs[p["ctg"]]), p["nl"], p.get("shift", 0)
            st = {"start": sh, "end": L - sh - nl, "whole": 0, "inside": p.get("st", 0)}[p["where"]]
            assert 0 <= st and st + nl <= L and (p["where"] != "whole" or nl == L)
            st_of[k] = st
            strand = COMP[contigs[p["ctg"]][::-1]] if p["rev"] else contigs[p["ctg"]]
            windows.append(bytes(strand[st:st + nl]))
    tasks, meta = [], []
    for k, p in enumerate(pairs):
        for s in p["slices"]:
            aa_off, al, mode = s[:3]
            assert 0 <= aa_off and al >= 1 and aa_off + al <= len(query_seqs[p["qid"]])
            fl = FLAG[mode]
            tasks.append((st_of[k], p["ctg"] << 1 | p["rev"], len(windows[k]), p["qid"], aa_off, al, fl | (s[3] if len(s) > 3 else 0), io, len(tasks)))
            meta.append((k, fl, io, aa_off, al))
    return Case(contigs, list(query_seqs), np.array(tasks, dtype=mpa.DP_TASK), meta, windows)


def _protein(rng, n):
    return bytes(AA[i] for i in rng.integers(0, 20, n))


def _inside(rng, nt, qid, slices, n_ctg=3):
    return dict(nt=nt, qid=qid, ctg=int(rng.integers(0, n_ctg)), rev=int(rng.integers(0, 2)), where="inside", slices=slices)


def tiny(seed=7001):
    """windows of 0 .. 5 rows x every al of EDGES: traceback calls for every nl, both extension modes from three rows up; random bases,
    every fourth case with an N; plus the extension calls of fewer than three rows (nl 0 .. 2 x both modes x TINY_EXT_AL), which the
    planner answers without a sweep.  Interleaved with about 60 ordinary calls and three long windows, so that the planner's
    rows-descending order puts tiny calls into waves that also hold long ones and into partly filled last waves."""
    rng = np.random.default_rng(seed)
    edge, queries = [], []

    def add(nl, al, modes, k):
        nt = rng.integers(0, 4, nl).astype(np.uint8)
        if k % 4 == 3 and nl > 0:
            nt[int(rng.integers(0, nl))] = 4
        queries.append(_protein(rng, al))
        edge.append(_inside(rng, bytes(nt), len(queries) - 1, [(0, al, m) for m in modes]))

    k = 0
    for nl in range(6):
        for al in EDGES:
            add(nl, al, ("cigar",) if nl < 3 else MODES, k)
            k += 1
    for nl in range(3):
        for al in TINY_EXT_AL:
            add(nl, al, ("left", "right"), k)
            k += 1
    filler = []
    for j in range(63):
        nt, aa = long_window(rng, (8, 40, 128)[j // 21]) if j % 21 == 10 else make_task(rng)
        queries.append(aa)
        filler.append(_inside(rng, nt, len(queries) - 1, [(0, len(aa), m) for m in (("cigar",) if j % 21 == 10 else MODES)]))
    # (a few more, so that in every class that packs several calls into a wave the ordinary calls end in the middle of a descriptor)
    for al, modes in ((20, ("left",)), (28, ("left", "cigar")), (50, ("left",))):
        nt, aa = make_task(rng, al=al, p_indel=0.0)
        queries.append(aa)
        filler.append(_inside(rng, nt, len(queries) - 1, [(0, len(aa), m) for m in modes]))
    pairs = []
    step = len(edge) / len(filler)
    for j, f in enumerate(filler):                      # a filler call after every two or three edge calls
        pairs += edge[int(j * step):int((j + 1) * step)] + [f]
    assert len(pairs) == len(edge) + len(filler)
    return place(pairs, queries, rng)


# (front, middle, end) slice lengths of twelve queries: every al of EDGES occurs, up to what the query allows
SLICE_PLAN = [(40, (1, 7, 8)), (70, (9, 16, 17)), (130, (32, 33, 64)), (200, (65, 1, 128)), (300, (129, 7, 33)), (520, (256, 8, 16)),
              (600, (257, 9, 17)), (700, (512, 32, 64)), (1030, (513, 65, 128)), (1100, (1024, 1, 33)), (1200, (1025, 7, 129)), (1200, (1100, 8, 65))]


def slices(seed=7002):
    """twelve queries of 40 .. 1 200 residues, three slices each -- at the front (aa_off 0), in the middle, ending exactly at the query's
    last residue (the last query's: the last byte of the buffer) -- in all three modes: 108 calls, nine per qid.  The window of a slice
    is make_task's nucleotide string for a protein of the slice's length (flank 200, about four introns in the long ones), and the
    slice holds make_task's query for it; the residues between the slices are random."""
    rng = np.random.default_rng(seed)
    assert set(EDGES) <= {a for _, s in SLICE_PLAN for a in s}
    queries, pairs = [], []
    for qid, (qlen, lens) in enumerate(SLICE_PLAN):
        free = qlen - sum(lens)
        assert free >= 1
        gap1 = (free + 1) // 2
        offs = (0, lens[0] + gap1, qlen - lens[2])
        q = bytearray(_protein(rng, qlen))
        for aa_off, al in zip(offs, lens):
            nt, aa = make_task(rng, al=al, flank=200, p_indel=0.0, p_intron=min(0.08, 4.0 / al))
            assert len(aa) == al
            q[aa_off:aa_off + al] = aa
            pairs.append(_inside(rng, nt, qid, [(aa_off, al, m) for m in MODES]))
        queries.append(bytes(q))
    return place(pairs, queries, rng)


ENDS_CTG_LEN = (1001, 3, 17, 64, 4096)                  # the first and the last contig of the index hold packed positions 0 and l_seq - 1
ENDS_AL = (1, 8, 33, 70, 130, 300)
ENDS_N = (2, 3)                                         # contigs with an N on their first and last base


def ends(seed=7003):
    """five contigs of 3, 17, 64, 1 001 and 4 096 bases (two of them with N on the first and last base; odd lengths put the next contig
    on an odd nibble of the packed genome), and on both strands of each: windows that start at strand position 0, end at the last
    base, are the whole contig, and start / end 1, 5 and 6 bases off either end -- both sides of the 6-nibble lead packed_window16()
    fetches.  al in ENDS_AL as far as 3 * al fits the bases there are (al = 1 always); all three modes (traceback only where fewer than
    three rows are left); every other left extension carries MPA_F_SS_SKIP0.  The contigs are make_task windows laid end to end, the
    queries make_task's for the first gene of each length on each contig, so windows at the start of a forward strand hold a real gene and
    the others mostly do not."""
    rng = np.random.default_rng(seed)
    qlist, qid_of = [], {}
    contigs = []
    for c, L in enumerate(ENDS_CTG_LEN):
        parts, n = [], 0
        for al in [a for a in reversed(ENDS_AL) if 3 * a <= L] * 8:
            if n >= L:
                break
            nt, aa = make_task(rng, al=al, flank=10, p_indel=0.0, p_intron=min(0.08, 2.0 / al), p_n=0.0)
            if (c, al) not in qid_of:                     # the contig's first gene of al residues is the query of its al-residue calls
                qid_of[(c, al)] = len(qlist)
                qlist.append(aa)
            parts.append(np.frombuffer(nt, dtype=np.uint8))
            n += len(nt)
        contigs.append(np.concatenate(parts)[:L].copy())
        for al in ENDS_AL:                                # (a length the contig was full before: a query of its own)
            if (c, al) not in qid_of and (al == 1 or 3 * al <= L):
                qid_of[(c, al)] = len(qlist)
                qlist.append(make_task(rng, al=al, p_indel=0.0)[1])
    for c in ENDS_N:
        contigs[c][0] = contigs[c][-1] = 4
    pairs, n_left = [], 0
    for c, L in enumerate(ENDS_CTG_LEN):
        for rev in (0, 1):
            for where, shift in [("start", 0), ("end", 0), ("whole", 0)] + [(w, s) for w in ("start", "end") for s in (1, 5, 6)]:
                room = L - shift
                if room < 1:
                    continue
                for al in ENDS_AL:
                    if al > 1 and 3 * al > room:
                        continue
                    qid = qid_of[(c, al)]
                    nl = room if where == "whole" else min(room, 3 * al + 30)
                    sl = []
                    for m in (MODES if nl >= 3 else ("cigar",)):
                        extra = 0
                        if m == "left":
                            extra, n_left = (SS_SKIP0 if n_left % 2 else 0), n_left + 1
                        sl.append((0, len(qlist[qid]), m, extra))
                    pairs.append(dict(ctg=c, rev=rev, where=where, shift=shift, nl=nl, qid=qid, slices=sl))
    return place(pairs, qlist, rng, io=39, contigs=contigs)


def alphabet(seed=7004):
    """150 ordinary calls whose queries have 30 % of their bytes replaced by bytes from 1 to 255: lowercase, BZJOUX*-, digits, bytes of
    128 and above (0 would end the C string the reference's entry takes)"""
    rng = np.random.default_rng(seed)
    queries, pairs = [], []
    for _ in range(150):
        nt, aa = make_task(rng)
        q = np.frombuffer(aa, dtype=np.uint8).copy()
        hit = rng.random(len(q)) < 0.3
        q[hit] = rng.integers(1, 256, int(hit.sum())).astype(np.uint8)
        queries.append(bytes(q))
        pairs.append(_inside(rng, nt, len(queries) - 1, [(0, len(q), m) for m in MODES]))
    return place(pairs, queries, rng)


FAMILIES = dict(tiny=tiny, slices=slices, ends=ends, alphabet=alphabet)
_cases, _expect = {}, {}


def case(name):
    if name not in _cases:
        _cases[name] = FAMILIES[name]()
    return _cases[name]


def params_for(P, io):
    return refbind.DpParams(P.mat, go=P.go, ge=P.ge, io=io, fs=P.fs, xdrop=P.xdrop, end_bonus=P.end_bonus, sp=P.sp, sp_null_bonus=P.sp_null_bonus, ie_coef=P.ie_coef)


def evaluate(cs, P, fn, ss=None, skip=()):
    """fn (refbind.ora_nasw / refbind.ref_nasw) over the calls of a Case; ss[k]: the splice-score bytes of call k; calls in `skip`: None"""
    out = []
    for k, ((nt, aa), (p, fl, io, a, n)) in enumerate(zip(cs.calls(), cs.meta)):
        out.append(None if k in skip else fn(nt, aa, params_for(P, io), fl, None if ss is None else ss[k]))
    return out


def expected(name, P, key, which="ora", ss=None):
    """the oracle's (or, which="ref", the reference's) results for a family under the parameters P, computed once per (family, key);
    the reference's list has None for the extension calls of fewer than three rows, which it asserts on"""
    k = (name, key, which)
    if k not in _expect:
        cs = case(name)
        _expect[k] = evaluate(cs, P, refbind.ora_nasw, ss) if which == "ora" else evaluate(cs, P, refbind.ref_nasw, ss, skip=set(cs.tiny_ext()))
    return _expect[k]


def spsc_bytes(cs, idx):
    """per call the ss[] bytes the reference would hand the DP (tests/test_dp_gpu.py::test_splice_score_track), MPA_F_SS_SKIP0 applied"""
    out = []
    for t in cs.tasks:
        st, nl, vid = int(t["nt_off"]), int(t["nl"]), int(t["vid"])
        ss = (idx.get_spsc(vid, st - 1, st + nl)[1:] if st > 0 else idx.get_spsc(vid, 0, nl)).copy()
        if int(t["flag"]) & SS_SKIP0:
            ss[0] = 0xff
        out.append(bytes(ss))
    return out
