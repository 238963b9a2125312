"""Inputs of the spans tests (tests/test_spans_cpu.py, tests/test_spans_gpu.py; MPA_GPU_SPANS): the golden cases (those of
planscases), runs with the dump of tests/spansdump.py switched on, the step's notes, the branches a dump shows, and hand-made inputs
for mpa_dbg_spans -- the table tests/spans_check.cpp runs through the core under the sanitizers, and a generator of many plans."""
import os
import numpy as np
import miniprot_amd as mpa
import planscases
import spansdump

MODEL_NOTE = "spans: shared core"
DEVICE_NOTE = "spans on the GPU"
NO_WORDS = " 0 CIGAR words"
CASES = planscases.CASES
case_inputs = planscases.case_inputs


def with_dump(monkeypatch, path, run):
    """run() with MPA_SPANS_DUMP=path (a fresh file); returns (what run() returned, the dump's bytes)"""
    if os.path.exists(path):
        os.remove(path)
    monkeypatch.setenv("MPA_SPANS_DUMP", path)
    try:
        out = run()
    finally:
        monkeypatch.delenv("MPA_SPANS_DUMP")
    return out, spansdump.read(path)


BRANCHES = ("left repeat taken", "right repeat taken", "a plan without a right span", "a shortcut span", "a DP span", "a merged boundary")


def branches(dump):
    """how often each of BRANCHES occurs in a dump"""
    n = dict.fromkeys(BRANCHES, 0)
    for _, plans in spansdump.parse(dump):
        for p, _ in plans:
            f = int(p["flags"])
            n["left repeat taken"] += bool(f & spansdump.LEFT_REPEAT)
            n["right repeat taken"] += bool(f & spansdump.RIGHT_REPEAT)
            n["a plan without a right span"] += not f & spansdump.RIGHT
            n["a merged boundary"] += bool(f & spansdump.MERGED)
            spans = [p["left"]] + ([p["right"]] if f & spansdump.RIGHT else [])
            n["a shortcut span"] += sum(int(s["task"]) < 0 for s in spans)
            n["a DP span"] += sum(int(s["task"]) >= 0 for s in spans)
    return n


# ---- mpa_dbg_spans ----------------------------------------------------------------------------------------------------------------
PLAN_IN = np.dtype([("as", "<i8"), ("ae", "<i8"), ("vs0", "<i8"), ("vs1", "<i8"), ("mid_ve", "<i8"), ("reg", "<i4"), ("as1", "<i4"), ("mid_qe", "<i4"), ("has_right", "<i4"),
                    ("t_left", "<i4"), ("t_left2", "<i4"), ("t_right", "<i4"), ("t_right2", "<i4"), ("gap0", "<i4"), ("n_gap", "<i4"), ("q_off", "<i8"), ("qid", "<i4"),
                    ("qlen", "<i4"), ("vid", "<u4"), ("base1", "<i4")])
SEG = np.dtype(spansdump.SEG)
TASK = np.dtype(spansdump.TASK)
RST = np.dtype([("nt_len", "<i4"), ("aa_len", "<i4"), ("score", "<i4"), ("n_cigar", "<i4"), ("cigar_off", "<i8")])
SPAN_REC = np.dtype([("vs", "<i8"), ("qs", "<i4"), ("l_nt", "<i4"), ("l_aa", "<i4"), ("r_nt", "<i4"), ("r_aa", "<i4"), ("flags", "<i4"), ("left", SEG), ("right", SEG)])
ASM_REC = np.dtype([("ve", "<i8"), ("cig_off", "<i8"), ("qe", "<i4"), ("dp_score", "<i4"), ("n_cigar", "<i4"), ("n_exon", "<i4"), ("bad", "<i4"), ("n_merged", "<i4")])
assert PLAN_IN.itemsize == 104 and SEG.itemsize == 24 and RST.itemsize == 24 and SPAN_REC.itemsize == 80 and ASM_REC.itemsize == 40 and TASK.itemsize == 40


def dbg_spans(ctx, idx, mo, q, plans, segs, rst1, pool1, rst2=None, pool2=None):
    """mpa.dbg_spans with its records parsed: (span records, round-2 tasks) for rst2 None, else (span records, tasks, assemble
    records, [cigar words per plan])"""
    out = mpa.dbg_spans(ctx, idx, mo, q, plans, segs, rst1, pool1, rst2, pool2)
    rec, tasks = np.frombuffer(out[0], SPAN_REC), np.frombuffer(out[1], TASK)
    if rst2 is None:
        return rec, tasks
    arec = np.frombuffer(out[2], ASM_REC)
    return rec, tasks, arec, [out[3][int(a["cig_off"]):int(a["cig_off"]) + int(a["n_cigar"])].copy() for a in arec]


# ---- hand-made inputs: the cases of tests/spans_check.cpp as a table, and many random plans ---------------------------------------
KMER2, MAX_EXT = 5, 10000                             # of default_mapopt(): what the thresholds below are written against


def W(op, n):
    return n << 4 | op


def dp_gap(words, score=7):
    """a gap segment that went through the DP: 40 bases against 9 residues (above kmer2)"""
    return (40, 9, list(words), score)


def short_gap(alen, score=3):
    """a gap segment that took the ungapped shortcut"""
    return (3 * alen, alen, None, score)


def world(seed=11):
    """(index, queries, map options): two contigs with an N now and then, four proteins of 3 000 residues"""
    rng = np.random.default_rng(seed)
    contigs = []
    for n in (9000, 5000):
        c = rng.integers(0, 4, n).astype(np.uint8)
        c[rng.random(n) < 0.02] = 4
        contigs.append(c)
    prots = ["".join(rng.choice(list("ARNDCQEGHILKMFPSTWYV"), 3000)) for _ in range(4)]
    mo = mpa.default_mapopt()
    assert mo.kmer2 == KMER2 and mo.max_ext == MAX_EXT
    return mpa.Index.from_nt4(contigs, ["chr1", "chr2"]), mpa.Queries(prots), mo


class Plans:
    """plans for mpa_dbg_spans, built as tests/spans_check.cpp builds its cases; words[j] = what plan j's two spans come back with"""

    def __init__(self, q):
        self.q, self.plans, self.segs, self.rst1, self.pool1, self.words = q, [], [(9, 9, 9, 9, -1, 9)] * 2, [], [0xdead] * 5, []

    def add(self, left=(0, 0), left2=None, right=None, right2=None, gaps=(), qid=0, vid=0, vs0=3000, as1=100, left_words=(W(0, 1),), right_words=(W(0, 1),), ae=8000):
        """left / left2 / right / right2: (nt_len, aa_len) of the extension's first call and of its repeat (None: not issued; right None:
        has_right == 0); right as 'end' + nt_len: an extension that reaches the end of the protein"""
        qlen, base1 = len(self.q.seqs[qid]), len(self.rst1)
        t = [-1] * 4
        mid_qe, ne, gap0 = as1 + sum(g[1] for g in gaps), 600, len(self.segs)
        for k, x in enumerate((left, left2, right, right2)):
            if x is not None:
                t[k] = len(self.rst1) - base1
                self.rst1.append((x[0], qlen - mid_qe if x[1] == "end" else x[1], 5, 0, 0))
        ae0 = as1
        for nlen, alen, words, score in gaps:
            task = -1
            if words is not None:
                task = len(self.rst1) - base1
                self.rst1.append((nlen, alen, score, len(words), len(self.pool1)))
                self.pool1 += words
            self.segs.append((ne, ne + nlen, ae0, ae0 + alen, task, score if task < 0 else 0))
            ne, ae0 = ne + nlen, ae0 + alen
        self.plans.append((0, ae, vs0, vs0 + 600, vs0 + ne, 0, as1, mid_qe, int(right is not None), t[0], t[1], t[2], t[3], gap0, len(gaps), int(self.q.off[qid]), qid, qlen,
                           vid, base1))
        self.words.append((list(left_words), list(right_words)))
        return len(self.plans) - 1

    def arrays(self):
        return (np.array(self.plans, PLAN_IN), np.array(self.segs, SEG), np.array(self.rst1, RST), np.array(self.pool1, "<u4"))

    def round2(self, rec):
        """(rst2, pool2) for the span records of the first step: every DP span comes back with its plan's words"""
        n = int(max([int(r["left"]["task"]) for r in rec] + [int(r["right"]["task"]) for r in rec])) + 1
        rst2, pool2 = np.zeros(n, RST), [0xbeef] * 3
        for j, r in enumerate(rec):
            for side, seg in enumerate((r["left"], r["right"])):
                if int(seg["task"]) >= 0:
                    w = self.words[j][side]
                    rst2[int(seg["task"])] = (int(seg["ne1"]) - int(seg["ne0"]), int(seg["ae1"]) - int(seg["ae0"]), 11 + 2 * side + j % 7, len(w), len(pool2))
                    pool2 += w
        return rst2, np.array(pool2, "<u4")


def canonical_words(rng, n):
    """n words as a DP call returns them: no two mergeable neighbours"""
    out = []
    while len(out) < n:
        op = int(rng.choice([0, 1, 2, 3, 10, 11, 12, 13]))
        if out and out[-1] & 0xf == op and op not in (10, 11):
            continue
        out.append(W(op, 1 + int(rng.integers(40))))
    return out


def handmade(q):
    """the table: [(what it is for, plan number)] and the Plans that hold them"""
    rng = np.random.default_rng(5)
    P, T = Plans(q), []

    def case(name, **kw):
        T.append((name, P.add(**kw)))
    case("empty left span, then M", gaps=[dp_gap([W(0, 12), W(3, 80), W(0, 4)])])
    case("left repeat: l_nt == max_ext - 1", left=(MAX_EXT - 1, 60), left2=(500, 100))
    case("left repeat: l_nt == max_ext", left=(MAX_EXT, 60), left2=(500, 100))
    case("left repeat: l_aa == as1", left=(300, 100), left2=(500, 100))
    case("left repeat: one residue short", left=(300, 60), left2=(500, 99))
    case("right repeat: r_nt == max_ext - 1", left2=(0, 0), right=(MAX_EXT - 1, 50), right2=(700, "end"), gaps=[dp_gap([W(0, 9)])])
    case("right repeat: r_nt == max_ext", left2=(0, 0), right=(MAX_EXT, 50), right2=(700, "end"), gaps=[dp_gap([W(0, 9)])])
    case("right repeat: r_aa reaches the end", left2=(0, 0), right=(400, "end"), right2=(700, "end"), gaps=[dp_gap([W(0, 9)])])
    case("right span: r_nt == 0", right=(0, 4), gaps=[dp_gap([W(0, 9)])])
    case("right span: r_aa == 0", right=(12, 0), gaps=[dp_gap([W(0, 9)])])
    case("right span: has_right == 0", gaps=[dp_gap([W(0, 9)])])
    case("right span: made", right=(12, 4), gaps=[dp_gap([W(0, 9)])])
    case("shortcut: alen == kmer2", left=(3 * KMER2, KMER2), qid=1, vid=1)
    case("shortcut: alen == kmer2 + 1", left=(3 * KMER2 + 3, KMER2 + 1), qid=1, vid=2)
    case("shortcut: nlen != 3 alen", left=(3 * KMER2 + 1, KMER2), qid=2, vid=3)
    for k in range(40):                                   # (2 % of the bases are N: some of these shortcut spans hold one)
        case("shortcut over bases %d" % k, left=(3 * KMER2, KMER2), qid=k % 4, vid=k % 4, vs0=700 + 97 * k, as1=40 + 13 * k)
    for name, a, b in (("M|M", 0, 0), ("M|I", 0, 1), ("10|10", 10, 10), ("11|11", 11, 11), ("N|N", 3, 3)):
        case(name, gaps=[dp_gap([W(1, 2), W(a, 7)]), dp_gap([W(b, 5), W(2, 3)])])
    case("seven single-word M segments", left=(9, 3), gaps=[short_gap(3) if i % 2 else dp_gap([W(0, 9)]) for i in range(7)])
    for n in (0, 1, 63, 64, 65, 200):
        case("%d gap segments" % n, left=(90, 31), left_words=[W(0, 20), W(3, 27), W(0, 1)], right=(33, 12), right_words=[W(0, 11), W(10, 1)],
             gaps=[short_gap(1 + i % 5) if i % 3 == 0 else dp_gap(canonical_words(rng, 1 + int(rng.integers(4))), int(rng.integers(50))) for i in range(n)])
    for n in (1, 64, 65, 300):
        case("a segment of %d words" % n, left=(200, 40), left_words=canonical_words(rng, n), gaps=[dp_gap([W(0, 5)]), dp_gap(canonical_words(rng, n)), short_gap(2)])
    case("an empty segment between two M", gaps=[dp_gap([W(2, 3), W(0, 6)]), dp_gap([]), dp_gap([W(0, 2)])])
    return T, P


def many_plans(q, n=1000, seed=3):
    """n plans of 0 - 2 round-2 tasks each: the task numbers cross the workgroups of k_spans (256 plans each)"""
    rng = np.random.default_rng(seed)
    P = Plans(q)
    for j in range(n):
        left = (3 * 4, 4) if rng.integers(2) else (int(rng.integers(30, 400)), int(rng.integers(10, 90)))
        kind = int(rng.integers(3))
        right = None if kind == 0 else (9, 3) if kind == 1 else (int(rng.integers(30, 400)), int(rng.integers(10, 90)))
        P.add(left=left, right=right, qid=j % 4, vid=j % 4, vs0=700 + j % 1500, gaps=[dp_gap(canonical_words(rng, 1 + j % 3))] if j % 5 else [],
              left_words=canonical_words(rng, 1 + j % 4), right_words=canonical_words(rng, 1 + j % 2))
    return P


def short_gene(n_aa=30, seed=3):
    """(index, queries, map options): a protein that aligns end to end without a gap to a gene between two stop codons"""
    rng = np.random.default_rng(seed)
    aas = "KNKNTTTTRSRSIIMIQHQHPPPPRRRRLLLLEDEDAAAAGGGGVVVV*Y*YSSSS*CWCLFLF"
    first = {a: i for i, a in reversed(list(enumerate(aas)))}
    prot = "".join(rng.choice(list("ARNDCQEGHILKMFPSTWYV"), n_aa))
    g = rng.integers(0, 4, 4000).astype(np.uint8)
    g[2000:2000 + 3 * n_aa] = np.array([[first[a] >> 4 & 3, first[a] >> 2 & 3, first[a] & 3] for a in prot], np.uint8).ravel()
    g[1997:2000] = g[2000 + 3 * n_aa:2003 + 3 * n_aa] = [3, 0, 0]
    idx = mpa.Index.from_nt4([g], ["chr1"])
    mpa._check(mpa.lib().mpa_idx_build_kmers(idx.h, 4))
    return idx, mpa.Queries([prot]), mpa.default_mapopt()
