"""MPA_SPANS_DUMP=<file>: what the step between the DP rounds (the accepted spans and the round-2 tasks) and step (a) behind them (the
region CIGARs) left in every query's state, whichever path produced it -- the host functions of host_align.cpp (take_round1_emit_round2,
assemble_alignment, count_exons), the shared core on the host (MPA_GPU_SPANS=model) or k_spans / k_assemble on the device
(MPA_GPU_SPANS=1).  Written before the final selection reorders the regions.

Layout (little endian, appended batch after batch, inside a batch in query and plan order):
    per query   int32 qid, plans
    per plan    184 bytes: int32 l_nt, l_aa, r_nt, r_aa, flags (1: left span, 2: right span, 4 / 8: the left / right terminal-exon repeat
                counted, 16: a segment boundary merged two words), qs, qe, dp_score, n_exon, n_cigar;
                int64 vs, ve; the left and the right span segment, 24 bytes each: int32 ne0, ne1, ae0, ae1, task (-1: the ungapped
                shortcut), score (a right span that was not made: zeros with task -1); their round-2 task records, mpa_dp_task_t, 40
                bytes each (zeros for a shortcut): int64 nt_off; int32 vid, nl, qid, aa_off, al, flag, io, tag
                then n_cigar uint32 words (len << 4 | op)
"""
import numpy as np

HEAD = np.dtype([("qid", "<i4"), ("n_plan", "<i4")])
SEG = [("ne0", "<i4"), ("ne1", "<i4"), ("ae0", "<i4"), ("ae1", "<i4"), ("task", "<i4"), ("score", "<i4")]
TASK = [("nt_off", "<i8"), ("vid", "<i4"), ("nl", "<i4"), ("qid", "<i4"), ("aa_off", "<i4"), ("al", "<i4"), ("flag", "<i4"), ("io", "<i4"), ("tag", "<i4")]
PLAN = np.dtype([("l_nt", "<i4"), ("l_aa", "<i4"), ("r_nt", "<i4"), ("r_aa", "<i4"), ("flags", "<i4"), ("qs", "<i4"), ("qe", "<i4"), ("dp_score", "<i4"), ("n_exon", "<i4"),
                 ("n_cigar", "<i4"), ("vs", "<i8"), ("ve", "<i8"), ("left", np.dtype(SEG)), ("right", np.dtype(SEG)), ("t_left", np.dtype(TASK)), ("t_right", np.dtype(TASK))])
assert HEAD.itemsize == 8 and PLAN.itemsize == 184
LEFT, RIGHT, LEFT_REPEAT, RIGHT_REPEAT, MERGED = 1, 2, 4, 8, 16


def parse(data):
    """[(qid, [(plan record, cigar words)])] in file order"""
    out, at = [], 0
    while at < len(data):
        h = np.frombuffer(data, HEAD, 1, at)[0]
        at += HEAD.itemsize
        plans = []
        for _ in range(int(h["n_plan"])):
            p = np.frombuffer(data, PLAN, 1, at)[0].copy()
            at += PLAN.itemsize
            n = int(p["n_cigar"])
            plans.append((p, np.frombuffer(data, "<u4", n, at).copy()))
            at += 4 * n
        out.append((int(h["qid"]), plans))
    assert at == len(data), "a truncated dump"
    return out


def read(path):
    """the dump's bytes; none for a run that never reached the steps (-A: no DP rounds, no file)"""
    import os
    if not os.path.exists(path):
        return b""
    with open(path, "rb") as f:
        return f.read()


def first_difference(a, b):
    """None when two dumps (bytes) are equal; otherwise a sentence that names the first differing query, plan and field"""
    if a == b:
        return None
    pa, pb = parse(a), parse(b)
    if len(pa) != len(pb):
        return "%d queries against %d" % (len(pa), len(pb))
    for k, ((qa, la), (qb, lb)) in enumerate(zip(pa, pb)):
        if qa != qb or len(la) != len(lb):
            return "entry %d: query %d with %d plans against query %d with %d" % (k, qa, len(la), qb, len(lb))
        for i, ((ra, ca), (rb, cb)) in enumerate(zip(la, lb)):
            if ra.tobytes() != rb.tobytes():
                return "entry %d (query %d), plan %d: %r against %r" % (k, qa, i, ra, rb)
            if ca.tobytes() != cb.tobytes():
                return "entry %d (query %d), plan %d: cigar %r against %r" % (k, qa, i, ca[:40], cb[:40])
    return "the bytes differ, the parsed fields do not"
