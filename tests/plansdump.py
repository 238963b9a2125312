"""MPA_PLANS_DUMP=<file>: what the step from the refinement chains of every window to the round-1 DP tasks left in every query's
state, whichever path produced it -- the host functions of host_plan.cpp (stage_refine_to_plan, plan_round1), the shared core on the
host (MPA_GPU_PLANS=model) or k_plans on the device (MPA_GPU_PLANS=1).  This is how the tests see the step without an exported symbol.

Layout (little endian, appended batch after batch, inside a batch in query order):
    per query   int32 qid, regions, plans, tasks, gap segments
                regions   64 bytes: int32 cnt, id, parent, n_sub, subsc, chn_sc, chn_sc_ungap; uint32 vid; int32 qs, qe; int64 vs, ve;
                          int32 split, off
                plans     80 bytes: int64 as, ae, vs0, vs1, mid_ve; int32 reg, as1, mid_qe, has_right, t_left, t_left2, t_right,
                          t_right2, first gap segment, gap segments
                tasks     mpa_dp_task_t, 40 bytes: int64 nt_off; int32 vid, nl, qid, aa_off, al, flag, io, tag
                segments  24 bytes: int32 ne0, ne1, ae0, ae1, task (-1: the ungapped shortcut), score (INT32_MIN for a shortcut
                          segment that lacks its one-word cigar alen << 4)
"""
import numpy as np

HEAD = np.dtype([("qid", "<i4"), ("n_reg", "<i4"), ("n_plan", "<i4"), ("n_task", "<i4"), ("n_seg", "<i4")])
REG = np.dtype([("cnt", "<i4"), ("id", "<i4"), ("parent", "<i4"), ("n_sub", "<i4"), ("subsc", "<i4"), ("chn_sc", "<i4"), ("chn_sc_ungap", "<i4"), ("vid", "<u4"),
                ("qs", "<i4"), ("qe", "<i4"), ("vs", "<i8"), ("ve", "<i8"), ("split", "<i4"), ("off", "<i4")])
PLAN = np.dtype([("as", "<i8"), ("ae", "<i8"), ("vs0", "<i8"), ("vs1", "<i8"), ("mid_ve", "<i8"), ("reg", "<i4"), ("as1", "<i4"), ("mid_qe", "<i4"), ("has_right", "<i4"),
                 ("t_left", "<i4"), ("t_left2", "<i4"), ("t_right", "<i4"), ("t_right2", "<i4"), ("gap0", "<i4"), ("n_gap", "<i4")])
TASK = np.dtype([("nt_off", "<i8"), ("vid", "<i4"), ("nl", "<i4"), ("qid", "<i4"), ("aa_off", "<i4"), ("al", "<i4"), ("flag", "<i4"), ("io", "<i4"), ("tag", "<i4")])
SEG = np.dtype([("ne0", "<i4"), ("ne1", "<i4"), ("ae0", "<i4"), ("ae1", "<i4"), ("task", "<i4"), ("score", "<i4")])
assert HEAD.itemsize == 20 and REG.itemsize == 64 and PLAN.itemsize == 80 and TASK.itemsize == 40 and SEG.itemsize == 24
PARTS = (("region", REG, "n_reg"), ("plan", PLAN, "n_plan"), ("task", TASK, "n_task"), ("segment", SEG, "n_seg"))


def parse(data):
    """[(qid, regions, plans, tasks, segments)] in file order"""
    out, at = [], 0
    while at < len(data):
        h = np.frombuffer(data, HEAD, 1, at)[0]
        at += HEAD.itemsize
        entry = [int(h["qid"])]
        for _, dt, cnt in PARTS:
            n = int(h[cnt])
            entry.append(np.frombuffer(data, dt, n, at).copy())
            at += n * dt.itemsize
        out.append(tuple(entry))
    assert at == len(data), "a truncated dump"
    return out


def read(path):
    with open(path, "rb") as f:
        return f.read()


def first_difference(a, b):
    """None when two dumps (bytes) are equal; otherwise a sentence that names the first differing query, record and field"""
    if a == b:
        return None
    pa, pb = parse(a), parse(b)
    if len(pa) != len(pb):
        return "%d queries against %d" % (len(pa), len(pb))
    for k, (ea, eb) in enumerate(zip(pa, pb)):
        if ea[0] != eb[0]:
            return "entry %d: query %d against %d" % (k, ea[0], eb[0])
        for (what, dt, _), ra, rb in zip(PARTS, ea[1:], eb[1:]):
            if len(ra) != len(rb):
                return "entry %d (query %d): %d %ss against %d" % (k, ea[0], len(ra), what, len(rb))
            for i in range(len(ra)):
                for f in dt.names:
                    if ra[i][f] != rb[i][f]:
                        return "entry %d (query %d), %s %d: %s %d against %d" % (k, ea[0], what, i, f, ra[i][f], rb[i][f])
    return "the bytes differ, the parsed fields do not"
