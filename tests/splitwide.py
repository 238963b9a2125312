"""Helpers of the MPA_DP_SPLIT_WIDE tests (tests/test_dp_split_wide_cpu.py, tests/test_dp_split_wide_gpu.py): extension calls of
1 025..3 072 columns on the classes X_SPLIT8 / X_SPLIT12 (8 / 12 workgroups per pair of calls) instead of the one-wave int32 sweep.
Task tables for the planner hooks with queries long enough for such calls, the int16 guard's limit computed from its predicate, the
parser of the *_wide serialisations, and the (window, protein) pairs of the GPU tests."""
import os
import numpy as np
import miniprot_amd as mpa
import dpplan
from dpplan import EXT, GLOB

CTG_LEN = [12000, 9000, 20000]
Q_LEN = [3300, 700, 300, 3150]
KNOBS = dict(dpplan.KNOBS, split_wide=1)
X_W2, X_W4, X_SPLIT2, X_SPLIT4, X_HUGE, X_128, X_SPLIT8, X_SPLIT12 = 3, 4, 5, 6, 7, 8, 9, 10      # DpClass (dp_device.h)
U_EXT_SPLIT = 5                                                                                   # DpUnitKind
N_BLK = {X_SPLIT2: 2, X_SPLIT4: 4, X_SPLIT8: 8, X_SPLIT12: 12}


def q_off():
    return np.concatenate([[0], np.cumsum(Q_LEN)]).astype(np.int64)


def table(rng, spec):
    """dpplan._table with this module's contigs and queries; spec: (mode, al, nl) per call"""
    t = np.zeros(len(spec), dtype=mpa.DP_TASK)
    for k, (mode, al, nl) in enumerate(spec):
        qid = int(rng.choice([q for q, l in enumerate(Q_LEN) if l >= al]))
        cid = int(rng.integers(0, len(CTG_LEN)))
        t[k] = (int(rng.integers(0, CTG_LEN[cid] - nl + 1)), 2 * cid + int(rng.integers(0, 2)), nl, qid, int(rng.integers(0, Q_LEN[qid] - al + 1)), al,
                mpa.F_CIGAR if mode == GLOB else (mpa.F_EXT_LEFT, mpa.F_EXT_RIGHT)[int(rng.integers(0, 2))], int(rng.integers(10, 41)), k)
    return t


def low_matrix(cap=4):
    """option override: the default matrix with every entry above `cap` lowered to it, so that the guard admits 3 072 columns"""
    o = dpplan.dpopt()
    return dict(mat=type(o.mat)(*[min(int(v), cap) for v in o.mat]))


def may_saturate(al, o):
    """the planner's int16 guard (dp_plan_core.h, dp_classify_call) for a call of al residues under the options o (a DpOpt)"""
    ncol = (al + 7) // 8 * 8
    max_mat = max(0, max(int(v) for v in o.mat))
    return al * max_mat + ncol * o.ge + max(o.end_bonus, 0) > 32000 or o.go + ncol * o.ge > 32000


def guard_limit(o, hi=8192):
    """the widest al the guard admits (the predicate is monotonic in al)"""
    al = 1
    while al < hi and not may_saturate(al + 1, o):
        al += 1
    return al


def expected_class(al, o, knobs):
    """the extension class of a call of al residues, from the rules of the classes (not from the planner's code)"""
    ncol = (al + 7) // 8 * 8
    wide_ge = o.ge > 255 or o.fs > 255
    split_wide = knobs.get("split_wide", 0) and not knobs.get("pool", 0) and not knobs.get("no_split", 0)
    if wide_ge or may_saturate(al, o):
        return X_HUGE
    for cls, cols in ((0, 16), (1, 32), (2, 64), (X_W2, 128), (X_W4, 256), (X_SPLIT2, 512), (X_SPLIT4, 1024), (X_SPLIT8, 2048), (X_SPLIT12, 3072)):
        if ncol <= cols:
            if cls in (X_SPLIT8, X_SPLIT12) and not split_wide:
                return X_HUGE
            if cls in (X_SPLIT2, X_SPLIT4) and knobs.get("no_split", 0):
                return X_HUGE
            if cls == X_W2 and knobs.get("ext_dual", 1) and not knobs.get("antidiag", 0):
                return X_128
            return cls
    return X_HUGE


class WidePlan(dpplan.Plan):
    """a *_wide serialisation: dpplan.Plan of the common part, then first / count of X_SPLIT8 and X_SPLIT12 and n_bound"""

    def __init__(self, buf):
        self.common = bytes(buf[:-mpa.DP_PLAN_WIDE_TAIL])
        super().__init__(self.common)
        t = np.frombuffer(buf[-mpa.DP_PLAN_WIDE_TAIL:], dtype="<i8")
        self.s8, self.s12, self.n_bound = (int(t[0]), int(t[1])), (int(t[2]), int(t[3])), int(t[4])
        self.buf = bytes(buf)


def plan(tasks, opt_over=None, knobs=None):
    """the host planner through mpa_dbg_dp_plan_wide -> WidePlan, or (code, message)"""
    kn = dict(KNOBS)
    kn.update(knobs or {})
    r = mpa.dbg_dp_plan_wide(dpplan.dpopt(**(opt_over or {})), CTG_LEN, q_off(), tasks, kn)
    return r if isinstance(r, tuple) else WidePlan(r)


def device_plan(ctx, tasks, opt_over=None, knobs=None):
    """the device planner (ctx None: its model) through mpa_dbg_dp_plan_device_wide -> WidePlan, or (code, message)"""
    kn = dict(KNOBS)
    kn.update(knobs or {})
    r = mpa.dbg_dp_plan_device_wide(ctx, dpplan.dpopt(**(opt_over or {})), CTG_LEN, q_off(), tasks, kn)
    return r if isinstance(r, tuple) else WidePlan(r)


def planner_tables():
    """name -> (tasks, option overrides): tables both planners take with split_wide = 1 (no call of class X_HUGE)"""
    t = {}
    g = guard_limit(dpplan.dpopt())
    r = np.random.default_rng(9301)
    spec = [(EXT, al, int(r.integers(3, 2501))) for al in dpplan.EDGES + [1536, 2040, 2048, 2049, 2305, g - 1, g]]
    for _ in range(200):                                                     # like dpplan's a_ext, with al up to the guard
        hi = int(r.choice([16, 32, 64, 128, 256, 512, 1024, 1100, 2048, g]))
        spec.append((EXT, int(r.integers(1, hi + 1)), int(r.integers(3, 2501))))
    t["a_ext_to_the_guard"] = (table(r, spec), {})
    r = np.random.default_rng(9302)
    spec = [(EXT, int(r.integers(1025, 2049)), int(r.integers(3, 2501))) for _ in range(5)] + [(EXT, int(r.integers(2049, g + 1)), int(r.integers(3, 2501))) for _ in range(2)]
    spec += [(EXT, 3072, 777), (EXT, 40, 100), (GLOB, 30, 500)]
    t["odd_counts"] = (table(r, spec), low_matrix())                         # five and three calls: a group with an empty half in each class
    r = np.random.default_rng(9303)
    nls = [50, 200, 400, 900]
    spec = []
    for _ in range(3000):
        wide = r.random() < 0.03
        spec.append(((EXT, GLOB)[0 if wide else int(r.integers(0, 2))], int(r.integers(1025, g + 1)) if wide else int(r.integers(1, 301)), int(r.choice(nls))))
    t["mixed_3000"] = (table(r, spec), {})
    return t


# ---- the (window, protein) pairs of the GPU tests
def wide_pair(rng, al, flank=30, rows=None, **kw):
    """dpgen.make_task for a protein of al residues exactly (no indels in the query, so that the class is known); rows: the window cut to
    that many rows"""
    from dpgen import make_task
    kw.setdefault("p_indel", 0.0)
    nt, aa = make_task(rng, al=al, flank=flank, **kw)
    assert len(aa) == al
    return (nt[:rows] if rows is not None else nt), aa


class knob:
    """MPA_DP_SPLIT_WIDE in the environment while a context is created (it is read then)"""

    def __init__(self, value="1"):
        self.value = value

    def __enter__(self):
        self.old = os.environ.get("MPA_DP_SPLIT_WIDE")
        if self.value is None:
            os.environ.pop("MPA_DP_SPLIT_WIDE", None)
        else:
            os.environ["MPA_DP_SPLIT_WIDE"] = self.value

    def __exit__(self, *a):
        if self.old is None:
            os.environ.pop("MPA_DP_SPLIT_WIDE", None)
        else:
            os.environ["MPA_DP_SPLIT_WIDE"] = self.old


# ---- the whole path: one small genome, a few ordinary proteins and one of about 2 400 residues of which only the last 400 are planted,
# so that its left extension has about 2 000 columns.  Everything derives from fixed seeds; the reference's output (-I -u, and --gff) is
# tests/golden/split_wide.ref.paf / .ref.gff, written by `python tests/splitwide.py` where oracle/_ref/miniprot exists.
WP_GENOME, WP_SEED, WP_HEAD, WP_TAIL, WP_ORDINARY = 600000, 931, 2000, 400, 4
WP_FLAGS = ["-I", "-u"]
DEVICE_KNOBS = ("MPA_GPU_SEED", "MPA_GPU_SKETCH", "MPA_GPU_REFINE", "MPA_GPU_REGIONS", "MPA_GPU_PLANS", "MPA_GPU_SPANS", "MPA_GPU_DPPLAN", "MPA_GPU_ROUND2",
                "MPA_GPU_STATS", "MPA_GPU_CS", "MPA_GPU_ROWS")


def whole_path_case():
    """-> (contigs, proteins, names); the long protein is the last one"""
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import gen_synth
    contigs, prots, names = gen_synth.generate(WP_GENOME, 1, 3 * WP_ORDINARY, WP_SEED, imax=3000)
    g = contigs[0]
    rng = np.random.default_rng([WP_SEED, 2048])
    planted, gene = gen_synth.make_gene(rng, WP_TAIL, 7.5, 1.5, 70, 3000)
    at = WP_GENOME // 2                                                      # behind the ordinary genes' slots (the first third)
    g[at:at + len(gene)] = gene
    head = bytes(b"ARNDCQEGHILKMFPSTWYV"[i] for i in rng.integers(0, 20, WP_HEAD))
    long_q = head + bytes(gen_synth.mutate(rng, planted))
    # the extension left of the first anchor has more than WP_HEAD - a few columns: beyond 1 024, inside the int16 guard whatever the anchor
    assert WP_HEAD > 1100 and not may_saturate(len(long_q), dpplan.dpopt())
    return contigs, [bytes(p) for p in prots[:WP_ORDINARY]] + [long_q], list(names[:WP_ORDINARY]) + ["long_tail_planted"]


def whole_path_mapopt():
    mo = mpa.default_mapopt()
    mo.flag |= 0x4                                                           # -u
    return mo


if __name__ == "__main__":
    import subprocess
    import sys
    import tempfile
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import gen_synth
    import golden
    import refbind
    contigs, prots, names = whole_path_case()
    with tempfile.TemporaryDirectory() as tmp:
        fa, faa = os.path.join(tmp, "g.fa"), os.path.join(tmp, "p.fa")
        gen_synth.write_fasta_nt(fa, contigs)
        gen_synth.write_fasta_aa(faa, prots, names)
        for ext, flags in ((".ref.paf", WP_FLAGS), (".ref.gff", WP_FLAGS + ["--gff"])):
            out = subprocess.run([refbind.REF_BIN, "-t4"] + flags + [fa, faa], capture_output=True, check=True).stdout
            open(golden.path("split_wide" + ext), "wb").write(out)
            print("split_wide" + ext, len(out), "bytes", out.count(b"\n"), "lines")
