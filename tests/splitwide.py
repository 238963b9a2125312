"""Helpers of the MPA_DP_SPLIT_WIDE tests (tests/test_dp_split_wide_cpu.py, tests/test_dp_split_wide_gpu.py,
tests/test_dp_split_wide_range_gpu.py): extension calls of 1 025..3 072 columns on the classes X_SPLIT8 / X_SPLIT12 (8 / 12 workgroups
per pair of calls) instead of the one-wave int32 sweep.  Task tables for the planner hooks with queries long enough for such calls, the
int16 guard's limit computed from its predicate, the parser of the *_wide serialisations, the (window, protein) pairs of the GPU tests,
and the batches of the range tests (capped matrix, penalty points, int16 bound) with their expected classes and values."""
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
    """the widest al in [1, hi] the guard admits (the predicate is monotonic in al: by bisection)"""
    lo = 1
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if may_saturate(mid, o):
            hi = mid - 1
        else:
            lo = mid
    return lo


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


# ---- the classes over the penalty range (tests/test_dp_split_wide_range_gpu.py; the same tables without a device in
# tests/test_dp_split_wide_cpu.py): a capped matrix so that all twelve column blocks are live, the wide penalty points, calls at the
# int16 bound, the hottest pair a matrix allows
WIDE_KW = dict(p_intron=0.004, max_intron=200, flank=30)            # rows = 3 al + a few short introns
BOTH = ("left", "right")
ALL_MODES = ("cigar", "left", "right")
MIXED_ALS = (12, 16, 24, 32, 40, 64, 72, 128, 200, 256, 400, 600, 1000)   # every narrower extension class (and, as traceback calls, the plain sweeps)
TWELVE_BLOCK_ALS = (2666, 2815, 2816, 2817, 3064, 3065, 3072)  # past the default guard; both sides of block 11's first column; a padded and a full last group
SHORT_ROWS_3072 = (3, 14, 49, 97, 600)                          # block 11 starts about 550 rows behind block 0


def capped_matrix(cap, fs=23):
    """refbind.mapping_matrix(fs) with every entry above `cap` lowered to it: the matrix counterpart of low_matrix()"""
    import refbind
    return np.minimum(refbind.mapping_matrix(fs), cap).astype(np.int8)


def wide_params(kw=None, cap=None):
    """refbind.DpParams of the keyword arguments kw (as tests/test_dp_penalties_gpu.py builds them) on the matrix capped at `cap`"""
    import refbind
    kw = dict(kw or {})
    fs = min(kw.get("fs", 23), 127)
    return refbind.DpParams(refbind.mapping_matrix(fs) if cap is None else capped_matrix(cap, fs), **kw)


def opt_overrides(P):
    """the options of P as overrides for dpplan.dpopt(): what plan() / device_plan() take"""
    o = dpplan.dpopt()
    return dict(mat=type(o.mat)(*[int(v) for v in P.mat.reshape(-1)]), go=P.go, ge=P.ge, fs=P.fs, xdrop=P.xdrop, end_bonus=P.end_bonus)


def hot_pair(rng, al, flag):
    """the highest score the matrix can give: W x al against TGG x al, and 20 random bases on the far side of the extension"""
    far = bytes(rng.integers(0, 4, 20).astype(np.uint8))
    body = bytes([3, 2, 2]) * al
    return (far + body if flag == mpa.F_EXT_LEFT else body + far), b"W" * al


def wide_penalty_points():
    """the entries of dpgen.PENALTY_POINTS whose guard admits calls of the new classes -> [(keyword arguments, guard limit)]"""
    from dpgen import PENALTY_POINTS
    from dputil import dpopt_from_params
    out = []
    for kw in PENALTY_POINTS:
        lim = guard_limit(dpopt_from_params(wide_params(kw)))
        if lim > 1024:
            out.append((kw, lim))
    return out


def mixed_pairs(rng):
    """one pair of every narrower class, of known width (no indels in the query)"""
    from dpgen import make_task
    return [make_task(rng, al=al, p_intron=0.01, max_intron=300, flank=200, p_indel=0.0) for al in MIXED_ALS]


class Table:
    """pairs under the parameters P as one mpa.dp_run batch: build_workload's layout, the expected class of every extension call,
    the oracle's and the reference's results (computed once per table, a few calls at a time)"""

    def __init__(self, P, pairs, seed, pair_modes=None, modes=BOTH):
        from dputil import build_workload, dpopt_from_params
        self.P, self.pairs = P, pairs
        self.contigs, self.queries, self.tasks, self.meta = build_workload(pairs, np.random.default_rng(seed), modes=modes, io=P.io, io_alt=max(0, P.io - 10),
                                                                           pair_modes=pair_modes)
        self.opt = dpopt_from_params(P)
        self._expect = {}

    def ext_als(self):
        return [len(self.pairs[k][1]) for k, fl, _ in self.meta if fl != mpa.F_CIGAR]

    def class_counts(self, split_wide):
        """extension calls per DpClass (a list of 16, like mpa.dbg_dp_last_classes) by the rules of the classes"""
        kn = dict(KNOBS, split_wide=split_wide)
        out = [0] * 16
        for al in self.ext_als():
            out[expected_class(al, self.opt, kn)] += 1
        return out

    def n_wide(self):
        return sum(1 for al in self.ext_als() if al > 1024)

    def plan(self, split_wide=1):
        """the host planner on this very table"""
        q_off = np.concatenate([[0], np.cumsum([len(aa) for _, aa in self.pairs])]).astype(np.int64)
        r = mpa.dbg_dp_plan_wide(self.opt, [len(c) for c in self.contigs], q_off, self.tasks, dict(KNOBS, split_wide=split_wide))
        return r if isinstance(r, tuple) else WidePlan(r)

    def expect(self, which="oracle"):
        """(nt_len, aa_len, score, CIGAR) of every call from refbind.ora_nasw ("oracle") or refbind.ref_nasw ("reference")"""
        import refbind
        from concurrent.futures import ThreadPoolExecutor
        if which not in self._expect:
            fn = refbind.ora_nasw if which == "oracle" else refbind.ref_nasw
            refbind.ora() if which == "oracle" else refbind.ref()      # (load the library before the threads do)
            P = self.P

            def one(m):
                k, fl, io = m
                PP = refbind.DpParams(P.mat, go=P.go, ge=P.ge, io=io, fs=P.fs, xdrop=P.xdrop, end_bonus=P.end_bonus, sp=P.sp, sp_null_bonus=P.sp_null_bonus, ie_coef=P.ie_coef)
                return fn(self.pairs[k][0], self.pairs[k][1], PP, fl)
            with ThreadPoolExecutor(max_workers=8) as ex:
                self._expect[which] = list(ex.map(one, self.meta))
        return self._expect[which]


def check_classes(cls, table, split_wide, want):
    """cls: mpa.dbg_dp_last_classes() after the table's run on a context created with the knob at split_wide.  want: the calls of
    X_SPLIT8, X_SPLIT12 and X_HUGE as the test spells them out ({class: calls}, a missing class: none).  They must also be what the rules
    of the classes give for the table, so that a call that quietly took another sweep fails here and not in the values."""
    exp = table.class_counts(split_wide)
    for c, name in ((X_SPLIT8, "X_SPLIT8"), (X_SPLIT12, "X_SPLIT12"), (X_HUGE, "X_HUGE")):
        assert want.get(c, 0) == exp[c], "%s: the test expects %d calls, the rules of the classes give %d" % (name, want.get(c, 0), exp[c])
        assert cls[c] == want.get(c, 0), "%s swept %d calls, expected %d (classes %s)" % (name, cls[c], want.get(c, 0), list(cls))


_TABLES = {}


def _once(key, make):
    """a table is built once per process: its expected values are computed once and shared by the tests that use it"""
    if key not in _TABLES:
        _TABLES[key] = make()
    return _TABLES[key]


def range_tables():
    """name -> (Table, {class: calls} with the knob on): the tables of the range tests that belong to no penalty point or bound case"""
    return _once("range", _range_tables)


def _range_tables():
    t = {}
    P4 = wide_params(cap=4)
    rng = np.random.default_rng(9500)
    t["twelve_blocks"] = (Table(P4, [wide_pair(rng, al, **WIDE_KW) for al in TWELVE_BLOCK_ALS], 9501), {X_SPLIT12: 2 * len(TWELVE_BLOCK_ALS)})
    # right-only, rows descending: (3 072, 2 049) share a group -- one half dies in block 8, the other is live to the end --, the 3 072
    # call cut to 5 000 rows is alone in the next one (an empty half through twelve blocks); 3 073 residues are beyond the class
    rng = np.random.default_rng(9510)
    pairs = [wide_pair(rng, 2049, **WIDE_KW), wide_pair(rng, 3072, **WIDE_KW), wide_pair(rng, 3072, rows=5000, **WIDE_KW), wide_pair(rng, 3073, **WIDE_KW)]
    t["group_shapes"] = (Table(P4, pairs, 9511, modes=("right",)), {X_SPLIT12: 3, X_HUGE: 1})
    rng = np.random.default_rng(9520)
    t["short_windows"] = (Table(P4, [wide_pair(rng, 3072, rows=r, **WIDE_KW) for r in SHORT_ROWS_3072], 9521), {X_SPLIT12: 2 * len(SHORT_ROWS_3072)})
    # flanks of up to 2 000 random bases stop an extension in its first rows; a protein whose middle third is unrelated to the window
    # stops the right extension a third of the way in and the left extension a third of the way from the end
    rng = np.random.default_rng(9530)
    far = wide_pair(rng, 2900, p_intron=0.004, max_intron=200, flank=2000)
    nt, aa = wide_pair(rng, 2900, flank=1, p_intron=0.0, p_fs=0.0, p_sub=0.05)      # (an intron or a frameshift costs about the x-drop itself)
    mid = (nt, aa[:967] + bytes(b"ARNDCQEGHILKMFPSTWYV"[i] for i in rng.integers(0, 20, 966)) + aa[1933:])
    t["xdrop_stops"] = (Table(wide_params(dict(xdrop=30), cap=4), [far, mid], 9531), {X_SPLIT12: 4})
    return t


def penalty_table(kw, lim):
    return _once(("penalty", repr(kw), lim), lambda: _penalty_table(kw, lim))


def _penalty_table(kw, lim):
    """a wide penalty point's batch: left and right extensions at 1 032, min(limit, 2 048), the guard limit and limit + 1 (X_HUGE), with
    calls of every narrower class and traceback calls in the same round"""
    import zlib
    P = wide_params(kw)
    rng = np.random.default_rng(zlib.crc32(("wide" + repr(kw)).encode()))
    als = sorted({1032, min(lim, 2048), lim, lim + 1})
    wide = [wide_pair(rng, al, **WIDE_KW) for al in als]
    mixed = mixed_pairs(rng)
    want = {X_SPLIT8: 2 * sum(al <= 2048 for al in als[:-1]), X_SPLIT12: 2 * sum(al > 2048 for al in als[:-1]), X_HUGE: 2}
    return Table(P, wide + mixed, int(rng.integers(1 << 30)), pair_modes=[BOTH] * len(wide) + [ALL_MODES] * len(mixed)), want


def bound_table(case, over):
    return _once(("bound", repr(case), over), lambda: _bound_table(case, over))


def _bound_table(case, over):
    """a dpgen.WIDE_BOUND_CASES entry with its decisive sum at 32000 + over: a random pair (left and right) and a hot pair for each side
    at al, a random pair at al - 8 and at al + 8.  -> (Table, {class: calls}); the expectation of every call comes from may_saturate."""
    import zlib
    from dpgen import bound_params
    al, cap = case[0], case[3]
    kw = bound_params(case, over)
    P = wide_params(kw, cap)
    rng = np.random.default_rng(zlib.crc32(("wide" + repr(kw) + repr(cap)).encode()))
    pairs = [wide_pair(rng, al, **WIDE_KW), hot_pair(rng, al, mpa.F_EXT_LEFT), hot_pair(rng, al, mpa.F_EXT_RIGHT), wide_pair(rng, al - 8, **WIDE_KW), wide_pair(rng, al + 8, **WIDE_KW)]
    tab = Table(P, pairs, int(rng.integers(1 << 30)), pair_modes=[BOTH, ("left",), ("right",), BOTH, BOTH])
    want = {}
    for a in tab.ext_als():
        c = X_HUGE if may_saturate(a, tab.opt) or a > 3072 else X_SPLIT4 if a <= 1024 else X_SPLIT8 if a <= 2048 else X_SPLIT12
        want[c] = want.get(c, 0) + 1
    want.pop(X_SPLIT4, None)
    return tab, want


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
