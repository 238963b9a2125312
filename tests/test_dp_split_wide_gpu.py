"""MPA_DP_SPLIT_WIDE on the GPU: extension calls of 1 025..3 072 columns swept by 8 / 12 workgroups (X_SPLIT8 / X_SPLIT12) against the
oracle, bit-exact on (nt_len, aa_len, score); the same tables on a context without the knob (k_ext_huge); the guard; the forced hand-off
failure; four contexts at once; the device planner.  mpa_dbg_dp_last_classes says which class swept the calls."""
import os
import subprocess
import sys
import threading
import numpy as np
import pytest
import miniprot_amd as mpa
import refbind
import splitwide as sw
from dpgen import make_task
from dputil import build_workload, oracle_eval, dpopt_from_params, compare

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDE_KW = dict(p_intron=0.004, max_intron=200, flank=30)            # rows = 3 al + a few short introns


def params(**kw):
    return refbind.DpParams(refbind.mapping_matrix(23), **kw)


def guard(P):
    return sw.guard_limit(dpopt_from_params(P))


@pytest.fixture(scope="module")
def ctx_on():
    with sw.knob("1"):
        c = mpa.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def ctx_off():
    with sw.knob(None):
        c = mpa.Context(0)
    yield c
    c.close()


class Workload:
    """a table with its oracle results, computed once"""

    def __init__(self, pairs, P, seed, modes=("left", "right")):
        self.pairs, self.P = pairs, P
        self.contigs, self.queries, self.tasks, self.meta = build_workload(pairs, np.random.default_rng(seed), modes=modes, io=P.io)
        self.expect = oracle_eval(pairs, self.meta, P)
        self.n_wide = sum(1 for k, _, _ in self.meta if len(pairs[k][1]) > 1024)

    def results(self, ctx):
        idx = mpa.Index.from_nt4(self.contigs)
        idx.to_device(ctx)
        rst, cig = mpa.dp_run(ctx, idx, dpopt_from_params(self.P), self.queries, self.tasks)
        idx.close()
        return rst, cig

    def run(self, ctx):
        rst, cig = self.results(ctx)
        bad, msg = compare(rst, cig, self.expect, self.meta, self.pairs)
        assert not bad, "%d/%d DP calls differ from the oracle\n%s" % (len(bad), len(self.tasks), msg)
        return mpa.dbg_dp_last_classes(ctx)


def check_on(ctx, w, n_huge=0):
    cls = w.run(ctx)
    assert cls[sw.X_HUGE] == n_huge and cls[sw.X_SPLIT8] + cls[sw.X_SPLIT12] == w.n_wide - n_huge, cls
    assert ctx.handoff_retries() == 0
    return cls


def check_off(ctx, w):
    cls = w.run(ctx)
    assert cls[sw.X_HUGE] == w.n_wide and cls[sw.X_SPLIT8] + cls[sw.X_SPLIT12] == 0, cls


def singles(k):
    P = params()
    als = ((1025, 1032, 1280, 1281), (1536, 2040, 2048, 2049), (2305, guard(P)))[k]
    rng = np.random.default_rng(9400 + k)
    pairs = [sw.wide_pair(rng, al, **WIDE_KW) for al in als]
    if k == 2:
        pairs += [make_task(rng) for _ in range(40)]                 # 40 ordinary pairs in the same batch
    return Workload(pairs, P, 9410 + k)


def shared_groups():
    """(1 100, 2 000): unequal widths in one 8-workgroup group; (2 049, 2 100): 12 workgroups of which three are dead; a lone call"""
    P = params()
    rng = np.random.default_rng(9420)
    return [Workload([sw.wide_pair(rng, al, **WIDE_KW) for al in als], P, 9421 + k, modes=(("right",), ("left",), ("right",))[k]) for k, als in enumerate(((1100, 2000), (2049, 2100), (1500,)))]


def xdrop_table():
    P = params(xdrop=30, end_bonus=11)
    rng = np.random.default_rng(9430)
    return Workload([sw.wide_pair(rng, al, p_intron=0.004, max_intron=200, flank=2000, p_indel=0.0) for al in (1300, 2100)], P, 9431)


def short_windows(al, rows):
    P = params()
    rng = np.random.default_rng(9440 + al)
    return Workload([sw.wide_pair(rng, al, rows=r, **WIDE_KW) for r in rows], P, 9441 + al, modes=("right",) if al == 1500 else ("left",))


SHORT_ROWS = (3, 13, 14, 26, 49, 97)        # the generic rows alone, the first asm block, one and two fetches from the left, a wrap of the 96-row rings


# ---- 1. against the oracle, every wide call in a new class
@pytest.mark.parametrize("k", [0, 1, 2])
def test_single_widths(ctx_on, oracle_built, k):
    """each width as a left and a right extension (the two share a group).  On the parent no call is in X_SPLIT8 / X_SPLIT12."""
    w = singles(k)
    cls = check_on(ctx_on, w)
    if k < 2:
        assert (cls[sw.X_SPLIT8], cls[sw.X_SPLIT12]) == ((8, 0), (6, 2))[k]


def test_calls_that_share_a_group(ctx_on, oracle_built):
    want = ((2, 0), (0, 2), (1, 0))
    for w, n in zip(shared_groups(), want):
        cls = check_on(ctx_on, w)
        assert (cls[sw.X_SPLIT8], cls[sw.X_SPLIT12]) == n


def test_xdrop_stops_a_wide_extension(ctx_on, oracle_built):
    check_on(ctx_on, xdrop_table())


@pytest.mark.parametrize("al", [1500, 2100])
def test_short_windows(ctx_on, oracle_built, al):
    check_on(ctx_on, short_windows(al, SHORT_ROWS))


def test_two_row_windows(ctx_on, ctx_off, oracle_built):
    """A window of two rows has no DP row at all.  The reference does not define the result: its search for the best column runs over a
    row it never filled and ends in assert(j < al) (nasw-sse.c:436-441); the oracle, a restatement without the assert, reports
    (0, al + 1, INT32_MIN), and that is the contract of mpa_dp_run() (include/mpamd.h).  Every extension kernel of this project would
    report aa_len 0 (measured on the MI355X before the contract was set), so the planner gives such a call no unit -- class X_NONE with
    the knob on and off, no X_SPLIT8 / X_SPLIT12 group, no X_HUGE call -- and the result rule writes the triple."""
    P = params()
    rng = np.random.default_rng(9450)
    w = Workload([sw.wide_pair(rng, al, rows=2, **WIDE_KW) for al in (1500, 2100)], P, 9451, modes=("right",))
    on, _ = w.results(ctx_on)
    cls = mpa.dbg_dp_last_classes(ctx_on)
    assert (cls[sw.X_SPLIT8], cls[sw.X_SPLIT12], cls[sw.X_HUGE], cls[mpa.X_NONE]) == (0, 0, 0, 2)
    off, _ = w.results(ctx_off)
    cls = mpa.dbg_dp_last_classes(ctx_off)
    assert (cls[sw.X_HUGE], cls[mpa.X_NONE]) == (0, 2)
    for k, e in enumerate(w.expect):
        assert e[:3] == (0, len(w.pairs[k][1]) + 1, -2 ** 31)
        for r in (on[k], off[k]):
            assert (int(r["nt_len"]), int(r["aa_len"]), int(r["score"])) == e[:3], (k, r, e[:3])


# ---- 2. knob off: the same tables as X_HUGE; knob on at the guard
def test_knob_off_runs_the_one_wave_sweep(ctx_off, oracle_built):
    for w in [singles(1)] + shared_groups() + [short_windows(1500, SHORT_ROWS)]:
        check_off(ctx_off, w)


def test_past_the_guard_stays_on_the_one_wave_sweep(ctx_on, oracle_built):
    P = params()
    g = guard(P)
    rng = np.random.default_rng(9460)
    w = Workload([sw.wide_pair(rng, al, **WIDE_KW) for al in (g, g + 1)], P, 9461)
    cls = check_on(ctx_on, w, n_huge=2)
    assert cls[sw.X_SPLIT12] == 2


# ---- 3. forced hand-off failure: the round is repeated with the calls on k_ext_huge
def test_forced_handoff_failure(oracle_built):
    code = ("import numpy as np, sys; sys.path.insert(0, 'tests'); import conftest, miniprot_amd as mpa\n"
            "import test_dp_split_wide_gpu as t, splitwide as sw\n"
            "rng = np.random.default_rng(9470); P = t.params()\n"
            "pairs = [sw.wide_pair(rng, al, **t.WIDE_KW) for al in (1100, 2100)] + [t.make_task(rng, al=al) for al in (40, 90)]\n"
            "w = t.Workload(pairs, P, 9471)\n"
            "ctx = mpa.Context(0)\n"
            "cls = w.run(ctx)\n"
            "print('retries', ctx.handoff_retries(), 'huge', cls[sw.X_HUGE], 'split', cls[sw.X_SPLIT8] + cls[sw.X_SPLIT12])\n")
    env = dict(os.environ, MPA_TEST_HANDOFF_FAIL="1", MPA_DP_SPLIT_WIDE="1")
    out = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "retries 1 huge 4 split 0" in out.stdout, out.stdout + out.stderr


# ---- 4. load: four contexts on four host threads
def test_four_contexts_at_once(oracle_built):
    P = params()
    rng = np.random.default_rng(9480)
    w = Workload([sw.wide_pair(rng, al, **WIDE_KW) for al in (1100, 1600, 2048, 2500)] + [make_task(rng) for _ in range(60)], P, 9481)
    errs = []

    def worker():
        try:
            with lock, sw.knob("1"):
                c = mpa.Context(0)
            for _ in range(2):
                check_on(c, w)
            c.close()
        except BaseException as e:                                   # noqa: BLE001 (reported in the main thread)
            errs.append(repr(e))

    lock = threading.Lock()
    th = [threading.Thread(target=worker) for _ in range(4)]
    [t.start() for t in th]
    [t.join() for t in th]
    assert not errs, errs


# ---- 5. the device planner
@pytest.mark.parametrize("name", ["a_ext_to_the_guard", "odd_counts", "mixed_3000"])
def test_device_planner_equals_the_host_planner(ctx_on, name):
    tasks, over = sw.planner_tables()[name]
    want, got = sw.plan(tasks, over), sw.device_plan(ctx_on, tasks, over)
    assert isinstance(want, sw.WidePlan), want
    assert isinstance(got, sw.WidePlan), got
    assert got.buf == want.buf


def test_rounds_planned_on_the_device(oracle_built):
    """MPA_GPU_DPPLAN=1: a table whose wide calls fit the new classes is not declined; one call past the guard and it is, as before"""
    code = ("import numpy as np, sys; sys.path.insert(0, 'tests'); import conftest, miniprot_amd as mpa\n"
            "import test_dp_split_wide_gpu as t, splitwide as sw\n"
            "P = t.params(); g = t.guard(P); past = int(sys.argv[1])\n"
            "rng = np.random.default_rng(9490)\n"
            "als = [1, 8, 17, 33, 65, 129, 257, 513, 1024, 1025, 1100, 2049, g + past]\n"
            "pairs = [sw.wide_pair(rng, al, **t.WIDE_KW) for al in als] + [t.make_task(rng) for _ in range(30)]\n"
            "w = t.Workload(pairs, P, 9491, modes=('right',))\n"
            "ctx = mpa.Context(0)\n"
            "cls = w.run(ctx)\n"
            "print('huge', cls[sw.X_HUGE], 'split', cls[sw.X_SPLIT8] + cls[sw.X_SPLIT12])\n")
    env = dict(os.environ, MPA_GPU_DPPLAN="1", MPA_DP_SPLIT_WIDE="1", MPA_TIMING="1")
    out = subprocess.run([sys.executable, "-c", code, "0"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "huge 0 split 4" in out.stdout and "plan on device" in out.stderr and "declined" not in out.stderr, out.stdout + out.stderr
    out = subprocess.run([sys.executable, "-c", code, "1"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "huge 1 split 3" in out.stdout and "one-wave int32" in out.stderr, out.stdout + out.stderr


# ---- 6. the whole path: a protein whose last 400 residues are planted has a left extension of about 2 000 columns
SPLIT_NOTE = "groups of the 2048- / 3072-column extension classes"


def test_whole_path(monkeypatch, capfd):
    """the reference's bytes (PAF and GFF) with the knob off, with the knob on, and with every device knob together; with the knob on a
    round sweeps a call in one of the new classes (the rounds of mpa_map_batch run on the context's DP lanes: the note of MPA_TIMING=1
    says so, where mpa_dbg_dp_last_classes of one context would show the last round of that lane only)"""
    import golden
    from hostpipe import map_batch_gpu
    contigs, prots, names = sw.whole_path_case()
    q = mpa.Queries(prots, names)
    case = dict(genome=sw.WP_GENOME, n_ctg=1, flags=sw.WP_FLAGS)
    monkeypatch.setenv("MPA_TIMING", "1")
    for dev in sw.DEVICE_KNOBS:
        monkeypatch.delenv(dev, raising=False)
    for leg in ("off", "on", "on_all_device_knobs"):
        if leg == "on_all_device_knobs":
            for dev in sw.DEVICE_KNOBS:
                monkeypatch.setenv(dev, "1")
        with sw.knob(None if leg == "off" else "1"):
            ctx = mpa.Context(0)
        idx = mpa.Index.from_nt4(contigs, ["chr1"])
        mpa._check(mpa.lib().mpa_idx_build_kmers(idx.h, 4))
        idx.to_device(ctx)
        for ext, flags in ((".ref.paf", sw.WP_FLAGS), (".ref.gff", sw.WP_FLAGS + ["--gff"])):
            mo = golden.apply_flags(mpa.default_mapopt(), flags, case)
            capfd.readouterr()
            ours = golden.file_header(dict(flags=flags)) + map_batch_gpu(ctx, idx, mo, q, 4)
            notes = capfd.readouterr().err
            assert ours == open(golden.path("split_wide" + ext), "rb").read(), (leg, ext)
            assert (SPLIT_NOTE in notes) == (leg != "off"), (leg, ext)
            assert "one-wave int32" not in notes or leg != "on_all_device_knobs", (leg, ext)
        idx.close()
        ctx.close()
