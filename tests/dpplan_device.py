"""Task tables for the device planner of a DP round (MPA_GPU_DPPLAN; mpa_dbg_dp_plan_device) and the comparison with the host planner's
serialised plan (mpa_dbg_dp_plan, tests/dpplan.py).  Shared by tests/test_dp_plan_model_cpu.py (the model: ctx None) and
tests/test_dp_plan_gpu.py (a context)."""
import numpy as np
import miniprot_amd as mpa
import dpplan
from dpplan import EXT, GLOB, _spread, _table

C_WIDE = dict(lite_min=3, lite_wide=1)                      # the knob sets of dpplan.cases()' c_wide and k_no_dual_no_prio
K_NO_DUAL_NO_PRIO = dict(ext_dual=0, unit_prio=0)


def planned():
    """name -> (tasks, option overrides, knobs): tables the device planner takes"""
    t = {}
    for k, (name, knobs) in enumerate((("spread_default", {}), ("spread_c_wide", C_WIDE), ("spread_k_no_dual_no_prio", K_NO_DUAL_NO_PRIO))):
        r = np.random.default_rng(9200 + k)
        t[name] = (_table(r, _spread(r, EXT, 120, al_max=1024) + _spread(r, GLOB, 120, al_max=1100)), {}, knobs)   # (1100 columns: T_MB is in)
    # 3 000 calls with four distinct row counts: the index decides most ties in the order, and most unit costs are equal
    r = np.random.default_rng(9210)
    nls = [50, 200, 400, 900]
    spec = [((EXT, GLOB)[int(r.integers(0, 2))], int(r.integers(1, 301)), int(r.choice(nls))) for _ in range(3000)]
    t["ties_3000"] = (_table(r, spec), {}, C_WIDE)
    # class runs that are no multiple of the calls per wave
    for n in (1, 7, 8, 9):
        r = np.random.default_rng(9220 + n)
        t["x16_run_%d" % n] = (_table(r, [(EXT, int(r.integers(1, 17)), int(r.integers(3, 900))) for _ in range(n)] + [(EXT, 40, 100), (GLOB, 20, 50)]), {}, {})
    for n in (1, 3):
        r = np.random.default_rng(9230 + n)
        t["lite_w4_run_%d" % n] = (_table(r, [(GLOB, int(r.integers(129, 257)), int(r.integers(400, 2000))) for _ in range(n)] + [(GLOB, 20, 500)]), {}, dict(lite_wide=1))
    # the prep chunk edge, and the shortest window
    r = np.random.default_rng(9240)
    t["prep_chunk_edge"] = (_table(r, [(m, al, nl) for m in (EXT, GLOB) for al in (30, 200) for nl in (1023, 1024, 1025, 3)]), {}, {})
    r = np.random.default_rng(9241)
    t["only_ext"] = (_table(r, _spread(r, EXT, 60, al_max=1024)), {}, {})
    r = np.random.default_rng(9242)
    t["only_glob"] = (_table(r, _spread(r, GLOB, 60, al_max=1100)), {}, {})
    r = np.random.default_rng(9243)
    t["one_ext"] = (_table(r, [(EXT, 77, 300)]), {}, {})
    t["one_glob"] = (_table(r, [(GLOB, 77, 500)]), {}, {})
    c = dpplan.cases()
    for name in ("b_glob", "c_wide", "k_no_dual_no_prio"):
        t["cases_" + name] = c[name]
    # extension calls of fewer than three rows (class X_NONE: no descriptor, no unit) of every width -- 1 100 columns too, which with more
    # rows is the class the device planner declines -- between ordinary calls and traceback calls of as few rows
    r = np.random.default_rng(9244)
    spec = [(EXT, al, nl) for nl in (0, 1, 2) for al in (1, 8, 24, 50, 100, 200, 400, 800, 1025, 1100)] + [(GLOB, al, nl) for nl in (0, 1, 2) for al in (1, 40, 300, 1100)]
    spec += _spread(r, EXT, 20, al_max=1024) + _spread(r, GLOB, 20, al_max=300)
    t["tiny_ext"] = (_table(r, [spec[k] for k in r.permutation(len(spec))]), {}, {})
    return t


def big():
    """20 000 calls of at most 64 rows"""
    r = np.random.default_rng(9250)
    spec = [((EXT, GLOB)[int(r.integers(0, 2))], int(r.integers(1, 201)), int(r.integers(3, 65))) for _ in range(20000)]
    return _table(r, spec), {}, {}


DECLINED_CASES = ("a_ext", "d_budget", "e_wide_ge", "f_saturate", "g_no_split", "h_pool", "i_antidiag")


def declined():
    """name -> (tasks, option overrides, knobs): tables the device planner leaves to the host planner"""
    c = dpplan.cases()
    t = {name: c[name] for name in DECLINED_CASES}
    for name, (tasks, over) in dpplan.refusals().items():
        t["refusal_" + name] = (tasks, over, {})
    return t


def device_plan(ctx, tasks, opt_over=None, knobs=None):
    """-> dpplan.Plan, or (code, message)"""
    kn = dict(dpplan.KNOBS)
    kn.update(knobs or {})
    r = mpa.dbg_dp_plan_device(ctx, dpplan.dpopt(**(opt_over or {})), dpplan.CTG_LEN, dpplan.q_off(), tasks, kn)
    return r if isinstance(r, tuple) else dpplan.Plan(r)


def assert_same_plan(got, want):
    """every section and every header field, byte for byte"""
    assert isinstance(want, dpplan.Plan), want
    assert isinstance(got, dpplan.Plan), got
    diff = {k: (got.header[k], want.header[k]) for k in dpplan.HEADER if got.header[k] != want.header[k]}
    assert not diff, diff
    for name in dpplan.SECTIONS:
        if got.raw[name] != want.raw[name]:
            a, b = got.sec[name], want.sec[name]
            assert len(a) == len(b), (name, len(a), len(b))
            first = next(k for k in range(len(a)) if a[k] != b[k])
            raise AssertionError("section %s differs first at record %d of %d: %r != %r" % (name, first, len(a), a[first], b[first]))
