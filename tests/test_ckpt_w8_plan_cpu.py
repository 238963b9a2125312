"""The checkpointed traceback class of 257..512-column calls (T_LITE_W8, MPA_DP_LITE_W8) in the host planner, through mpa_dbg_dp_plan_w8 (no
device): which calls take the class -- both sides of 256 and of 512 columns, of the row threshold, of the int16 bound; what keeps the
plain sweep -- a gap extension above 255, the worker pool, the knob at 0; how its calls are packed (two per eight-wave group, pools by
the group's longer call, no traceback-matrix words, a sixth walk list); and that with the knob at 0 the plan is, byte for byte, the one
mpa_dbg_dp_plan_wide and mpa_dbg_dp_plan give."""
import struct
import numpy as np
import pytest
import miniprot_amd as mpa
import dpplan
from dpgen import BOUND_CASES, bound_params

T_W4, T_W8, T_W16, T_LITE128, T_LITE_W4, T_LITE_W8 = 4, 5, 6, 11, 12, 13          # DpClass, traceback calls (dp_device.h)
TB_BLOCK = 96
KN = dict(dpplan.KNOBS, split_wide=0)


def _plan(tasks, over=None, **knobs):
    """-> (Plan, (first, count of T_LITE_W8 descriptors, calls of its walk list), the bytes)"""
    kn = dict(KN)
    kn.update(knobs)
    buf = mpa.dbg_dp_plan_w8(dpplan.dpopt(**(over or {})), dpplan.CTG_LEN, dpplan.q_off(), tasks, kn)
    assert isinstance(buf, bytes), buf
    return dpplan.Plan(buf), struct.unpack("<3q", buf[-mpa.DP_PLAN_W8_TAIL:]), buf


def _glob(spec, seed=9300):
    return dpplan._table(np.random.default_rng(seed), [(dpplan.GLOB, al, nl) for al, nl in spec])


def _ncol(al):
    return (al + 7) // 8 * 8


def _plain(al):
    c = 0
    while c < 7 and _ncol(al) > (16 << c):
        c += 1
    return c


EDGE_ALS = (249, 256, 257, 264, 505, 512, 513, 520)


@pytest.mark.parametrize("lite_min", [3, 100, 384])
def test_routing_at_the_class_edges(lite_min):
    """columns on both sides of 256 and of 512 (8 * ceil(al / 8) decides) at rows on both sides of the threshold: with both knobs set the
    calls of 257..512 columns and at least lite_min rows take class 13, those of 129..256 class 12, wider ones and shorter ones the
    plain sweep of their width; MPA_DP_LITE_WIDE does not matter to class 13, nor MPA_DP_LITE_W8 to class 12"""
    spec = [(al, nl) for al in EDGE_ALS for nl in (max(3, lite_min - 1), lite_min, lite_min + 1, 1200)]
    tasks = _glob(spec)
    for wide in (0, 1):
        for w8 in (0, 1):
            P, tail, _ = _plan(tasks, lite_min=lite_min, lite_wide=wide, lite_w8=w8)
            n_w8 = 0
            for (al, nl), t in zip(spec, P.sec["tasks"]):
                want = _plain(al)
                many = nl >= max(lite_min, 3)
                if many and want == T_W4 and wide:
                    want = T_LITE_W4
                if many and want == T_W8 and w8:
                    want = T_LITE_W8
                    assert t["pw"] == 512
                    n_w8 += 1
                assert t["cls"] == want, (al, nl, wide, w8, int(t["cls"]), want)
            assert tail[2] == n_w8 and tail[1] == (n_w8 + 1) // 2
            assert (n_w8 > 0) == (w8 == 1)


@pytest.mark.parametrize("over", [0, 1], ids=["at32000", "at32001"])
def test_int16_bound(over):
    """BOUND_CASES' 512-column entry: al * max_mat + ncol * ge + end_bonus at exactly 32 000 takes the packed sweep, at 32 001 the int32 one"""
    case = [c for c in BOUND_CASES if c[0] == 512][0]
    kw = bound_params(case, over)
    o = dpplan.dpopt(**kw)
    assert 512 * int(max(o.mat)) + 512 * o.ge + o.end_bonus == 32000 + over and o.go + 512 * o.ge <= 32000
    P, tail, _ = _plan(_glob([(512, 400), (504, 400), (300, 400)]), kw, lite_w8=1)
    cls = [int(c) for c in P.sec["tasks"]["cls"]]
    assert cls[0] == (T_LITE_W8 if over == 0 else T_W8), cls
    assert cls[1] == T_LITE_W8 and cls[2] == T_LITE_W8, cls                 # (narrower calls stay under the bound)
    assert tail[2] == 3 - over


def test_what_keeps_the_plain_sweep():
    """a gap extension of 300 (the records' byte), the worker pool, the knob at 0"""
    tasks = _glob([(300, 500), (400, 900), (512, 384), (200, 500)])
    for over, kn in ((dict(ge=300), dict(lite_w8=1, lite_min=3)), ({}, dict(lite_w8=1, pool=1, lite_min=3)), ({}, dict(lite_w8=0, lite_min=3))):
        P, tail, _ = _plan(tasks, over, **kn)
        assert [int(c) for c in P.sec["tasks"]["cls"][:3]] == [T_W8] * 3, (over, kn)
        assert tail[1] == 0 and tail[2] == 0
    P, tail, _ = _plan(tasks, {}, lite_w8=1, lite_min=3)
    assert [int(c) for c in P.sec["tasks"]["cls"][:3]] == [T_LITE_W8] * 3 and tail[1:] == (2, 3)


def test_packing_pools_and_walk_list():
    """two calls per group in (rows descending) order, a lone one last; bit words and checkpoints of the documented size per group, sized by
    the group's longer call, back to back behind class 12's; no traceback-matrix words for the class; the sixth walk list"""
    nls = [3, 4, 5, 23, 24, 25, 97, 98, 99, 194, 300, 1500, 100]
    spec = [(int(al), nl) for al, nl in zip(np.random.default_rng(9301).integers(257, 513, len(nls)), nls)]
    spec += [(200, 700), (150, 50), (300, 2), (100, 500), (40, 400), (600, 400)]
    tasks = _glob(spec, 9302)
    P, (first, cnt, n_walk), _ = _plan(tasks, lite_min=3, lite_wide=1, lite_w8=1)
    H, S = P.header, P.sec
    T, EW = S["tasks"], S["ewaves"]
    w8 = np.nonzero(T["cls"] == T_LITE_W8)[0]
    assert len(w8) == len(nls) == n_walk and cnt == (len(nls) + 1) // 2
    assert T["cls"][len(nls) + 2] == T_W8, "a call of fewer than three rows keeps the plain class"
    assert first + cnt == H["n_ewaves"] and first == H["l12_first"] + H["l12_cnt"], "class 13's descriptors are the last, behind class 12's"
    order = sorted(w8, key=lambda k: (-int(T["nl"][k]), k))
    at_l = at_c = None
    for g in range(cnt):
        w = EW[first + g]
        ids = [int(x) for x in w["task"] if x >= 0]
        assert ids == [int(x) for x in order[2 * g:2 * g + 2]] and (w["task"][len(ids):] == -1).all()
        max_nl = int(T["nl"][ids].max())
        assert w["max_nl"] == max_nl == int(T["nl"][ids[0]])
        if at_l is None:
            at_l, at_c = int(w["lite_off"]), int(w["ck_off"])
        assert (int(w["lite_off"]), int(w["ck_off"])) == (at_l, at_c)
        at_l += (max_nl // 3 + 2) * 512
        at_c += (max(0, (max_nl - 3) // TB_BLOCK) if max_nl > 3 else 0) * 9 * 512
        assert list((T["flag"][ids] >> 8) & 15) == list(range(len(ids)))
        assert (T["tb_off"][ids] == w["lite_off"]).all() and (T["bnd_off"][ids] == w["ck_off"]).all()
    assert (at_l, at_c) == (H["lite_total"], H["ck_total"]) and H["lite_total"] * 4 <= H["sz_lite"] and H["ck_total"] * 4 <= H["sz_ckpt"]
    # no traceback-matrix words: the chunks' words are those of the plain-sweep calls alone
    plain = [k for k in range(len(T)) if T["cls"][k] < 8]
    assert sum(int(r["tb_words"]) for r in S["chunk_tab"]) == sum(int(T["nl"][k]) * int(T["ncol"][k]) for k in plain)
    assert H["n_reg_glob"] == len(plain) and H["n_lite"] == len(T) - len(plain)
    # the walk lists: classes 8 .. 12 as before, class 13's calls behind them
    assert int(S["walk_launches"].sum()) + n_walk == H["n_lite"] and len(S["walk_launches"]) == 5
    assert sorted(S["wlist"][-n_walk:]) == sorted(w8) and (T["cls"][S["wlist"][:-n_walk]] < T_LITE_W8).all()
    assert H["st_n_glob"] == len(T) and H["st_n_ckpt"] + H["st_n_ckpt_wide"] == H["n_lite"]
    # no unit of the round names the class's descriptors: its groups are k_lite_w8's
    for u in S["units"]:
        if u["kind"] in (12, 13, 14, 15, 17):
            assert u["first"] + u["count"] <= first


@pytest.mark.parametrize("name", ["b_glob", "c_wide", "d_budget", "h_pool"])
def test_knob_off_is_todays_plan(name):
    """tables that hold traceback calls of 257..512 columns and many rows: with the knob at 0 the serialisation is mpa_dbg_dp_plan_wide's and
    mpa_dbg_dp_plan's byte for byte (tests/test_dp_plan_cpu.py pins those to the recorded digests), with three zero words behind"""
    tasks, over, kn = dpplan.cases()[name]
    T8 = [t for t in tasks if not (t["flag"] & (mpa.F_EXT_LEFT | mpa.F_EXT_RIGHT)) and 256 < _ncol(int(t["al"])) <= 512 and t["nl"] >= kn.get("lite_min", 384)]
    assert T8, "the table holds calls the class would take"
    knobs = dict(KN, **kn)
    P, tail, buf = _plan(tasks, over, **dict(kn, lite_w8=0))
    wide = mpa.dbg_dp_plan_wide(dpplan.dpopt(**over), dpplan.CTG_LEN, dpplan.q_off(), tasks, knobs)
    plain = mpa.dbg_dp_plan(dpplan.dpopt(**over), dpplan.CTG_LEN, dpplan.q_off(), tasks, {k: knobs[k] for k in dpplan.KNOBS})
    assert buf[:-mpa.DP_PLAN_W8_TAIL] == wide and wide[:-mpa.DP_PLAN_WIDE_TAIL] == plain
    assert tail[1:] == (0, 0) and tail[0] == P.header["n_ewaves"]
    assert P.digests() == dpplan.golden()["cases"][name]["digest"], "the plan of the recorded digests"
    if not knobs["pool"]:
        _, tail_on, buf_on = _plan(tasks, over, **dict(kn, lite_w8=1))
        assert tail_on[2] == len(T8) and buf_on != buf
