"""The plan of a DP round (dp_plan.cpp through mpa_dbg_dp_plan: what mpa_dp_run would upload and launch for a task table; no device):
1. invariants of the plan, computed from its serialised sections -- every call in exactly one slot of one descriptor, descriptors of
   one class, pool ranges disjoint and inside the sizes asked for, traceback chunks under the budget, the unit list covering the
   round's descriptors exactly once in the order the kernels rely on;
2. identity with the executor before the planner was split off: a 64-bit FNV-1a digest per section and case equals the digest that
   mpa_dp_run_impl of the parent of that commit produced for the same table (tests/golden/dp_plan_digests.json says how they were recorded);
   a digest that differs means the plan changed -- order, priorities, packing included, which no GPU test would notice;
3. the planner alone, built with the host compiler under AddressSanitizer / UBSan, over a few hundred random tables.
The tables (tests/dpplan.py) hold lengths only: sequence content never reaches the planner."""
import os
import subprocess
import numpy as np
import pytest
import miniprot_amd as mpa
import dpplan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = dpplan.cases()
_plans = {}

# DpUnitKind (dp_device.h)
(U_EXT16, U_EXT32, U_EXT64, U_EXT_W2, U_EXT_W4, U_EXT_SPLIT, U_GLOB16, U_GLOB32, U_GLOB64, U_GLOB_MB, U_GLOB_W2, U_GLOB_W4,
 U_LITE16, U_LITE32, U_LITE64, U_LITE128, U_EXT128, U_LITE_W4) = range(18)
X_32, X_W2, X_SPLIT2, X_SPLIT4, X_HUGE, X_128 = 1, 3, 5, 6, 7, 8                       # DpClass, extension calls
T_W2, T_W4, T_W8, T_W16, T_MB, T_LITE16, T_LITE128, T_LITE_W4 = 3, 4, 5, 6, 7, 8, 11, 12   # ... traceback calls
TB_BLOCK = 96
GROUP_KINDS = (U_EXT_W4, U_EXT_SPLIT, U_GLOB_W4)


def the_plan(name):
    if name not in _plans:                                             # (planned once, shared by the tests, never modified)
        tasks, over, kn = CASES[name]
        _plans[name] = dpplan.plan(tasks, over, kn)
        assert isinstance(_plans[name], dpplan.Plan), (name, _plans[name])
    return _plans[name]


def is_ext(t):
    return (t["flag"] & (mpa.F_EXT_LEFT | mpa.F_EXT_RIGHT)) != 0


def disjoint_inside(ranges, limit, what):
    """half-open ranges, pairwise disjoint and inside [0, limit)"""
    end = 0
    for lo, hi in sorted(ranges):
        assert lo >= end and hi >= lo, (what, lo, hi, end)
        end = hi
    assert end <= limit, (what, end, limit)


def lite_dwords(cls, max_nl):
    """(extension-bit dwords, checkpoint dwords) of one packed-sweep descriptor: dp_device.h, lanes of one wave or (class 12) of four"""
    lanes = 256 if cls == T_LITE_W4 else 64
    return (max_nl // 3 + 2) * lanes, (max(0, (max_nl - 3) // TB_BLOCK) if max_nl > 3 else 0) * 9 * lanes


@pytest.mark.parametrize("name", sorted(CASES))
def test_invariants(name):
    P = the_plan(name)
    H, S = P.header, P.sec
    kn = dict(dpplan.KNOBS, **CASES[name][2])
    T, EW, U = S["tasks"], S["ewaves"], S["units"]
    n = H["n"]
    assert len(T) == n == len(CASES[name][0]) and list(T["out_idx"]) == list(range(n))
    ext = is_ext(T)
    # ---- every call in exactly one slot of exactly one wave descriptor, chunk GlobWave or huge list; descriptors of one class
    seen = np.zeros(n, dtype=int)
    ck = S["chunk_tab"]
    assert len(ck) == H["n_tb_chunks"] and int(ck["n_gw"].sum()) == len(S["gwaves"])
    for waves, is_extwave in ((EW, True), (S["gwaves"], False), (S["huge_waves"], False)):
        for w in waves:
            ids = w["task"][w["task"] >= 0]
            assert len(ids) >= 1 and (w["task"][:len(ids)] >= 0).all(), "slots are filled from the front"
            np.add.at(seen, ids, 1)
            assert len(set(T["cls"][ids])) == 1 and len(set(ext[ids])) == 1, "the calls of a descriptor share a class"
            assert w["max_nl"] == T["nl"][ids].max()
            if is_extwave:
                assert w["rec_base"] == T["rec_off"][ids].min()
    assert (seen == 1).all(), np.nonzero(seen != 1)
    assert list(S["huge_waves"]["task"][:, 0]) == list(S["huge_list"]) and len(S["huge_list"]) == H["n_huge"]
    assert set(S["huge_list"]) == set(np.nonzero(ext & (T["cls"] == X_HUGE))[0])
    assert sorted(S["glist"]) == sorted(S["gwaves"]["task"][S["gwaves"]["task"] >= 0])
    lite_calls = np.nonzero(~ext & (T["cls"] >= T_LITE16))[0]
    assert sorted(S["wlist"]) == sorted(lite_calls) and H["n_lite"] == len(lite_calls)
    if H["n_lite"]:                                                    # the walk: one launch per class over consecutive stretches of the list
        assert S["walk_launches"].sum() == H["n_lite"]
        at = 0
        for c, cnt in enumerate(S["walk_launches"]):
            assert (T["cls"][S["wlist"][at:at + cnt]] == T_LITE16 + c).all()
            at += cnt
    # ---- pool ranges: pairwise disjoint, inside the size asked for
    rec_end = int((T["rec_off"] + T["nl"]).max())
    disjoint_inside([(int(t["rec_off"]), int(t["rec_off"] + t["nl"])) for t in T], H["rec_total"] - H["rec_pad"], "records")
    assert rec_end + H["rec_pad"] <= H["rec_total"] and H["rec_total"] * 4 <= H["sz_rec"], "the prefetch padding behind the last record lies inside the pool"
    assert H["rec_pad"] >= H["max_nl"] + 96 and H["max_nl"] == T["nl"].max()
    disjoint_inside([(int(t["prof_off"]), int(t["prof_off"] + 22 * t["pw"])) for t in T], H["prof_total"], "profiles")
    assert (T["pw"] >= T["ncol"]).all() and H["prof_total"] * 2 <= H["sz_prof"]
    G = T[~ext]
    disjoint_inside([(int(t["cig_off"]), int(t["cig_off"] + t["cig_cap"])) for t in G], H["cig_total"], "CIGAR slots")
    assert (G["cig_cap"] >= G["nl"] + G["al"]).all() and H["cig_total"] * 4 <= H["sz_cig"]
    bnd = T[(ext & (T["cls"] == X_HUGE)) | (~ext & (T["cls"] == T_MB))]
    disjoint_inside([(int(t["bnd_off"]), int(t["bnd_off"] + t["nl"])) for t in bnd], H["bnd_total"], "boundary scratch")
    assert H["bnd_total"] * 16 <= H["sz_bnd"]
    huge = T[ext & (T["cls"] == X_HUGE)]
    disjoint_inside([(int(t["tb_off"]), int(t["tb_off"] + t["nl"])) for t in huge], H["hkey_total"], "huge-call keys")
    assert ((H["hkey_total"] * 8 + 15) & ~15) + (32 + 4) * H["n_huge"] <= H["sz_hkey"], "keys, then the huge calls' waves and list"
    lite_at, ck_at = 0, 0                                               # bit words and checkpoints: one range per descriptor, back to back, of the documented size
    lite_w = [w for w in EW if not ext[w["task"][0]] and T["cls"][w["task"][0]] >= T_LITE16]
    for w in lite_w:
        ids = w["task"][w["task"] >= 0]
        cls = int(T["cls"][ids[0]])
        assert w["lite_off"] == lite_at and w["ck_off"] == ck_at, "ranges equal lite_wide_bits_dwords / lite_wide_ckpt_dwords (class 12) or their one-wave form"
        bits, ckpt = lite_dwords(cls, int(w["max_nl"]))
        lite_at, ck_at = lite_at + bits, ck_at + ckpt
        assert (T["tb_off"][ids] == w["lite_off"]).all() and (T["bnd_off"][ids] == w["ck_off"]).all()
        assert list((T["flag"][ids] >> 8) & 15) == list(range(len(ids))), "the call's slot in its wave"
    assert lite_at == H["lite_total"] and ck_at == H["ck_total"] and H["lite_total"] * 4 <= H["sz_lite"] and H["ck_total"] * 4 <= H["sz_ckpt"]
    # ---- traceback chunks: contiguous over the plain-sweep calls, words inside the pool and under the budget unless a call alone exceeds it
    at, gw_at = 0, 0
    for r in ck:
        assert r["first"] == at and r["last"] > r["first"]
        at = int(r["last"])
        ids = S["gwaves"][gw_at:gw_at + r["n_gw"]]["task"]
        ids = ids[ids >= 0]
        gw_at += int(r["n_gw"])
        assert len(ids) == r["last"] - r["first"]
        disjoint_inside([(int(t["tb_off"]), int(t["tb_off"] + t["nl"] * t["ncol"])) for t in T[ids]], r["tb_words"], "traceback matrices")
        assert r["tb_words"] * 2 <= kn["tb_budget"] or len(ids) == 1
        assert r["tb_words"] <= H["tb_max"] and H["tb_max"] * 2 <= H["sz_tb"]
        assert r["cls_cnt"].sum() == r["n_gw"]
        for c in range(8):
            for w in S["gwaves"][gw_at - r["n_gw"]:][r["cls_first"][c]:r["cls_first"][c] + r["cls_cnt"][c]]:
                assert T["cls"][w["task"][0]] == c and not ext[w["task"][0]]
        assert len(ids) * 4 <= H["up_gw"] - H["up_list"] and r["n_gw"] * 32 <= H["up_units"] - H["up_gw"], "a chunk's list and waves fit their staging slots"
        assert ((n * 4 + 63) & ~63) + r["n_gw"] * 32 <= H["sz_list"]
    assert at == H["n_reg_glob"] == H["n_glob"] - H["n_lite"]
    if kn["tb_budget"] < 8 << 30:
        assert len(ck) > 2, "the case is there for several chunks"
    # ---- the units reference every descriptor of the round exactly once (a split group: n_blk adjacent units in column order)
    assert len(U) == H["n_units"]
    ew_seen, gw_seen = np.zeros(len(EW), dtype=int), np.zeros(int(ck[0]["n_gw"]) if len(ck) else 0, dtype=int)
    ext_kind = {0: U_EXT16, 1: U_EXT32, 2: U_EXT64, X_W2: U_EXT_W4 if kn["pool"] else U_EXT_W2, 4: U_EXT_W4, X_SPLIT2: U_EXT_SPLIT, X_SPLIT4: U_EXT_SPLIT, X_128: U_EXT128}
    glob_kind = {0: U_GLOB16, 1: U_GLOB32, 2: U_GLOB64, T_W2: U_GLOB_W4 if kn["pool"] else U_GLOB_W2, T_W4: U_GLOB_W4, T_MB: U_GLOB_MB}
    k = 0
    while k < len(U):
        u = U[k]
        assert u["count"] >= 1 and (u["count"] == 1 or (u["count"] <= 4 and not kn["pool"]))
        if U_GLOB16 <= u["kind"] <= U_GLOB_W4:
            assert H["round_has_glob"]
            for d in range(u["first"], u["first"] + u["count"]):
                gw_seen[d] += 1
                assert glob_kind[int(T["cls"][S["gwaves"][d]["task"][0]])] == u["kind"]
        else:
            for d in range(u["first"], u["first"] + u["count"]):
                c0 = EW[d]["task"][0]
                want = ext_kind[int(T["cls"][c0])] if ext[c0] else U_LITE16 + int(T["cls"][c0]) - T_LITE16
                assert want == u["kind"], (k, want, u)
            if u["kind"] == U_EXT_SPLIT:
                nb = 4 if T["cls"][EW[u["first"]]["task"][0]] == X_SPLIT4 else 2
                grp = U[k:k + nb]
                assert list(grp["blk"]) == list(range(nb)) and (grp["n_blk"] == nb).all() and (grp["first"] == u["first"]).all() and (grp["kind"] == U_EXT_SPLIT).all()
                assert len(set(grp["sgroup"])) == 1 and len(set(grp["xg_first"])) == 1 and 0 <= u["sgroup"] < H["n_split"] and u["xg_first"] + nb - 1 <= H["n_bound"]
                k += nb - 1
            ew_seen[u["first"]:u["first"] + u["count"]] += 1
        k += 1
    in_round = np.array([not (not ext[w["task"][0]] and T["cls"][w["task"][0]] == T_LITE_W4) and not (kn["antidiag"] and ext[w["task"][0]] and T["cls"][w["task"][0]] == X_32)
                         for w in EW], dtype=int)
    assert (ew_seen == in_round).all(), "every descriptor of the round exactly once; the class-12 groups (and the anti-diagonal class) have launches of their own"
    if H["round_has_glob"]:
        own_launch = np.array([T["cls"][w["task"][0]] in (T_W8, T_W16) for w in S["gwaves"][:len(gw_seen)]], dtype=int)
        assert (gw_seen == 1 - own_launch).all()
    assert H["round_has_glob"] == (len(ck) > 0 and not H["wide_ge"])
    split_groups = sorted(set(U["sgroup"][U["kind"] == U_EXT_SPLIT]))
    assert split_groups == list(range(H["n_split"]))
    # ---- order: costliest first -- priorities never rise along the list; with the pool, whole-workgroup units before one-wave units
    is_group = np.isin(U["kind"], GROUP_KINDS)
    if kn["pool"]:
        assert H["n_group_units"] == is_group.sum() and is_group[:H["n_group_units"]].all()
        for part in (U[:H["n_group_units"]], U[H["n_group_units"]:]):
            assert (np.diff(part["prio"]) <= 0).all()
    else:
        assert H["n_group_units"] == 0 and (np.diff(U["prio"]) <= 0).all()
    assert ((U["prio"] >= 0) & (U["prio"] <= 3)).all() and (len(U) == 0 or U["prio"][0] == (3 if kn["unit_prio"] else 0))
    if not kn["unit_prio"]:
        assert (U["prio"] == 0).all()
    # ---- every section fits its staging slot and its device pool
    up = [H[k] for k in "up_tasks up_chunks up_q up_waves up_list up_gw up_units up_off up_ids up_args up_wl up_end".split()]
    assert up[0] == 0 and all(a <= b and a % 256 == 0 for a, b in zip(up[:-1], up[1:]))
    for name_, size in (("tasks", len(P.raw["tasks"])), ("chunks", len(P.raw["chunks"])), ("q", H["q_bytes"]), ("waves", len(P.raw["ewaves"])), ("units", len(P.raw["units"])),
                        ("off", 8 * H["n_glob"]), ("ids", 4 * H["n_glob"]), ("wl", 4 * H["n_lite"])):
        nxt = up[up.index(H["up_" + name_]) + 1] if name_ != "wl" else H["up_end"]
        assert H["up_" + name_] + size <= nxt, name_
    assert len(P.raw["tasks"]) <= H["sz_tasks"] and len(P.raw["chunks"]) <= H["sz_chunks"] and len(P.raw["ewaves"]) <= H["sz_waves"] and len(P.raw["units"]) <= H["sz_units"]
    assert H["q_bytes"] <= H["sz_qseq"] and ((4 * H["n_lite"] + 63) & ~63) + 8 <= H["sz_wlist"] and min(H["sz_extout"] // 16, H["sz_score"] // 4, H["sz_ncig"] // 4) >= n
    dn = [H[k] for k in "dn_eo dn_sc dn_nc dn_err dn_wb dn_end".split()]
    assert dn[0] == 0 and dn[1] >= 16 * n and dn[2] - dn[1] >= 4 * n and dn[3] - dn[2] >= 4 * n and dn[4] - dn[3] >= 4 and dn[5] - dn[4] >= 8
    if H["n_split"]:
        assert H["xg_bytes"] == H["n_bound"] * H["key_stride"] * 16 and H["xg_tail"] >= (2 * H["n_split"] + 1) * 4 and H["sz_xg"] >= H["xg_bytes"] + H["xg_tail"]
    wide = [w for w in EW if ext[w["task"][0]] and X_W2 <= T["cls"][w["task"][0]] <= X_SPLIT4]
    assert H["n_wide_groups"] == len(wide) and all(w["max_nl"] < H["key_stride"] for w in wide) and H["n_wide_groups"] * 2 * H["key_stride"] * 4 <= H["sz_rowkey"]
    # ---- the prep chunks cover every row of every call once
    rows = np.zeros(n, dtype=int)
    for c in S["chunks"]:
        assert c["row0"] % 1024 == 0 and c["row0"] < T["nl"][c["task"]]
        rows[c["task"]] += min(1024, int(T["nl"][c["task"]]) - int(c["row0"]))
    assert (rows == T["nl"]).all()
    # ---- the statistics that follow from the plan
    cells = np.maximum(0, T["nl"].astype(np.int64) - 2) * T["ncol"]
    assert H["st_n_ext"] == ext.sum() and H["st_n_glob"] == (~ext).sum() and H["st_cells_ext"] == cells[ext].sum() and H["st_cells_glob"] == cells[~ext].sum()
    assert H["st_rows_prep"] == H["rec_total"] and H["st_n_ckpt"] + H["st_n_ckpt_wide"] == H["n_lite"] and H["st_n_ckpt_wide"] == (~ext & (T["cls"] == T_LITE_W4)).sum()


def test_the_cases_cover_every_class_and_unit_kind():
    """fails when a case table stops containing a class or a unit kind of the round"""
    ext_cls, tb_cls, kinds = set(), set(), set()
    for name in CASES:
        P = the_plan(name)
        T = P.sec["tasks"]
        ext_cls |= set(T["cls"][is_ext(T)])
        tb_cls |= set(T["cls"][~is_ext(T)])
        kinds |= set(P.sec["units"]["kind"])
    assert ext_cls == set(range(9)), ext_cls
    assert tb_cls == set(range(13)), tb_cls
    assert kinds == set(range(U_LITE_W4)), kinds                       # (U_LITE_W4 is swept next to the round)
    assert the_plan("e_wide_ge").header["wide_ge"] == 1 and the_plan("e_wide_ge").header["n_units"] == 0
    sat = the_plan("f_saturate").sec["tasks"]                          # may_saturate at a few dozen columns: int32 sweeps from 48 columns on
    assert (sat["cls"][is_ext(sat) & (sat["ncol"] >= 48)] == X_HUGE).all() and (sat["cls"][is_ext(sat) & (sat["ncol"] <= 40)] < X_HUGE).all()
    assert (sat["cls"][~is_ext(sat) & (sat["ncol"] >= 48)] < T_LITE16).all()
    ns = the_plan("g_no_split")
    assert ns.header["n_split"] == 0 and (ns.sec["tasks"]["cls"][ns.sec["tasks"]["ncol"] > 256] == X_HUGE).all()
    assert the_plan("a_ext").header["n_split"] > 0
    c = the_plan("c_wide")
    assert c.header["l12_cnt"] == 8 and sorted(len(w["task"][w["task"] >= 0]) for w in c.sec["ewaves"][c.header["l12_first"]:][:8]) == [1] + [2] * 7, "pairs and an odd group"
    assert (the_plan("h_pool").sec["tasks"]["cls"] != T_LITE_W4).all()


@pytest.mark.parametrize("name", sorted(CASES))
def test_plan_identical_to_the_parent_commit(name):
    P = the_plan(name)
    gold = dpplan.golden()["cases"][name]
    assert list(gold["header"]) == dpplan.HEADER
    assert {k: v for k, v in P.header.items() if v != gold["header"][k]} == {}, "header fields that differ from the parent's"
    mine = P.digests()
    assert sorted(mine) == sorted(gold["digest"])
    assert {k: v for k, v in mine.items() if v != gold["digest"][k]} == {}, "sections whose bytes differ from what the parent uploaded"


def test_refusals_keep_code_and_message():
    gold = dpplan.golden()["refusals"]
    tables = dpplan.refusals()
    assert sorted(gold) == sorted(tables)
    for name, (tasks, over) in tables.items():
        assert dpplan.plan(tasks, over) == (gold[name]["code"], gold[name]["message"]), name
    assert dpplan.plan(tables["malformed"][0][:0]).header["n"] == 0   # an empty table is a plan, not a refusal


PROG = r"""
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <vector>
#include "dp_plan.h"
using namespace mpa;
static uint64_t state = 88172645463325252ULL;
static uint32_t rnd(uint32_t n) { state ^= state << 13, state ^= state >> 7, state ^= state << 17; return (uint32_t)((state >> 11) % n); }
int main()
{
	const int64_t ctg_len[3] = { 6000, 9000, 4000 }, q_off[5] = { 0, 1200, 1900, 2200, 3350 };
	const mpa_qbatch_t q{ 4, nullptr, q_off };
	const int widths[] = { 16, 32, 64, 128, 256, 512, 1024, 1100 }, lite_mins[] = { 0, 3, 100, 384 };
	const size_t round_args_bytes = 1400;                                 // (the executor passes sizeof(DpRoundArgs): any size lays out the same way)
	long planned = 0, refused = 0, bytes = 0, unswept = 0;
	for (int round = 0; round < 400; ++round) {
		mpa_dpopt_t opt = {};
		opt.go = round % 7 == 3 ? 20000 : 11, opt.ge = round % 5 == 4 ? 300 : round % 7 == 3 ? 255 : 1, opt.fs = 23, opt.xdrop = 100, opt.end_bonus = 5, opt.ie_coef = .5f;
		for (int k = 0; k < 484; ++k) opt.mat[k] = (int8_t)(k % 23 == k / 22 ? 11 : -4);
		DpPlanKnobs kn;
		kn.lite_min = lite_mins[rnd(4)], kn.lite_wide = rnd(2), kn.no_split = rnd(4) == 0, kn.antidiag = rnd(4) == 0, kn.pool = rnd(3) == 0;
		kn.ext_dual = rnd(4) != 0, kn.unit_prio = rnd(4) != 0, kn.tb_budget = rnd(3) ? (int64_t)8 << 30 : (int64_t)1 << 20;
		const int n = round < 4 ? round / 2 : (int)rnd(300);             // empty and one-call tables first
		std::vector<mpa_dp_task_t> t((size_t)n);
		for (auto &x : t) {
			x.qid = (int32_t)rnd(4);
			const int32_t ql = (int32_t)(q_off[x.qid + 1] - q_off[x.qid]);
			x.al = 1 + (int32_t)rnd((uint32_t)std::min(ql, widths[rnd(8)]));
			x.aa_off = (int32_t)rnd((uint32_t)(ql - x.al + 1));
			x.vid = (int32_t)rnd(6), x.nl = (int32_t)rnd(2501);
			x.nt_off = rnd((uint32_t)(ctg_len[x.vid >> 1] - x.nl + 1));
			x.flag = rnd(2) ? MPA_F_CIGAR : rnd(2) ? MPA_F_EXT_LEFT : MPA_F_EXT_RIGHT;
			x.io = (int32_t)rnd(41), x.tag = 0;
			if (rnd(4000) == 0) x.al = 0;                                  // (now and then a table the planner refuses)
		}
		DpPlan P;
		if (dp_plan(t.data(), n, ctg_len, sizeof(int64_t), 3, &q, &opt, kn, round_args_bytes, P) != MPA_OK) { if (P.err.empty()) return printf("FAIL refusal without a message\n"), 1; ++refused; continue; }
		const int64_t need = dp_plan_serialize(P, kn, nullptr, 0);         // (runs the later stages: chunk waves, units, statistics)
		if (need < 0) return printf("FAIL round %d: %s\n", round, P.err.c_str()), 1;
		std::vector<int> seen((size_t)n, 0);
		for (const ExtWave &w : P.ewaves) for (int32_t id : w.task) if (id >= 0) ++seen[(size_t)id];
		for (const DpTbChunk &r : P.chunks) for (const GlobWave &w : r.waves) for (int32_t id : w.task) if (id >= 0) ++seen[(size_t)id];
		for (int32_t id : P.huge_ids) ++seen[(size_t)id];
		for (int k = 0; k < n; ++k) {                                      // (an extension call of fewer than three rows is swept by nobody: class X_NONE)
			const int want = dp_ext_unswept(t[(size_t)k].flag, t[(size_t)k].nl) ? 0 : 1;
			if (want == 0) ++unswept;
			if (seen[(size_t)k] != want || (want == 0) != (P.tasks[(size_t)k].cls == X_NONE && !(t[(size_t)k].flag & MPA_F_CIGAR))) return printf("FAIL round %d: call %d in %d slots\n", round, k, seen[(size_t)k]), 1;
		}
		std::vector<char> buf((size_t)need);                               // exactly the size asked for: a write past it is an error
		if (dp_plan_serialize(P, kn, buf.data(), need) != need) return printf("FAIL serialised size\n"), 1;
		++planned, bytes += need;
	}
	if (unswept < 10) return printf("FAIL only %ld extension calls of fewer than three rows\n", unswept), 1;
	printf("OK %ld tables planned, %ld refused, %ld bytes serialised\n", planned, refused, bytes);
	return 0;
}
"""


def test_planner_alone_under_sanitizers(tmp_path):
    """dp_plan.cpp and a small main, host compiler only (no HIP header, nothing of the library): 400 random tables -- empty and
    one-call tables, every knob, wide_ge and may_saturate options, a 1-MB traceback budget -- planned and serialised under
    AddressSanitizer / UBSan; the program exits 0 only when clean.  Every call sits in exactly one slot of one descriptor, except the
    extension calls of fewer than three rows (class X_NONE), which sit in none"""
    src = tmp_path / "dp_plan_main.cpp"
    src.write_text(PROG)
    exe = str(tmp_path / "dp_plan_main")
    csrc = os.path.join(ROOT, "miniprot_amd", "csrc")
    subprocess.run(["g++", "-std=c++17", "-O0", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",   # (-O0: the compile is the test's time)
                    "-I" + csrc, "-I" + os.path.join(ROOT, "include"), str(src), os.path.join(csrc, "dp_plan.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("OK "), r.stdout + r.stderr
