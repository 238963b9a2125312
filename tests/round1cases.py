"""Inputs of the round-1 tests (tests/test_round1_cpu.py, tests/test_round1_gpu.py; MPA_GPU_ROUND1): the plans, gap segments and round-1 DP
tasks of a batch, read from its MPA_PLANS_DUMP (tests/plansdump.py), as the tables mpa_dbg_round1_chain and mpa_dbg_spans take -- per
query a unit (plans with query-local task numbers, the query's tasks, its gap segments) -- and tables of a wanted size tiled from them:
unit after unit, round and round, every copy with its base1 and its first gap segment shifted by what lies before it."""
import numpy as np
import miniprot_amd as mpa
import plansdump
import spanscases

EXT_BITS = mpa.F_EXT_LEFT | mpa.F_EXT_RIGHT


def units(dump, q):
    """[(plans as spanscases.PLAN_IN with base1 = 0 and gap0 local to the unit, tasks, segments)] of the queries of a dump that have a plan"""
    out = []
    for qid, regs, plans, tasks, segs in plansdump.parse(dump):
        if len(plans) == 0:
            continue
        p = np.zeros(len(plans), spanscases.PLAN_IN)
        for f in plansdump.PLAN.names:
            p[f] = plans[f]
        p["q_off"], p["qid"], p["qlen"], p["base1"] = int(q.off[qid]) - int(q.off[0]), qid, len(q.seqs[qid]), 0
        p["vid"] = regs["vid"][plans["reg"]]
        s = np.zeros(len(segs), spanscases.SEG)
        for f in plansdump.SEG.names:
            s[f] = segs[f]
        s["score"][s["score"] == np.iinfo(np.int32).min] = 0
        out.append((p, np.ascontiguousarray(tasks, dtype=mpa.DP_TASK), s))
    return out


def _join(parts):
    plans, tasks, segs, n_task, n_seg = [], [], [], 0, 0
    for p, t, s in parts:
        p = p.copy()
        p["base1"] += n_task
        p["gap0"] += n_seg
        plans.append(p), tasks.append(t), segs.append(s)
        n_task, n_seg = n_task + len(t), n_seg + len(s)
    return np.concatenate(plans), np.concatenate(tasks), np.concatenate(segs)


def _cycle(us, enough):
    parts, k = [], 0
    while not enough(parts):
        parts.append(us[k % len(us)])
        k += 1
    return parts


def tile_plans(us, n_plan):
    """(plans, tasks, segments) of exactly n_plan plans: whole units, the last one cut short (its tasks and segments all stay)"""
    plans, tasks, segs = _join(_cycle(us, lambda parts: sum(len(p[0]) for p in parts) >= n_plan))
    return plans[:n_plan].copy(), tasks, segs


def tile_tasks(us, n_task):
    """(plans, tasks, segments) with a table of exactly n_task calls: whole units, the table cut at n_task and with it every plan that
    names a call behind the cut"""
    plans, tasks, segs = _join(_cycle(us, lambda parts: sum(len(p[1]) for p in parts) >= n_task))
    keep = []
    for j, p in enumerate(plans):
        last = max(int(p[f]) for f in ("t_left", "t_left2", "t_right", "t_right2"))
        g = segs[int(p["gap0"]):int(p["gap0"]) + int(p["n_gap"])]["task"]
        last = max(last, int(g.max(initial=-1)))
        if int(p["base1"]) + last < n_task:
            keep.append(j)
    assert keep, "no plan fits the table"
    return plans[keep].copy(), tasks[:n_task].copy(), segs


def only_extension_calls(tasks):
    return bool(((tasks["flag"] & EXT_BITS) != 0).all())


def spans_block_bytes(n_plan, n_seg, text_bytes):
    """what the step's block holds without its record section, as SpansLayout (dev_layout.h) lays it out: the tables' KB, the plans in a
    16-byte section, the gap segments, the text"""
    return 1024 + (104 * n_plan + 15) // 16 * 16 + 24 * n_seg + text_bytes


def planner_upload_bytes(n, n_seq):
    """the device planner's upload for a table that goes up: task records and query offsets, each in a 256-byte section"""
    return (40 * n + 255) // 256 * 256 + (8 * (n_seq + 1) + 255) // 256 * 256
