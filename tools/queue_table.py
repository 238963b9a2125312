#!/usr/bin/env python3
"""Which hardware queue every stream of the pipeline sits on, from a rocprofv3 --kernel-trace rocpd database (the table tools/timeline.py
prints dispatch by dispatch, condensed per stream).   python tools/queue_table.py t_results.db

A stream's role is read off the kernels it ran: k_dp_round -> a DP lane's main stream; k_refine_* -> a planner; k_seed_sift / k_prechain_fwd /
k_sketch_* -> a seeder; k_lite_wide / k_ext_huge* / k_ext_replay / k_glob_wide without a round -> a lane's side stream.  A
stream that ran no kernel (a seeder's idle main stream in the legacy layout, copies only) is not in a kernel trace.

Per lane, `queued behind others` is an estimate from start and end times alone (a kernel trace has no enqueue times): a dispatch d of
the lane counts as having waited for a kernel o of ANOTHER stream on the same queue when d starts within 100 us of o's end; it is
charged o's run time from the later of o's start and the end of the lane's previous dispatch (before that the lane itself was not
ready).  Copies and events wait in the same way and are not in the trace: the figure is a lower bound of what the lane's operations
lost, and an upper bound for the kernels it names."""
import collections
import re
import sqlite3
import sys

db = sqlite3.connect(sys.argv[1])
cur = db.cursor()
sym = {r[0]: r[1] for r in cur.execute("select id, kernel_name from rocpd_info_kernel_symbol")}
rows = list(cur.execute("select kernel_id,queue_id,stream_id,start,end,tid from rocpd_kernel_dispatch order by start"))


def short(n):
    m = re.search(r"(k_[a-z0-9_]+)", n)
    return m.group(1) if m else n[:24]


ROLE = (("lane", ("k_dp_round",)), ("planner", ("k_refine",)), ("seeder", ("k_seed_sift", "k_prechain_fwd", "k_sketch_count", "k_sketch_emit")),
        ("side", ("k_lite_wide", "k_ext_huge", "k_ext_replay", "k_glob_wide", "k_ext_antidiag")))
by_stream = collections.defaultdict(list)
for k, q, s, st, en, tid in rows:
    by_stream[s].append((st, en, q, short(sym[k]), tid))


def role_of(ds):
    names = set(d[3] for d in ds)
    for role, keys in ROLE:
        if any(n.startswith(key) for n in names for key in keys):
            return role
    return "other"


t0, t1 = rows[0][3], max(r[4] for r in rows)
print("trace: %.1f ms, %d dispatches, %d streams with kernels on %d queues" % ((t1 - t0) / 1e6, len(rows), len(by_stream), len(set(r[1] for r in rows))))
roles = {s: role_of(ds) for s, ds in by_stream.items()}
by_queue = collections.defaultdict(list)
for k, q, s, st, en, tid in rows:
    by_queue[q].append((st, en, s, short(sym[k])))
print("\nstream  role     queue(s)  tid     dispatches  busy ms  longest kernels")
for s in sorted(by_stream, key=lambda s: (roles[s], s)):
    ds = by_stream[s]
    qs = sorted(set(d[2] for d in ds))
    top = collections.Counter()
    for st, en, q, n, tid in ds:
        top[n] += en - st
    print("s%-5d  %-7s  %-8s  %-6d  %10d  %7.1f  %s" % (s, roles[s], ",".join("q%d" % q for q in qs), ds[0][4] % 100000, len(ds), sum(d[1] - d[0] for d in ds) / 1e6,
                                                     " ".join("%s %.0f" % (n, v / 1e6) for n, v in top.most_common(3))))
print("\nqueue  streams on it (role)")
for q in sorted(by_queue):
    ss = sorted(set(d[2] for d in by_queue[q]))
    print("q%-4d  %s" % (q, "  ".join("s%d(%s)" % (s, roles[s]) for s in ss)))
qs_of = collections.defaultdict(set)
for s, ds in by_stream.items():
    qs_of[roles[s]].update(d[2] for d in ds)
print("\nqueues by role: " + "; ".join("%s %s" % (r, ",".join("q%d" % q for q in sorted(v))) for r, v in sorted(qs_of.items())))
for r in ("seeder", "planner", "side"):
    both = qs_of[r] & qs_of["lane"]
    print("%s streams share %d of their %d queue(s) with lane main streams%s" % (r, len(both), len(qs_of[r]), (": " + ",".join("q%d" % q for q in sorted(both))) if both else ""))
lane_qs = collections.Counter()
for s, r in roles.items():
    if r == "lane":
        for q in set(d[2] for d in by_stream[s]):
            lane_qs[q] += 1
print("lane main streams per queue: " + " ".join("q%d:%d" % (q, n) for q, n in sorted(lane_qs.items())))

EPS = 100e3
print("\nqueued behind others (estimate, see the header): stream  role  waits  ms  share of trace  behind whom (ms)")
for s in sorted(by_stream, key=lambda s: (roles[s], s)):
    if roles[s] not in ("lane", "seeder", "planner"):
        continue
    lost, n, whom = 0.0, 0, collections.Counter()
    prev_end = None
    for st, en, q, name, tid in by_stream[s]:
        best = None
        for ost, oen, os_, oname in by_queue[q]:
            if ost > st:
                break
            if os_ != s and oen <= st + 1000 and st - oen < EPS and (best is None or oen > best[1]):
                best = (ost, oen, os_, oname)
        if best:
            ready = max(best[0], prev_end if prev_end is not None else best[0])
            if best[1] > ready:
                lost += best[1] - ready
                n += 1
                whom["%s of s%d(%s)" % (best[3], best[2], roles[best[2]])] += best[1] - ready
        prev_end = en
    print("s%-5d %-7s %5d %8.1f %6.1f %%   %s" % (s, roles[s], n, lost / 1e6, 100.0 * lost / (t1 - t0), "  ".join("%s %.0f" % (k, v / 1e6) for k, v in whom.most_common(3))))
