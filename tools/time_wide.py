"""Kernel-time microbenchmark of the DP classes: n_tasks right-extension calls (flag 4) or traceback calls (flag 1) of `al` columns x
`nl` rows (results are not checked here).  python tools/time_wide.py al nl n_tasks [flag] [antidiag]
antidiag = 1: the 32-column extension class on the anti-diagonal prototype (dp_antidiag.hip) instead of the row sweep.
python tools/time_wide.py split_wide [repeats]: the table of the 1 025..3 072-column extension classes (MPA_DP_SPLIT_WIDE) -- a pair of
calls of 1 100, 1 500, 2 000 and 2 600 columns x 20 000 rows, first with the knob off (k_ext_huge, the one-wave int32 sweep), then with
the knob on (X_SPLIT8 / X_SPLIT12), the pair of legs `repeats` times (default 3); 1 000 columns (X_SPLIT4 in both legs) for comparison.
python tools/time_wide.py huge_wg [repeats]: the table of MPA_DP_HUGE_WG -- a pair of right-extension calls of 20 000 rows at 1 100, 1 500,
2 000, 2 600, 3 300 and 6 800 columns with MPA_DP_SPLIT_WIDE unset (all X_HUGE), knob off (k_ext_huge, one wave per call) and knob on
(k_ext_huge_wg, one wave per column block), interleaved; then ms_total of the mixed batch of the tests (tests/hugewg.py, mixed_table:
X_HUGE calls of 4, W + 1 and 2 W + 1 blocks next to a round of 40 ordinary pairs), the same way.
python tools/time_wide.py mb_wg [repeats]: the table of MPA_DP_MB_WG -- a pair of traceback calls (flag 1) of 20 000 rows at 1 100, 1 500,
2 000, 2 600 and 3 300 columns (class T_MB), knob off (one wave per call, in the round kernel) and knob on (k_glob_mb_wg, one wave per
column block), interleaved; the clock is ms_glob, the traceback sweeps of the batch; the two legs' records and CIGAR pools must agree.
Then ms_total of the mixed batch of the tests (tests/mbwg.py, mixed_table: T_MB calls of 17, 33 and 49 blocks next to 40 ordinary
pairs), the same way.
python tools/time_wide.py lite_w8 [repeats]: the table of MPA_DP_LITE_W8 -- 1, 2 and 64 traceback calls (flag 1) of 20 000 rows at 264, 384
and 512 columns, knob off (the plain int32 sweep k_glob_wide<8> + k_backtrack) and knob on (k_lite_w8 + k_walk_w8), interleaved on one
device; per leg the sweep (ms_glob) as ns per row, ms_backtrack (k_backtrack; the checkpointed walk is not timed apart), the batch on the
device (ms_total) and what is left of it behind prep and sweep -- with the knob on: the walk and the downloads --, the blocks walked, and
the bytes of traceback memory the leg asks for (off: the matrix of direction words; on: bit words and checkpoints).  The two legs'
records and CIGAR pools must agree."""
import sys, os
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests")); sys.path.insert(0, ROOT)
import numpy as np, miniprot_amd as mpa


def split_wide_table(repeats, nl=20000, n=2):
    rng = np.random.default_rng(1)
    g = rng.integers(0, 4, nl * n + 1000).astype(np.uint8)
    idx = mpa.Index.from_nt4([g], ["c"])
    ctxs = {}
    for knob in (0, 1):                                # the knob is read when a context is created
        os.environ["MPA_DP_SPLIT_WIDE"] = str(knob)
        ctxs[knob] = mpa.Context(0)
        idx.to_device(ctxs[knob])
    dp = mpa.dpopt_from(mpa.default_mapopt())
    dp.xdrop = 32000                                   # never stop: time all rows
    print("# ns per row of a pair of right-extension calls, %d rows each; knob off: ms_ext of the k_ext_huge + k_ext_replay launch, knob on: the round kernel" % nl)
    print("%6s %4s %8s %14s %14s %8s" % ("al", "rep", "classes", "off ns/row", "on ns/row", "off/on"))
    for al in (1000, 1100, 1500, 2000, 2600):
        aa = bytes(rng.choice(list(b"ACDEFGHIKLMNPQRSTVWY"), al * n).tolist())
        q = mpa.Queries([aa[i * al:(i + 1) * al] for i in range(n)])
        tasks = np.zeros(n, mpa.DP_TASK)
        for i in range(n):
            tasks[i]["nt_off"] = i * nl; tasks[i]["nl"] = nl; tasks[i]["qid"] = i; tasks[i]["al"] = al; tasks[i]["flag"] = 4; tasks[i]["io"] = 29
        for rep in range(repeats + 1):                 # (the first pair of legs warms both contexts up and is not printed)
            ns, cls = {}, {}
            for knob in (0, 1):
                mpa.dp_run(ctxs[knob], idx, dp, q, tasks)
                st = ctxs[knob].dp_stats()
                ns[knob] = st["ms_ext"] * 1e6 / nl
                c = mpa.dbg_dp_last_classes(ctxs[knob])
                cls[knob] = "+".join("%d:%d" % (k, v) for k, v in enumerate(c) if v)
            if rep:
                print("%6d %4d %8s %14.1f %14.1f %8.2f" % (al, rep, cls[0] + "|" + cls[1], ns[0], ns[1], ns[0] / ns[1]))


def huge_wg_table(repeats, nl=20000, n=2):
    rng = np.random.default_rng(1)
    g = rng.integers(0, 4, nl * n + 1000).astype(np.uint8)
    idx = mpa.Index.from_nt4([g], ["c"])
    os.environ.pop("MPA_DP_SPLIT_WIDE", None)
    ctxs = {}
    for knob in (0, 1):                                # the knob is read when a context is created
        os.environ["MPA_DP_HUGE_WG"] = str(knob)
        ctxs[knob] = mpa.Context(0)
        idx.to_device(ctxs[knob])
    dp = mpa.dpopt_from(mpa.default_mapopt())
    dp.xdrop = 32000                                   # never stop: time all rows
    print("# (W, R, MIN_BLOCKS) = %s" % (mpa.dbg_dp_huge_wg_info(),))
    print("# ns per row of a pair of right-extension calls, %d rows each: ms_ext of the huge calls' launches + k_ext_replay; huge: mpa_dbg_dp_last_huge off|on" % nl)
    print("%6s %4s %28s %14s %14s %8s" % ("al", "rep", "huge", "off ns/row", "on ns/row", "off/on"))
    for al in (1100, 1500, 2000, 2600, 3300, 6800):
        aa = bytes(rng.choice(list(b"ACDEFGHIKLMNPQRSTVWY"), al * n).tolist())
        q = mpa.Queries([aa[i * al:(i + 1) * al] for i in range(n)])
        tasks = np.zeros(n, mpa.DP_TASK)
        for i in range(n):
            tasks[i]["nt_off"] = i * nl; tasks[i]["nl"] = nl; tasks[i]["qid"] = i; tasks[i]["al"] = al; tasks[i]["flag"] = 4; tasks[i]["io"] = 29
        for rep in range(repeats + 1):                 # (the first pair of legs warms both contexts up and is not printed)
            ns, huge, rst = {}, {}, {}
            for knob in (0, 1):
                rst[knob], _ = mpa.dp_run(ctxs[knob], idx, dp, q, tasks)
                ns[knob] = ctxs[knob].dp_stats()["ms_ext"] * 1e6 / nl
                huge[knob] = ",".join(str(x) for x in mpa.dbg_dp_last_huge(ctxs[knob]))
            assert [tuple(r) for r in rst[0]] == [tuple(r) for r in rst[1]], "the two kernels disagree at %d columns" % al
            if rep:
                print("%6d %4d %28s %14.1f %14.1f %8.2f" % (al, rep, huge[0] + "|" + huge[1], ns[0], ns[1], ns[0] / ns[1]))
    idx.close()
    # the mixed batch: does the 64 KB workgroup wait for the round's workgroups to leave a CU?
    import hugewg as hw
    tab, want = hw.mixed_table()
    idx = mpa.Index.from_nt4(tab.contigs)
    for knob in (0, 1):
        idx.to_device(ctxs[knob])
    print("# the mixed batch (X_HUGE calls of %s blocks, %d calls in all): ms of the batch on the device, of the extension launches, of the round" % (sorted(set(want)), len(tab.tasks)))
    print("%4s %28s %12s %12s %12s %12s" % ("rep", "huge", "off ms_total", "on ms_total", "off ms_ext", "on ms_ext"))
    for rep in range(repeats + 1):
        st, huge = {}, {}
        for knob in (0, 1):
            mpa.dp_run(ctxs[knob], idx, tab.opt, tab.queries, tab.tasks)
            st[knob] = ctxs[knob].dp_stats()
            huge[knob] = ",".join(str(x) for x in mpa.dbg_dp_last_huge(ctxs[knob]))
        if rep:
            print("%4d %28s %12.3f %12.3f %12.3f %12.3f" % (rep, huge[0] + "|" + huge[1], st[0]["ms_total"], st[1]["ms_total"], st[0]["ms_ext"], st[1]["ms_ext"]))


def mb_wg_table(repeats, nl=20000, n=2):
    rng = np.random.default_rng(1)
    g = rng.integers(0, 4, nl * n + 1000).astype(np.uint8)
    idx = mpa.Index.from_nt4([g], ["c"])
    ctxs = {}
    for knob in (0, 1):                                # the knob is read when a context is created
        os.environ["MPA_DP_MB_WG"] = str(knob)
        ctxs[knob] = mpa.Context(0)
        idx.to_device(ctxs[knob])
    dp = mpa.dpopt_from(mpa.default_mapopt())
    W, R, _ = mpa.dbg_dp_huge_wg_info()
    print("# (W, R) = (%d, %d)" % (W, R))
    print("# ns per row of a pair of traceback calls, %d rows each: ms_glob, the batch's traceback sweeps (knob off: the round kernel with its two U_GLOB_MB waves;" % nl)
    print("# knob on: the round kernel without them next to k_glob_mb_wg); per block / per pass: ns per row divided by the call's column blocks / passes; mb: mpa_dbg_dp_last_mb off|on")
    print("%6s %4s %24s %12s %12s %8s %14s %14s" % ("al", "rep", "mb", "off ns/row", "on ns/row", "off/on", "off per block", "on per pass"))
    for al in (1100, 1500, 2000, 2600, 3300):
        aa = bytes(rng.choice(list(b"ACDEFGHIKLMNPQRSTVWY"), al * n).tolist())
        q = mpa.Queries([aa[i * al:(i + 1) * al] for i in range(n)])
        tasks = np.zeros(n, mpa.DP_TASK)
        for i in range(n):
            tasks[i]["nt_off"] = i * nl; tasks[i]["nl"] = nl; tasks[i]["qid"] = i; tasks[i]["al"] = al; tasks[i]["flag"] = 1; tasks[i]["io"] = 29
        nblk = ((al + 7) // 8 * 8 + 63) // 64
        for rep in range(repeats + 1):                 # (the first pair of legs warms both contexts up and is not printed)
            ns, mb, out = {}, {}, {}
            for knob in (0, 1):
                rst, cig = mpa.dp_run(ctxs[knob], idx, dp, q, tasks)
                out[knob] = ([tuple(r) for r in rst], np.asarray(cig).tobytes())
                ns[knob] = ctxs[knob].dp_stats()["ms_glob"] * 1e6 / nl
                mb[knob] = ",".join(str(x) for x in mpa.dbg_dp_last_mb(ctxs[knob]))
            if out[0] != out[1]:
                sys.exit("the two legs' records or CIGAR pools differ at %d columns" % al)
            if rep:
                print("%6d %4d %24s %12.1f %12.1f %8.2f %14.1f %14.1f" % (al, rep, mb[0] + "|" + mb[1], ns[0], ns[1], ns[0] / ns[1], ns[0] / nblk, ns[1] / ((nblk + W - 1) // W)))
    idx.close()
    # the mixed batch: does the 64 KB workgroup wait for the round's workgroups to leave a CU?
    import mbwg
    tab, want = mbwg.mixed_table()
    idx = mpa.Index.from_nt4(tab.contigs)
    for knob in (0, 1):
        idx.to_device(ctxs[knob])
    print("# the mixed batch (T_MB calls of %s blocks, %d calls in all): ms of the batch on the device, of its traceback sweeps, of the round" % (sorted(want), len(tab.tasks)))
    print("%4s %24s %12s %12s %12s %12s %12s %12s" % ("rep", "mb", "off ms_total", "on ms_total", "off ms_glob", "on ms_glob", "off ms_round", "on ms_round"))
    for rep in range(repeats + 1):
        st, mb, out = {}, {}, {}
        for knob in (0, 1):
            rst, cig = mpa.dp_run(ctxs[knob], idx, tab.opt, tab.queries, tab.tasks)
            out[knob] = ([tuple(r) for r in rst], np.asarray(cig).tobytes())
            st[knob] = ctxs[knob].dp_stats()
            mb[knob] = ",".join(str(x) for x in mpa.dbg_dp_last_mb(ctxs[knob]))
        if out[0] != out[1]:
            sys.exit("the two legs' records or CIGAR pools differ on the mixed batch")
        if rep:
            print("%4d %24s %12.3f %12.3f %12.3f %12.3f %12.3f %12.3f" % (rep, mb[0] + "|" + mb[1], st[0]["ms_total"], st[1]["ms_total"], st[0]["ms_glob"], st[1]["ms_glob"], st[0]["ms_round"], st[1]["ms_round"]))


def lite_w8_table(repeats, nl=20000):
    rng = np.random.default_rng(1)
    n_max = 64
    g = rng.integers(0, 4, nl * n_max + 1000).astype(np.uint8)
    idx = mpa.Index.from_nt4([g], ["c"])
    os.environ["MPA_DP_LITE_WIDE"] = "0"
    ctxs = {}
    for knob in (0, 1):                                # the knob is read when a context is created
        os.environ["MPA_DP_LITE_W8"] = str(knob)
        ctxs[knob] = mpa.Context(0)
        idx.to_device(ctxs[knob])
    dp = mpa.dpopt_from(mpa.default_mapopt())
    print("# traceback calls of %d rows; sweep: ms_glob as ns per row (off: k_glob_wide<8>, one call per 512-thread group; on: k_lite_w8, two calls per group);" % nl)
    print("# bt: ms_backtrack (off: k_backtrack); total: ms_total, the batch on the device; rest: ms_total - ms_prep - ms_glob (on: k_walk_w8 and the downloads) and its share of total;")
    print("# tb bytes: off 2 B per cell of nl x ncol, on 4 B per bit word and checkpoint dword of the eight-wave groups; w8: mpa_dbg_dp_last_w8 of the on leg")
    print("%4s %3s %4s %11s %11s %7s %8s %8s %9s %9s %9s %9s %6s %13s %12s %s" % ("al", "n", "rep", "off ns/row", "on ns/row", "off/on", "off bt", "on bt", "off total", "on total", "off rest", "on rest", "share", "off tb bytes", "on tb bytes", "w8"))
    for al in (264, 384, 512):
        ncol = (al + 7) // 8 * 8
        for n in (1, 2, 64):
            aa = bytes(rng.choice(list(b"ACDEFGHIKLMNPQRSTVWY"), al * n).tolist())
            q = mpa.Queries([aa[i * al:(i + 1) * al] for i in range(n)])
            tasks = np.zeros(n, mpa.DP_TASK)
            for i in range(n):
                tasks[i]["nt_off"] = i * nl; tasks[i]["nl"] = nl; tasks[i]["qid"] = i; tasks[i]["al"] = al; tasks[i]["flag"] = 1; tasks[i]["io"] = 29
            groups = (n + 1) // 2
            tb_off = 2 * n * nl * ncol
            tb_on = 4 * groups * ((nl // 3 + 2) * 512 + (nl - 3) // 96 * 9 * 512)
            for rep in range(repeats + 1):             # (the first pair of legs warms both contexts up and is not printed)
                st, out, w8 = {}, {}, None
                for knob in (0, 1):
                    rst, cig = mpa.dp_run(ctxs[knob], idx, dp, q, tasks)
                    out[knob] = ([tuple(r) for r in rst], np.asarray(cig).tobytes())
                    st[knob] = ctxs[knob].dp_stats()
                    if knob:
                        w8 = mpa.dbg_dp_last_w8(ctxs[knob])
                if out[0] != out[1]:
                    sys.exit("the two legs' records or CIGAR pools differ at %d columns, %d calls" % (al, n))
                if w8[0] != n or mpa.dbg_dp_last_w8(ctxs[0])[0] != 0:
                    sys.exit("routing: %s calls of the class with the knob on" % (w8,))
                if rep:
                    ns = [st[k]["ms_glob"] * 1e6 / nl for k in (0, 1)]
                    rest = [st[k]["ms_total"] - st[k]["ms_prep"] - st[k]["ms_glob"] for k in (0, 1)]
                    print("%4d %3d %4d %11.1f %11.1f %7.2f %8.3f %8.3f %9.3f %9.3f %9.3f %9.3f %6.2f %13d %12d %s" % (al, n, rep, ns[0], ns[1], ns[0] / ns[1], st[0]["ms_backtrack"], st[1]["ms_backtrack"],
                          st[0]["ms_total"], st[1]["ms_total"], rest[0], rest[1], rest[1] / st[1]["ms_total"], tb_off, tb_on, ",".join(str(x) for x in w8)))
    idx.close()


if sys.argv[1] == "lite_w8":
    lite_w8_table(int(sys.argv[2]) if len(sys.argv) > 2 else 3)
    sys.exit(0)
if sys.argv[1] == "mb_wg":
    mb_wg_table(int(sys.argv[2]) if len(sys.argv) > 2 else 3)
    sys.exit(0)
if sys.argv[1] == "huge_wg":
    huge_wg_table(int(sys.argv[2]) if len(sys.argv) > 2 else 3)
    sys.exit(0)
if sys.argv[1] == "split_wide":
    split_wide_table(int(sys.argv[2]) if len(sys.argv) > 2 else 3)
    sys.exit(0)
al, nl, n = int(sys.argv[1]), int(sys.argv[2]), int(sys.argv[3])
flag = int(sys.argv[4]) if len(sys.argv) > 4 else 4      # 4 = right extension (score only), 1 = global with traceback
rng = np.random.default_rng(1)
g = rng.integers(0, 4, nl * n + 1000).astype(np.uint8)
idx = mpa.Index.from_nt4([g], ["c"])
ctx = mpa.Context(0); idx.to_device(ctx)
antidiag = int(sys.argv[5]) if len(sys.argv) > 5 else 0
if antidiag:
    import ctypes as C
    mpa.lib().mpa_dbg_antidiag.argtypes = [C.c_void_p, C.c_int]
    mpa.lib().mpa_dbg_antidiag(ctx.h, 1)
aa = bytes(rng.choice(list(b"ACDEFGHIKLMNPQRSTVWY"), al * n).tolist())
q = mpa.Queries([aa[i * al:(i + 1) * al] for i in range(n)])
tasks = np.zeros(n, mpa.DP_TASK)
for i in range(n):
    tasks[i]["nt_off"] = i * nl; tasks[i]["vid"] = 0; tasks[i]["nl"] = nl; tasks[i]["qid"] = i; tasks[i]["aa_off"] = 0; tasks[i]["al"] = al
    tasks[i]["flag"] = flag; tasks[i]["io"] = 29
dp = mpa.dpopt_from(mpa.default_mapopt())
dp.xdrop = 32000                                   # never stop: time all rows
for it in range(3):
    mpa.dp_run(ctx, idx, dp, q, tasks)
    st = ctx.dp_stats()
    ms = st["ms_ext"] if flag != 1 else st["ms_glob"]
    tot = ctx.dp_stats(total=True, reset=True)
    if tot["ms_round"] > 0:                        # worker pool (default): the round is a k_dp_worker launch on the worker stream
        ms = tot["ms_round"]
    print("al %d nl %d x %d flag %d%s: %.2f ms -> %.1f ns/row (backtrack %.2f ms; batch on the device %.2f ms; %d + %d checkpointed, %d blocks walked)" % (al, nl, n, flag, " ANTIDIAG" if antidiag else "", ms, ms * 1e6 / nl, st["ms_backtrack"], st["ms_total"], st["n_ckpt"], st["n_ckpt_wide"], st["walk_blocks"]))
