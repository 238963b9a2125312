"""Time the k-mer table build of a synthetic genome: on the device (mpa_idx_build_kmers_device), in one pass or under a key budget
that forces several, and on the host cores.
python tools/index_bench.py GENOME_MBP N_CTG [--repeat R] [--budget-mb MB | --passes P] [--host-threads T] [--genome-cache FILE.npy]
--budget-mb sets MPA_IDX_BUILD_MB; --passes sizes the budget from the key count of a first build so that the plan has P passes;
--genome-cache keeps the generated genome for the next run (one flat array, contigs of equal length).  MPA_LIB_PATH selects
another build of the library (an older one has no pass statistics: they print as n/a).  One line per build, then the median."""
import argparse, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np, miniprot_amd as mpa, gen_synth

ap = argparse.ArgumentParser()
ap.add_argument("genome_mbp", type=float)
ap.add_argument("n_ctg", type=int)
ap.add_argument("--repeat", type=int, default=3)
ap.add_argument("--budget-mb", type=int, default=0)
ap.add_argument("--passes", type=int, default=0)
ap.add_argument("--host-threads", type=int, default=0)
ap.add_argument("--genome-cache", default=None)
args = ap.parse_args()

if args.genome_cache and os.path.exists(args.genome_cache):
    contigs = list(np.load(args.genome_cache).reshape(args.n_ctg, -1))
else:
    contigs, _, _ = gen_synth.generate(int(args.genome_mbp * 1e6), args.n_ctg, 10, 3)
    if args.genome_cache:
        np.save(args.genome_cache, np.concatenate(contigs))
names = ["chr%d" % (i + 1) for i in range(args.n_ctg)]
has_stats = hasattr(mpa.lib(), "mpa_idx_build_last_stats")
ctx = mpa.Context(0)
idx = mpa.Index.from_nt4(contigs, names)
idx.to_device(ctx)


def build_once():
    t0 = time.time()
    where = idx.build_kmers(1, ctx)
    dt = time.time() - t0
    if where != "gpu":
        raise SystemExit("the device build declined: " + mpa.last_error())
    return dt, (ctx.idx_build_stats() if has_stats else None)


dt, st = build_once()                                                 # warm-up: code objects, the sort's first call
print("warm-up %.3f s  %s" % (dt, st if st else "n/a"))
if args.budget_mb:
    os.environ["MPA_IDX_BUILD_MB"] = str(args.budget_mb)
if args.passes:
    ctx.idx_build_budget(-(-44 * st["n_keys"] * 1002 // (1000 * args.passes)))
times = []
for r in range(args.repeat):
    dt, st = build_once()
    times.append(dt)
    print("device build %d: %.3f s  passes %s  keys %s  fullest pass %s" % ((r, dt) + ((st["n_pass"], st["n_keys"], st["max_pass_keys"]) if st else ("n/a",) * 3)))
print("device build: median %.3f s, min %.3f s, max %.3f s over %d (%.0f Mbp, %d contigs)" % (statistics.median(times), min(times), max(times), len(times),
                                                                                            args.genome_mbp, args.n_ctg))
if args.host_threads:
    host = mpa.Index.from_nt4(contigs, names)
    times = []
    for r in range(args.repeat):
        t0 = time.time()
        assert host.build_kmers(args.host_threads) == "host"
        times.append(time.time() - t0)
        print("host build %d (%d threads): %.3f s" % (r, args.host_threads, times[-1]))
    print("host build: median %.3f s over %d" % (statistics.median(times), len(times)))
