"""Made-up kernel outputs for the result stages of a DP round (miniprot_amd/csrc/dp_results_core.h; MPA_GPU_ROUND2)
and the host loop they replace, restated in numpy.  Shared by tests/test_dp_results_cpu.py (the stages with a team of one, through
mpa_dbg_dp_run_resident without a context) and tests/test_round2_gpu.py."""
import numpy as np
import miniprot_amd as mpa
import dpplan
from dpplan import EXT, GLOB, _table

EXT_BITS = mpa.F_EXT_LEFT | mpa.F_EXT_RIGHT


def is_ext(tasks):
    return (tasks["flag"] & EXT_BITS) != 0


def made_up(tasks, rng, nc=None, zero_every=0):
    """(ext_out [n, 4], score [n], n_cigar [n], gids): random outputs for every call -- also where the call's mode never reads them -- and
    the traceback calls in a shuffled order, as a planner that sorts by class and rows leaves them"""
    n = len(tasks)
    eo = rng.integers(-5000, 1 << 20, (n, 4)).astype(np.int32)
    sc = rng.integers(-(1 << 20), 1 << 20, n).astype(np.int32)
    words = rng.integers(1, 3000, n).astype(np.int32) if nc is None else np.asarray(nc, dtype=np.int32)
    if zero_every:
        words[::zero_every] = 0
    gids = np.flatnonzero(~is_ext(tasks)).astype(np.int32)
    rng.shuffle(gids)
    return eo, sc, words, gids


def host_loop(tasks, eo, sc, nc, gids):
    """dp_assemble()'s offsets and its last loop as they were before the shared rule: dense offsets in sorted-call order, then one record
    per call from the caller's own task (an extension call of fewer than three rows: (0, al + 1, INT32_MIN), which no kernel computes)"""
    off_of, pool_n = {}, 0
    for g in gids.tolist():
        off_of[g] = pool_n
        pool_n += int(nc[g])
    rst = np.zeros(len(tasks), dtype=mpa.DP_RST)
    for k in range(len(tasks)):
        if int(tasks["flag"][k]) & EXT_BITS and int(tasks["nl"][k]) < 3:   # no row to sweep: the contract of include/mpamd.h, whatever the outputs hold
            rst[k] = (0, int(tasks["al"][k]) + 1, -2 ** 31, 0, 0)
        elif int(tasks["flag"][k]) & EXT_BITS:
            rst[k] = (eo[k, 0], eo[k, 1], eo[k, 2], 0, 0)
        else:
            rst[k] = (tasks["nl"][k], tasks["al"][k], sc[k], nc[k], off_of[k])
    return rst, pool_n


def table(seed, n_ext, n_glob):
    """n_ext extension and n_glob traceback calls of small shapes, interleaved"""
    r = np.random.default_rng(seed)
    spec = [(EXT, int(r.integers(1, 200)), int(r.integers(3, 900))) for _ in range(n_ext)] + [(GLOB, int(r.integers(1, 200)), int(r.integers(3, 900))) for _ in range(n_glob)]
    order = r.permutation(len(spec))
    return _table(r, [spec[k] for k in order])


def bounds_of(tasks):
    """dp_plan_prep_bound(): the sum of ceil(nl / 1024), the largest nl, the largest al (none below 0)"""
    nl = np.maximum(tasks["nl"].astype(np.int64), 0)
    return int(((nl + 1023) // 1024).sum()), int(nl.max(initial=0)), int(max(int(tasks["al"].max(initial=0)), 0))
