"""Shared by tests/test_seed_nopre_cpu.py and tests/test_seed_nopre_gpu.py: the binding of mpa_dbg_sift_kept and the keep rule of
the direct seeding route (a run without a pre-chain, MPA_GPU_SEED_NOPRE=1) stated in numpy."""
import ctypes as C
import numpy as np
import miniprot_amd as mpa

UNSUPPORTED = -3                                       # MPA_ERR_UNSUPPORTED (include/mpamd.h)
SIFT_REACH_MAX = 15                                    # beyond it the sift keeps every anchor (mpa_internal.h: kSiftReachMax)


def reach_of(mo, bbit):
    """blocks the main chain can bridge on the target: max_dist_x >> bbit with mp_chain's max_dist_x = max(max_intron, bw) (chain.c:164)"""
    return max(int(mo.max_intron), int(mo.bw)) >> bbit


def sift_kept(ctx, idx, mo, q, threads=4):
    """(rc or total, off, kept anchors, hand-back flags, reach) from mpa_dbg_sift_kept; off .. reach are None when rc < 0"""
    L = mpa.lib()
    L.mpa_dbg_sift_kept.restype = C.c_int64
    L.mpa_dbg_sift_kept.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(mpa.MapOpt), C.POINTER(mpa.QBatch), C.c_int, C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p,
                                    C.POINTER(C.c_int32)]
    n_q = len(q.seqs)
    off, flag = np.zeros(n_q + 1, np.int64), np.full(n_q, -1, np.int32)
    out, reach = C.c_void_p(), C.c_int32(-1)
    n = L.mpa_dbg_sift_kept(ctx.h if ctx else None, idx.h, C.byref(mo), C.byref(q.c), threads, off.ctypes.data, C.byref(out), flag.ctypes.data, C.byref(reach))
    if n < 0:
        return int(n), None, None, None, None
    a = np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_uint64)), (max(n, 1),))[:n].copy()
    L.mpa_free(out)
    return int(n), off, a, flag, int(reach.value)


def rule_keeps(a, reach):
    """the kept ones of one query's sorted anchors (block << 32 | query position): those whose predecessor or successor in the list
    lies at most `reach` blocks away -- not a run of one under the run rule of the chain's forward pass; all of them when the reach
    is beyond what the sift filters by"""
    if reach > SIFT_REACH_MAX or len(a) == 0:
        return a
    blk = (a >> np.uint64(32)).astype(np.int64)
    near = np.diff(blk) <= reach                          # near[i]: anchors i and i + 1 are within reach
    keep = np.zeros(len(a), bool)
    keep[1:] |= near
    keep[:-1] |= near
    return a[keep]
