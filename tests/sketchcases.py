"""Shared by tests/test_sketch_host.py and tests/test_sketch_gpu.py: the binding of mpa_dbg_seed_jobs / mpa_idx_bucket_counts, the
queries that reach the branches of the sketch stage (map.c:126-170, sketch.c:18-38) and a numpy restatement of that stage built
from the oracle's mpo_sketch_prot (pinned to the reference in tests/test_oracle.py)."""
import ctypes as C
import os
import numpy as np
import miniprot_amd as mpa
import refbind
import seedopts

NCPU = min(16, os.cpu_count() or 4)
MAX_OCC = [None, 200]                                   # mp_mapopt_t::max_occ: the default, and one that cuts below the boxplot bound


def seed_jobs(ctx, idx, mo, q, threads=NCPU):
    """(queries the device handed to the host, off[n + 1], triples[off[-1], 3] = (qpos, bucket, cnt), max_occ[n])"""
    L = mpa.lib()
    L.mpa_dbg_seed_jobs.restype = C.c_int64
    L.mpa_dbg_seed_jobs.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(mpa.MapOpt), C.POINTER(mpa.QBatch), C.c_int, C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p)]
    n = len(q.seqs)
    off, mocc = np.zeros(n + 1, np.int64), np.full(max(n, 1), -7, np.int32)
    out = C.c_void_p()
    back = L.mpa_dbg_seed_jobs(ctx.h if ctx else None, idx.h, C.byref(mo), C.byref(q.c), threads, off.ctypes.data, mocc.ctypes.data, C.byref(out))
    assert back >= 0, mpa.last_error()
    m = int(off[-1])
    t = np.ctypeslib.as_array(C.cast(out, C.POINTER(C.c_int32)), (max(3 * m, 1),))[:3 * m].copy().reshape(m, 3)
    L.mpa_free(out)
    return int(back), off, t, mocc[:n]


def bucket_counts(idx, bucket):
    L = mpa.lib()
    L.mpa_idx_bucket_counts.restype = C.c_int
    L.mpa_idx_bucket_counts.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
    b = np.ascontiguousarray(bucket, dtype=np.uint32)
    cnt = np.zeros(max(len(b), 1), np.int64)
    assert L.mpa_idx_bucket_counts(idx.h, len(b), b.ctypes.data, cnt.ctypes.data) == 0, mpa.last_error()
    return cnt[:len(b)]


def restated(idx, kmer, mod_bit, seqs, max_occ):
    """map.c:126-170 restated: per query (sketch size, cut-off in force, kept (qpos, bucket, cnt) triples in ascending position)"""
    res = []
    for s in seqs:
        buf = np.zeros(len(s) + 1, np.uint64)
        n = int(refbind.ora().mpo_sketch_prot(s, len(s), kmer, mod_bit, buf.ctypes.data))
        sk = buf[:n]
        bkt, pos = (sk >> np.uint64(32)).astype(np.int64), (sk & np.uint64(0xffffffff)).astype(np.int64)
        cnt = bucket_counts(idx, bkt)
        mo = max_occ
        if n >= 8:                                           # mp_cal_max_occ (map.c:126-141)
            srt = np.sort(cnt)
            q25, q75 = int(srt[int(n * .25 + .499)]), int(srt[int(n * .75 + .499)])
            mo = min(mo, int(q75 + (q75 - q25) * 1.5 + 10.))
        keep = (cnt > 0) & (cnt <= mo)
        res.append((n, mo, np.stack([pos[keep], bkt[keep], cnt[keep]], axis=1).astype(np.int32).reshape(-1, 3)))
    return res


def branch_queries(seqs, kmer):
    """queries chosen for the branches, from the proteins of seedopts.tandem_genome(): lengths k .. k + 20 (sketches of 0 .. ~20 seeds
    on both sides of the n >= 8 branch), run resets (X, *, U, lower case, bytes that are no letters), equal counts at the quantile
    positions (poly-K, a repeated domain), an empty query"""
    p0, p1, p2 = seqs[40], seqs[41], seqs[42]                 # planted originals
    out = [p[3:3 + n] for p in (p0, p1, p2) for n in range(kmer, kmer + 21)]
    broken = bytearray(p2[:240])
    for at, c in ((17, b"X"), (40, b"*"), (41, b"*"), (63, b"U"), (90, b"-"), (117, b"1"), (150, b"\xff"), (171, b"\x00"), (200, b" ")):
        broken[at:at + 1] = c
    broken[100:112] = bytes(broken[100:112]).lower()
    out += [bytes(broken), b"M" + b"K" * 50, p0[:120] * 4, b"", b"X" * 30, p1[:kmer - 1]]
    return out


def all_queries(kmer):
    contigs, seqs = seedopts.tandem_genome(5, 35)
    return contigs, list(seqs) + branch_queries(seqs, kmer)


def mapopt(max_occ):
    mo = mpa.default_mapopt()
    if max_occ is not None:
        mo.max_occ = max_occ
    return mo
