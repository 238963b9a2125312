"""Operator parity on the GPU between miniprot's default scores and the limits mpa_dp_run() accepts: every parameter point of
dpgen.PENALTY_POINTS and both sides of every int16 bound case (dpgen.BOUND_CASES) is one mpa.dp_run batch holding calls of every
executor class -- extension calls of 16, 32 and 64 lanes, the 65..128-column one-wave class, the wide classes with and without the
split hand-off, k_ext_huge, the plain traceback sweep and the checkpointed one.  (nt_len, aa_len, score, CIGAR) of every call
against the oracle and, where it is built, against the reference's ns_global_gs16b; and the routing: every call is accepted, a
call that could saturate int16 never takes the checkpointed sweep."""
import os
import zlib
from concurrent.futures import ThreadPoolExecutor
import numpy as np
import pytest
import miniprot_amd as mpa
import refbind
from dpgen import make_task, long_window, PENALTY_POINTS, BOUND_CASES, bound_params
from dputil import build_workload, dpopt_from_params, compare

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = mpa.Context(0)
    yield c
    c.close()


def _params(kw):
    return refbind.DpParams(refbind.mapping_matrix(min(kw.get("fs", 23), 127)), **kw)


def _may_saturate(P, al):
    """dp_plan.cpp's predicate: the call goes to the int32 sweeps"""
    ncol = (al + 7) // 8 * 8
    return al * int(P.mat.max()) + ncol * P.ge + max(0, P.end_bonus) > 32000 or P.go + ncol * P.ge > 32000


def _checkpointed(P, nl, al, lite_min):
    # (a restatement of the routing: the n_ckpt assertion shows that the executor routes as intended; whether the bound sits in the
    # right place is shown by the comparison with the oracle and the reference on both sides of it, test_int16_bound)
    return lite_min > 0 and P.ge <= 255 and P.fs <= 255 and not _may_saturate(P, al) and (al + 7) // 8 * 8 <= 128 and nl >= max(lite_min, 3)


def _class_pairs(rng, extra=()):
    """short windows of every extension class (and, as traceback calls, of the plain sweep), then windows of >= 384 rows and
    <= 128 columns (the checkpointed sweep)"""
    pairs = [make_task(rng, al=al, p_intron=0.01, max_intron=300, flank=200)
             for al in (12, 16, 24, 32, 40, 64, 72, 128, 200, 256, 400, 600, 1030) + tuple(extra)]
    pairs += [long_window(rng, al) for al in (8, 20, 40, 64, 90, 128)]
    return pairs


def _expect(fn, P, pairs, meta):
    """fn (refbind.ora_nasw / ref_nasw) on every call, a few at a time (ctypes lets go of the GIL; both are reentrant)"""
    refbind.ora(), refbind.have_ref() and refbind.ref()                # (load the libraries before the threads do)

    def one(m):
        k, fl, io = m
        PP = refbind.DpParams(P.mat, go=P.go, ge=P.ge, io=io, fs=P.fs, xdrop=P.xdrop, end_bonus=P.end_bonus, sp=P.sp,
                              sp_null_bonus=P.sp_null_bonus, ie_coef=P.ie_coef)
        return fn(pairs[k][0], pairs[k][1], PP, fl)
    with ThreadPoolExecutor(max_workers=8) as ex:
        return list(ex.map(one, meta))


def _run(ctx, P, pairs, rng, lite_min=384, what=""):
    contigs, queries, tasks, meta = build_workload(pairs, rng, io=P.io, io_alt=max(0, P.io - 10))
    idx = mpa.Index.from_nt4(contigs)
    idx.to_device(ctx)
    try:
        rst, cig = mpa.dp_run(ctx, idx, dpopt_from_params(P), queries, tasks)     # (MpaError: a call was refused)
        st = ctx.dp_stats()
    finally:
        idx.close()
    bad, msg = compare(rst, cig, _expect(refbind.ora_nasw, P, pairs, meta), meta, pairs)
    assert not bad, "%s: %d/%d DP calls differ from the oracle\n%s" % (what, len(bad), len(tasks), msg)
    if refbind.have_ref():
        bad, msg = compare(rst, cig, _expect(refbind.ref_nasw, P, pairs, meta), meta, pairs)
        assert not bad, "%s: %d/%d DP calls differ from the REFERENCE\n%s" % (what, len(bad), len(tasks), msg)
    n_ckpt = sum(_checkpointed(P, len(pairs[k][0]), len(pairs[k][1]), lite_min) for k, fl, _ in meta if fl == mpa.F_CIGAR)
    assert st["n_ckpt"] == n_ckpt, "%s: %d checkpointed traceback calls, expected %d" % (what, st["n_ckpt"], n_ckpt)
    return meta


def _lite_min_of_this_process():
    s = os.environ.get("MPA_DP_LITE_MIN")
    return int(s) if s is not None else 384


@pytest.mark.parametrize("kw", PENALTY_POINTS, ids=lambda kw: ",".join("%s=%s" % x for x in kw.items()))
def test_penalty_point(ctx, oracle_built, kw):
    P = _params(kw)
    rng = np.random.default_rng(zlib.crc32(repr(kw).encode()))
    _run(ctx, P, _class_pairs(rng), rng, _lite_min_of_this_process(), what=str(kw))


@pytest.mark.parametrize("over", [0, 1], ids=["at32000", "at32001"])
@pytest.mark.parametrize("case", BOUND_CASES, ids=lambda c: "al%d-%s" % (c[0], c[2]))
def test_int16_bound(ctx, oracle_built, case, over):
    """calls whose larger sum of may_saturate is exactly 32000 (packed kernels) or 32001 (int32 sweeps), next to calls 8 columns
    narrower and wider, in a batch of every class"""
    al = case[0]
    kw = bound_params(case, over)
    P = _params(kw)
    ncol = (al + 7) // 8 * 8
    assert max(al * int(P.mat.max()) + ncol * P.ge + max(0, P.end_bonus), P.go + ncol * P.ge) == 32000 + over
    assert _may_saturate(P, al) == (over == 1)
    rng = np.random.default_rng(zlib.crc32(repr(kw).encode()))
    pairs = []
    for a in (al, al, al - 8, al + 8):                              # (no amino-acid indels: the query keeps a residues)
        pairs.append(make_task(rng, al=a, p_intron=0.01, max_intron=300, flank=200, p_indel=0.0))
        if a <= 136:
            pairs.append(long_window(rng, a, p_indel=0.0))
    pairs += _class_pairs(rng)
    lite_min = _lite_min_of_this_process()
    meta = _run(ctx, P, pairs, rng, lite_min, what=str(kw))
    assert sum(len(aa) == al for _, aa in pairs) >= 2
    if al <= 128 and lite_min <= 384:                             # the checkpointed calls at the bound were there to be routed
        assert any(fl == mpa.F_CIGAR and len(pairs[k][1]) == al and len(pairs[k][0]) >= 384 for k, fl, _ in meta)


def test_lowered_row_threshold_on_a_fresh_context(oracle_built, monkeypatch):
    """MPA_DP_LITE_MIN is read when a context is created: lowered to 3 on a new context (after other contexts of the process have
    run DP rounds), windows of one and of two 96-row blocks take the checkpointed sweep -- unless the call could saturate"""
    monkeypatch.setenv("MPA_DP_LITE_MIN", "3")
    c2 = mpa.Context(0)
    try:
        P = _params(dict(go=30400, ge=25))                       # go + ncol * ge > 32000 from 72 columns on
        rng = np.random.default_rng(77)
        pairs = []
        for lo, hi, als in ((3, 97, (1, 8, 12, 16, 17, 24)), (97, 193, (17, 24, 32, 40, 48, 56))):
            for al in als:
                while True:
                    nt, aa = make_task(rng, al=al, p_intron=0.02, max_intron=60, flank=int(rng.integers(1, 60)))
                    if lo <= len(nt) < hi:
                        break
                pairs.append((nt, aa))
        pairs += _class_pairs(rng)
        _run(c2, P, pairs, rng, 3, what="lite_min 3")
        assert c2.dp_stats()["n_ckpt"] >= 20                     # (the 12 windows above, and most of _class_pairs' up to 64 columns)
    finally:
        c2.close()


def test_columns_times_ge_beyond_the_int32_sweeps(ctx, oracle_built):
    """ncol * ge >= 2^19 is the documented limit of the int32 sweeps: such a call is refused, alone in its batch, in both modes"""
    rng = np.random.default_rng(5)
    P = _params(dict(ge=255))
    pairs = [make_task(rng, al=2064, p_intron=0.0, p_indel=0.0, flank=20)]            # 2064 * 255 = 526 320 >= 2^19
    for mode in ("right", "cigar"):
        contigs, queries, tasks, meta = build_workload(pairs, rng, modes=(mode,), io=P.io)
        idx = mpa.Index.from_nt4(contigs)
        idx.to_device(ctx)
        try:
            with pytest.raises(mpa.MpaError, match="2\\^19"):
                mpa.dp_run(ctx, idx, dpopt_from_params(P), queries, tasks)
        finally:
            idx.close()
