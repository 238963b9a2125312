"""mpa_dp_run() at the edges of a call's inputs (tests/dpedges.py): windows of fewer than three rows, slices of longer queries (also
behind a prefix that belongs to no query), windows at contig and buffer ends on both strands (also under a splice-score track), query
bytes outside the amino-acid alphabet.  Bit-exact on (nt_len, aa_len, score, CIGAR) against the oracle and, where it is built, against
the reference, which tests/test_dp_edges_cpu.py shows to agree on every one of these calls.  The extension calls of fewer than three
rows, on which the reference fails its own assertion, must return the oracle's (0, al + 1, INT32_MIN): the contract of include/mpamd.h.

Default context over all four families; tiny, slices and ends again under every executor setting that changes which kernel sweeps a
call (the knobs are read when a context is created: each setting is an environment and a fresh context) and under penalties that
route to the exact kernels.  Expectations are computed once per family and scoring point and shared."""
import os
import numpy as np
import pytest
import miniprot_amd as mpa
import dpedges
import dpplan
import golden
import refbind
from dputil import dpopt_from_params, compare

pytestmark = pytest.mark.gpu

KNOB_ENV = ("MPA_DP_LITE_MIN", "MPA_DP_LITE_WIDE", "MPA_DP_SPLIT_WIDE", "MPA_DP_HUGE_WG", "MPA_TB_BUDGET_MB")
SWEPT = ("tiny", "slices", "ends")                      # the families run under every setting
X_HUGE, X_SPLIT8 = 7, 9


def params(**over):
    return refbind.DpParams(refbind.mapping_matrix(23), **over)


@pytest.fixture(scope="module")
def ctx():
    c = mpa.Context(0)
    yield c
    c.close()


def fresh_context(monkeypatch, **env):
    for k in KNOB_ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    return mpa.Context(0)


def check(cs, rst, cig, expect, what):
    bad, msg = compare(rst, cig, expect, cs.meta3(), cs.calls())
    assert not bad, "%s: %d/%d DP calls differ\n%s" % (what, len(bad), len(cs.tasks), msg)


def run_family(ctx, name, P, key, queries=None):
    """one mpa_dp_run() over the family against the oracle and the reference; returns the context's statistics of the run"""
    cs = dpedges.case(name)
    idx = mpa.Index.from_nt4(cs.contigs)
    idx.to_device(ctx)
    try:
        rst, cig = mpa.dp_run(ctx, idx, dpopt_from_params(P), queries or cs.queries, cs.tasks)
    finally:
        idx.close()
    ora = dpedges.expected(name, P, key)
    check(cs, rst, cig, ora, "%s (%s) against the oracle" % (name, key))
    if refbind.have_ref():                              # (the extension calls of fewer than three rows: the contract, which is the oracle's triple)
        ref = [o if r is None else r for o, r in zip(ora, dpedges.expected(name, P, key, "ref"))]
        check(cs, rst, cig, ref, "%s (%s) against the REFERENCE" % (name, key))
    for k in cs.tiny_ext():
        got = (int(rst[k]["nt_len"]), int(rst[k]["aa_len"]), int(rst[k]["score"]), int(rst[k]["n_cigar"]))
        assert got == (0, int(cs.tasks["al"][k]) + 1, -2 ** 31, 0), (k, got)
    return ctx.dp_stats()


def planned(name, over=None, **knobs):
    cs = dpedges.case(name)
    p = dpplan.plan(cs.tasks, over, knobs, ctg_len=cs.ctg_len(), qoff=cs.q_off())
    assert isinstance(p, dpplan.Plan), p
    return p


@pytest.mark.parametrize("name", sorted(dpedges.FAMILIES))
def test_default_context(ctx, oracle_built, name):
    st = run_family(ctx, name, params(), "default")
    cs = dpedges.case(name)
    ext = (cs.tasks["flag"] & (mpa.F_EXT_LEFT | mpa.F_EXT_RIGHT)) != 0
    assert st["n_ext"] == ext.sum() and st["n_glob"] == (~ext).sum() and st["n_ckpt"] == planned(name).header["st_n_ckpt"]


def test_slices_of_a_batch_behind_a_prefix(ctx, oracle_built):
    """the same query buffer passed as a slice of a larger one: q_off[0] = 37, and 37 bytes in front that belong to no query"""
    run_family(ctx, "slices", params(), "default", queries=dpedges.PrefixedQueries(dpedges.case("slices").queries))


def test_ends_with_a_splice_score_track(ctx, oracle_built, tmp_path):
    """the ends family once more with --spsc loaded: the track is addressed like the genome (g.spsc + (rev ? l_seq : 0) + off), so its
    first and last bytes on both strands are read by windows with nt_off = 0 and by windows that end their contig; calls with and
    without MPA_F_SS_SKIP0; the expectation is fed the bytes idx.get_spsc returns"""
    cs = dpedges.case("ends")
    P = params(io=39, sp_null_bonus=-7)
    idx = mpa.Index.from_nt4(cs.contigs, ["chr%d" % (i + 1) for i in range(len(cs.contigs))])
    idx.set_spsc(golden.write_spsc({"spsc": 77}, cs.contigs, str(tmp_path / "s.tsv")), mpa.default_mapopt(), keep_io=True)
    ss = dpedges.spsc_bytes(cs, idx)
    idx.to_device(ctx)
    dp = dpopt_from_params(P)
    dp.sp_null_bonus = P.sp_null_bonus
    try:
        rst, cig = mpa.dp_run(ctx, idx, dp, cs.queries, cs.tasks)
    finally:
        idx.close()
    check(cs, rst, cig, dpedges.evaluate(cs, P, refbind.ora_nasw, ss), "ends with a score track against the oracle")
    if refbind.have_ref():
        check(cs, rst, cig, dpedges.evaluate(cs, P, refbind.ref_nasw, ss), "ends with a score track against the REFERENCE")
    # the same track, same calls, without it: some results must differ, or the track was not applied
    plain = dpedges.expected("ends", params(), "default")
    assert sum(int(r["score"]) != e[2] for r, e in zip(rst, plain)) > 20


@pytest.mark.parametrize("lite_min", ["3", "0"])
@pytest.mark.parametrize("name", SWEPT)
def test_checkpointed_from_three_rows(oracle_built, monkeypatch, name, lite_min):
    """MPA_DP_LITE_MIN=3: traceback calls of three to five rows and up to 128 columns take the packed sweep and k_walk with a single,
    partial block; exactly the calls the planner says are counted as checkpointed, and with 0 none"""
    c = fresh_context(monkeypatch, MPA_DP_LITE_MIN=lite_min)
    try:
        st = run_family(c, name, params(), "default")
    finally:
        c.close()
    want = planned(name, lite_min=int(lite_min)).header["st_n_ckpt"]
    assert st["n_ckpt"] == want and (want > 0 if lite_min == "3" else want == 0), (st["n_ckpt"], want)
    assert st["n_ckpt_wide"] == 0


@pytest.mark.parametrize("name", SWEPT)
def test_checkpointed_up_to_256_columns(oracle_built, monkeypatch, name):
    """... with MPA_DP_LITE_WIDE=1: 129 .. 256 columns on the four-wave packed sweep"""
    c = fresh_context(monkeypatch, MPA_DP_LITE_MIN="3", MPA_DP_LITE_WIDE="1")
    try:
        st = run_family(c, name, params(), "default")
    finally:
        c.close()
    pool = int(os.environ.get("MPA_DP_POOL") or 0) != 0  # (tests/test_dp_pool_gpu.py: the worker pool keeps 129 .. 256 columns on the plain sweep)
    h = planned(name, lite_min=3, lite_wide=1, pool=int(pool)).header
    assert st["n_ckpt"] == h["st_n_ckpt"] and st["n_ckpt_wide"] == h["st_n_ckpt_wide"] and (pool or h["st_n_ckpt_wide"] > 0)


@pytest.mark.parametrize("name", SWEPT)
def test_split_wide_classes(oracle_built, monkeypatch, name):
    """MPA_DP_SPLIT_WIDE=1: the 1 025- and 1 100-column extension calls of three rows and more on eight workgroups with their HBM hand-off"""
    c = fresh_context(monkeypatch, MPA_DP_SPLIT_WIDE="1")
    try:
        run_family(c, name, params(), "default")
        classes = mpa.dbg_dp_last_classes(c)
        assert c.handoff_retries() == 0
    finally:
        c.close()
    cs = dpedges.case(name)
    wide = int((((cs.tasks["flag"] & (mpa.F_EXT_LEFT | mpa.F_EXT_RIGHT)) != 0) & (cs.tasks["al"] > 1024) & (cs.tasks["nl"] >= 3)).sum())
    assert classes[X_SPLIT8] + classes[X_HUGE] == wide and (name == "ends" or wide > 0)


@pytest.mark.parametrize("name", SWEPT)
def test_huge_calls_block_parallel(oracle_built, monkeypatch, name):
    """MPA_DP_HUGE_WG=1: the int32 extension sweep with one wave per column block, down to a single swept row"""
    c = fresh_context(monkeypatch, MPA_DP_HUGE_WG="1")
    try:
        run_family(c, name, params(), "default")
    finally:
        c.close()


@pytest.mark.parametrize("name", SWEPT)
def test_several_traceback_rounds(oracle_built, monkeypatch, name):
    """MPA_TB_BUDGET_MB=1: the traceback calls in several chunks, tiny calls in each"""
    c = fresh_context(monkeypatch, MPA_TB_BUDGET_MB="1")
    try:
        run_family(c, name, params(), "default")
    finally:
        c.close()
    assert planned(name, tb_budget=1 << 20).header["n_tb_chunks"] > 1


@pytest.mark.parametrize("over", [dict(ge=300), dict(go=31000, ge=100)], ids=["wide_ge", "may_saturate"])
@pytest.mark.parametrize("name", SWEPT)
def test_penalties_that_route_to_the_exact_kernels(ctx, oracle_built, name, over):
    """ge = 300: the kernels that read a record's byte 2 as a stop flag (every call on the stand-alone int32 sweeps); go = 31 000,
    ge = 100: the int16 guard sends calls of 16 columns and more to the int32 sweeps"""
    run_family(ctx, name, params(**over), "go%d_ge%d" % (over.get("go", 11), over["ge"]))
