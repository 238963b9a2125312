"""The edge-case DP calls of tests/dpedges.py, without a device: (1) the oracle equals the reference on every generated call, so that what
tests/test_dp_edges_gpu.py expects is the reference's own; (2) the families contain what they promise, read from the task tables and
from the host planner's plan of them (tests/dpplan.py: the routing is not restated here); (3) the planner gives an extension call of
fewer than three rows no descriptor and no unit, on the host and in the model of the device planner.

The only calls the reference is not run on are the extension calls of fewer than three rows, on which it fails its own assertion
(nasw-sse.c:441): 48 of them, all in the family `tiny` (nl 0, 1, 2 x left, right x al 8, 24, 50, 100, 200, 400, 800, 1100), none elsewhere.
For those the oracle returns (0, al + 1, INT32_MIN), which is the contract of mpa_dp_run() (include/mpamd.h).

Calls and classes (default knobs; DpClass numbers of dp_device.h; extension 11 = X_NONE, traceback 8 .. 12 = checkpointed):
  family    calls  extension classes            traceback classes
  tiny        463  0 1 2 4 5 6 7 8 11           0 1 2 3 4 5 6 7 8 9 10 11
  slices      108  0 1 2 4 5 6 7 8              0 4 5 6 7 8 9 10 11
  ends        832  0 2 4 5 8                    0 2 3 4 5 8 10 11
  alphabet    450  0 1 2 4 8                    0 1 2 4 8 9 10 11
With MPA_DP_LITE_MIN=3 and MPA_DP_LITE_WIDE=1 the three first families together hold every checkpointed class 8 .. 12, with
MPA_DP_EXT_DUAL=0 extension class 3 (X_W2).  X_SPLIT8 takes tiny's and slices' 1 025- and 1 100-column extension calls under
MPA_DP_SPLIT_WIDE=1; X_SPLIT12 needs more than 2 048 columns and is not reached by these families (tests/test_dp_split_wide_gpu.py)."""
import numpy as np
import pytest
import miniprot_amd as mpa
import dpedges
import dpplan
import dpplan_device as dd
import golden
import refbind

INT32_MIN = -2 ** 31
TINY_EXT = {"tiny": 48, "slices": 0, "ends": 0, "alphabet": 0}
X_16, X_32, X_64, X_W2, X_W4, X_SPLIT2, X_SPLIT4, X_HUGE, X_128, X_NONE = 0, 1, 2, 3, 4, 5, 6, 7, 8, 11
EXT = mpa.F_EXT_LEFT | mpa.F_EXT_RIGHT

needs_ref = pytest.mark.skipif(not refbind.have_ref(), reason="the reference is not built here")


def host_plan(cs, over=None, knobs=None):
    p = dpplan.plan(cs.tasks, over, knobs, ctg_len=cs.ctg_len(), qoff=cs.q_off())
    assert isinstance(p, dpplan.Plan), p
    return p


def classes(cs, over=None, knobs=None):
    T = host_plan(cs, over, knobs).sec["tasks"]
    ext = (T["flag"] & EXT) != 0
    return set(int(c) for c in T["cls"][ext]), set(int(c) for c in T["cls"][~ext])


@needs_ref
@pytest.mark.parametrize("name", sorted(dpedges.FAMILIES))
def test_oracle_equals_reference(name, oracle_built):
    cs = dpedges.case(name)
    P = refbind.DpParams(refbind.mapping_matrix(23))
    ora, ref = dpedges.expected(name, P, "default"), dpedges.expected(name, P, "default", "ref")
    left_out = [k for k, r in enumerate(ref) if r is None]
    assert left_out == cs.tiny_ext() and len(left_out) == TINY_EXT[name], "only the extension calls of fewer than three rows are left out"
    bad = [(k, ora[k], ref[k]) for k in range(len(ora)) if ref[k] is not None and ora[k] != ref[k]]
    assert not bad, "%d/%d calls: oracle != reference, first %r" % (len(bad), len(ora), bad[0])


@pytest.mark.parametrize("name", sorted(dpedges.FAMILIES))
def test_tiny_extension_set(name, oracle_built):
    """the set the reference comparison leaves out: counted, and exactly nl 0 .. 2 x both modes x TINY_EXT_AL in `tiny`; the oracle
    returns what the reference computes with its assertions compiled out"""
    cs = dpedges.case(name)
    te = cs.tiny_ext()
    assert len(te) == TINY_EXT[name]
    if name == "tiny":
        got = sorted((int(cs.tasks["nl"][k]), int(cs.tasks["flag"][k]), int(cs.tasks["al"][k])) for k in te)
        assert got == sorted((nl, fl, al) for nl in (0, 1, 2) for fl in (mpa.F_EXT_LEFT, mpa.F_EXT_RIGHT) for al in dpedges.TINY_EXT_AL)
    ora = dpedges.expected(name, refbind.DpParams(refbind.mapping_matrix(23)), "default")
    for k in te:
        assert ora[k] == (0, int(cs.tasks["al"][k]) + 1, INT32_MIN, []), (k, ora[k])


@needs_ref
def test_oracle_equals_reference_with_a_splice_score_track(oracle_built, tmp_path):
    cs = dpedges.case("ends")
    idx = mpa.Index.from_nt4(cs.contigs, ["chr%d" % (i + 1) for i in range(len(cs.contigs))])
    assert idx.set_spsc(golden.write_spsc({"spsc": 77}, cs.contigs, str(tmp_path / "s.tsv")), mpa.default_mapopt(), keep_io=True) > 100
    ss = dpedges.spsc_bytes(cs, idx)
    idx.close()
    assert sum(any(b != 0xff for b in s) for s in ss) > len(ss) // 2, "most windows see a score"
    P = refbind.DpParams(refbind.mapping_matrix(23), io=39, sp_null_bonus=-7)
    ora, ref = dpedges.evaluate(cs, P, refbind.ora_nasw, ss), dpedges.evaluate(cs, P, refbind.ref_nasw, ss)
    bad = [(k, a, b) for k, (a, b) in enumerate(zip(ora, ref)) if a != b]
    assert not bad, "%d/%d calls: oracle != reference, first %r" % (len(bad), len(ora), bad[0])


def test_tiny_holds_every_shape_it_promises():
    cs = dpedges.case("tiny")
    T = cs.tasks
    ext = (T["flag"] & EXT) != 0
    for nl in range(6):
        for al in dpedges.EDGES:
            here = (T["nl"] == nl) & (T["al"] == al) & (T["aa_off"] == 0)
            assert (here & (T["flag"] == mpa.F_CIGAR)).any(), (nl, al)
            if nl >= 3:
                assert (here & (T["flag"] == mpa.F_EXT_LEFT)).any() and (here & (T["flag"] == mpa.F_EXT_RIGHT)).any(), (nl, al)
    with_n = [k for k, (p, *_) in enumerate(cs.meta) if T["nl"][k] in (1, 2, 3, 4, 5) and 4 in cs.windows[p]]
    assert len(with_n) >= 20
    assert (T["nl"][~ext] >= 384).sum() >= 3 and (T["nl"] >= 6).sum() >= 150 and ((T["nl"] >= 6) & (T["nl"] < 384)).sum() >= 50, "long windows and ordinary calls in the same batch"
    # rows descending inside a class: tiny calls share wave descriptors with long ones, and fill last waves partly
    P = host_plan(cs)
    Tp = P.sec["tasks"]
    mixed, partly = set(), set()
    for sec, per in (("ewaves", {0: 8, 1: 4, 2: 2}), ("gwaves", {0: 4, 1: 2})):      # the classes that pack several calls into a wave: X_16 .. X_64, T_16, T_32
        for w in P.sec[sec]:
            ids = w["task"][w["task"] >= 0]
            cls, nls = int(Tp["cls"][ids[0]]), Tp["nl"][ids]
            if cls in per and ((Tp["flag"][ids[0]] & EXT) != 0) == (sec == "ewaves"):
                if nls.min() <= 5 < nls.max():
                    mixed.add((sec, cls))
                if nls.min() <= 5 and len(ids) < per[cls]:
                    partly.add((sec, cls))
    assert mixed == {("ewaves", 0), ("ewaves", 1), ("ewaves", 2), ("gwaves", 0), ("gwaves", 1)}, mixed
    assert partly, "a last wave that is partly filled with tiny calls"


def test_slices_hold_every_offset_family():
    cs = dpedges.case("slices")
    T, off = cs.tasks, cs.q_off()
    qlen = (off[1:] - off[:-1])[T["qid"]]
    assert len(cs.query_seqs) == 12 and 40 <= qlen.min() and qlen.max() == 1200
    front = (T["aa_off"] == 0) & (T["al"] < qlen)
    middle = (T["aa_off"] > 0) & (T["aa_off"] + T["al"] < qlen)
    end = (T["aa_off"] > 0) & (T["aa_off"] + T["al"] == qlen)
    last = end & (T["qid"] == len(cs.query_seqs) - 1)
    for fam in (front, middle, end):
        assert set(T["qid"][fam]) == set(range(12)), "every query has the slice"
        assert set(T["flag"][fam]) == {mpa.F_CIGAR, mpa.F_EXT_LEFT, mpa.F_EXT_RIGHT}
    assert set(T["flag"][last]) == {mpa.F_CIGAR, mpa.F_EXT_LEFT, mpa.F_EXT_RIGHT}, "the last residue of the buffer"
    assert (front | middle | end).all() and not (T["al"] == qlen).any(), "every call is a slice"
    assert set(dpedges.EDGES) == set(int(a) for a in T["al"])
    assert np.bincount(T["qid"]).min() >= 9, "calls share a qid"
    pre = dpedges.PrefixedQueries(cs.queries)
    assert pre.off[0] == 37 and pre.buf[37:] == cs.queries.buf and (pre.off - 37 == off).all()


def test_ends_reach_both_ends_of_every_contig_and_of_the_buffer():
    cs = dpedges.case("ends")
    T = cs.tasks
    L = np.array(cs.ctg_len())
    assert sorted(L) == [3, 17, 64, 1001, 4096] and (L[:-1] % 2 == 1).sum() >= 3, "odd lengths: the next contig starts on an odd nibble"
    assert sum(int(c[0] == 4 and c[-1] == 4) for c in cs.contigs) == 2
    cid, rev, st, en = T["vid"] >> 1, T["vid"] & 1, T["nt_off"], T["nt_off"] + T["nl"]
    modes = lambda m: set(int(f) & 7 for f in T["flag"][m])
    for c in range(len(L)):
        for r in (0, 1):
            here = (cid == c) & (rev == r)
            for name, m in (("starts the strand", st == 0), ("ends it", en == L[c]), ("is the contig", (st == 0) & (en == L[c]))):
                assert mpa.F_CIGAR in modes(here & m), (c, r, name)
                if L[c] >= 3:
                    assert modes(here & m & (T["nl"] >= 3)) == {mpa.F_CIGAR, mpa.F_EXT_LEFT, mpa.F_EXT_RIGHT}, (c, r, name)
            if L[c] > 12:
                for d in (1, 5, 6):
                    assert (here & (st == d)).any() and (here & (en == L[c] - d)).any(), (c, r, d)
    # the packed genome: position 0 is the first base of contig 0, l_seq - 1 the last base of the last contig; a window of the minus
    # strand reaches them from the other side
    last = len(L) - 1
    for r in (0, 1):
        at_0 = (cid == 0) & (rev == r) & ((st == 0) if r == 0 else (en == L[0]))
        at_end = (cid == last) & (rev == r) & ((en == L[last]) if r == 0 else (st == 0))
        assert at_0.any() and at_end.any(), r
    assert set(int(a) for a in T["al"]) == set(dpedges.ENDS_AL)
    left = (T["flag"] & mpa.F_EXT_LEFT) != 0
    skip0 = (T["flag"] & dpedges.SS_SKIP0) != 0
    assert (skip0 & ~left).sum() == 0 and (left & skip0).sum() > 50 and (left & ~skip0).sum() > 50
    assert (left & skip0 & (st == 0)).any() and (left & ~skip0 & (st == 0)).any() and (~left & (st == 0)).any(), "windows with nt_off = 0 in every flavour"


def test_alphabet_reaches_the_whole_byte_range():
    cs = dpedges.case("alphabet")
    assert len(cs.query_seqs) == 150
    seen = set(b"".join(cs.query_seqs))
    assert 0 not in seen and len(seen) >= 250, len(seen)
    assert set(b"abxzBZJOUX*-019") <= seen and any(b >= 128 for b in seen)
    n = sum(len(q) for q in cs.query_seqs)
    odd = sum(1 for q in cs.query_seqs for b in q if b not in dpedges.AA)
    assert 0.2 * n < odd < 0.4 * n


def test_every_class_occurs():
    """from the host planner's plan of the families (the debug hook): every extension and traceback class dp_classify_call can give a
    call of at most 1 100 columns occurs in tiny, slices and ends"""
    ext, tb = set(), set()
    for name in ("tiny", "slices", "ends"):
        e, t = classes(dpedges.case(name))
        ext |= e
        tb |= t
    assert ext == {X_16, X_32, X_64, X_W4, X_SPLIT2, X_SPLIT4, X_HUGE, X_128, X_NONE}, ext
    assert set(range(8)) <= tb and tb <= set(range(12)), tb          # T_16 .. T_MB, and the long windows' checkpointed classes
    lite, dual = set(), set()
    for name in ("tiny", "slices", "ends"):
        lite |= classes(dpedges.case(name), knobs=dict(lite_min=3, lite_wide=1))[1]
        dual |= classes(dpedges.case(name), knobs=dict(ext_dual=0))[0]
    assert {8, 9, 10, 11, 12} <= lite, lite                           # T_LITE16 .. T_LITE128, T_LITE_W4
    assert X_W2 in dual and X_128 not in dual
    # the exact kernels: ge = 300 puts every swept extension call on the int32 sweep; go = 31000, ge = 100 those of 16 columns or more
    for name in ("tiny", "slices", "ends"):
        cs = dpedges.case(name)
        T = host_plan(cs, dict(ge=300)).sec["tasks"]
        e = (T["flag"] & EXT) != 0
        assert set(int(c) for c in T["cls"][e]) <= {X_HUGE, X_NONE} and (T["cls"][~e] < 8).all()
        T = host_plan(cs, dict(go=31000, ge=100)).sec["tasks"]
        e = (T["flag"] & EXT) != 0
        assert (T["cls"][e & (T["ncol"] >= 16) & (T["nl"] >= 3)] == X_HUGE).all() and (T["cls"][e & (T["ncol"] <= 8) & (T["nl"] >= 3)] == X_16).all()


def test_the_planner_sweeps_no_extension_call_of_fewer_than_three_rows():
    """class X_NONE: in no wave descriptor, in no huge list, behind no unit -- whatever class the call's columns and the options would
    have given it; the plan without those calls has the same descriptors and units"""
    cs = dpedges.case("tiny")
    te = cs.tiny_ext()
    keep = np.ones(len(cs.tasks), dtype=bool)
    keep[te] = False
    for over, knobs in (({}, {}), ({}, dict(lite_min=3, lite_wide=1)), (dict(ge=300), {}), (dict(go=31000, ge=100), {}), ({}, dict(pool=1)), ({}, dict(no_split=1)),
                        ({}, dict(tb_budget=1 << 20)), ({}, dict(ext_dual=0))):
        P = host_plan(cs, over, knobs)
        T = P.sec["tasks"]
        is_ext = (T["flag"] & EXT) != 0
        assert (T["cls"][te] == X_NONE).all() and (T["cls"][keep & is_ext] != X_NONE).all()
        in_waves = set(int(i) for w in P.sec["ewaves"] for i in w["task"] if i >= 0) | set(int(i) for i in P.sec["huge_list"])
        assert not in_waves & set(te)
        ext = np.nonzero(((T["flag"] & EXT) != 0) & keep)[0]
        assert set(int(i) for i in ext) <= in_waves, "every other extension call is swept"
        Q = dpplan.plan(cs.tasks[keep], over, knobs, ctg_len=cs.ctg_len(), qoff=cs.q_off())
        for k in ("n_units", "n_ewaves", "n_huge", "n_split", "n_glob", "st_cells_ext", "st_cells_glob"):
            assert P.header[k] == Q.header[k], (k, over, knobs)
        assert P.header["n_ext"] == Q.header["n_ext"] + len(te)
        assert (P.sec["units"]["kind"] == Q.sec["units"]["kind"]).all() and (P.sec["units"]["count"] == Q.sec["units"]["count"]).all()


def test_the_device_planner_routes_them_the_same_way():
    """the model of the device planner (its stages with a team of one) on a table with such calls: the host planner's plan, byte for
    byte -- among them calls of 1 100 columns, which with three rows or more are of the class the device planner declines"""
    tasks, over, knobs = dd.planned()["tiny_ext"]
    want = dpplan.plan(tasks, over, knobs)
    T = want.sec["tasks"]
    tiny = ((T["flag"] & EXT) != 0) & (T["nl"] < 3)
    assert tiny.sum() >= 24 and (T["cls"][tiny] == X_NONE).all() and (T["ncol"][tiny] > 1024).any() and want.header["n_huge"] == 0
    dd.assert_same_plan(dd.device_plan(None, tasks, over, knobs), want)
