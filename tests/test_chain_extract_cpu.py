"""The chain extraction on synthetic anchors, without a device: every case of tests/chaincases.py through mpa_dbg_chain_extract with no
context -- the host forward pass, the views a device route would build, and chain_extract_core with a team of one in work space of the
kernel's sizes -- against the oracle's mp_chain.  This validates the cases (tests/test_chain_extract_gpu.py runs the same ones through
k_chain_extract) and asserts, from the hook's path records, that they reach the branches they are built for: the GPU file cannot pass
by missing its targets."""
import ctypes as C
import numpy as np
import pytest
import miniprot_amd as mpa
import chaincases as cc

SPARSE = (cc.SPARSE_SET, cc.SPARSE_CHAINS)
_runs = {}


def host_run(c, args, mode):
    key = (c["name"], tuple(args), mode)
    if key not in _runs:
        _runs[key] = mpa.dbg_chain_extract(None, list(args), c["probs"], mode)
    return _runs[key]


def all_records(mode):
    """{(case, problem): [records]} over every run of the file in that mode"""
    out = {}
    for c in cc.cases():
        for args, modes in c["runs"]:
            if mode in modes:
                rec = host_run(c, args, mode)[3]
                for q in range(len(rec)):
                    out.setdefault((c["name"], q), []).append((rec[q], args))
    return out


@pytest.mark.parametrize("name", [c["name"] for c in cc.cases()])
def test_host_extraction_equals_the_oracle(name, oracle_built):
    c = cc.case(name)
    for args, modes in c["runs"]:
        want = cc.expected(c, args)
        for mode in modes:
            n = cc.check_against(c, args, mode, host_run(c, args, mode), want, "host")
            assert n >= len(c["probs"]) - 8                       # (what a run declines is not counted: a few problems of (h) and (i))


def test_every_case_is_one_mixed_launch():
    for c in cc.cases():
        sizes = [len(p) for p in c["probs"]]
        assert 0 in sizes and len(set(sizes)) >= 5, c["name"]
        assert 1 in sizes or c["name"] == "i_min_cnt_sparse", c["name"]
        assert all(np.all(p[1:] > p[:-1]) for p in c["probs"]), c["name"]          # sorted, distinct


@pytest.mark.parametrize("mode", SPARSE)
def test_sparse_runs_reach_every_path(mode, oracle_built):
    recs = all_records(mode)
    cls = lambda k: {key for key, rs in recs.items() for r, _ in rs if r[4] == k}
    one, two, full, declined = cls(mpa.CHAIN_ONE_LEVEL), cls(mpa.CHAIN_TWO_LEVEL), cls(mpa.CHAIN_FULL_LIST), cls(mpa.CHAIN_DECLINED)
    two_recs = [r for rs in recs.values() for r, _ in rs if r[4] == mpa.CHAIN_TWO_LEVEL]
    assert len(one) >= 40 and len(two) >= 40 and len(full) >= 30, (len(one), len(two), len(full))
    pick = lambda f: len({key for key, rs in recs.items() for r, _ in rs if r[4] == mpa.CHAIN_TWO_LEVEL and f(r)})
    assert pick(lambda r: r[5] <= 64) >= 8 and pick(lambda r: 0 < r[6] <= 256) >= 8 and pick(lambda r: r[6] > 256) >= 8
    assert all(r[1] > 64 and 256 <= r[3] < 65536 and r[7] == 0 for r in two_recs)
    assert set(cc.BUCKETS) <= {int(r[6]) for r in two_recs}
    assert {63, 64, 65, 66} <= {int(r[5]) for r in two_recs}
    why = lambda bit: len({key for key, rs in recs.items() for r, _ in rs if r[4] == mpa.CHAIN_FULL_LIST and r[7] & bit})
    assert why(mpa.CHAIN_WHY_MAX_F) >= 2
    assert why(mpa.CHAIN_WHY_MIN_CNT) >= 5 and why(mpa.CHAIN_WHY_MIN_SC) >= 5 and why(mpa.CHAIN_WHY_SMALL) >= 5
    assert len(declined) >= 6 and 20 * len(declined) <= len(recs), (len(declined), len(recs))
    by_why = {int(r[7]) for rs in recs.values() for r, _ in rs if r[4] == mpa.CHAIN_DECLINED}
    assert {mpa.CHAIN_WHY_MAX_F, mpa.CHAIN_WHY_MIN_CNT, mpa.CHAIN_WHY_MIN_SC} <= by_why                  # (h) and both of (i)
    # every n_total of (a) and every number of chain ends of (b) -- the latter on the replayed path, among at least 200 lone roots
    assert set(cc.N_TOTALS) <= {int(r[1]) for rs in recs.values() for r, _ in rs}
    assert set(cc.N_ENDS) <= {int(r[2]) for rs in recs.values() for r, _ in rs if r[4] == mpa.CHAIN_ONE_LEVEL and r[1] >= r[0] + 200}


def test_dense_runs_cover_the_parameters_and_the_refinement():
    seen, refine = set(), set()
    for c in cc.cases():
        for args, modes in c["runs"]:
            if cc.DENSE in modes:
                seen.add((args[5], args[6]))
                if args[10] == 0:
                    refine |= {len(p) for p, t in zip(c["probs"], c["tags"]) if t and t[0] == "refine"}
                rec = host_run(c, args, cc.DENSE)[3]
                assert np.all(rec[:, 0] == rec[:, 1]) and not np.any(rec[:, 4] == mpa.CHAIN_DECLINED)
    assert {(c, s) for c in (1, 2, 3, 4) for s in (0, 6, 7, 20)} <= seen
    assert len(refine) >= 5 and min(refine) <= 5 and max(refine) >= 500


def _forward(args, a):
    L = mpa.lib()
    L.mpa_dbg_chain_forward.argtypes = [C.c_void_p] + [C.c_int32] * 5 + [C.c_float] + [C.c_int32] * 4 + [C.c_void_p] * 4
    first = np.array([0, len(a)], np.int64)
    f, pred = np.zeros(len(a) + 1, np.int32), np.zeros(len(a) + 1, np.int32)
    fwd = list(args[:5]) + list(args[7:])
    assert L.mpa_dbg_chain_forward(None, *fwd, 1, first.ctypes.data, a.ctypes.data, f.ctypes.data, pred.ctypes.data) == 0
    return f[:len(a)], pred[:len(a)]


def test_family_c_puts_the_intended_ends_into_one_tree():
    """the lanes of one group of the extraction loop contend for owner[root] only if their ends share a predecessor tree: the host
    forward pass (which tests/test_host_core.py pins to the oracle) must link the planted trees as chaincases.trunk_tree says"""
    c = cc.case("c_trees")
    for args, _ in c["runs"]:
        largest, lone64 = set(), False
        for p, t in zip(c["probs"], c["tags"]):
            if not t:
                continue
            f, pred = _forward(args, p)
            root = np.arange(len(p))
            for i in range(len(p)):                               # (pred[i] < i: one pass)
                if pred[i] >= 0:
                    root[i] = root[pred[i]]
            ends = np.bincount(root[pred >= 0], minlength=len(p))
            if t[0] == "tree":
                assert np.any(ends == t[1]) and ends.max() in (t[1], 17), (t, int(ends.max()))    # (17: the twin fragment next to it)
                sc = np.sort(f[(pred >= 0) & (root == int(np.flatnonzero(ends == t[1])[0]))])
                assert np.all(np.diff(sc) <= 8)                    # near-equal scores: the tree's ends are neighbours in the sorted list
                largest.add(t[1])
            else:
                lone64 = int((pred >= 0).sum()) == 64 and ends.max() == 1
        assert largest == set(cc.TREE_ENDS) and lone64


def test_family_e_has_lows_for_the_team_merge_to_move(oracle_built):
    """the merge of the moved and the low list only has work when high chain ends found in region 0 (positions below c0) displace
    CHAINED low-score anchors from behind c0: both kinds must be there in numbers, in the sparse and in the dense view"""
    c = cc.case("e_moved_lows")
    for args, modes in c["runs"]:
        rec = host_run(c, args, modes[0])[3]
        n = 0
        for q, (p, t) in enumerate(zip(c["probs"], c["tags"])):
            if not t:
                continue
            f, pred = _forward(args, p)
            c0 = int(rec[q][5])
            pos = np.arange(len(p))
            assert rec[q][4] == mpa.CHAIN_TWO_LEVEL and c0 > 64
            assert int(((pos < c0) & (pred >= 0) & (f >= 256)).sum()) >= 60 and int(((pos >= c0) & (pred >= 0) & (f < 256)).sum()) >= 30, (q, c0)
            n += 1
        assert n == 8


def test_family_j_breaks_the_walk_back_at_max_drop(oracle_built):
    """without splicing max_drop = bw: the planted chain is ONE path through every one of its anchors, and the best chain end walks back
    only as far as the expensive links -- the oracle's best chain is shorter than the path; with splicing it takes all of it"""
    c = cc.case("j_max_drop")
    (unspliced, _), (spliced, _) = c["runs"][0], c["runs"][1]
    assert unspliced[8] == 0 and spliced[8] == 1 and unspliced[2] == 300
    n = 0
    for q, (p, t) in enumerate(zip(c["probs"], c["tags"])):
        if not t:
            continue
        f, pred = _forward(unspliced, p)
        end = int(f.argmax())
        depth, i = 0, end
        while i >= 0:
            depth, i = depth + 1, pred[i]
        best = lambda args: int(max(cc.expected(c, args)[q][0]) & np.uint64(0xffffffff))
        assert depth > 70 and best(unspliced) < depth - 40, (q, depth, best(unspliced))
        f1, pred1 = _forward(spliced, p)
        depth1, i = 0, int(f1.argmax())
        while i >= 0:
            depth1, i = depth1 + 1, pred1[i]
        assert best(spliced) == depth1 > 70
        n += 1
    assert n == 3


def test_family_h_declines_only_what_does_not_fit(oracle_built):
    c = cc.case("h_max_f")
    for args, modes in c["runs"]:
        for mode in modes:
            us, as_, status, rec = host_run(c, args, mode)
            for q, t in enumerate(c["tags"]):
                if t and t[0] == "max_f":
                    assert rec[q][3] >= 65536 and 8500 <= len(c["probs"][q]) <= 9300
                    declined = mode != cc.DENSE and t[1] == "declined"
                    assert status[q] == (1 if declined else 0) and (len(as_[q]) == 0) == declined, (q, t, mode)
                    assert rec[q][4] == (mpa.CHAIN_DECLINED if declined else mpa.CHAIN_FULL_LIST)
                    if declined:
                        assert rec[q][1] - rec[q][0] >= 70
                else:
                    assert status[q] == 0
