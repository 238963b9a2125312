"""The checkpointed traceback for calls of 257..512 columns (class 13, T_LITE_W8: an eight-wave packed sweep per pair of calls, k_lite_w8,
and the walk k_walk_w8 over up to eight 64-column blocks; dp_device.h, MPA_DP_LITE_W8): (nt_len, aa_len, score, CIGAR) of every call
against the oracle and, where it is built, against the reference's ns_global_gs16b; and the routing, through mpa_dbg_dp_last_w8 (calls
and padded cells of the class, groups swept, blocks the walk recomputed).  Thresholds and the knob are read when a context is created:
every context here is a fresh one.  MPA_DP_LITE_WIDE stays 0 throughout: the two knobs are independent."""
from concurrent.futures import ThreadPoolExecutor
import numpy as np
import pytest
import miniprot_amd as mpa
import refbind
from dpgen import make_task, long_window, back_translate, AA, BOUND_CASES, bound_params
from dputil import build_workload, dpopt_from_params, compare

pytestmark = pytest.mark.gpu

TB_BLOCK = 96


def _params(kw):
    return refbind.DpParams(refbind.mapping_matrix(min(kw.get("fs", 23), 127)), **kw)


def _ncol(al):
    return (al + 7) // 8 * 8


def _may_saturate(P, al):
    return al * int(P.mat.max()) + _ncol(al) * P.ge + max(0, P.end_bonus) > 32000 or P.go + _ncol(al) * P.ge > 32000


def _takes(P, nl, al, lite_min):
    """does a traceback call take class 13 with the knob set (a restatement of dp_classify_call's routing)"""
    return 256 < _ncol(al) <= 512 and lite_min > 0 and P.ge <= 255 and P.fs <= 255 and not _may_saturate(P, al) and nl >= max(lite_min, 3)


def _expect(fn, P, pairs, meta):
    refbind.ora(), refbind.have_ref() and refbind.ref()                # (load the libraries before the threads do)

    def one(m):
        k, fl, io = m
        PP = refbind.DpParams(P.mat, go=P.go, ge=P.ge, io=io, fs=P.fs, xdrop=P.xdrop, end_bonus=P.end_bonus, sp=P.sp,
                              sp_null_bonus=P.sp_null_bonus, ie_coef=P.ie_coef)
        return fn(pairs[k][0], pairs[k][1], PP, fl)
    with ThreadPoolExecutor(max_workers=8) as ex:
        return list(ex.map(one, meta))


class Batch:
    """one batch of traceback calls laid out once, with the oracle's (and the reference's) results computed once"""

    def __init__(self, P, pairs, seed):
        self.P, self.pairs = P, pairs
        rng = np.random.default_rng(seed)
        self.contigs, self.queries, self.tasks, self.meta = build_workload(pairs, rng, modes=("cigar",), io=P.io)
        self.ora = _expect(refbind.ora_nasw, P, pairs, self.meta)
        self.ref = _expect(refbind.ref_nasw, P, pairs, self.meta) if refbind.have_ref() else None

    def expected(self, lite_min, w8=1):
        """(calls, padded cells, groups) of the class"""
        mine = [(len(nt), len(aa)) for nt, aa in self.pairs if int(w8) != 0 and _takes(self.P, len(nt), len(aa), lite_min)]
        return len(mine), sum((nl - 2) * _ncol(al) for nl, al in mine), (len(mine) + 1) // 2

    def run(self, monkeypatch, lite_min, w8=1, what=""):
        """on a fresh context with the threshold and the knob set: parity of every call, and the hook's counts; returns (results,
        statistics, hook)"""
        monkeypatch.setenv("MPA_DP_LITE_MIN", str(lite_min))
        monkeypatch.setenv("MPA_DP_LITE_WIDE", "0")
        monkeypatch.setenv("MPA_DP_LITE_W8", str(w8))
        ctx = mpa.Context(0)
        idx = mpa.Index.from_nt4(self.contigs)
        try:
            idx.to_device(ctx)
            rst, cig = mpa.dp_run(ctx, idx, dpopt_from_params(self.P), self.queries, self.tasks)
            st = ctx.dp_stats()
            hook = mpa.dbg_dp_last_w8(ctx)
        finally:
            idx.close()
            ctx.close()
        what = "%s lite_min %s w8 %s" % (what, lite_min, w8)
        bad, msg = compare(rst, cig, self.ora, self.meta, self.pairs)
        assert not bad, "%s: %d/%d DP calls differ from the oracle\n%s" % (what, len(bad), len(self.tasks), msg)
        if self.ref is not None:
            bad, msg = compare(rst, cig, self.ref, self.meta, self.pairs)
            assert not bad, "%s: %d/%d DP calls differ from the REFERENCE\n%s" % (what, len(bad), len(self.tasks), msg)
        assert hook[:3] == self.expected(lite_min, w8), "%s: (calls, cells, groups) of class 13 %s, expected %s" % (what, hook[:3], self.expected(lite_min, w8))
        assert st["n_ckpt_wide"] == hook[0], (what, st["n_ckpt_wide"], hook)       # (MPA_DP_LITE_WIDE=0: the statistic counts class 13 alone)
        if hook[0] == 0:
            assert hook[3] == 0
        flat = [(int(r["nt_len"]), int(r["aa_len"]), int(r["score"]), tuple(int(x) for x in cig[r["cigar_off"]: r["cigar_off"] + r["n_cigar"]])) for r in rst]
        return flat, st, hook


P0 = None


def _p0():
    global P0
    if P0 is None:
        P0 = refbind.DpParams(refbind.mapping_matrix(23))
    return P0


def _forty(rng):
    return [make_task(rng, al=int(rng.integers(257, 513)), max_intron=1500, flank=300, p_fs=0.05, p_indel=0.06, p_n=0.01) for _ in range(40)]


_SHAPES = {}


def _shape_batches():
    """the four group shapes, built (and evaluated by the oracle) once"""
    if not _SHAPES:
        rng = np.random.default_rng(1701)
        P = _p0()
        _SHAPES["lone"] = Batch(P, [long_window(rng, 400)], 1)
        _SHAPES["three"] = Batch(P, [long_window(rng, al) for al in (400, 265, 512)], 2)
        # one block of rows against many: a window of 100 rows under a 300-residue protein next to a window of >= 1500 rows
        short = (bytes(rng.integers(0, 4, 100).astype(np.uint8)), bytes(AA[i] for i in rng.integers(0, 20, 300)))
        while True:
            tall = make_task(rng, al=400, max_intron=3000, flank=700, p_intron=0.1)
            if len(tall[0]) >= 1500:
                break
        _SHAPES["pair"] = Batch(P, [short, tall], 3)
        _SHAPES["forty"] = Batch(P, _forty(rng), 4)
    return _SHAPES


def test_class_edges_and_block_phases(oracle_built, monkeypatch):
    """columns on both sides of 256 and of 512 (8 * ceil(al / 8) decides), every count of live 64-column blocks from five to eight with and
    without padded lanes, and flanks that put the path's state changes at several phases of the 96-row blocks; threshold 3: every call
    of 257..512 columns and at least three rows is swept by the eight-wave groups"""
    rng = np.random.default_rng(1700)
    pairs = []
    for al in (249, 256, 257, 264, 313, 320, 321, 384, 385, 448, 449, 505, 512, 513, 520):
        for flank in (3, 90, 200, 700):
            pairs.append(make_task(rng, al=al, max_intron=int(rng.choice([300, 1500, 5000])), flank=flank, p_intron=0.05))
    b = Batch(_p0(), pairs, 5)
    n, _, _ = b.expected(3)
    ncols = [_ncol(len(aa)) for _, aa in pairs]                         # (indels move a protein's length off the one asked for by a few residues)
    assert n >= 36 and sum(c <= 256 for c in ncols) >= 4 and sum(c > 512 for c in ncols) >= 4       # (both sides of both edges are there)
    assert {256, 264, 320, 328, 384, 392, 448, 456, 512, 520} <= set(ncols)
    b.run(monkeypatch, 3, what="class edges")


@pytest.mark.parametrize("lite_min", [3, 100, 384])
@pytest.mark.parametrize("shape", ["lone", "three", "pair", "forty"])
def test_group_shapes(oracle_built, monkeypatch, shape, lite_min):
    """a lone call (an empty second half), a full group plus a lone call, a pair of very different row counts (the group iterates the
    longer one; at the higher thresholds the short call leaves the class and the tall one is alone), and forty random calls of 257..512
    columns with frameshifts, indels and N runs -- at three row thresholds"""
    b = _shape_batches()[shape]
    _, _, hook = b.run(monkeypatch, lite_min, what=shape)
    assert hook[0] >= 1
    if shape == "pair":
        assert hook[0] == (2 if lite_min <= 100 else 1) and hook[2] == 1


SHORT_ROWS = (3, 4, 5, 12, 13, 23, 24, 25, 27)
_SHORT = {}


def _short_calls():
    """two long calls and one call of every short row count, all under a 400-residue protein"""
    if not _SHORT:
        rng = np.random.default_rng(1710)
        _SHORT["long"] = [long_window(rng, 400), long_window(rng, 400)]
        for nl in SHORT_ROWS:
            _SHORT[nl] = (bytes(rng.integers(0, 4, nl).astype(np.uint8)), bytes(AA[i] for i in rng.integers(0, 20, 400)))
    return _SHORT


@pytest.mark.parametrize("nl", SHORT_ROWS)
def test_short_groups(oracle_built, monkeypatch, nl):
    """a call of 3 .. 27 rows (before, at and behind the row at which the last of the eight waves starts -- 23 --, inside and at the end
    of the twelve generic rows) next to one long call: as the second half of the long call's group, and alone in a group of its own
    behind a full group of two long calls.  Every wave of a group passes the same number of barriers whatever the group's rows: a
    mismatch would hang the launch"""
    s = _short_calls()
    b = Batch(_p0(), [s["long"][0], s[nl]], 10 + nl)
    _, _, hook = b.run(monkeypatch, 3, what="short %d paired with a long call" % nl)
    assert hook[0] == 2 and hook[2] == 1
    b = Batch(_p0(), [s["long"][0], s["long"][1], s[nl]], 40 + nl)
    _, _, hook = b.run(monkeypatch, 3, what="short %d alone" % nl)
    assert hook[0] == 3 and hook[2] == 2


def test_short_groups_paired_with_each_other(oracle_built, monkeypatch):
    """the nine short calls behind two long ones: groups (27, 25), (24, 23), (13, 12), (5, 4) and 3 alone"""
    s = _short_calls()
    b = Batch(_p0(), s["long"] + [s[nl] for nl in SHORT_ROWS], 70)
    _, _, hook = b.run(monkeypatch, 3, what="short calls paired")
    assert hook[0] == 11 and hook[2] == 6


def _planted_intron_call(rng, al=400, ilen=30000, flank=200):
    prot = bytes(AA[i] for i in rng.integers(0, 20, al))
    half = al // 2
    body = list(rng.integers(0, 4, ilen))
    body[0:2] = [2, 3]                                                 # GT[AG] ... [CT]AG: the canonical signal, phase 0
    body[2] = int(rng.choice([0, 2]))
    body[-2:] = [0, 2]
    body[-3] = int(rng.choice([1, 3]))
    nt = list(rng.integers(0, 4, flank)) + list(back_translate(prot[:half], rng)) + body + list(back_translate(prot[half:], rng)) + list(rng.integers(0, 4, flank))
    q = bytearray(prot)
    for k in rng.integers(0, al, 10):
        q[int(k)] = AA[int(rng.integers(0, 20))]
    return bytes(np.array(nt, dtype=np.uint8)), bytes(q)


def test_runs_across_blocks(oracle_built, monkeypatch):
    """one 400-residue call across a planted canonical intron of 30 000 bases, about 330 blocks of 96 rows: the walk follows the intron on
    the extension bits and recomputes the blocks of traceback words only where the path is in another state -- at most half of the
    call's blocks (the path outside the intron spans about 1 200 rows plus the flanks: some twenty blocks; a walk that recomputed
    every block would not pass)"""
    P = _p0()
    for seed in range(1800, 1810):
        rng = np.random.default_rng(seed)
        pair = _planted_intron_call(rng)
        b = Batch(P, [pair], seed)
        cig = b.ora[0][3]
        long_runs = [c for c in cig if (c & 0xf) in (3, 12, 13) and (c >> 4) > 29000]
        if len(long_runs) == 1:
            break
    else:
        pytest.fail("no seed gave a path with exactly one intron run longer than 29 000 rows")
    _, st, hook = b.run(monkeypatch, 384, what="planted intron")
    assert hook[0] == 1 and hook[2] == 1
    total_blocks = (len(pair[0]) - 2 + TB_BLOCK - 1) // TB_BLOCK
    assert total_blocks > 300
    assert 0 < hook[3] <= total_blocks // 2, (hook, total_blocks)
    assert st["walk_blocks"] == hook[3]


def test_other_scoring(oracle_built, monkeypatch):
    """gap extension 2, intron open 40, frameshift 17, the mammalian splice model: the bits follow the penalties"""
    P2 = refbind.DpParams(refbind.mapping_matrix(17), go=5, ge=2, io=40, fs=17, xdrop=50, end_bonus=0, sp=(8, 15, 21, 30, 4, 4), ie_coef=1.0)
    rng = np.random.default_rng(1900)
    pairs = [make_task(rng, al=int(rng.integers(257, 513)), max_intron=2000, flank=300) for _ in range(24)]
    b = Batch(P2, pairs, 6)
    _, _, hook = b.run(monkeypatch, 200, what="P2")
    assert hook[0] >= 20


@pytest.mark.parametrize("over", [0, 1], ids=["at32000", "at32001"])
def test_int16_bound(oracle_built, monkeypatch, over):
    """BOUND_CASES' 512-column entry: a long-window call whose decisive sum of may_saturate is exactly 32 000 takes the packed eight-wave
    sweep; at 32 001 it stays on the int32 sweep -- next to calls 8 columns narrower and wider, parity on both sides"""
    case = [c for c in BOUND_CASES if c[0] == 512][0]
    al = case[0]
    P = _params(bound_params(case, over))
    assert _may_saturate(P, al) == (over == 1)
    rng = np.random.default_rng(2000 + over)
    pairs = []
    for a in (al, al - 8, al + 8):
        pairs.append(long_window(rng, a, p_indel=0.0))
        pairs.append(make_task(rng, al=a, p_intron=0.01, max_intron=300, flank=200, p_indel=0.0))
    b = Batch(P, pairs, 7)
    assert len(pairs[0][1]) == al and len(pairs[0][0]) >= 384
    assert _takes(P, len(pairs[0][0]), al, 384) == (over == 0)
    _, _, hook = b.run(monkeypatch, 384, what="bound al %d over %d" % (al, over))
    assert hook[0] == (4 if over == 0 else 2)


def test_wide_gap_extension_keeps_the_plain_sweep(oracle_built, monkeypatch):
    """ge = 300 does not fit the row records' byte: no call is checkpointed, whatever its width"""
    P = _params(dict(ge=300))
    rng = np.random.default_rng(2100)
    pairs = [long_window(rng, al) for al in (264, 400, 512)] + [make_task(rng, al=300, flank=50)]
    b = Batch(P, pairs, 8)
    _, st, hook = b.run(monkeypatch, 3, what="ge 300")
    assert hook == (0, 0, 0, 0) and st["n_ckpt"] == 0


def test_knob_off_keeps_the_plain_sweep(oracle_built, monkeypatch):
    """MPA_DP_LITE_W8=0 on a fresh context: the forty calls of 257..512 columns keep the plain sweep and give the same results"""
    b = _shape_batches()["forty"]
    on, st_on, hook_on = b.run(monkeypatch, 100, w8=1, what="knob on")
    off, st_off, hook_off = b.run(monkeypatch, 100, w8=0, what="knob off")
    assert hook_off == (0, 0, 0, 0) and hook_on[0] > 0 and hook_on[2] > 0
    assert on == off
    assert st_on["n_glob"] == st_off["n_glob"] and st_on["cells_glob"] == st_off["cells_glob"]


# ---- the whole path
EVERY_KNOB = dict(MPA_GPU_SPANS="1", MPA_GPU_ROUND1="1", MPA_GPU_ROUND2="1", MPA_GPU_DPPLAN="1", MPA_GPU_PLANS="1", MPA_GPU_REGIONS="1", MPA_GPU_STATS="1", MPA_GPU_CS="1",
                  MPA_GPU_ROWS="1", MPA_GPU_SKETCH="1", MPA_GPU_SEED="1", MPA_GPU_REFINE="1", MPA_GPU_FINISH="1", MPA_GPU_FORMAT="1")
DECLINE_WHY = "a call of the eight-wave checkpointed traceback class"


@pytest.mark.parametrize("mode", ["on", "off", "every-knob"])
def test_whole_path_case(monkeypatch, capfd, mode):
    """w8cases.CASE: a mapping that issues a traceback call of 257..512 columns.  mpa_map_batch with the row threshold at 3 prints the bytes of
    the committed reference output with the class on and off; with it on the calls are counted; with every device knob set as well a
    round that holds such a call is declined by the device planner -- with the note that says why -- and runs through mpa_dp_run: the
    same bytes"""
    import w8cases
    from hostpipe import map_batch_gpu
    for k in EVERY_KNOB:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("MPA_DP_LITE_MIN", "3")
    monkeypatch.setenv("MPA_DP_LITE_WIDE", "0")
    monkeypatch.setenv("MPA_DP_LITE_W8", "0" if mode == "off" else "1")
    monkeypatch.setenv("MPA_TIMING", "1")
    if mode == "every-knob":
        for k, v in EVERY_KNOB.items():
            monkeypatch.setenv(k, v)
    ctx = mpa.Context(0)
    idx, mo, q, head, ref = w8cases.inputs()
    try:
        idx.to_device(ctx)
        capfd.readouterr()
        out = head + map_batch_gpu(ctx, idx, mo, q, 4)
        err = capfd.readouterr().err
        st = ctx.dp_stats(total=True)
    finally:
        idx.close()
        ctx.close()
    assert out == ref
    assert (st["n_ckpt_wide"] > 0) == (mode != "off"), st                # (MPA_DP_LITE_WIDE=0: class 13's calls alone)
    if mode == "every-knob":
        notes = [l for l in err.split("\n") if DECLINE_WHY in l]
        assert notes and all("declined (" in l for l in notes), [l for l in err.split("\n") if "declined" in l][:8]
        assert any("resident declined (" in l and l.endswith("): mpa_dp_run") for l in notes), notes[:8]
    else:
        assert DECLINE_WHY not in err
