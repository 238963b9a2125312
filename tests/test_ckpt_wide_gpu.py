"""The checkpointed traceback for calls of 129..256 columns (class 12: a four-wave packed sweep per pair of calls, k_lite_wide, and the
walk over up to four 64-column blocks; dp_device.h, MPA_DP_LITE_WIDE): (nt_len, aa_len, score, CIGAR) of every call against the oracle
and, where it is built, against the reference's ns_global_gs16b; and the routing, through the statistics n_ckpt_wide (129..256 columns)
and n_ckpt (up to 128 columns).  Thresholds and the knob are read when a context is created: every context here is a fresh one."""
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


def _may_saturate(P, al):
    ncol = (al + 7) // 8 * 8
    return al * int(P.mat.max()) + ncol * P.ge + max(0, P.end_bonus) > 32000 or P.go + ncol * P.ge > 32000


def _packed(P, nl, al, lite_min):
    """the predicate every checkpointed class shares (a restatement of dp_plan.cpp's routing)"""
    return lite_min > 0 and P.ge <= 255 and P.fs <= 255 and not _may_saturate(P, al) and nl >= max(lite_min, 3)


def _ncol(al):
    return (al + 7) // 8 * 8


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

    def expected_counts(self, lite_min, wide_on=True):
        n_wide = sum(wide_on and 128 < _ncol(len(aa)) <= 256 and _packed(self.P, len(nt), len(aa), lite_min) for nt, aa in self.pairs)
        n_narrow = sum(_ncol(len(aa)) <= 128 and _packed(self.P, len(nt), len(aa), lite_min) for nt, aa in self.pairs)
        return n_wide, n_narrow

    def run(self, monkeypatch, lite_min, wide=1, what=""):
        """on a fresh context with the threshold and the knob set (whatever the knob's default is): parity of every call and both
        counts; returns (results, statistics)"""
        monkeypatch.setenv("MPA_DP_LITE_MIN", str(lite_min))
        monkeypatch.setenv("MPA_DP_LITE_WIDE", str(wide))
        ctx = mpa.Context(0)
        idx = mpa.Index.from_nt4(self.contigs)
        try:
            idx.to_device(ctx)
            rst, cig = mpa.dp_run(ctx, idx, dpopt_from_params(self.P), self.queries, self.tasks)
            st = ctx.dp_stats()
        finally:
            idx.close()
            ctx.close()
        what = "%s lite_min %s wide %s" % (what, lite_min, wide)
        bad, msg = compare(rst, cig, self.ora, self.meta, self.pairs)
        assert not bad, "%s: %d/%d DP calls differ from the oracle\n%s" % (what, len(bad), len(self.tasks), msg)
        if self.ref is not None:
            bad, msg = compare(rst, cig, self.ref, self.meta, self.pairs)
            assert not bad, "%s: %d/%d DP calls differ from the REFERENCE\n%s" % (what, len(bad), len(self.tasks), msg)
        n_wide, n_narrow = self.expected_counts(lite_min, int(wide) != 0)
        assert st["n_ckpt_wide"] == n_wide, "%s: %d calls of 129..256 columns checkpointed, expected %d" % (what, st["n_ckpt_wide"], n_wide)
        assert st["n_ckpt"] == n_narrow, "%s: %d calls of <= 128 columns checkpointed, expected %d" % (what, st["n_ckpt"], n_narrow)
        flat = [(int(r["nt_len"]), int(r["aa_len"]), int(r["score"]), tuple(int(x) for x in cig[r["cigar_off"]: r["cigar_off"] + r["n_cigar"]])) for r in rst]
        return flat, st


P0 = None


def _p0():
    global P0
    if P0 is None:
        P0 = refbind.DpParams(refbind.mapping_matrix(23))
    return P0


def _sixty(rng):
    return [make_task(rng, al=int(rng.integers(129, 257)), max_intron=2500, flank=400, p_fs=0.05, p_indel=0.06, p_n=0.01) for _ in range(60)]


_SHAPES = {}


def _shape_batches():
    """the four group shapes of test 2, built (and evaluated by the oracle) once"""
    if not _SHAPES:
        rng = np.random.default_rng(1201)
        P = _p0()
        _SHAPES["lone"] = Batch(P, [long_window(rng, 200)], 1)
        _SHAPES["three"] = Batch(P, [long_window(rng, al) for al in (200, 137, 256)], 2)
        # one block of rows against many: a window of 100 rows under a 150-residue protein next to a window of >= 1500 rows
        short = (bytes(rng.integers(0, 4, 100).astype(np.uint8)), bytes(AA[i] for i in rng.integers(0, 20, 150)))
        while True:
            tall = make_task(rng, al=200, max_intron=3000, flank=700, p_intron=0.1)
            if len(tall[0]) >= 1500:
                break
        _SHAPES["pair"] = Batch(P, [short, tall], 3)
        _SHAPES["sixty"] = Batch(P, _sixty(rng), 4)
    return _SHAPES


def test_class_edges_and_block_phases(oracle_built, monkeypatch):
    """columns on both sides of 128 and of 256 (8 * ceil(al / 8) decides), every count of live 64-column blocks with and without padded
    lanes, and flanks that put the path's state changes at several phases of the 96-row blocks; threshold 3: every call of at least
    three rows is checkpointed, those of 129..256 columns by the four-wave sweep"""
    rng = np.random.default_rng(1200)
    pairs = []
    for al in (121, 128, 129, 130, 136, 137, 160, 191, 192, 193, 200, 248, 249, 255, 256, 257, 264):
        for flank in (3, 90, 200, 700):
            pairs.append(make_task(rng, al=al, max_intron=int(rng.choice([300, 1500, 5000])), flank=flank, p_intron=0.15))
    b = Batch(_p0(), pairs, 5)
    n_wide, n_narrow = b.expected_counts(3)
    assert n_wide >= 40 and n_narrow >= 4 and n_wide + n_narrow < len(pairs)       # (both sides of both edges are there)
    b.run(monkeypatch, 3, what="class edges")


@pytest.mark.parametrize("lite_min", [3, 100, 384])
@pytest.mark.parametrize("shape", ["lone", "three", "pair", "sixty"])
def test_group_shapes(oracle_built, monkeypatch, shape, lite_min):
    """a lone call (an empty second half), a full group plus a lone call, a pair of very different row counts (the group iterates the
    longer one; at the higher thresholds the short call leaves the class and the tall one is alone), and 60 random calls of 129..256
    columns with frameshifts, indels and N runs -- at three row thresholds"""
    b = _shape_batches()[shape]
    _, st = b.run(monkeypatch, lite_min, what=shape)
    assert st["n_ckpt_wide"] >= 1
    if shape == "pair":
        assert st["n_ckpt_wide"] == (2 if lite_min <= 100 else 1)


def _planted_intron_call(rng, al=200, ilen=30000, flank=200):
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
    """one 200-column call across a planted canonical intron of 30 000 bases, about 320 blocks of 96 rows: the walk follows the intron
    on the extension bits and recomputes the blocks of traceback words only where the path is in another state -- at most half of
    the call's blocks (the path outside the intron spans about 600 rows plus the flanks: a handful of blocks; a walk that
    recomputed every block would not pass)"""
    P = _p0()
    for seed in range(1300, 1310):
        rng = np.random.default_rng(seed)
        pair = _planted_intron_call(rng)
        b = Batch(P, [pair], seed)
        cig = b.ora[0][3]
        long_runs = [c for c in cig if (c & 0xf) in (3, 12, 13) and (c >> 4) > 29000]
        if len(long_runs) == 1:
            break
    else:
        pytest.fail("no seed gave a path with exactly one intron run longer than 29 000 rows")
    _, st = b.run(monkeypatch, 384, what="planted intron")
    assert st["n_ckpt_wide"] == 1
    total_blocks = (len(pair[0]) - 2 + TB_BLOCK - 1) // TB_BLOCK
    assert total_blocks > 300
    assert 0 < st["walk_blocks"] <= total_blocks // 2, (st["walk_blocks"], total_blocks)


def test_other_scoring(oracle_built, monkeypatch):
    """gap extension 2, intron open 40, frameshift 17, the mammalian splice model: the bits follow the penalties"""
    P2 = refbind.DpParams(refbind.mapping_matrix(17), go=5, ge=2, io=40, fs=17, xdrop=50, end_bonus=0, sp=(8, 15, 21, 30, 4, 4), ie_coef=1.0)
    rng = np.random.default_rng(1400)
    pairs = [make_task(rng, al=int(rng.integers(129, 257)), max_intron=3000, flank=300) for _ in range(40)]
    b = Batch(P2, pairs, 6)
    _, st = b.run(monkeypatch, 200, what="P2")
    assert st["n_ckpt_wide"] >= 30


@pytest.mark.parametrize("over", [0, 1], ids=["at32000", "at32001"])
@pytest.mark.parametrize("case", [c for c in BOUND_CASES if c[0] in (136, 256)], ids=lambda c: "al%d-%s" % (c[0], c[2]))
def test_int16_bound(oracle_built, monkeypatch, case, over):
    """a long-window call whose decisive sum of may_saturate is exactly 32 000 takes the packed four-wave sweep; at 32 001 it stays on
    the int32 sweep -- next to calls 8 columns narrower and wider, parity on both sides"""
    al = case[0]
    P = _params(bound_params(case, over))
    assert _may_saturate(P, al) == (over == 1)
    rng = np.random.default_rng(1500 + al + over)
    pairs = []
    for a in (al, al - 8, al + 8):
        pairs.append(long_window(rng, a, p_indel=0.0))
        pairs.append(make_task(rng, al=a, p_intron=0.01, max_intron=300, flank=200, p_indel=0.0))
    b = Batch(P, pairs, 7)
    assert len(pairs[0][1]) == al and len(pairs[0][0]) >= 384
    _, st = b.run(monkeypatch, 384, what="bound al %d over %d" % (al, over))
    at_bound = 128 < _ncol(al) <= 256 and _packed(P, len(pairs[0][0]), al, 384)
    assert at_bound == (over == 0)
    if over == 0:
        assert st["n_ckpt_wide"] >= 1


def test_wide_gap_extension_keeps_the_plain_sweep(oracle_built, monkeypatch):
    """ge = 300 does not fit the row records' byte: no call is checkpointed, whatever its width"""
    P = _params(dict(ge=300))
    rng = np.random.default_rng(1600)
    pairs = [long_window(rng, al) for al in (136, 200, 256)] + [make_task(rng, al=180, flank=50)]
    b = Batch(P, pairs, 8)
    _, st = b.run(monkeypatch, 3, what="ge 300")
    assert st["n_ckpt_wide"] == 0 and st["n_ckpt"] == 0


def test_knob_off_keeps_the_plain_sweep(oracle_built, monkeypatch):
    """MPA_DP_LITE_WIDE=0 on a fresh context: the 60 calls of 129..256 columns keep the plain sweep and give the same results"""
    b = _shape_batches()["sixty"]
    on, st_on = b.run(monkeypatch, 100, wide=1, what="knob on")
    off, st_off = b.run(monkeypatch, 100, wide=0, what="knob off")
    assert st_off["n_ckpt_wide"] == 0 and st_on["n_ckpt_wide"] > 0
    assert on == off
    assert st_on["n_glob"] == st_off["n_glob"] and st_on["cells_glob"] == st_off["cells_glob"]


@pytest.mark.parametrize("wide", ["1", "0"])
def test_whole_path_golden_case(monkeypatch, wide):
    """golden case syn_e (tests/golden.py; -u --gff): its mapping issues one traceback call of 131 residues across 11 404 rows, the only
    committed case with a call of 129..256 columns.  mpa_map_batch with the row threshold at 3 prints the bytes of
    tests/golden/syn_e.ref.paf with the class on and off, and with it on the call is counted"""
    import golden
    from hostpipe import map_batch_gpu
    monkeypatch.setenv("MPA_DP_LITE_MIN", "3")
    monkeypatch.setenv("MPA_DP_LITE_WIDE", wide)
    case = [c for c in golden.SYNTH_CASES if c["name"] == "syn_e"][0]
    contigs, prots, names = golden.synth_inputs(case)
    ctx = mpa.Context(0)
    idx = mpa.Index.from_nt4(contigs, ["chr%d" % (i + 1) for i in range(len(contigs))])
    try:
        mpa._check(mpa.lib().mpa_idx_build_kmers(idx.h, 4))
        idx.to_device(ctx)
        out = golden.file_header(case) + map_batch_gpu(ctx, idx, golden.mapopt_for(case), mpa.Queries(prots, names), 4)
        st = ctx.dp_stats(total=True)
    finally:
        idx.close()
        ctx.close()
    assert out == open(golden.path("syn_e.ref.paf"), "rb").read()
    assert (st["n_ckpt_wide"] > 0) == (wide == "1"), st
