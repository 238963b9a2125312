"""Device seeding where map.c:186 runs no pre-chain (-S, --no-pre-chain) -- the direct route, MPA_GPU_SEED_NOPRE=1: k_seed_sift<4096, true>
keeps by the reach of the MAIN chain, k_chain_fwd / k_chain_fwd_wave chain the kept anchors, k_chain_extract reads them as a sparse
view.  Every comparison is exact: the device's kept anchors against the keep rule in numpy (tests/seednopre.py; the library's host
restatement is pinned to it by tests/test_seed_nopre_cpu.py), its main chains against the reference's own mp_chain() over ALL raw
anchors, the whole path against the reference's output.  The figures in POINTS were taken from the host stages."""
import os
import numpy as np
import pytest
import miniprot_amd as mpa
import golden
import gen_synth
import refbind
import seedopts
from hostpipe import map_batch_gpu
from seednopre import SIFT_REACH_MAX, sift_kept, rule_keeps, reach_of
from test_seed_gpu import main_chains, raw_anchors
from test_seed_options_gpu import _Tandem

pytestmark = pytest.mark.gpu
NCPU = min(16, os.cpu_count() or 4)
SEED_NOTE = "seeding on the GPU"

# grouped by index point (one index at a time is resident): (index point, flags, reach D, anchors, anchors the rule keeps (None: all of them -- D is beyond what the sift filters by), main chains)
POINTS = [
    ((8, 30, 6, 1), ["-S"], 3, 16403, 7414, 161),
    ((8, 30, 6, 1), ["--no-pre-chain", "-G", "2000"], 7, 16403, 8058, 133),
    ((8, 30, 6, 1), ["--no-pre-chain"], 781, 16403, None, 82),
    ((6, 20, 5, 0), ["-S"], 15, 275996, 232066, 3713),
    ((6, 20, 5, 0), ["--no-pre-chain", "-G", "2000"], 31, 275996, None, 7437),
    ((12, 30, 6, 1), ["-S"], 0, 16388, 8105, 212),
    ((10, 40, 7, 4), ["--no-pre-chain", "-G", "2000"], 1, 748, 647, 63),
    ((4, 10, 4, 0), ["-S"], 62, 4138238, None, 228930),
]
GRID = [(p, seg) for p in POINTS for seg in (None, "300")]


def _pid(g):
    (ip, flags, D, _, _, _), seg = g
    return "%s%s-D%d%s" % (seedopts.index_name(ip), "".join(flags), D, "-seg" + seg if seg else "")


@pytest.fixture(scope="module")
def ctx():
    c = mpa.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def tandem(tmp_path_factory):
    t = _Tandem(tmp_path_factory.mktemp("tandem_nopre"))
    yield t
    t.close()


@pytest.fixture(autouse=True)
def knobs(monkeypatch):
    monkeypatch.setenv("MPA_GPU_SEED", "1")
    monkeypatch.setenv("MPA_GPU_SEED_NOPRE", "1")


_REFERENCE = {}


def _reference(idx, q, ip, flags, mo):
    """per point, once (the run with small segments shares it): the raw anchors of every query, what the rule keeps of them, and the
    reference's main chains over ALL of them"""
    key = (ip, tuple(flags))
    if key not in _REFERENCE:
        bbit, _, kmer, _ = ip
        a_off, a = raw_anchors(idx, mo, q, NCPU)
        D = reach_of(mo, bbit)
        per = []
        for i in range(len(q.seqs)):
            ai = a[a_off[i]:a_off[i + 1]]
            u, ca = refbind.ref_chain(ai, seedopts.chain_args(mo, kmer, bbit, False))
            per.append((rule_keeps(ai, D), u, ca))
        _REFERENCE.clear()                                     # (one point at a time: the -k4 point holds 4 M anchors)
        _REFERENCE[key] = (int(a_off[-1]), D, per)
    return _REFERENCE[key]


@pytest.mark.skipif(not refbind.have_ref(), reason="oracle/_ref/libminiprot_ref.so not built")
@pytest.mark.parametrize("point,seg", GRID, ids=[_pid(g) for g in GRID])
def test_direct_route_sift_and_main_chains(tandem, ctx, point, seg, monkeypatch):
    """The sift with a reach and the main chain behind it, at D = 0, 1, 3, 7, 15 (filtered: carries of D blocks, probes D blocks to
    either side of a segment, ranges narrower than D) and D = 31, 62, 781 (every anchor kept), whole queries and segments of 300
    anchors.  No block of these inputs holds more than 324 anchors and no D + 1 consecutive blocks more than 736 -- within the carry
    of 1 024 and the buffer of 4 096 -- so the sift may hand no query back; the extraction may hand back fewer than a quarter."""
    ip, flags, D, n_anchor, n_keep, n_chain = point
    if seg:
        monkeypatch.setenv("MPA_SIFT_SEG", seg)
    idx, q = tandem.index(ip, ctx), tandem.q
    mo = golden.apply_flags(mpa.default_mapopt(), flags)
    total, reach, per = _reference(idx, q, ip, flags, mo)
    assert (total, reach) == (n_anchor, D)
    n, off, kept, flag, dev_reach = sift_kept(ctx, idx, mo, q, NCPU)
    assert n >= 0, mpa.last_error()
    assert dev_reach == D and (n_keep is None) == (D > SIFT_REACH_MAX)
    assert not flag.any(), ("the sift handed queries back", np.flatnonzero(flag).tolist())
    for i, (want, _, _) in enumerate(per):
        assert np.array_equal(kept[off[i]:off[i + 1]], want), ("kept anchors: device != rule", i, len(want), int(off[i + 1] - off[i]))
    n_back, du_off, du, da_off, da = main_chains(ctx, idx, mo, q, NCPU)      # (fails with "the device did not chain" if it did not)
    for i, (_, u, ca) in enumerate(per):
        assert np.array_equal(u, du[du_off[i]:du_off[i + 1]]), ("main chains, u: device != mp_chain", i)
        assert np.array_equal(ca, da[da_off[i]:da_off[i + 1]]), ("main chains, anchors: device != mp_chain", i)
    print("%s: %d anchors, %d kept, %d chains, %d queries handed back" % (_pid((point, seg)), total, n, int(du_off[-1]), n_back))
    # not passing on nothing
    assert n >= (n_anchor if n_keep is None else n_keep) // 2 and du_off[-1] >= n_chain // 2, (n, int(du_off[-1]))
    assert n_back < len(q.seqs) // 4, n_back


def _host_chains_and_no_device_result(ctx, idx, q, mo, kmer, bbit, capfd):
    a_off, a = raw_anchors(idx, mo, q, NCPU)
    capfd.readouterr()
    n_back, du_off, du, da_off, da = main_chains(ctx, idx, mo, q, NCPU)
    notes = capfd.readouterr().err
    assert n_back == 0                                          # (counts queries a DEVICE run handed back)
    assert SEED_NOTE not in notes and "declined" not in notes, notes[-500:]
    for i in range(len(q.seqs)):
        u, ca = refbind.ref_chain(a[a_off[i]:a_off[i + 1]], seedopts.chain_args(mo, kmer, bbit, False))
        assert np.array_equal(u, du[du_off[i]:du_off[i + 1]]) and np.array_equal(ca, da[da_off[i]:da_off[i + 1]]), i
    return int(du_off[-1])


@pytest.mark.skipif(not refbind.have_ref(), reason="oracle/_ref/libminiprot_ref.so not built")
def test_min_chain_count_of_one_stays_on_the_host(tandem, ctx, monkeypatch, capfd):
    """-n 1: one-anchor chains count, so a view may leave no anchor out (chain_core.h): the batch takes the host stages, silently"""
    monkeypatch.setenv("MPA_TIMING", "1")
    ip = (8, 30, 6, 1)
    idx = tandem.index(ip, ctx)
    mo = golden.apply_flags(mpa.default_mapopt(), ["-S", "-n", "1"])
    assert _host_chains_and_no_device_result(ctx, idx, tandem.q, mo, ip[2], ip[0], capfd) >= 161


@pytest.mark.skipif(not refbind.have_ref(), reason="oracle/_ref/libminiprot_ref.so not built")
def test_base_resolution_index_stays_on_the_host(ctx, tmp_path, monkeypatch, capfd):
    """-b 0: no blocks to sift by"""
    monkeypatch.setenv("MPA_TIMING", "1")
    contigs, prots, names = gen_synth.generate(200000, 1, 5, 3)
    idx = mpa.Index.read_fasta(seedopts.write_genome(tmp_path, contigs), (0, 30, 6, 1))
    assert idx.build_kmers(4) == "host"
    idx.to_device(ctx)
    mo = golden.apply_flags(mpa.default_mapopt(), ["-S"])
    assert _host_chains_and_no_device_result(ctx, idx, mpa.Queries(prots, names), mo, 6, 0, capfd) >= 3
    idx.close()


def _case(name):
    return [c for c in golden.SYNTH_CASES + golden.OPTION_CASES if c["name"] == name][0]


def _case_index(case, ctx, tmp_path):
    contigs, prots, names = golden.synth_inputs(case)
    if "idx" in case:
        idx = mpa.Index.read_fasta(seedopts.write_genome(tmp_path, contigs), case["idx"])
    else:
        idx = mpa.Index.from_nt4(contigs, ["chr%d" % (i + 1) for i in range(len(contigs))])
    assert idx.build_kmers(4) == "host"
    idx.to_device(ctx)
    return idx, prots, names


def _both_ways(ctx, idx, mo, prots, names, capfd):
    """(bytes, notes) of the blocking call and of a 3-batch stream"""
    capfd.readouterr()
    one = map_batch_gpu(ctx, idx, mo, mpa.Queries(prots, names), 4)
    notes_one = capfd.readouterr().err
    n = len(prots)
    batches = [mpa.Queries(prots[a:b], names[a:b]) for a, b in ((0, n // 3), (n // 3, 2 * n // 3), (2 * n // 3, n))]
    stream = b"".join(mpa.map_batches(ctx, idx, mo, batches, 4))
    return (one, notes_one), (stream, capfd.readouterr().err)


@pytest.mark.parametrize("name,sketch", [("syn_h", False), ("opt_noprechain", False), ("syn_h", True)], ids=["syn_h", "opt_noprechain", "syn_h-gpu-sketch"])
def test_whole_path_bytes_with_the_direct_route(ctx, name, sketch, tmp_path, monkeypatch, capfd):
    """-S -u (reach 3) and --no-pre-chain -u (every anchor kept) through the blocking call and a 3-batch stream: the reference's
    bytes, seeded on the device and nowhere declined; -S once more with the device sketch feeding the sift"""
    monkeypatch.setenv("MPA_TIMING", "1")
    if sketch:
        monkeypatch.setenv("MPA_GPU_SKETCH", "1")
    case = _case(name)
    idx, prots, names = _case_index(case, ctx, tmp_path)
    ref = open(golden.path(name + ".ref.paf"), "rb").read()
    for what, (ours, notes) in zip(("blocking call", "stream"), _both_ways(ctx, idx, golden.mapopt_for(case), prots, names, capfd)):
        assert SEED_NOTE in notes and "direct route" in notes, (what, notes[-800:])
        assert "declined" not in notes, (what, [l for l in notes.split("\n") if "declined" in l][:3])
        assert ("sketch on the GPU" in notes) == sketch, what
        assert ours == ref, "%s: output differs from the reference for %s" % (what, name)
    idx.close()


@pytest.mark.parametrize("name", ["syn_h", "opt_noprechain"])
def test_whole_path_with_the_knob_unset_keeps_the_host_route(ctx, name, tmp_path, monkeypatch, capfd):
    monkeypatch.setenv("MPA_TIMING", "1")
    monkeypatch.delenv("MPA_GPU_SEED_NOPRE")
    case = _case(name)
    idx, prots, names = _case_index(case, ctx, tmp_path)
    ref = open(golden.path(name + ".ref.paf"), "rb").read()
    for what, (ours, notes) in zip(("blocking call", "stream"), _both_ways(ctx, idx, golden.mapopt_for(case), prots, names, capfd)):
        assert SEED_NOTE not in notes and "declined" not in notes, what
        assert ours == ref, "%s: output differs from the reference for %s" % (what, name)
    idx.close()
