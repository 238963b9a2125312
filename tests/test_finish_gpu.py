"""MPA_GPU_FINISH=1: ranking and flat result of a batch on the device (k_finish_rank, k_finish_scan, k_finish_gather of finish_kernels.hip;
the code is finish_core.h, which tests/test_finish_cpu.py pins against the reference on the CPU).

1. mpa_dbg_finish on a context against the shared core on the host (ctx == NULL) on every generated table of tests/finishcases.py, byte
   for byte on every output array; a subset also against the reference's own ranking (tests/finish_ref_shim.c).
2. The whole path with MPA_GPU_STATS=1 MPA_GPU_FINISH=1: the text is the golden / live-reference text, the result's flat arrays are
   those of the run with MPA_GPU_FINISH unset, the device's note is there with `kept` equal to the result's hits, nothing declines, and
   MPA_CS_DUMP holds the same bytes.
3. Declines: without MPA_GPU_STATS the step says so and the host ranks, with the same bytes; MPA_MF_NO_ALIGN says nothing."""
import os
import re
import subprocess
import numpy as np
import pytest
import miniprot_amd as mpa
import refbind
import alnstats
import finishcases
import golden
import gen_synth

pytestmark = pytest.mark.gpu

GPU_NOTE = re.compile(r"finish on the GPU: (\d+) queries, (\d+) hits in, (\d+) kept, (\d+) bytes down")
STATS = {"MPA_GPU_STATS": "1"}
WALKS = {"MPA_GPU_STATS": "1", "MPA_GPU_CS": "1", "MPA_GPU_ROWS": "1"}
EVERY = dict(WALKS, MPA_GPU_SEED="1", MPA_GPU_SKETCH="1", MPA_GPU_REGIONS="1", MPA_GPU_REFINE="1", MPA_GPU_PLANS="1", MPA_GPU_DPPLAN="1")
EVERY_SPANS = dict(EVERY, MPA_GPU_SPANS="1", MPA_GPU_ROUND2="1")
KNOBS = sorted(set(EVERY_SPANS) | {"MPA_GPU_FINISH", "MPA_TIMING", "MPA_CS_DUMP"})


@pytest.fixture(scope="module")
def ctx():
    c = mpa.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def shim_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("finish_shim")


def _real_bytes(flat, n_query):
    """what a device call writes into its pinned block for this result: the counts' prefix, a hit record and two references per hit, and
    the dense arrays at their real length"""
    n_hit = len(flat["hits"]) // finishcases.HIT.itemsize
    return 64 * (n_query + 1) + n_hit * (136 + 16 + 24) + len(flat["cigars"]) + len(flat["feats"]) + len(flat["cs_text"]) + len(flat["rows_text"])


# ---- 1. the hook
_host = {}


def _host_flat(k):
    if k not in _host:
        _host[k] = finishcases.run(None, finishcases.tables()[k])
    return _host[k]


@pytest.mark.parametrize("k", range(len(finishcases.tables())), ids=[t["name"] for t in finishcases.tables()])
def test_device_equals_the_shared_core_on_every_table(ctx, k):
    t = finishcases.tables()[k]
    got = finishcases.run(ctx, t)
    d = finishcases.first_difference(got, _host_flat(k))
    assert d is None, "%s: %s" % (t["name"], d)
    n_q, n_in, kept, down, n_big, waits = mpa.dbg_finish_last(ctx)
    sizes = np.diff(t["first"])
    assert (n_q, n_in, kept) == (len(sizes), int(t["first"][-1]), len(got["hits"]) // finishcases.HIT.itemsize)
    assert n_big == int((sizes > 64).sum()) and waits == 1
    assert down == _real_bytes(got, len(sizes))           # (the kernels write the pinned block: what the result holds is what travels)


def test_tables_reach_the_hbm_scratch_and_several_scan_steps():
    """a guard on the generator alone (it passes without the feature): queries on both sides of the LDS capacity of 64 regions, and more
    queries than two steps of the scan"""
    sizes = [np.diff(t["first"]) for t in finishcases.tables()]
    assert any((s == 64).any() for s in sizes) and any((s == 65).any() for s in sizes) and any((s > 256).any() for s in sizes) and any(len(s) > 2 * 256 for s in sizes)


@pytest.mark.skipif(not refbind.have_ref(), reason="oracle/_ref/libminiprot_ref.so not built")
@pytest.mark.parametrize("name", ["sizes", "keys", "parents", "select_n1", "gather_edges", "fuzz0"])
def test_device_equals_the_reference_ranking(ctx, name, shim_dir):
    t = [x for x in finishcases.tables() if x["name"] == name][0]
    want = finishcases.expected_flat(t, finishcases.reference_ranks(t, shim_dir))
    d = finishcases.first_difference(finishcases.run(ctx, t), want)
    assert d is None, "%s: %s" % (name, d)


# ---- 2. the whole path
def _map(ctx, idx, mo, q, env, capfd, dump=None):
    """one blocking batch under `env` (every other knob of this file unset): (text, flat arrays, stderr, cs dump bytes)"""
    env = dict(env, MPA_TIMING="1")
    if dump is not None:
        env["MPA_CS_DUMP"] = str(dump)
    keep = {k: os.environ.get(k) for k in KNOBS}
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        capfd.readouterr()
        res = mpa.map_batch(ctx, idx, mo, q, 4)
        os.environ.pop("MPA_CS_DUMP", None)
        flat = mpa.result_flat(res)
        flat["last"] = mpa.dbg_finish_last(ctx)
        flat["n_query"] = len(q.seqs)
        text = mpa.format_output(idx, mo, q, res)[0]
        err = capfd.readouterr().err
    finally:
        for k, v in keep.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    return text, flat, err, open(str(dump), "rb").read() if dump is not None and os.path.exists(str(dump)) else b"", env


def _check_pair(off, on, ref):
    assert "finish" not in off[2].replace("take 2 + finish", "").replace("batch_finish", "")
    m = GPU_NOTE.findall(on[2])
    assert len(m) == 1, "MPA_GPU_FINISH=1 did not run the step on the device:\n" + "\n".join(l for l in on[2].split("\n") if "finish" in l or "declined" in l)
    declined = [l for l in on[2].split("\n") if "finish declined" in l]
    assert not declined, declined[:3]
    n_hit = len(on[1]["hits"]) // finishcases.HIT.itemsize
    assert n_hit > 0 and int(m[0][2]) == n_hit and int(m[0][1]) >= n_hit
    # the step ran inside the walks' call: ONE host wait for walks and finish together, nothing of the walks' own output came down (their
    # `... slots: ... bytes down` notes are the unset run's alone), and what came down is the result at its real size
    n_q, n_in, kept, down, n_big, waits = on[1]["last"]
    assert (n_q, kept, waits) == (on[1]["n_query"], n_hit, 1) and n_in == int(m[0][1])
    assert down == int(m[0][3]) == _real_bytes(on[1], n_q)
    assert "cs slots:" not in on[2] and "rows slots:" not in on[2]
    if "MPA_GPU_CS" in off[4]:
        assert "cs slots:" in off[2]
    if ref is not None:
        assert off[0] == ref and on[0] == ref, "text differs from the reference"
    assert on[0] == off[0]
    d = finishcases.first_difference(on[1], off[1])
    assert d is None, d
    assert len(off[3]) > 0 and on[3] == off[3], "MPA_CS_DUMP differs"


@pytest.mark.parametrize("name", ["syn_a", "syn_d", "syn_m"])
@pytest.mark.parametrize("knobs", [STATS, EVERY, EVERY_SPANS], ids=["stats", "every", "every_spans"])
def test_golden_cases(ctx, name, knobs, capfd, tmp_path):
    idx, mo, q, ref = alnstats.case_inputs(name, tmp_path)
    idx.to_device(ctx)
    off = _map(ctx, idx, mo, q, knobs, capfd, tmp_path / "off.cs")
    on = _map(ctx, idx, mo, q, dict(knobs, MPA_GPU_FINISH="1"), capfd, tmp_path / "on.cs")
    idx.close()
    _check_pair(off, on, ref)
    if knobs is not STATS and b"cs:Z:" in ref:
        assert len(on[1]["cs"]) > 0                       # (the cs bodies travelled with the hits through the device's gather)
    # both CIGAR sources: with MPA_GPU_SPANS=1 the gather reads k_assemble's pool on the device, otherwise the words the walks uploaded
    assert ("the assembled pool is on the device" in on[2]) == (knobs is EVERY_SPANS)


def test_edge_genome(ctx, capfd, tmp_path):
    import regioncases
    contigs, prots, names, mo = regioncases.edge_genome()
    idx, q = regioncases.edge_index(contigs), mpa.Queries(prots, names)
    ref = open(golden.path(regioncases.EDGE_REF), "rb").read()
    idx.to_device(ctx)
    off = _map(ctx, idx, mo, q, WALKS, capfd, tmp_path / "off.cs")
    on = _map(ctx, idx, mo, q, dict(WALKS, MPA_GPU_FINISH="1"), capfd, tmp_path / "on.cs")
    idx.close()
    _check_pair(off, on, ref)


def _families():
    """the gene-family genome of tests/test_scale_gpu.py (12 diverged copies of each of 16 two-exon genes over both strands of two contigs)
    and its options, -N 30 --outn=30 --outs=0.3 -p 0.3 -u: a dozen near-equal regions per query.  The family proteins and a few others"""
    codon = {"A": "GCT", "C": "TGT", "D": "GAT", "E": "GAA", "F": "TTT", "G": "GGT", "H": "CAT", "I": "ATT", "K": "AAA", "L": "CTG", "M": "ATG",
             "N": "AAT", "P": "CCT", "Q": "CAA", "R": "CGT", "S": "TCT", "T": "ACT", "V": "GTT", "W": "TGG", "Y": "TAT"}
    code = {"A": 0, "C": 1, "G": 2, "T": 3}
    comp = np.array([3, 2, 1, 0, 4], dtype=np.uint8)
    contigs, prots, names = gen_synth.generate(40_000_000, 2, 300, 17, mu=7.0, sigma=1.2, imax=20000)
    rng = np.random.default_rng(171)
    fam_prots, fam_names = [], []
    for f in range(16):
        p = bytes(prots[f]).decode()
        cds = np.array([code[c] for a in p for c in codon.get(a, "GCT")], np.uint8)
        cut = 3 * int(rng.integers(len(p) // 3, 2 * len(p) // 3)) + int(rng.integers(0, 3))
        ilen = int(rng.integers(200, 6000))
        intron = rng.integers(0, 4, ilen).astype(np.uint8)
        intron[:2] = [2, 3]; intron[-2:] = [0, 2]; intron[2] = 0; intron[-3] = 1
        gene = np.concatenate([cds[:cut], intron, cds[cut:], np.array([3, 0, 0], np.uint8)])
        for k in range(12):
            cp = gene.copy()
            m = rng.random(len(cp)) < rng.uniform(0.02, 0.09)
            cp[m] = rng.integers(0, 4, int(m.sum())).astype(np.uint8)
            if k % 4 == 3:
                cp = np.delete(cp, int(rng.integers(30, len(cp) - 30)))
            c = int(rng.integers(0, 2))
            at = int(rng.integers(1000, len(contigs[c]) - len(cp) - 1000))
            contigs[c][at:at + len(cp)] = comp[cp[::-1]] if rng.random() < 0.5 else cp
        fam_prots.append(bytes(prots[f])), fam_names.append("fam%02d" % f)
    prots, names = list(prots[16:32]) + fam_prots, list(names[16:32]) + fam_names
    idx = mpa.Index.from_nt4(contigs, ["chr1", "chr2"])
    del contigs
    mpa._check(mpa.lib().mpa_idx_build_kmers(idx.h, min(16, os.cpu_count() or 4)))
    mo = mpa.default_mapopt()
    mo.flag |= 4
    mo.best_n, mo.out_n, mo.out_sim, mo.pri_ratio = 30, 30, 0.3, 0.3
    return idx, mo, prots, names


@pytest.mark.skipif(not os.path.exists(refbind.REF_BIN), reason="oracle/_ref/miniprot not present")
def test_gene_families_against_the_live_reference(ctx, capfd, tmp_path):
    idx, mo, prots, names = _families()
    q = mpa.Queries(prots, names)
    idx.to_device(ctx)
    off = _map(ctx, idx, mo, q, WALKS, capfd, tmp_path / "off.cs")
    on = _map(ctx, idx, mo, q, dict(WALKS, MPA_GPU_FINISH="1"), capfd, tmp_path / "on.cs")
    mpi, faa = str(tmp_path / "g.mpi"), str(tmp_path / "p.faa")
    idx.dump(mpi)
    gen_synth.write_fasta_aa(faa, prots, names)
    idx.close()
    ref = subprocess.run([refbind.REF_BIN, "-t16", "-N", "30", "--outn=30", "--outs=0.3", "-p", "0.3", "-u", mpi, faa], stdout=subprocess.PIPE, stderr=subprocess.DEVNULL, check=True).stdout
    os.remove(mpi)
    _check_pair(off, on, ref)
    hits = np.frombuffer(on[1]["hits"], finishcases.HIT)
    assert (np.bincount(hits["qid"]) >= 8).sum() >= 8, "the families did not produce their secondaries"
    assert (hits["parent"] != hits["id"]).any()


def test_stream_of_three_batches(ctx, capfd, monkeypatch):
    """mpa_map_batches(): the step runs on the lanes' contexts -- the text (the stream hands out no results) and a note per batch"""
    idx, mo, q, ref = alnstats.case_inputs("syn_a")
    idx.to_device(ctx)
    n = len(q.seqs)
    batches = [mpa.Queries(q.seqs[a:b], q.names[a:b]) for a, b in ((0, n // 3), (n // 3, 2 * n // 3), (2 * n // 3, n))]
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in dict(WALKS, MPA_GPU_FINISH="1", MPA_TIMING="1").items():
        monkeypatch.setenv(k, v)
    capfd.readouterr()
    texts = mpa.map_batches(ctx, idx, mo, batches, 4)
    err = capfd.readouterr().err
    idx.close()
    assert b"".join(texts) == ref
    assert len(GPU_NOTE.findall(err)) == 3 and "finish declined" not in err


# ---- 3. declines
def test_without_device_statistics_the_step_declines_and_says_so(ctx, capfd, tmp_path):
    idx, mo, q, ref = alnstats.case_inputs("syn_a", tmp_path)
    idx.to_device(ctx)
    off = _map(ctx, idx, mo, q, {}, capfd)
    on = _map(ctx, idx, mo, q, {"MPA_GPU_FINISH": "1"}, capfd)
    idx.close()
    assert "finish declined (MPA_GPU_STATS is not 1)" in on[2] and not GPU_NOTE.findall(on[2])
    assert on[0] == ref and off[0] == ref
    assert finishcases.first_difference(on[1], off[1]) is None


def test_no_align_keeps_the_early_return_silently(ctx, capfd, tmp_path):
    idx, mo, q, ref = alnstats.case_inputs("syn_a", tmp_path)
    mo.flag |= 0x2                                        # MPA_MF_NO_ALIGN
    idx.to_device(ctx)
    off = _map(ctx, idx, mo, q, STATS, capfd)
    on = _map(ctx, idx, mo, q, dict(STATS, MPA_GPU_FINISH="1"), capfd)
    idx.close()
    assert "finish" not in on[2].replace("take 2 + finish", "").replace("batch_finish", "")
    assert on[0] == off[0] and finishcases.first_difference(on[1], off[1]) is None
