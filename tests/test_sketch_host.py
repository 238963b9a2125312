"""The host's sketch stage (host_plan.cpp stage_seeds: protein sketch, bucket lookup, occurrence cut-off; map.c:126-170) pinned
directly: mpa_dbg_seed_jobs(ctx = NULL) against a numpy restatement built from the oracle's mpo_sketch_prot (pinned to the reference
in tests/test_oracle.py) and mpa_idx_bucket_counts -- same kept seeds, same order, same cut-off per query.  This stage is the
yardstick of tests/test_sketch_gpu.py; until now it was pinned only through whole-path goldens."""
import numpy as np
import pytest
import miniprot_amd as mpa
import seedopts
import sketchcases as sc


@pytest.fixture(scope="module")
def genome(tmp_path_factory):
    contigs, _ = seedopts.tandem_genome(5, 35)
    return seedopts.write_genome(tmp_path_factory.mktemp("sketch"), contigs)


@pytest.mark.parametrize("point", seedopts.INDEX_POINTS, ids=seedopts.index_name)
def test_host_seed_jobs_equal_the_restated_stage(genome, point):
    _, _, kmer, mod_bit = point
    _, seqs = sc.all_queries(kmer)
    idx = mpa.Index.read_fasta(genome, point)
    assert idx.build_kmers(sc.NCPU) == "host"
    q = mpa.Queries(seqs)
    sizes, n_cut = set(), 0
    for max_occ in sc.MAX_OCC:
        mo = sc.mapopt(max_occ)
        back, off, trip, mocc = sc.seed_jobs(None, idx, mo, q)
        assert back == 0
        want = sc.restated(idx, kmer, mod_bit, seqs, int(mo.max_occ))
        for i, (n, cut, t) in enumerate(want):
            sizes.add(n)
            assert int(mocc[i]) == cut, (i, n, int(mocc[i]), cut)
            assert np.array_equal(trip[off[i]:off[i + 1]], t), (i, n)
            n_cut += cut < mo.max_occ
        assert off[-1] == sum(len(t) for _, _, t in want)
        assert off[-1] > 300, int(off[-1])                      # not passing on nothing (one k-mer in 16 at -M4: 757 kept seeds)
    if kmer >= 6:                                               # the boxplot bound does cut below max_occ (at -k4 / -k5 on 3 Mbp every bucket is fuller than that)
        assert n_cut > 0
    # both sides of the n >= 8 branch, and the empty sketch
    assert 0 in sizes and any(0 < n < 8 for n in sizes) and any(n >= 8 for n in sizes), sorted(sizes)[:30]
    if mod_bit <= 1:                                            # (one k-mer in 16 kept: a 27-residue query has a seed or two)
        assert {5, 6, 7} & sizes and {8, 9, 10} & sizes, sorted(sizes)[:30]      # ... and close to it on both sides
    idx.close()


def test_bucket_counts_refuse_a_bucket_beyond_the_table(genome):
    idx = mpa.Index.read_fasta(genome, seedopts.INDEX_POINTS[0])
    assert idx.build_kmers(sc.NCPU) == "host"
    n_bucket = 1 << (4 * 6 - 1)
    cnt = sc.bucket_counts(idx, np.arange(n_bucket - 4, n_bucket))
    assert (cnt >= 0).all()
    L = mpa.lib()
    bad = np.array([n_bucket], np.uint32)
    out = np.zeros(1, np.int64)
    assert L.mpa_idx_bucket_counts(idx.h, 1, bad.ctypes.data, out.ctypes.data) < 0 and "beyond" in mpa.last_error()
    idx.close()
