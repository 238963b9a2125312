"""The keep rule of the direct seeding route (-S / --no-pre-chain with MPA_GPU_SEED_NOPRE=1: sift by the main chain's reach, then the
main chain, no pre-chain) as the library restates it on the host -- mpa_dbg_sift_kept(ctx = NULL), the statement that
tests/test_seed_nopre_gpu.py compares the device's sift with -- against the rule written in numpy, and where the route applies."""
import os
import numpy as np
import pytest
import miniprot_amd as mpa
import golden
import seedopts
from seednopre import UNSUPPORTED, sift_kept, rule_keeps, reach_of
from test_seed_gpu import raw_anchors

NCPU = min(16, os.cpu_count() or 4)
POINT = (8, 30, 6, 1)


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    contigs, seqs = seedopts.tandem_genome(5, 35)
    idx = mpa.Index.read_fasta(seedopts.write_genome(tmp_path_factory.mktemp("nopre"), contigs), POINT)
    assert idx.build_kmers(NCPU) == "host"
    yield idx, mpa.Queries(seqs)
    idx.close()


def test_host_restatement_equals_the_numpy_rule(world, monkeypatch):
    """(8,30,6,1) -S: reach 1000 >> 8 = 3 blocks; the rule keeps 7 414 of the 16 403 anchors (a reach of one block would keep 7 035)"""
    idx, q = world
    monkeypatch.setenv("MPA_GPU_SEED_NOPRE", "1")
    mo = golden.apply_flags(mpa.default_mapopt(), ["-S"])
    a_off, a = raw_anchors(idx, mo, q, NCPU)
    n, off, kept, flag, reach = sift_kept(None, idx, mo, q, NCPU)
    assert n >= 0, mpa.last_error()
    assert reach == reach_of(mo, POINT[0]) == 3
    assert not flag.any()
    total, narrow = 0, 0
    for i in range(len(q.seqs)):
        want = rule_keeps(a[a_off[i]:a_off[i + 1]], reach)
        assert np.array_equal(kept[off[i]:off[i + 1]], want), i
        total += len(want)
        narrow += len(rule_keeps(a[a_off[i]:a_off[i + 1]], 1))
    print("anchors %d, kept %d (reach 1: %d)" % (a_off[-1], total, narrow))
    assert n == total == off[-1]
    assert (int(a_off[-1]), total, narrow) == (16403, 7414, 7035)


def test_keep_all_beyond_the_widest_filtered_reach(world, monkeypatch):
    """--no-pre-chain with splicing: reach 200 000 >> 8 = 781 blocks, far beyond what the sift filters by: every anchor, in order"""
    idx, q = world
    monkeypatch.setenv("MPA_GPU_SEED_NOPRE", "1")
    mo = golden.apply_flags(mpa.default_mapopt(), ["--no-pre-chain"])
    a_off, a = raw_anchors(idx, mo, q, NCPU)
    n, off, kept, flag, reach = sift_kept(None, idx, mo, q, NCPU)
    assert n >= 0, mpa.last_error()
    assert reach == 781 and np.array_equal(off, a_off) and np.array_equal(kept, a) and n == 16403


def test_unsupported_where_the_direct_route_does_not_apply(world, monkeypatch):
    idx, q = world
    nosplice = golden.apply_flags(mpa.default_mapopt(), ["-S"])
    monkeypatch.delenv("MPA_GPU_SEED_NOPRE", raising=False)
    assert sift_kept(None, idx, nosplice, q, NCPU)[0] == UNSUPPORTED                      # the knob is unset
    monkeypatch.setenv("MPA_GPU_SEED_NOPRE", "0")
    assert sift_kept(None, idx, nosplice, q, NCPU)[0] == UNSUPPORTED
    monkeypatch.setenv("MPA_GPU_SEED_NOPRE", "1")
    assert sift_kept(None, idx, nosplice, q, NCPU)[0] >= 0
    one = golden.apply_flags(mpa.default_mapopt(), ["-S", "-n", "1"])
    assert sift_kept(None, idx, one, q, NCPU)[0] == UNSUPPORTED                           # -n 1: a sparse view is not valid
    assert sift_kept(None, idx, mpa.default_mapopt(), q, NCPU)[0] == UNSUPPORTED          # a run with a pre-chain
