"""The multi-pass device index build (dev_index_build_passes: k_index_scan<INDEX_HIST>, the RANGED count / emit instantiations,
idx_plan_passes) on a 3 Mbp genome whose key budget is set so low that the build needs 2 .. thousands of passes.  Every comparison
is of bytes: the .mpi a multi-pass build dumps against the host build's (which the CPU tests pin to `miniprot -d`) and, where the
reference binary travelled with the tree, against `miniprot -d` itself.  The budget is the bytes the keys may take while they are
sorted, 44 per key (include/mpamd.h): a budget of 44 * n is "room for n keys"."""
import os
import subprocess
import numpy as np
import pytest
import miniprot_amd as mpa
import golden                                          # (puts tools/ on the path: gen_synth)
import gen_synth
import refbind
import seedopts

pytestmark = pytest.mark.gpu
UNSUPPORTED = -3                                       # MPA_ERR_UNSUPPORTED (include/mpamd.h)
NCPU = min(16, os.cpu_count() or 4)
KEY_BYTES = 44
DEFAULT = (8, 30, 6, 1)                                # (bbit, min_aa_len, kmer, mod_bit) of mp_idxopt_init
# -k5 -M0 -b6 -L20; -k7 -M3: 25 bucket bits, 8 192 buckets per histogram bin; -k4 -M6: 10 bucket bits, fewer than the histogram's 12
POINTS = [DEFAULT, (6, 20, 5, 0), (8, 30, 7, 3), (8, 30, 4, 6)]


@pytest.fixture(scope="module")
def ctx():
    c = mpa.Context(0)
    yield c
    c.close()


class _World:
    """the genome as a FASTA file and, per index point, what every test compares with: the host build's .mpi, `miniprot -d`'s where
    the binary exists and accepts the point, and the number of keys (from a one-pass device build's statistics)"""

    def __init__(self, tmp, ctx):
        self.tmp, self.ctx = str(tmp), ctx
        contigs, _, _ = gen_synth.generate(3_000_000, 3, 4, 123)
        self.fa = seedopts.write_genome(self.tmp, contigs)
        self.host, self.ref, self.keys = {}, {}, {}

    def host_mpi(self, point, fa=None):
        key = (point, fa)
        if key not in self.host:
            idx = mpa.Index.read_fasta(fa or self.fa, point)
            assert idx.build_kmers(NCPU) == "host"
            self.host[key] = dump_bytes(idx, self.tmp)
            idx.close()
        return self.host[key]

    def ref_mpi(self, point):
        """the reference's index at this point, or None (no binary here, or it does not take these options)"""
        if point not in self.ref:
            self.ref[point] = None
            if os.path.exists(refbind.REF_BIN):
                out = os.path.join(self.tmp, "ref.mpi")
                r = subprocess.run([refbind.REF_BIN, "-t%d" % NCPU] + seedopts.index_flags(point) + ["-d", out, self.fa], capture_output=True)
                if r.returncode == 0 and os.path.exists(out):
                    self.ref[point] = open(out, "rb").read()
                    os.remove(out)
        return self.ref[point]

    def n_keys(self, point):
        if point not in self.keys:
            where, st, data = device_build(self, point, 0)
            assert where == "gpu" and st["n_pass"] == 1 and st["hist_bits"] == 0 and st["max_bin_keys"] == 0, st
            assert st["max_pass_keys"] == st["n_keys"] > 1000, st
            assert data == self.host_mpi(point)
            self.keys[point] = st["n_keys"]
        return self.keys[point]


def dump_bytes(idx, tmp):
    path = os.path.join(tmp, "dump.mpi")
    idx.dump(path)
    data = open(path, "rb").read()
    os.remove(path)
    return data


def device_build(world, point, budget, fa=None):
    """(where it was built, the context's build statistics, the dumped .mpi) with `budget` bytes for the keys (0: the default)"""
    ctx = world.ctx
    idx = mpa.Index.read_fasta(fa or world.fa, point)
    ctx.idx_build_budget(budget)
    try:
        where = idx.build_kmers(NCPU, ctx)
    finally:
        ctx.idx_build_budget(0)
    st = ctx.idx_build_stats()
    data = dump_bytes(idx, world.tmp)
    idx.close()
    return where, st, data


@pytest.fixture(scope="module")
def world(tmp_path_factory, ctx):
    return _World(tmp_path_factory.mktemp("passes"), ctx)


def mpi_tables(data):
    """(ki, n_kb, bucket bits) of a .mpi image (index.c:189-202: magic, options, n_kb, ..., ki[], kb[] at the end)"""
    _, _, kmer, mod_bit = np.frombuffer(data, "<i4", 4, 4)
    n_kb = int(np.frombuffer(data, "<i8", 1, 24)[0])
    bits = int(4 * kmer - mod_bit)
    ki = np.frombuffer(data, "<i8", 1 << bits, len(data) - 4 * n_kb - 8 * (1 << bits))
    return ki, n_kb, bits


@pytest.mark.parametrize("div,min_pass", [(2, 2), (8, 8), (64, 33)])
def test_byte_identity_across_pass_counts(world, div, min_pass):
    n = world.n_keys(DEFAULT)
    where, st, data = device_build(world, DEFAULT, KEY_BYTES * n // div)
    print("budget 44 * %d / %d: %s" % (n, div, st))
    assert where == "gpu", mpa.last_error()
    assert st["n_pass"] >= min_pass and st["hist_bits"] == 12 and st["n_keys"] == n, st
    assert st["max_bin_keys"] <= st["max_pass_keys"] <= n // div and st["budget_bytes"] == KEY_BYTES * n // div, st
    assert data == world.host_mpi(DEFAULT)
    if world.ref_mpi(DEFAULT) is not None:
        assert data == world.ref_mpi(DEFAULT)


def test_the_edge_of_one_pass(world):
    n = world.n_keys(DEFAULT)
    where, st, data = device_build(world, DEFAULT, KEY_BYTES * n)
    assert where == "gpu" and st["n_pass"] == 1 and st["hist_bits"] == 0 and st["max_bin_keys"] == 0, st
    assert data == world.host_mpi(DEFAULT)
    where, st, data = device_build(world, DEFAULT, KEY_BYTES * (n - 1))
    assert where == "gpu" and st["n_pass"] == 2 and st["hist_bits"] == 12 and st["max_pass_keys"] < n, st
    assert data == world.host_mpi(DEFAULT)


def test_the_fullest_bin(world, ctx):
    """a budget of exactly the fullest bin's keys builds (a pass per bin, nearly); one key less cannot be planned: the build
    declines, leaves nothing behind on the device, and both the host build and a later device build work"""
    n = world.n_keys(DEFAULT)
    where, st, data = device_build(world, DEFAULT, KEY_BYTES * n // 8)
    assert where == "gpu" and st["n_pass"] >= 8, st
    big = st["max_bin_keys"]
    assert 0 < big <= n // 8
    where, st, data = device_build(world, DEFAULT, KEY_BYTES * big)
    print("budget of the fullest bin (%d keys): %s" % (big, st))
    assert where == "gpu", mpa.last_error()
    assert st["max_pass_keys"] == big == st["max_bin_keys"] and st["n_pass"] >= n // big, st
    assert data == world.host_mpi(DEFAULT)
    idx = mpa.Index.read_fasta(world.fa, DEFAULT)
    idx.to_device(ctx)                                                 # (the genome stays on the device whatever the build answers)
    before = ctx.device_bytes()
    ctx.idx_build_budget(KEY_BYTES * big - 1)
    try:
        rc = mpa.lib().mpa_idx_build_kmers_device(ctx.h, idx.h)
        msg = mpa.last_error()
        assert rc == UNSUPPORTED, (rc, msg)
        assert "bin " in msg and str(KEY_BYTES * big) in msg, msg      # names the bin and the bytes it would need
        st = ctx.idx_build_stats()
        assert st["n_pass"] == 0 and st["max_bin_keys"] == big and st["n_keys"] == n, st
        assert ctx.device_bytes() == before
        assert idx.build_kmers(NCPU, ctx) == "host"
        assert ctx.device_bytes() == before
    finally:
        ctx.idx_build_budget(0)
    assert dump_bytes(idx, world.tmp) == world.host_mpi(DEFAULT)
    assert idx.build_kmers(NCPU, ctx) == "gpu" and ctx.idx_build_stats()["n_pass"] == 1
    assert dump_bytes(idx, world.tmp) == world.host_mpi(DEFAULT)
    idx.close()


@pytest.mark.parametrize("point", POINTS, ids=[seedopts.index_name(p) for p in POINTS])
def test_histogram_and_index_options(world, ctx, point):
    """every index point at 8 or more passes: the bytes of the host build (and of the reference, on the points it accepts); and
    the histogram the passes were planned from -- its bins add up to the keys, and each bin holds at least the distinct keys the
    finished table has there, none where the table has none"""
    n = world.n_keys(point)
    where, st, data = device_build(world, point, KEY_BYTES * n // 8)
    hist = ctx.idx_build_hist()
    print("%s: %s" % (seedopts.index_name(point), st))
    assert where == "gpu", mpa.last_error()
    assert st["n_pass"] >= 8 and st["n_keys"] == n, st
    assert data == world.host_mpi(point)
    if world.ref_mpi(point) is not None:
        assert data == world.ref_mpi(point)
    ki, n_kb, bits = mpi_tables(data)
    assert st["hist_bits"] == min(bits, 12) and len(hist) == 1 << st["hist_bits"]
    assert int(hist.sum()) == n and int(hist.max()) == st["max_bin_keys"]
    per_bucket = np.diff(np.append(ki, n_kb))
    unique = per_bucket.reshape(len(hist), -1).sum(axis=1)
    assert int(unique.sum()) == n_kb
    assert np.all(hist >= unique) and np.array_equal(hist == 0, unique == 0)


def test_the_resident_table_serves_the_seeding_kernels(world, ctx, monkeypatch):
    """kb[] as the passes left it on the device, slice after slice: device seeding reads it and the output is the reference's"""
    case = [c for c in golden.SYNTH_CASES if c["name"] == "syn_a"][0]
    contigs, prots, names = golden.synth_inputs(case)
    idx = mpa.Index.from_nt4(contigs, ["chr%d" % (i + 1) for i in range(len(contigs))])
    assert idx.build_kmers(NCPU, ctx) == "gpu"
    n = ctx.idx_build_stats()["n_keys"]
    ctx.idx_build_budget(KEY_BYTES * n // 8)
    try:
        assert idx.build_kmers(NCPU, ctx) == "gpu"
    finally:
        ctx.idx_build_budget(0)
    assert ctx.idx_build_stats()["n_pass"] >= 8
    idx.to_device(ctx)
    monkeypatch.setenv("MPA_GPU_SEED", "1")
    ours = b"".join(mpa.map_batches(ctx, idx, golden.mapopt_for(case), [mpa.Queries(prots, names)], 4))
    assert ours == open(golden.path("syn_a.ref.paf"), "rb").read()
    idx.close()


def test_the_megabyte_knob_is_read_on_every_call(world, monkeypatch):
    n = world.n_keys(DEFAULT)
    monkeypatch.setenv("MPA_IDX_BUILD_MB", "1")
    where, st, data = device_build(world, DEFAULT, 0)
    print("MPA_IDX_BUILD_MB=1: %s" % st)
    assert where == "gpu", mpa.last_error()
    assert st["budget_bytes"] == 1 << 20 and st["max_pass_keys"] <= (1 << 20) // KEY_BYTES, st
    assert st["n_pass"] >= max(2, -(-n // ((1 << 20) // KEY_BYTES))), st
    assert data == world.host_mpi(DEFAULT)
    monkeypatch.delenv("MPA_IDX_BUILD_MB")
    where, st, data = device_build(world, DEFAULT, 0)
    assert where == "gpu" and st["n_pass"] == 1 and st["hist_bits"] == 0, st
    assert data == world.host_mpi(DEFAULT)


# A reading frame of 40 codons whose only -k4 -M6 key (one 4-mer in 64 is kept) falls into bucket 994 of 1 024 (found by building
# the table of random frames on the host); alone on a contig behind 2 500 Ns no other frame of either strand is 30 codons long
LATE_ORF = "GCAGCACGTGCTGAGGGGTCTACATCATTAGTGGTGGTGATCTGTAATTCGTTCCAATGGGTAAGGAGGGGTTCACTTGGTTCCCGCTCTGGAACATTTCTGGTGCAGCGGCCTTACGTG"
LATE_BUCKET = 994
K4M6 = (8, 30, 4, 6)


def test_awkward_contigs(world, ctx):
    """an empty contig, a 10-base contig, an all-N contig, a random one, and one contig per strand whose keys all land in the last
    of 8 or more passes (every chunk of theirs counts zero keys in all passes before): the bytes of the host build, at -k4 -M6 where
    the late contigs are what they were made to be, and at the default options"""
    comp = str.maketrans("ACGTN", "TGCAN")
    late_fwd = "N" * 2500 + LATE_ORF                                  # two chunks; the key sits in the second
    late_rev = late_fwd.translate(comp)[::-1]                          # the same frame on the reverse strand, in the first chunk
    rng = np.random.default_rng(9)
    body = "".join("ACGT"[i] for i in rng.integers(0, 4, 300000))
    fa = os.path.join(world.tmp, "awkward.fa")
    with open(fa, "w") as f:
        for name, seq in (("empty", ""), ("ten", "ACGTTGCAAC"), ("allN", "N" * 5000), ("body", body), ("late_fwd", late_fwd), ("late_rev", late_rev)):
            f.write(">%s\n" % name)
            for k in range(0, len(seq), 80):
                f.write(seq[k:k + 80] + "\n")
    # the premise: the late contigs alone have keys, and only in that bucket
    alone = os.path.join(world.tmp, "late.fa")
    with open(alone, "w") as f:
        f.write(">late_fwd\n%s\n>late_rev\n%s\n" % (late_fwd, late_rev))
    ki, n_kb, bits = mpi_tables(world.host_mpi(K4M6, alone))
    per_bucket = np.diff(np.append(ki, n_kb))
    assert bits == 10 and n_kb == 2 and per_bucket[LATE_BUCKET] == 2
    for point in (K4M6, DEFAULT):
        # the histogram of a first multi-pass build gives the smallest budget that plans 8 passes: seven that are as full as they
        # can be and an eighth that holds nearly as much, so that it begins well below the late contigs' bucket
        idx = mpa.Index.read_fasta(fa, point)
        assert idx.build_kmers(NCPU, ctx) == "gpu"
        n = ctx.idx_build_stats()["n_keys"]
        idx.close()
        where, st, data = device_build(world, point, KEY_BYTES * n // 8, fa)
        assert where == "gpu" and st["n_pass"] >= 8 and st["n_keys"] == n, (st, mpa.last_error())
        assert data == world.host_mpi(point, fa)
        hist = ctx.idx_build_hist()
        lo, hi = int(hist.max()), n                                    # (the fewest passes never grow with the budget)
        while lo < hi:
            mid = (lo + hi) // 2
            if len(mpa.idx_plan_passes(hist, mid)) - 1 <= 8:
                hi = mid
            else:
                lo = mid + 1
        plan = mpa.idx_plan_passes(hist, lo)
        assert len(plan) - 1 == 8, plan
        where, st, data = device_build(world, point, KEY_BYTES * lo, fa)
        print("awkward contigs, %s, %d keys per pass: %s, last pass from bin %d" % (seedopts.index_name(point), lo, st, plan[-2]))
        assert where == "gpu", mpa.last_error()
        assert st["n_pass"] == 8 and st["n_keys"] == n and st["max_pass_keys"] <= lo, st
        assert np.array_equal(ctx.idx_build_hist(), hist)
        assert data == world.host_mpi(point, fa)
        if point == K4M6:
            assert plan[-2] <= LATE_BUCKET                             # (one bucket per bin: the last pass takes the late contigs' keys)
