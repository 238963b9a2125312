"""CPU-only checks of the product's HOST logic (no GPU, no compute calls into the HIP executor):
the stage machine mpa_batch_* is driven with the oracle as DP executor and the resulting PAF must equal the
golden output of the real reference; plus index build/dump parity and C-ABI hygiene."""
import ctypes as C
import hashlib
import os
import re
import subprocess
import numpy as np
import pytest
import miniprot_amd as mpa
import refbind
import golden
from hostpipe import read_fasta, map_batch, oracle_executor


def test_library_exports_every_declared_symbol():
    hdr = open(os.path.join(refbind.ROOT, "include", "mpamd.h")).read()
    names = sorted(set(re.findall(r"\b(mpa_[a-z0-9_]+)\s*\(", hdr)))
    assert len(names) > 30
    L = mpa.lib()
    # the reference-signature entry points and globals of include/miniprot.h / include/nasw.h (boundary #1/#2 under the reference's names)
    for h in ("miniprot.h", "nasw.h"):
        txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(refbind.ROOT, "include", h)).read(), flags=re.S)
        txt = re.sub(r"static inline[^{]*\{.*?\n\}", "", txt, flags=re.S)
        names += sorted(set(re.findall(r"\b((?:mp|ns)_[a-z0-9_]+)\s*\(", txt)))
        names += re.findall(r"\*?((?:mp|ns)_[a-z0-9_]+)(?:\[\d+\])?(?=[,;])", " ".join(l for l in txt.split("\n") if l.startswith("extern ")))
    missing = [n for n in sorted(set(names)) if not hasattr(L, n)]
    assert not missing, "declared in include/ but not exported: %s" % missing
    assert "mp_map" in names and "ns_global_gs16b" in names and "ns_tab_codon" in names


def test_no_device_is_a_loud_error():
    """there is no CPU fallback: without a GPU a context cannot be created and mapping refuses to run"""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    with pytest.raises(mpa.MpaError):
        mpa.Context(0)
    idx = mpa.Index.from_fasta(golden.path("DPP3-hs.gen.fa.gz"))
    q = mpa.Queries([b"MKTAYIAKQR"], ["x"])
    res = C.c_void_p()
    rc = mpa.lib().mpa_map_batch(None, idx.h, C.byref(mpa.default_mapopt()), C.byref(q.c), 1, C.byref(res))
    assert rc == -1 and not res.value


def test_the_multi_device_mapper_refuses_without_contexts():
    """mpa_map_batches_multi (one pipeline per device in one process): no context list, a null context or more than eight contexts are
    errors with a message -- and, like every mapping entry point, it has no CPU fallback to slip into"""
    L = mpa.lib()
    L.mpa_map_batches_multi.restype = C.c_int
    L.mpa_map_batches_multi.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    idx = mpa.Index.from_nt4([np.zeros(500, np.uint8)], ["c"])
    q = mpa.Queries([b"MKTAYIAKQR"], ["x"])
    res = (C.c_void_p * 1)()
    mo = mpa.default_mapopt()
    assert L.mpa_map_batches_multi(0, None, idx.h, C.byref(mo), 1, C.byref(q.c), None, 1, res, None, None, None) == -1 and b"no device context" in L.mpa_last_error()
    none = (C.c_void_p * 2)(None, None)
    assert L.mpa_map_batches_multi(2, none, idx.h, C.byref(mo), 1, C.byref(q.c), None, 1, res, None, None, None) == -1 and b"null context" in L.mpa_last_error()
    nine = (C.c_void_p * 9)()
    assert L.mpa_map_batches_multi(9, nine, idx.h, C.byref(mo), 1, C.byref(q.c), None, 1, res, None, None, None) == -5 and b"eight" in L.mpa_last_error()
    assert not res[0]
    idx.close()


def test_error_paths_report_instead_of_guessing(tmp_path):
    """error behaviour of the C ABI: NULL / negative code + a message, never a silent default"""
    L = mpa.lib()
    L.mpa_idx_restore.restype = C.c_void_p
    assert not L.mpa_idx_restore(b"/nonexistent/ref.mpi") and b"cannot open" in L.mpa_last_error()
    junk = tmp_path / "junk.mpi"
    junk.write_bytes(b"not an index at all" * 10)
    assert not L.mpa_idx_restore(str(junk).encode()) and L.mpa_last_error()
    idx = mpa.Index.from_nt4([np.zeros(500, np.uint8)], ["c"])       # genome only: no k-mer table yet
    q = mpa.Queries([b"MKTAYIAKQR"], ["x"])
    L.mpa_batch_begin.restype = C.c_void_p
    assert not L.mpa_batch_begin(idx.h, C.byref(mpa.default_mapopt()), C.byref(q.c), 1) and b"k-mer table" in L.mpa_last_error()
    mo = mpa.default_mapopt()
    with pytest.raises(mpa.MpaError):
        idx.set_spsc(str(tmp_path / "missing.tsv"), mo)
    assert mo.io == 29 + 10                                            # (mp_set_spsc raises io before it reads the file, index.c:243)
    idx.close()


def test_product_does_not_link_the_oracle():
    out = subprocess.run(["ldd", mpa.LIB_PATH], capture_output=True, text=True).stdout
    assert "mporacle" not in out and "miniprot_ref" not in out and "nasw_sse41" not in out
    syms = subprocess.run(["nm", "-D", mpa.LIB_PATH], capture_output=True, text=True).stdout
    # (ns_global_gs16b / mp_map ARE exported since round 2, ns_global_gs32 / gs32b since round 3 -- by
    #  miniprot_amd/csrc/compat.cpp, on top of the HIP path; what must not be there is anything of the checker: the oracle's
    #  mpo_* or the reference's internals)
    assert "mpo_" not in syms and "mp_chain" not in syms and "mp_sketch_prot" not in syms and "kt_for" not in syms and "radix_sort_mp" not in syms
    assert "ns_global_gs32b" in syms and "ns_global_gs32\n" in syms + "\n"


def test_mapopt_defaults_match_reference_layout():
    mo = mpa.default_mapopt()
    assert C.sizeof(mpa.MapOpt) == 656                      # sizeof(mp_mapopt_t), SURVEY.md 8(b)
    assert (mo.max_intron, mo.max_ext, mo.io, mo.io_end, mo.fs, mo.kmer2, mo.best_n) == (200000, 10000, 29, 19, 23, 5, 30)
    if refbind.have_ref():
        buf = (C.c_char * 656)()
        refbind.ref().mp_mapopt_init(buf)
        assert bytes(buf)[:156] == bytes(mo)[:156]            # everything before gff_prefix
        assert bytes(buf)[-484:] == bytes(mo)[-484:]          # scoring matrix incl. the stop row/column


def test_index_build_is_byte_identical_to_golden_reference_index(tmp_path):
    idx = mpa.Index.from_fasta(golden.path("DPP3-hs.gen.fa.gz"))
    out = str(tmp_path / "x.mpi")
    idx.dump(out)
    # md5 of `miniprot -d` output for this genome with the reference (recorded by tools/make_golden.py run)
    md5 = hashlib.md5(open(out, "rb").read()).hexdigest()
    if refbind.have_ref():
        ref = str(tmp_path / "r.mpi")
        subprocess.run([refbind.REF_BIN, "-t2", "-d", ref, golden.path("DPP3-hs.gen.fa.gz")], capture_output=True, check=True)
        assert md5 == hashlib.md5(open(ref, "rb").read()).hexdigest()
    back = mpa.Index.restore(out)
    assert back.n_ctg() == 1 and back.ctg_len(0) == 27033 and back.ctg_name(0) == "chr11:66478458-66505490"


def test_dpp3_paf_identical(oracle_built):
    idx = mpa.Index.from_fasta(golden.path("DPP3-hs.gen.fa.gz"))
    names, seqs = read_fasta(golden.path("DPP3-mm.pep.fa.gz"))
    paf = map_batch(idx, mpa.default_mapopt(), mpa.Queries(seqs, names), oracle_executor)
    assert paf == open(golden.path("dpp3.ref.paf"), "rb").read()
    assert hashlib.md5(paf).hexdigest() == "74fd00200bda6c03380bb3062fb5178b"


def test_dpp3_gff_identical(oracle_built):
    """config 1 with --gff: md5 d08d9caa... recorded in SURVEY.md 8(c)"""
    idx = mpa.Index.from_fasta(golden.path("DPP3-hs.gen.fa.gz"))
    names, seqs = read_fasta(golden.path("DPP3-mm.pep.fa.gz"))
    mo = mpa.default_mapopt()
    mo.flag |= 0x8
    out = b"##gff-version 3\n" + map_batch(idx, mo, mpa.Queries(seqs, names), oracle_executor)
    assert hashlib.md5(out).hexdigest() == "d08d9caa27b8bd896ee4f14824597c54"


def test_dpp3_aln_trans_gtf_identical(oracle_built):
    """config 1 with --aln --trans --gtf: PAF line + residue rows (##ATN/##ATA/##AAS/##AQA), translation (##STA), GTF"""
    idx = mpa.Index.from_fasta(golden.path("DPP3-hs.gen.fa.gz"))
    names, seqs = read_fasta(golden.path("DPP3-mm.pep.fa.gz"))
    mo = mpa.default_mapopt()
    mo.flag |= 0x80 | 0x100 | 0x20
    out = map_batch(idx, mo, mpa.Queries(seqs, names), oracle_executor)
    assert out == open(golden.path("dpp3_aln_trans_gtf.ref.txt"), "rb").read()


@pytest.mark.parametrize("case", golden.SYNTH_CASES, ids=[c["name"] for c in golden.SYNTH_CASES])
def test_synthetic_paf_identical(oracle_built, case, tmp_path):
    contigs, prots, names = golden.synth_inputs(case)
    idx = mpa.Index.from_nt4(contigs, ["chr%d" % (i + 1) for i in range(len(contigs))])
    mpa._check(mpa.lib().mpa_idx_build_kmers(idx.h, 4))
    mo = golden.mapopt_for(case)
    if "spsc" in case:
        idx.set_spsc(golden.write_spsc(case, contigs, str(tmp_path / "spsc.tsv")), mo)
    paf = map_batch(idx, mo, mpa.Queries(prots, names), oracle_executor, n_threads=4)
    paf = golden.file_header(case) + paf
    ref = open(golden.path(case["name"] + ".ref.paf"), "rb").read()
    if paf != ref:
        for x, y in zip(paf.split(b"\n"), ref.split(b"\n")):
            if x != y:
                raise AssertionError("first differing line\n ours %r\n ref  %r" % (x[:300], y[:300]))
    assert paf == ref


@pytest.mark.parametrize("case", golden.OPTION_CASES, ids=[c["name"] for c in golden.OPTION_CASES])
def test_option_cases_paf_identical(oracle_built, case, tmp_path):
    """The host stages + oracle executor away from the default index and seeding / chaining options (-k -M -b -L, -c -l -g -w -n -m
    --max-skip --no-pre-chain -G): the bytes of the reference, which built its own index with the same flags.  The GPU tests of
    tests/test_seed_options_gpu.py lean on the host stages at these points."""
    import seedopts
    contigs, prots, names = golden.synth_inputs(case)
    idx = mpa.Index.read_fasta(seedopts.write_genome(tmp_path, contigs), case["idx"])
    assert idx.build_kmers(4) == "host"
    paf = map_batch(idx, golden.mapopt_for(case), mpa.Queries(prots, names), oracle_executor, n_threads=4)
    ref = open(golden.path(case["name"] + ".ref.paf"), "rb").read()
    if paf != ref:
        for x, y in zip(paf.split(b"\n"), ref.split(b"\n")):
            if x != y:
                raise AssertionError("first differing line\n ours %r\n ref  %r" % (x[:300], y[:300]))
    assert paf == ref
    idx.close()


def test_option_cases_name_the_index_their_flags_build():
    """the "idx" tuple of every option case is what its -b -L -k -M flags say over mp_idxopt_init's 8, 30, 6, 1 (several of these
    cases print the same bytes, -L37 and -L38 among them: a wrong tuple would put a GPU test on the other side of a guard unseen),
    and every seedopts point translates into the fields it names"""
    import seedopts
    for case in golden.OPTION_CASES:
        want = {"-b": 8, "-L": 30, "-k": 6, "-M": 1}
        fl = case["flags"]
        for i, f in enumerate(fl):
            if f in want:
                want[f] = int(fl[i + 1])
        assert tuple(case["idx"]) == (want["-b"], want["-L"], want["-k"], want["-M"]), case["name"]
        assert os.path.getsize(golden.path(case["name"] + ".ref.paf")) < 100000
    d = mpa.default_mapopt()
    got = {p.name: p.apply(mpa.default_mapopt()) for p in seedopts.CHAIN_POINTS + seedopts.REFINE_POINTS}
    m = got["skip2-w0.2-g200"]
    assert (m.max_chn_max_skip, round(m.chn_coef_log, 4), m.max_gap) == (2, 0.2, 200)
    m = got["n6-m40-c50"]
    assert (m.min_chn_cnt, m.min_chn_sc, m.max_occ) == (6, 40, 50)
    assert (got["G2000"].max_intron, got["G2000"].bw) == (2000, 2000)
    assert (got["iter20-skip0"].max_chn_iter, got["iter20-skip0"].max_chn_max_skip) == (20, 0)
    assert got["no-pre-chain"].flag & 0x40 and got["no-splice"].flag & 0x1 and not got["default"].flag & 0x41
    assert [got["l%d" % k].kmer2 for k in seedopts.REFINE_KMERS] == seedopts.REFINE_KMERS and d.kmer2 == 5
    assert [got["ava%d" % v].max_ava for v in seedopts.MAX_AVA] == seedopts.MAX_AVA and d.max_ava == 1000
    assert (d.max_chn_max_skip, d.max_chn_iter, d.min_chn_cnt, d.min_chn_sc, d.max_occ, d.max_gap) == (25, 1000000, 3, 0, 20000, 1000)


def test_threads_do_not_change_output(oracle_built):
    case = golden.SYNTH_CASES[0]
    contigs, prots, names = golden.synth_inputs(case)
    idx = mpa.Index.from_nt4(contigs, ["chr1"])
    mpa._check(mpa.lib().mpa_idx_build_kmers(idx.h, 2))
    q = mpa.Queries(prots[:12], names[:12])
    a = map_batch(idx, golden.mapopt_for(case), q, oracle_executor, n_threads=1)
    b = map_batch(idx, golden.mapopt_for(case), q, oracle_executor, n_threads=5)
    assert a == b


def test_mapped_index_with_misaligned_sections_maps_like_the_one_in_memory(tmp_path, oracle_built):
    """mpa_idx_restore() maps the .mpi instead of reading it: genome and occurrence lists are views into the mapping, and since the
    file packs its sections back to back the 32-bit occurrence lists start at ANY byte offset (contig names of different lengths
    shift them).  Four name lengths = four alignments: every restored index must map exactly like the index it was dumped from,
    byte for byte, and dump to the same file again."""
    import hashlib
    import gen_synth
    from hostpipe import map_batch_result, oracle_executor
    contigs, prots, names = gen_synth.generate(400000, 1, 6, 61)
    q = mpa.Queries(prots, names)
    mo = mpa.default_mapopt()
    mo.flag |= 4
    seen = set()
    for nm in ("c", "ch", "chr", "chr1"):
        idx = mpa.Index.from_nt4(contigs, [nm])
        mpa._check(mpa.lib().mpa_idx_build_kmers(idx.h, 2))
        want = mpa.format_output(idx, mo, q, map_batch_result(idx, mo, q, oracle_executor))[0]
        path = str(tmp_path / ("g_%s.mpi" % nm))
        idx.dump(path)
        idx.close()
        seen.add((44 + 8 + (len(contigs[0]) + 1) // 2 + len(nm) + 1 + 8 * (1 << 23)) % 4)     # byte offset of kb[] in the file, mod 4
        back = mpa.Index.restore(path)
        got = mpa.format_output(back, mo, q, map_batch_result(back, mo, q, oracle_executor))[0]
        assert got == want and want.count(b"\n") >= len(prots), nm
        again = str(tmp_path / ("again_%s.mpi" % nm))
        back.dump(again)
        back.close()
        assert hashlib.md5(open(again, "rb").read()).hexdigest() == hashlib.md5(open(path, "rb").read()).hexdigest(), nm
    assert len(seen) == 4, "the four name lengths were meant to give four alignments of the occurrence lists"
