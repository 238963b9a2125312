#!/usr/bin/env python3
"""Regenerate tests/golden/ from the REAL reference (oracle/_ref, compiled from /root/reference by
oracle/Makefile).  Run in the authoring container only; the outputs are committed.

  * DPP3 fixture (the reference's own test data) and the reference's PAF for it (config 1)
  * reference PAF for the synthetic cases of tests/golden.py (inputs are regenerated from their seeds)
  * dp_vectors.npz: random DP calls with the reference's ns_global_gs16b() answers (all three modes)
  * dp_vectors_penalties.npz: DP calls at the scores of tests/dpgen.py's PENALTY_POINTS and BOUND_CASES (defaults up to the limits
    mpa_dp_run() accepts) with the reference's ns_global_gs16b() answers: `make_golden.py penalties` makes only these
  * gs32_vectors.npz: calls of the 32-bit operator (ns_global_gs32b, -msse4.1 build of the reference): `make_golden.py gs32` makes only these
  * chain_vectors.npz / sketch vectors: anchor sets with the reference's mp_chain() output
  * opt_<name>.ref.paf: reference PAF for golden.OPTION_CASES (one genome, index and seeding / chaining options away from the
    defaults; the index flags go to the reference with the FASTA): `make_golden.py options` makes only these
  * long_u.ref.paf: reference PAF for the long-protein case of tests/longprot.py (device refinement past the LDS k-mer map):
    `make_golden.py long` makes only this
  * regions_edge.ref.paf: reference PAF for the edge genome of tests/regioncases.py (chains across strand and contig boundaries, more
    than 64 chains of one score): `make_golden.py regions` makes only this, after checking that the host path shows all three
  * ref_layout.txt: sizes and offsets of the reference's records as its own headers declare them (tests/test_compat.py):
    `make_golden.py layout <reference source dir>` makes only this
"""
import os
import shutil
import subprocess
import sys
import tempfile
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import refbind  # noqa: E402
import golden  # noqa: E402
import gen_synth  # noqa: E402
from dpgen import make_task, make_ss, PENALTY_POINTS, BOUND_CASES, CLASS_EDGES, bound_params  # noqa: E402

GOLD = golden.GOLD
os.makedirs(GOLD, exist_ok=True)
REF = refbind.REF_BIN


def run_ref(args):
    return subprocess.run([REF, "-t4"] + args, capture_output=True, check=True).stdout


def make_gs32_vectors():
    """tests/golden/gs32_vectors.npz: calls of the 32-bit operator with the answers of the reference's ns_global_gs32b in its
    -msse4.1 build (oracle/_ref/libnasw_sse41.so; oracle/Makefile and miniprot_amd/csrc/gs32_core.h say why that build)."""
    from gs32util import gs32_cases
    rng = np.random.default_rng(3232)
    nts, aas, sss, flags, pars, mats, scores, cigs = [], [], [], [], [], [], [], []
    for nt, aa, P, flag, ss in gs32_cases(rng, 180):
        r = refbind.ref_gs32(nt, aa, P, flag, ss)
        nts.append(np.frombuffer(nt, np.uint8)), aas.append(np.frombuffer(aa, np.uint8))
        sss.append(np.frombuffer(bytes(ss), np.uint8) if ss is not None else np.zeros(0, np.uint8))
        flags.append(flag), pars.append([P.go, P.ge, P.io, P.fs] + list(P.sp)), mats.append(P.mat.copy())
        scores.append(r[2]), cigs.append(np.array(r[3], np.uint32))
    np.savez_compressed(golden.path("gs32_vectors.npz"), nt=np.concatenate(nts), nt_len=np.array([len(x) for x in nts]),
                        aa=np.concatenate(aas), aa_len=np.array([len(x) for x in aas]), ss=np.concatenate(sss), ss_len=np.array([len(x) for x in sss]),
                        flag=np.array(flags), par=np.array(pars, np.int64), mat=np.array(mats, np.int8), score=np.array(scores, np.int64),
                        cig=np.concatenate(cigs), cig_len=np.array([len(x) for x in cigs]))
    print("gs32_vectors", len(flags), "calls,", sum(1 for x in scores if x > 32767), "with scores beyond int16")


def make_penalty_vectors():
    """tests/golden/dp_vectors_penalties.npz: per scoring point (PENALTY_POINTS, then both sides of every BOUND_CASES entry) two calls at
    kernel class edges (for a bound case one call at the bound's own al) in all three modes and a window of >= 384 rows in global mode,
    some with ss[]"""
    rng = np.random.default_rng(3131)
    points = [(kw, None) for kw in PENALTY_POINTS] + [(bound_params(c, over), c[0]) for c in BOUND_CASES for over in (0, 1)]
    nts, aas, sss, pair, flags, pars, coefs, mats, res, cigs = [], [], [], [], [], [], [], [], [], []
    for kw, al in points:
        P = refbind.DpParams(refbind.mapping_matrix(min(kw.get("fs", 23), 127)), **kw)
        edges = [al] if al else [int(rng.choice(CLASS_EDGES[:11])) for _ in range(2)]
        calls = [(make_task(rng, al=a, p_intron=0.02, max_intron=200, flank=100, p_indel=0.0), (1, 2, 4)) for a in edges]
        while True:                                        # (a window of 384..480 rows: long enough for the checkpointed sweep, and small)
            lw = make_task(rng, al=int(rng.integers(1, 129)), max_intron=300, flank=250, p_intron=0.05)
            if 384 <= len(lw[0]) <= 480:
                break
        for (nt, aa), modes in calls + [(lw, (1,))]:
            ss = make_ss(rng, len(nt)) if rng.random() < 0.25 else None
            nts.append(np.frombuffer(nt, np.uint8)), aas.append(np.frombuffer(aa, np.uint8))
            sss.append(np.frombuffer(ss, np.uint8) if ss is not None else np.zeros(0, np.uint8))
            for fl in modes:
                r = refbind.ref_nasw(nt, aa, P, fl, ss)
                pair.append(len(nts) - 1), flags.append(fl), pars.append([P.go, P.ge, P.io, P.fs, P.xdrop, P.end_bonus] + list(P.sp)), coefs.append(P.ie_coef), mats.append(P.mat.copy())
                res.append(r[:3]), cigs.append(np.array(r[3], np.uint32))
    np.savez_compressed(golden.path("dp_vectors_penalties.npz"), nt=np.concatenate(nts), nt_len=np.array([len(x) for x in nts]),
                        aa=np.concatenate(aas), aa_len=np.array([len(x) for x in aas]), ss=np.concatenate(sss), ss_len=np.array([len(x) for x in sss]),
                        pair=np.array(pair), flag=np.array(flags), par=np.array(pars, np.int64), ie_coef=np.array(coefs, np.float32), mat=np.array(mats, np.int8),
                        res=np.array(res, np.int64), cig=np.concatenate(cigs), cig_len=np.array([len(x) for x in cigs]))
    print("dp_vectors_penalties", len(flags), "calls")


def make_layout(ref_dir):
    """tests/golden/ref_layout.txt: what test_compat's layout probe prints when compiled against the reference's own headers"""
    import test_compat
    with tempfile.TemporaryDirectory() as tmp:
        src, exe = os.path.join(tmp, "layout.c"), os.path.join(tmp, "layout")
        open(src, "w").write(test_compat.LAYOUT_PROG)
        subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I" + ref_dir, src, "-o", exe], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    open(golden.path("ref_layout.txt"), "w").write(out)
    print("ref_layout", out.count("\n"), "lines")


def make_option_cases():
    """tests/golden/opt_<name>.ref.paf: the reference's output for golden.OPTION_CASES"""
    with tempfile.TemporaryDirectory() as tmp:
        for case in golden.OPTION_CASES:
            contigs, prots, names = golden.synth_inputs(case)
            fa, faa = os.path.join(tmp, "g.fa"), os.path.join(tmp, "p.fa")
            gen_synth.write_fasta_nt(fa, contigs)
            gen_synth.write_fasta_aa(faa, prots, names)
            out = run_ref(case["flags"] + [fa, faa])
            open(golden.path(case["name"] + ".ref.paf"), "wb").write(out)
            print(case["name"], len(out), "bytes", out.count(b"\n"), "lines,", sum(1 for l in out.split(b"\n") if l and l.split(b"\t")[5] != b"*"), "mapped")


def make_long_case():
    """tests/golden/long_u.ref.paf: the reference's output for tests/longprot.py's case"""
    import longprot
    c = longprot.case()
    with tempfile.TemporaryDirectory() as tmp:
        fa, faa = os.path.join(tmp, "g.fa"), os.path.join(tmp, "p.fa")
        gen_synth.write_fasta_nt(fa, c["contigs"])
        gen_synth.write_fasta_aa(faa, c["prots"], c["names"])
        out = run_ref(longprot.FLAGS + [fa, faa])
    open(golden.path("long_u.ref.paf"), "wb").write(out)
    print("long_u", len(out), "bytes", out.count(b"\n"), "lines")


def make_regions_edge():
    """tests/golden/regions_edge.ref.paf: the reference's output for the edge genome of tests/regioncases.py.  The genome is only
    worth a fixture if the host path meets on it what the tests assert first: the split flag in both directions, a query with more
    than 64 chains before the selection, and more than 64 kept regions of one chn_sc"""
    import miniprot_amd as mpa
    import regioncases
    import regionsdump
    from hostpipe import map_batch_result, oracle_executor
    contigs, prots, names, mo = regioncases.edge_genome()
    with tempfile.TemporaryDirectory() as tmp:
        dump = os.path.join(tmp, "regions.dump")
        os.environ.pop("MPA_GPU_REGIONS", None)
        os.environ["MPA_REGIONS_DUMP"] = dump
        idx, q = regioncases.edge_index(contigs), mpa.Queries(prots, names)
        ours = mpa.format_output(idx, mo, q, map_batch_result(idx, mo, q, oracle_executor, 4))[0]
        del os.environ["MPA_REGIONS_DUMP"]
        flags, most, ties = regioncases.edge_findings(regionsdump.read(dump))
        assert flags == {1, 2} and most > 64 and ties > 64, (flags, most, ties)
        fa, faa = os.path.join(tmp, "g.fa"), os.path.join(tmp, "p.fa")
        gen_synth.write_fasta_nt(fa, contigs)
        gen_synth.write_fasta_aa(faa, prots, names)
        out = run_ref(regioncases.EDGE_FLAGS + [fa, faa])
    assert ours == out, "the host path with the oracle executor does not print the reference's bytes for the edge genome"
    open(golden.path(regioncases.EDGE_REF), "wb").write(out)
    print("regions_edge", len(out), "bytes", out.count(b"\n"), "lines; split flags", sorted(flags), "chains", most, "equal scores", ties)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "regions":
        make_regions_edge()
        return
    if len(sys.argv) > 1 and sys.argv[1] == "options":
        make_option_cases()
        return
    if len(sys.argv) > 1 and sys.argv[1] == "long":
        make_long_case()
        return
    if len(sys.argv) > 2 and sys.argv[1] == "layout":
        make_layout(sys.argv[2])
        return
    refbind.build_oracle()
    if len(sys.argv) > 1 and sys.argv[1] == "gs32":
        make_gs32_vectors()
        return
    if len(sys.argv) > 1 and sys.argv[1] == "penalties":
        make_penalty_vectors()
        return
    # config 1
    for f in ("DPP3-hs.gen.fa.gz", "DPP3-mm.pep.fa.gz"):
        shutil.copy(os.path.join("/root/reference/test", f), os.path.join(GOLD, f))
    open(os.path.join(GOLD, "dpp3.ref.paf"), "wb").write(run_ref([golden.path("DPP3-hs.gen.fa.gz"), golden.path("DPP3-mm.pep.fa.gz")]))
    # synthetic cases
    with tempfile.TemporaryDirectory() as tmp:
        for case in golden.SYNTH_CASES:
            contigs, prots, names = golden.synth_inputs(case)
            fa, faa = os.path.join(tmp, "g.fa"), os.path.join(tmp, "p.fa")
            gen_synth.write_fasta_nt(fa, contigs)
            gen_synth.write_fasta_aa(faa, prots, names)
            extra = ["--spsc=" + golden.write_spsc(case, contigs, os.path.join(tmp, "spsc.tsv"))] if "spsc" in case else []
            out = run_ref(case["flags"] + extra + [fa, faa])
            open(golden.path(case["name"] + ".ref.paf"), "wb").write(out)
            print(case["name"], len(out), "bytes", out.count(b"\n"), "lines")
    # DP vectors
    rng = np.random.default_rng(2024)
    P = refbind.DpParams(refbind.mapping_matrix(23))
    nts, aas, flags, ios, res, cigs = [], [], [], [], [], []
    for k in range(300):
        nt, aa = make_task(rng)
        for fl in (1, 2, 4):
            io = 29 if fl == 1 or rng.random() < 0.7 else 19
            PP = refbind.DpParams(P.mat, io=io)
            r = refbind.ref_nasw(nt, aa, PP, fl)
            nts.append(np.frombuffer(nt, np.uint8)), aas.append(np.frombuffer(aa, np.uint8)), flags.append(fl), ios.append(io)
            res.append(r[:3]), cigs.append(np.array(r[3], np.uint32))
    np.savez_compressed(golden.path("dp_vectors.npz"), nt=np.concatenate(nts), nt_len=np.array([len(x) for x in nts]),
                        aa=np.concatenate(aas), aa_len=np.array([len(x) for x in aas]), flag=np.array(flags), io=np.array(ios),
                        res=np.array(res, np.int64), cig=np.concatenate(cigs), cig_len=np.array([len(x) for x in cigs]), mat=P.mat)
    print("dp_vectors", len(flags))
    make_gs32_vectors()
    make_penalty_vectors()
    make_option_cases()
    make_long_case()
    make_regions_edge()


if __name__ == "__main__":
    main()
