"""The whole-path case of tests/test_ckpt_w8_gpu.py: golden option case opt_l7 (tests/golden.py; -l 7 -u), the committed case whose mapping
issues the most traceback calls of 257..512 columns -- two of them, about five million padded cells, counted through the statistics
with MPA_DP_LITE_MIN=3 MPA_DP_LITE_W8=1 (opt_l6 and opt_L36k5M0l6 issue one each, no other golden or option case any; the two cases with
a splice-score file, syn_n and syn_o, were not counted).  The expected
bytes are the committed reference output tests/golden/opt_l7.ref.paf."""
import tempfile
import miniprot_amd as mpa
import golden
import seedopts

CASE = "opt_l7"


def inputs():
    """-> (index with its k-mer table built on the host, mapping options, queries, what the reference prints in front of the first batch,
    the reference's bytes)"""
    case = [c for c in golden.OPTION_CASES if c["name"] == CASE][0]
    contigs, prots, names = golden.synth_inputs(case)
    with tempfile.TemporaryDirectory() as d:
        idx = mpa.Index.read_fasta(seedopts.write_genome(d, contigs), case["idx"])
    mpa._check(mpa.lib().mpa_idx_build_kmers(idx.h, 4))
    with open(golden.path(CASE + ".ref.paf"), "rb") as f:
        ref = f.read()
    return idx, golden.mapopt_for(case), mpa.Queries(prots, names), golden.file_header(case), ref
