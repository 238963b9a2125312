"""Ranking and flat result of a batch through the code the device runs (miniprot_amd/csrc/finish_core.h), on
the CPU.

1. mpa_dbg_finish(NULL, ...) -- the shared core with a team of one -- on the generated tables of tests/finishcases.py against the
   REFERENCE ITSELF: mp_sort_reg, mp_select_multi_exon, mp_set_parent and mp_select_sub of oracle/_ref/libminiprot_ref.so, called through
   tests/finish_ref_shim.c.  Order, id, parent, n_sub, subsc, dp_max2 and which regions survive come from there; the layout of the flat
   arrays around them is restated in numpy (finishcases.expected_flat) and compared byte for byte.
2. MPA_GPU_FINISH=model through the stage machine with the oracle as DP executor: the text is the golden text, the result's flat arrays
   are those of the run with the knob unset, byte for byte, and the model's note is printed with the knob and only then."""
import os
import subprocess
import pytest
import numpy as np
import miniprot_amd as mpa
import refbind
import alnstats
import finishcases
import golden
from hostpipe import map_batch_result, oracle_executor

MODEL_NOTE = "finish: shared core"
needs_ref = pytest.mark.skipif(not refbind.have_ref(), reason="oracle/_ref/libminiprot_ref.so not built")


@pytest.fixture(scope="module")
def shim_dir(tmp_path_factory):
    return tmp_path_factory.mktemp("finish_shim")


@needs_ref
@pytest.mark.parametrize("k", range(len(finishcases.tables())), ids=[t["name"] for t in finishcases.tables()])
def test_shared_core_ranks_as_the_reference_and_lays_out_as_the_host(k, shim_dir):
    t = finishcases.tables()[k]
    ranks = finishcases.reference_ranks(t, shim_dir)      # (asserts first that the reference accepts every query's table)
    got = finishcases.run(None, t)
    hits = np.frombuffer(got["hits"], finishcases.HIT)
    off = np.frombuffer(got["hit_off"], np.int64)
    assert len(off) == len(ranks) + 1 and off[0] == 0 and off[-1] == len(hits)
    for q, rk in enumerate(ranks):                        # the ranking first, query by query, so that a failure names the field
        mine = hits[off[q]:off[q + 1]]
        assert len(mine) == len(rk), "%s query %d: %d regions survive, the reference keeps %d" % (t["name"], q, len(mine), len(rk))
        src = mine["dp_score"] - t["first"][q]
        for col, f in enumerate(("src", "id", "parent", "n_sub", "subsc", "dp_max2")):
            a = src if f == "src" else mine[f]
            assert (a == rk[:, col]).all(), "%s query %d: %s %s, the reference has %s" % (t["name"], q, f, a.tolist(), rk[:, col].tolist())
    d = finishcases.first_difference(got, finishcases.expected_flat(t, ranks))
    assert d is None, "%s: %s" % (t["name"], d)


@needs_ref
def test_tables_cover_what_the_ranking_distinguishes(shim_dir):
    """the generator's promises, read off the reference's answers: drops, swaps, secondaries of a later primary, squeezed-out entries"""
    seen = dict(dropped=0, secondary=0, second_primary=0, swapped=0, squeezed=0, big=0, empty=0, n_sub=0, dp_max2=0)
    for t in finishcases.tables():
        ranks = finishcases.reference_ranks(t, shim_dir)
        for q, rk in enumerate(ranks):
            r = t["recs"][t["first"][q]:t["first"][q + 1]]
            n = len(r)
            seen["big"] += n > 256
            seen["empty"] += n == 0
            seen["squeezed"] += n > 1 and bool((r["cnt"] <= 0).any())
            if not len(rk):
                continue
            seen["dropped"] += len(rk) < n - int((r["cnt"] <= 0).sum())
            seen["secondary"] += bool((rk[:, 2] != rk[:, 1]).any())
            seen["second_primary"] += bool(((rk[:, 2] != rk[:, 1]) & (rk[:, 2] > 0)).any())
            seen["swapped"] += n > 1 and r["dp_max"][rk[0, 0]] < r["dp_max"][rk[:, 0]].max()
            seen["n_sub"] += bool((rk[:, 3] > 0).any())
            seen["dp_max2"] += bool((rk[:, 5] > 0).any())
    assert all(v > 0 for v in seen.values()), seen


def test_the_hook_refuses_records_that_point_outside_their_arrays():
    t = dict(finishcases.tables()[1])
    recs = t["recs"].copy()
    recs["cig_off"][0] = len(t["words"])
    t["recs"] = recs
    with pytest.raises(mpa.MpaError):
        finishcases.run(None, t)


def test_core_against_plain_restatements_under_sanitizers(tmp_path):
    """tests/finish_check.cpp: the generator's kinds of cases written out in C++ (sizes around 64 / 65 and 257 / 300, equal scores and
    equal full keys, negative scores, the multi-exon swap at its edge, a region secondary to the second of two overlapping primaries,
    uncovered at mask_len and one above, the identical hit after DP, gaps at sub_diff and min_diff, best_n of 0, 1 and reached, one place
    twice, soft-deleted entries, the gather's lengths with cs bodies and rows present, absent and mixed) and 400 random tables; a team of
    one and a team of 64 threads, output arrays of exactly the result's size"""
    root = refbind.ROOT
    exe = str(tmp_path / "finish_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                    "-I" + os.path.join(root, "miniprot_amd", "csrc"), os.path.join(root, "tests", "finish_check.cpp"), "-o", exe, "-lpthread"], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "0 mismatches" in out.stdout and "ERROR" not in out.stderr


# ---- the whole path
def _memo(executor):
    seen = {}

    def run(idx, queries, dpopt, tasks):
        key = tasks.tobytes()
        if key not in seen:
            seen[key] = executor(idx, queries, dpopt, tasks)
        return seen[key]
    return run


def _run(idx, mo, q, ex, env, monkeypatch, capfd):
    """one batch through the stage machine and the formatter: (text, stderr, flat arrays)"""
    monkeypatch.setenv("MPA_TIMING", "1")
    for k in ("MPA_GPU_FINISH", "MPA_GPU_STATS", "MPA_GPU_CS", "MPA_GPU_ROWS", "MPA_GPU_SPANS"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    capfd.readouterr()
    res = map_batch_result(idx, mo, q, ex, n_threads=4)
    flat = mpa.result_flat(res)
    text = mpa.format_output(idx, mo, q, res)[0]
    return text, capfd.readouterr().err, flat


def _edge():
    import regioncases
    contigs, prots, names, mo = regioncases.edge_genome()
    return regioncases.edge_index(contigs), mo, mpa.Queries(prots, names), open(golden.path(regioncases.EDGE_REF), "rb").read()


WALK_MODELS = {"MPA_GPU_STATS": "model", "MPA_GPU_CS": "model", "MPA_GPU_ROWS": "model"}


@pytest.mark.parametrize("name,others", [("syn_a", {}), ("syn_d", {}), ("syn_k", {}), ("syn_m", {}), ("syn_m", WALK_MODELS), ("edge", {}), ("edge", WALK_MODELS)],
                         ids=["syn_a", "syn_d", "syn_k", "syn_m", "syn_m_models", "edge", "edge_models"])
def test_model_prints_the_golden_text_and_the_hosts_flat_arrays(oracle_built, name, others, tmp_path, monkeypatch, capfd):
    idx, mo, q, ref = _edge() if name == "edge" else alnstats.case_inputs(name, tmp_path)
    ex = _memo(oracle_executor)
    t_host, err_host, f_host = _run(idx, mo, q, ex, others, monkeypatch, capfd)
    t_model, err_model, f_model = _run(idx, mo, q, ex, dict(others, MPA_GPU_FINISH="model"), monkeypatch, capfd)
    idx.close()
    assert MODEL_NOTE in err_model, "MPA_GPU_FINISH=model did not run the shared core"
    assert "finish" not in err_host.replace("take 2 + finish", "").replace("batch_finish", "")
    assert "declined" not in err_model
    assert t_host == ref and t_model == ref
    assert len(f_host["hits"]) > 0
    if others:
        assert len(f_host["cs"]) > 0                      # (the cs bodies came with the hits in both runs)
    d = finishcases.first_difference(f_model, f_host)
    assert d is None, d


def test_cs_dump_holds_the_same_bytes_behind_the_model(oracle_built, tmp_path, monkeypatch, capfd):
    idx, mo, q, ref = alnstats.case_inputs("syn_a", tmp_path)
    ex = _memo(oracle_executor)
    dumps = []
    for knob, cs in ((None, None), ("model", None), (None, "model"), ("model", "model")):
        fn = tmp_path / ("cs_%s_%s.bin" % (knob, cs))
        env = {"MPA_CS_DUMP": str(fn)}
        if knob:
            env["MPA_GPU_FINISH"] = knob
        if cs:
            env["MPA_GPU_CS"] = cs
        _run(idx, mo, q, ex, env, monkeypatch, capfd)
        monkeypatch.delenv("MPA_CS_DUMP")
        dumps.append(open(str(fn), "rb").read())
    idx.close()
    assert len(dumps[0]) > 0 and dumps[1] == dumps[0] and dumps[3] == dumps[2]
