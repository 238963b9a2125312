"""MPA_GPU_FORMAT on the device: the output text of a flat result by k_format_size, k_format_scan and k_format_write of format_kernels.hip
(the code is format_core.h, which tests/test_format_cpu.py pins against the host formatter on the CPU).  All
comparisons are byte for byte.

1. mpa_dbg_format on a context against the shared core on the host (ctx == NULL) on every hand-made table of tests/formatcases.py and
   every id0 of formatcases.ID0S; mpa_dbg_format_last reports one host wait, the printed hits and the text's real byte count.
2. Results of real batches (MPA_GPU_STATS / CS / ROWS / FINISH = 1, so that the hits carry their cs bodies and rows): the device's text is
   the golden text and mpa_format_output()'s, with ids that run on from an id0.
3. Declines: a result whose hits do not carry the cs bodies the options print says so and gives the host formatter's bytes.
4. MPA_GPU_FORMAT=1, the whole path: mpa_map_batches with names writes a batch's text behind the finish step of the DP lane's last device
   call -- the golden text and the knob-unset run's, one note, no decline, one host wait for walks, finish and format together; ids that
   run across the batches of a stream; the width edge of the id; the declines and their notes; -A stays silent."""
import os
import re
import pytest
import miniprot_amd as mpa
import alnstats
import formatcases

pytestmark = pytest.mark.gpu

TABLES = [t["name"] for t in formatcases.tables()]
WALKS_FINISH = {"MPA_GPU_STATS": "1", "MPA_GPU_CS": "1", "MPA_GPU_ROWS": "1", "MPA_GPU_FINISH": "1"}
EVERY = dict(WALKS_FINISH, MPA_GPU_SEED="1", MPA_GPU_SKETCH="1", MPA_GPU_REGIONS="1", MPA_GPU_REFINE="1", MPA_GPU_PLANS="1", MPA_GPU_DPPLAN="1", MPA_GPU_SPANS="1", MPA_GPU_ROUND2="1")
KNOBS = sorted(set(EVERY) | {"MPA_GPU_FORMAT", "MPA_TIMING", "MPA_DP_LANES"})
GPU_NOTE = re.compile(r"format on the GPU: (\d+) queries, (\d+) hits printed, (\d+) bytes down, (\d+) id fields")


@pytest.fixture(scope="module")
def ctx():
    c = mpa.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("k", range(len(TABLES)), ids=TABLES)
def test_device_equals_the_shared_core_on_every_table(ctx, k):
    t = formatcases.tables()[k]
    idx, mo, q, res = formatcases.objects(t)
    try:
        for id0 in formatcases.ID0S:
            want, n_want, declined_want = mpa.dbg_format(None, idx, mo, q, res, id0)
            got, n, declined = mpa.dbg_format(ctx, idx, mo, q, res, id0)
            assert got == want, "%s, id0 %d: first difference at byte %d" % (t["name"], id0, next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), min(len(got), len(want))))
            assert n == n_want == formatcases.n_printed_expected(t) and declined == declined_want
            n_q, n_out, n_bytes, n_ids, waits, dev_declined = mpa.dbg_format_last(ctx)
            assert (n_q, n_out, waits, dev_declined) == (len(t["qlens"]), n, 1, 0)
            if not declined:
                assert n_bytes == len(got)                    # (the kernels wrote the text at its real size)
    finally:
        res.close()
        idx.close()


def _map(ctx, idx, mo, q, env):
    keep = {k: os.environ.get(k) for k in KNOBS}
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update(env)
    try:
        return mpa.map_batch(ctx, idx, mo, q, 4)
    finally:
        for k, v in keep.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


@pytest.mark.parametrize("name", ["syn_a", "syn_e", "syn_f", "syn_g", "syn_k", "syn_m"])
def test_results_of_real_batches(ctx, name, tmp_path):
    idx, mo, q, ref = alnstats.case_inputs(name, tmp_path)
    idx.to_device(ctx)
    res = _map(ctx, idx, mo, q, WALKS_FINISH)
    try:
        got, n, declined = mpa.dbg_format(ctx, idx, mo, q, res, 0)
        assert not declined and got == ref and n == res.n_output(mo, q)
        last = mpa.dbg_format_last(ctx)
        assert (last[0], last[1], last[2], last[4], last[5]) == (len(q.seqs), n, len(ref), 1, 0)
        for id0 in (41, 999990):
            want, id_after = mpa.format_output(idx, mo, q, res, id0)
            got, n, declined = mpa.dbg_format(ctx, idx, mo, q, res, id0)
            assert got == want and id_after == id0 + n
    finally:
        res.close()
        idx.close()


def test_hits_that_do_not_carry_their_cs_bodies_decline_and_say_so(ctx, tmp_path, capfd, monkeypatch):
    idx, mo, q, ref = alnstats.case_inputs("syn_a", tmp_path)
    idx.to_device(ctx)
    res = _map(ctx, idx, mo, q, {})
    monkeypatch.setenv("MPA_TIMING", "1")
    capfd.readouterr()
    got, n, declined = mpa.dbg_format(ctx, idx, mo, q, res, 0)
    err = capfd.readouterr().err
    res.close()
    idx.close()
    assert declined and "format declined (a blen of 0, or a cs string or rows that a hit does not carry)" in err
    assert got == ref and mpa.dbg_format_last(ctx)[5] == 1


# ---- 4. MPA_GPU_FORMAT=1: the stage inside a batch's own device call
def _stream(ctx, idx, mo, batches, env, capfd, id0=0):
    """mpa_map_batches with names under `env` (every other knob of this file unset): (texts, stderr, printed hits per batch)"""
    keep = {k: os.environ.get(k) for k in KNOBS}
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update(dict(env, MPA_TIMING="1"))
    try:
        capfd.readouterr()
        texts, results = mpa.map_batches(ctx, idx, mo, batches, 4, keep_results=True, id0=id0)
        err = capfd.readouterr().err
        n_out = [r.n_output(mo, b) for r, b in zip(results, batches)]
        for r in results:
            r.close()
    finally:
        for k, v in keep.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v
    return texts, err, n_out


@pytest.mark.parametrize("name", ["syn_a", "syn_d", "syn_e", "syn_f", "syn_g", "syn_k", "syn_m"])
@pytest.mark.parametrize("knobs", [WALKS_FINISH, EVERY], ids=["walks_finish", "every"])
def test_whole_path_writes_the_golden_text_on_the_device(ctx, name, knobs, capfd, tmp_path):
    idx, mo, q, ref = alnstats.case_inputs(name, tmp_path)
    idx.to_device(ctx)
    knobs = dict(knobs, MPA_DP_LANES="1")                 # (one DP lane: the caller's own context runs the batch, and its records can be read)
    off = _stream(ctx, idx, mo, [q], knobs, capfd)
    on = _stream(ctx, idx, mo, [q], dict(knobs, MPA_GPU_FORMAT="1"), capfd)
    last_fmt, last_fin = mpa.dbg_format_last(ctx), mpa.dbg_finish_last(ctx)
    idx.close()
    assert "format on the GPU" not in off[1] and "format declined" not in off[1]
    m = GPU_NOTE.findall(on[1])
    assert len(m) == 1, "MPA_GPU_FORMAT=1 did not write the text on the device:\n" + "\n".join(l for l in on[1].split("\n") if "format" in l)
    assert "format declined" not in on[1]
    assert off[0][0] == ref and on[0][0] == ref
    assert (int(m[0][0]), int(m[0][1]), int(m[0][2])) == (len(q.seqs), on[2][0], len(ref)) and on[2] == off[2]
    # ONE host wait for walks, finish and format together
    assert last_fmt[:3] == (len(q.seqs), on[2][0], len(ref)) and last_fmt[4] == 1 and last_fmt[5] == 0 and last_fin[5] == 1


def _thirds(q):
    n = len(q.seqs)
    return [mpa.Queries(q.seqs[a:b], q.names[a:b]) for a, b in ((0, n // 3), (n // 3, 2 * n // 3), (2 * n // 3, n))]


def test_ids_run_across_the_batches_of_a_stream(ctx, capfd, tmp_path):
    idx, mo, q, ref = alnstats.case_inputs("syn_e", tmp_path)              # -u --gff
    idx.to_device(ctx)
    texts, err, n_out = _stream(ctx, idx, mo, _thirds(q), dict(WALKS_FINISH, MPA_GPU_FORMAT="1"), capfd)
    idx.close()
    assert b"".join(texts) == ref
    m = GPU_NOTE.findall(err)
    assert len(m) == 3 and "format declined" not in err and sorted(int(x[1]) for x in m) == sorted(n_out) and all(int(x[3]) > 0 for x in m)


def test_the_batch_that_crosses_the_ids_width_edge_declines_and_the_next_ones_too(ctx, capfd, tmp_path):
    idx, mo, q, ref = alnstats.case_inputs("syn_e", tmp_path)
    idx.to_device(ctx)
    off = _stream(ctx, idx, mo, _thirds(q), WALKS_FINISH, capfd, id0=999990)
    on = _stream(ctx, idx, mo, _thirds(q), dict(WALKS_FINISH, MPA_GPU_FORMAT="1"), capfd, id0=999990)
    idx.close()
    assert on[0] == off[0] and b"ID=MP1000000;" in b"".join(on[0])
    crossing = [k for k in range(3) if 999990 + sum(on[2][:k + 1]) > 999999]
    assert crossing and on[1].count("format declined (ids reach seven digits)") == len(crossing)
    assert len(GPU_NOTE.findall(on[1])) == 3 - len(crossing)


@pytest.mark.parametrize("name,knobs,why", [("syn_a", {"MPA_GPU_STATS": "1", "MPA_GPU_CS": "1", "MPA_GPU_ROWS": "1"}, "the finish step does not run on the device"),
                                            ("syn_a", {}, "the finish step does not run on the device"),
                                            ("syn_k", {"MPA_GPU_STATS": "1", "MPA_GPU_CS": "1", "MPA_GPU_FINISH": "1"}, "residue rows are printed and MPA_GPU_ROWS is not 1"),
                                            ("syn_a", {"MPA_GPU_STATS": "1", "MPA_GPU_FINISH": "1"}, "cs strings are printed and MPA_GPU_CS is not 1")],
                         ids=["no_finish", "no_knob_at_all", "aln_without_rows", "cs_without_cs"])
def test_declines_and_says_so(ctx, name, knobs, why, capfd, tmp_path):
    idx, mo, q, ref = alnstats.case_inputs(name, tmp_path)
    idx.to_device(ctx)
    texts, err, _ = _stream(ctx, idx, mo, [q], dict(knobs, MPA_GPU_FORMAT="1"), capfd)
    idx.close()
    assert texts[0] == ref
    assert "format declined (%s)" % why in err and not GPU_NOTE.findall(err)


def test_no_align_stays_silent(ctx, capfd, tmp_path):
    idx, mo, q, ref = alnstats.case_inputs("syn_i", tmp_path)              # -A -u
    idx.to_device(ctx)
    texts, err, _ = _stream(ctx, idx, mo, [q], dict(WALKS_FINISH, MPA_GPU_FORMAT="1"), capfd)
    idx.close()
    assert texts[0] == ref
    assert "format declined" not in err and "format on the GPU" not in err


def test_map_batch_and_format_output_keep_the_host_formatter_silently(ctx, capfd, tmp_path):
    idx, mo, q, ref = alnstats.case_inputs("syn_e", tmp_path)
    idx.to_device(ctx)
    res = _map(ctx, idx, mo, q, dict(WALKS_FINISH, MPA_GPU_FORMAT="1", MPA_TIMING="1"))
    os.environ["MPA_GPU_FORMAT"] = "1"
    try:
        capfd.readouterr()
        text = mpa.format_output(idx, mo, q, res)[0]
        err = capfd.readouterr().err
    finally:
        os.environ.pop("MPA_GPU_FORMAT", None)
    res.close()
    idx.close()
    assert text == ref and "format declined" not in err and "format on the GPU" not in err
