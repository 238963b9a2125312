"""k_chain_extract -- the device instance of chain_extract_core (chain_core.h), whose 64-lane team code the host never runs -- on the
synthetic anchors of tests/chaincases.py, through mpa_dbg_chain_extract on a context: forward pass on the device, then the product's own
carving, status memset and launch.  The chains must equal the oracle's mp_chain bit for bit; status and path records must equal the host
hook's.  tests/test_chain_extract_cpu.py asserts, without a device, that the cases reach every branch they are built for (the rounds of
place_in_order, walk_buckets, the team merge, the LDS staging of a level-1 bucket, the tree-ownership protocol, coop_compact, the decline).
No genome and no index anywhere in this file; a launch holds many problems."""
import numpy as np
import pytest
import miniprot_amd as mpa
import chaincases as cc
import refbind

pytestmark = pytest.mark.gpu

GROUPS = {
    "a-b-c": ("a_n_total", "b_ends", "c_trees"),
    "d-e-f": ("d_bulk_ties", "e_two_levels_small", "f_short_bucket0"),
    "e-g": ("e_two_levels_3000", "e_two_levels_20000", "g_level1_bucket"),
    "e-moved": ("e_moved_lows",),
    "h-i": ("h_max_f", "i_min_cnt_sparse", "i_min_sc_sparse"),
    "i-dense": ("i_dense_params",),
    "j-k-l": ("j_max_drop", "k_refine", "l_mix_chains", "l_mix_prechain"),
}
_host = {}


@pytest.fixture(scope="module")
def ctx():
    c = mpa.Context(0)
    yield c
    c.close()


def host_run(c, args, mode):
    key = (c["name"], tuple(args), mode)
    if key not in _host:
        _host[key] = mpa.dbg_chain_extract(None, list(args), c["probs"], mode)
    return _host[key]


def device_run(ctx, c, args, mode):
    """one launch on the device: against the oracle, and status / path records against the host hook's"""
    got = mpa.dbg_chain_extract(ctx, list(args), c["probs"], mode)
    n = cc.check_against(c, args, mode, got, cc.expected(c, args), "device")
    ref = host_run(c, args, mode)
    assert np.array_equal(got[2], ref[2]), ("status", c["name"], list(args), mode, np.flatnonzero(got[2] != ref[2])[:8])
    assert np.array_equal(got[3], ref[3]), ("path records", c["name"], list(args), mode, np.flatnonzero((got[3] != ref[3]).any(axis=1))[:8])
    return got, n


@pytest.mark.parametrize("serial_run", ["48", "4"])
@pytest.mark.parametrize("group", list(GROUPS))
def test_device_extraction_equals_the_oracle(group, serial_run, ctx, oracle_built, monkeypatch):
    # serial_run: the forward pass walks runs longer than this with a wavefront (k_chain_fwd_wave); 4 sends almost every run there
    monkeypatch.setenv("MPA_CHAIN_SERIAL_RUN", serial_run)
    launches = 0
    for name in GROUPS[group]:
        c = cc.case(name)
        for args, modes in c["runs"]:
            for mode in modes:
                _, n = device_run(ctx, c, args, mode)
                assert n >= len(c["probs"]) - 8
                launches += 1
    assert launches <= 16


def test_every_case_runs_in_a_group():
    assert sorted(n for g in GROUPS.values() for n in g) == sorted(c["name"] for c in cc.cases())


def test_scratch_pool_is_reused_as_it_was_left(ctx, oracle_built):
    """the chaining pool of a context is carved anew for every launch and never zeroed (as SeedBufs::x_all in the product): a large launch,
    then smaller ones over what it left behind -- mark / owner / kept / the digit tables of other problems -- and the whole sequence again"""
    seq = [("e_two_levels_20000", cc.PRE, cc.SPARSE_SET), ("g_level1_bucket", cc.MAIN, cc.SPARSE_CHAINS), ("c_trees", cc.PRE, cc.SPARSE_SET),
           ("a_n_total", cc.MAIN, cc.DENSE), ("h_max_f", cc.PRE, cc.SPARSE_CHAINS), ("b_ends", cc.PRE, cc.SPARSE_CHAINS)]
    first, cap = None, 0
    for rep in range(2):
        outs = []
        for k, (name, args, mode) in enumerate(seq):
            got, _ = device_run(ctx, cc.case(name), tuple(args), mode)
            outs.append(got)
            if k == 0:
                now = dict(mpa.dbg_ctx_pools(ctx))["x_all"]
                assert now > 0 and (rep == 0 or now == cap)        # the second pass works in the very block the first one left
                cap = now
            else:
                assert dict(mpa.dbg_ctx_pools(ctx))["x_all"] == cap   # the smaller launches do not move it
        if first is None:
            first = outs
        else:
            for a, b in zip(first, outs):
                assert all(np.array_equal(x, y) for x, y in zip(a[0], b[0])) and all(np.array_equal(x, y) for x, y in zip(a[1], b[1]))


def test_device_chains_equal_the_reference_mp_chain(ctx, oracle_built):
    """families (c), (d), (e) and (g) against the reference's own mp_chain where it has been built (otherwise that leg is left out and the
    oracle alone stands): contended trees, bulk ties, two digit levels, the level-1 bucket at the LDS staging's capacity"""
    n_ref = 0
    for name in ("c_trees", "d_bulk_ties", "e_two_levels_small", "e_moved_lows", "g_level1_bucket"):
        c = cc.case(name)
        for args, mode in ((tuple(cc.PRE), cc.SPARSE_CHAINS), (tuple(cc.MAIN), cc.DENSE)):
            (us, as_, status, rec), _ = device_run(ctx, c, args, mode)
            if not refbind.have_ref():
                continue
            for q, p in enumerate(c["probs"]):
                ru, ra = refbind.ref_chain(p, args)
                assert np.array_equal(us[q], ru) and np.array_equal(as_[q], ra), ("reference", name, q, c["tags"][q], list(args), mode)
                n_ref += len(ru)
    assert n_ref > 1000 or not refbind.have_ref()
