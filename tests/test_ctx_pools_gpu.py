"""The device pools of a context register themselves (dev_ctx.h: CtxPool) and free and count themselves: what
mpa_dbg_ctx_pools lists is what the context holds, and what it holds is what mpa_device_bytes() loses when the context goes.

One child process (mpa_device_bytes() is process-wide, and other tests of this process may hold contexts) maps the DPP3 golden pair as
a stream of three batches with every device step forced on and --aln --trans output (cs strings included), so that pools of every stage exist, and
prints what the hook and the counter said; the tests below judge that record."""
import json
import os
import subprocess
import sys
import pytest

pytestmark = pytest.mark.gpu

EVERY_STEP = ("MPA_GPU_SEED", "MPA_GPU_SKETCH", "MPA_GPU_REFINE", "MPA_GPU_REGIONS", "MPA_GPU_PLANS", "MPA_GPU_SPANS", "MPA_GPU_STATS", "MPA_GPU_CS", "MPA_GPU_ROWS",
              "MPA_GPU_DPPLAN")
NEWEST = ("rg", "pl", "cs_out", "rows_out", "sp_in", "sp_cig", "dpp", "dp_trace")     # (the pools the report used to print as `?`, and the one no list had)

CHILD = """
import sys, os, json
sys.path.insert(0, 'tests')
import conftest, golden, miniprot_amd as mpa
from hostpipe import read_fasta
rec = {'b0': mpa.Context.device_bytes()}
ctx = mpa.Context(0)
rec['fresh'] = mpa.dbg_ctx_pools(ctx)
rec['no_sibling'] = mpa.dbg_ctx_pools(ctx, 1)
idx = mpa.Index.from_fasta(golden.path('DPP3-hs.gen.fa.gz'))
idx.to_device(ctx)
names, seqs = read_fasta(golden.path('DPP3-mm.pep.fa.gz'))
mo = mpa.default_mapopt()
mo.flag |= 0x80 | 0x100                # --aln, --trans (cs:Z strings are printed unless switched off)
texts = mpa.map_batches(ctx, idx, mo, [mpa.Queries(seqs, names) for _ in range(3)], 4)
rec['text_bytes'] = sum(len(t) for t in texts)
pools, k = [], 0
while True:
    p = mpa.dbg_ctx_pools(ctx, k)
    if p is None:
        break
    pools.append(p)
    k += 1
rec['pools'] = pools
rec['b_mapped'] = mpa.Context.device_bytes()
ctx.close()
rec['b_ctx_closed'] = mpa.Context.device_bytes()
idx.close()
rec['b_idx_closed'] = mpa.Context.device_bytes()
print('RECORD ' + json.dumps(rec))
"""


@pytest.fixture(scope="module")
def record():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, **{k: "1" for k in EVERY_STEP})
    r = subprocess.run([sys.executable, "-c", CHILD], cwd=root, env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    line = [l for l in r.stdout.split("\n") if l.startswith("RECORD ")]
    assert len(line) == 1, r.stdout + r.stderr
    return json.loads(line[0][len("RECORD "):])


def test_a_fresh_context_names_every_pool_once(record):
    names = [n for n, _ in record["fresh"]]
    assert len(names) > 0 and all(names) and len(set(names)) == len(names), names
    assert [n for n in NEWEST if n not in names] == []
    assert all(cap == 0 for _, cap in record["fresh"])                    # (nothing is allocated before it is asked for)
    assert record["no_sibling"] is None


def test_siblings_register_the_roots_pools_in_the_roots_order(record):
    pools = record["pools"]
    assert len(pools) > 1, "the stream of batches created no sibling context"
    root = [n for n, _ in pools[0]]
    assert root == [n for n, _ in record["fresh"]]
    for k, sib in enumerate(pools[1:], 1):
        assert [n for n, _ in sib] == root, "sibling %d" % k


def test_closing_the_context_returns_what_its_pools_held(record):
    S = sum(cap for ctx in record["pools"] for _, cap in ctx)
    held = sorted(set(n for ctx in record["pools"] for n, cap in ctx if cap))
    print("b0 %d, mapped %d, context closed %d, index closed %d; S %d in %d contexts; pools held: %s"
          % (record["b0"], record["b_mapped"], record["b_ctx_closed"], record["b_idx_closed"], S, len(record["pools"]), " ".join(held)))
    assert record["text_bytes"] > 0 and S > 0
    assert record["b_mapped"] - record["b_ctx_closed"] == S
    assert record["b_idx_closed"] == record["b0"]
