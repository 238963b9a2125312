"""The stream plan of the pipeline (miniprot_amd/csrc/stream_plan.h: which streams mpa_map_batches creates, in which priority class and
order, for the hardware queues the process has) without a device.  tests/stream_plan_check.cpp goes over Q in {1, 2, 4, 8, 16, 24},
1..8 lanes, 1..4 seeders, 1..6 planners and the four layouts and checks: every role has a stream and a seeder or planner exactly one; no
two lane streams on one (class, queue slot) while a slot carries none; the side-stream caps; the legacy layout, stream for stream, when Q
covers every busy stream or MPA_STREAM_PLAN=0 asks for it; the same plan from two calls.  A stand-alone program under AddressSanitizer +
UBSan in a child process."""
import os
import re
import subprocess

import miniprot_amd as mpa
import refbind

CSRC = os.path.join(refbind.ROOT, "miniprot_amd", "csrc")


def test_policy_under_sanitizers(tmp_path):
    exe = str(tmp_path / "stream_plan_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan", "-I" + CSRC,
                    os.path.join(refbind.ROOT, "tests", "stream_plan_check.cpp"), os.path.join(CSRC, "stream_plan.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "4608 plans, 0 violations" in out.stdout and "VIOLATION" not in out.stderr and "Sanitizer" not in out.stderr and "runtime error" not in out.stderr


def test_the_module_stands_alone():
    """stream_plan.h and stream_plan.cpp use no HIP and nothing of the library: the standard library and each other"""
    for name in ("stream_plan.h", "stream_plan.cpp"):
        text = open(os.path.join(CSRC, name)).read()
        assert "#include <hip" not in text and re.search(r"\bhip[A-Z_]", text) is None, name
        assert [l for l in text.splitlines() if l.startswith('#include "')] in ([], ['#include "stream_plan.h"']), name
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-x", "c++", os.path.join(CSRC, "stream_plan.h")], check=True, capture_output=True)


def test_the_hooks_are_in_the_hooks_library():
    """libmpamd.so's C ABI (tests/test_abi_symbols.py) is what it was"""
    for name in ("mpa_dbg_stream_plan", "mpa_dbg_stream_plan_for"):
        assert hasattr(mpa.dbg_lib(), name) and not hasattr(mpa.lib(), name)


def test_the_plan_through_the_hook():
    """the default stage counts at four queues (layout A: the fifth lane and the seeders high, planners and one side stream per lane
    low), at sixteen (legacy: every busy stream has a queue) and with MPA_STREAM_PLAN=0"""
    a = mpa.dbg_stream_plan_for(4, layout="A")
    assert a["layout"] == "A" and a["q"] == 4 and a["n_streams"] == 12
    assert [l["cls"] for l in a["lanes"]] == ["normal"] * 4 + ["high"] and [l["rank"] for l in a["lanes"]] == [0, 1, 2, 3, 4]
    assert [(s["cls"], s["rank"], s["seed_cls"], s["seed_rank"]) for s in a["seeders"]] == [("high", k, "high", k) for k in (5, 6, 7)]
    assert [(s["cls"], s["rank"]) for s in a["planners"]] == [("low", k) for k in (8, 9, 10, 11)]
    assert [(l["side_cap"], l["side_cls"]) for l in a["lanes"]] == [(1, "low")] * 5
    for layout in (None, "1", "A", "B", "C", "0"):
        p = mpa.dbg_stream_plan_for(16, layout=layout)
        assert p["layout"] == "legacy" and p["n_streams"] == 19 and all(l["side_cap"] == 16 for l in p["lanes"])
    assert mpa.dbg_stream_plan_for(4, layout="0") == dict(mpa.dbg_stream_plan_for(16, layout="0"), q=4)
    assert mpa.dbg_stream_plan_for(4, layout="B")["planners"][0]["cls"] == "normal" and mpa.dbg_stream_plan_for(4, layout="C")["lanes"][4]["cls"] == "normal"
