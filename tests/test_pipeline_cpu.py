"""The scheduler of the stream pipeline (miniprot_amd/csrc/host_pipeline.h) without a device: tests/pipeline_check.cpp drives it with
stub stages over 420 jobs (lanes 1..8, seeders 1..4, planners 1..6, 0..20 batches; claims in order, shuffled, ending early, repeated;
error codes and exceptions from every stage) and checks the event log of every run against what the waits of mpa_map_batches() promise.
A stand-alone program in a child process, once under ThreadSanitizer and once under AddressSanitizer + UBSan."""
import os
import subprocess

import pytest

import refbind

# one run of the finished program on the development machine: 2.5 s under ThreadSanitizer, 1.2 s under AddressSanitizer + UBSan (most
# of it the stubs' sleeps and thread starts).  The limits are ten times that: a deadlock of the scheduler fails here, it does not hang
BUILDS = {
    "thread": (["-fsanitize=thread"], 25),
    "address_undefined": (["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan"], 12),
}


@pytest.mark.parametrize("build", sorted(BUILDS))
def test_scheduler_under_sanitizers(tmp_path, build):
    """measured: 420 runs in 2.5 s (thread) and 1.2 s (address_undefined); limits 25 s and 12 s"""
    flags, limit = BUILDS[build]
    csrc = os.path.join(refbind.ROOT, "miniprot_amd", "csrc")
    exe = str(tmp_path / "pipeline_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-pthread"] + flags + ["-I" + csrc, os.path.join(refbind.ROOT, "tests", "pipeline_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=limit)
    assert out.returncode == 0, out.stdout + out.stderr
    assert " 0 violations" in out.stdout and "VIOLATION" not in out.stderr and "Sanitizer" not in out.stderr


def test_the_header_stands_alone():
    """host_pipeline.h includes the standard library only and compiles on its own"""
    csrc = os.path.join(refbind.ROOT, "miniprot_amd", "csrc")
    text = open(os.path.join(csrc, "host_pipeline.h")).read()
    assert '#include "' not in text
    subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-x", "c++", os.path.join(csrc, "host_pipeline.h")], check=True, capture_output=True)
