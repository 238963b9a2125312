"""How the device pools and pinned blocks are cut up (miniprot_amd/csrc/carve.h, dev_layout.h), on the CPU.

A stand-alone program (tests/carve_check.cpp, compiled here with AddressSanitizer and UBSan) holds Carve / Piece against plain
arithmetic -- alignments 1, 16, 64 and 256; sizes 0, 1, align - 1, align, align + 1 and 1 000 random ones below 2^33; an absent
optional part; a piece inside another -- and every layout of dev_layout.h (extraction scratch, counts and forward pass; regions tail;
plans tail; the walks with every combination of statistics / cs strings / residue rows on, empty and off; spans; assembly; the
resident round's results) against a restatement of the offset arithmetic the drivers used to spell out: every offset and total equal,
every piece aligned for its element type, inside its block and disjoint from the others.  No sanitizer goes near code loaded into
python."""
import os
import subprocess
import refbind


def test_layouts_against_plain_arithmetic_under_sanitizers(tmp_path):
    root = refbind.ROOT
    exe = str(tmp_path / "carve_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-static-libasan",
                    "-I" + os.path.join(root, "miniprot_amd", "csrc"), os.path.join(root, "tests", "carve_check.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    assert " 0 mismatches" in out.stdout and "MISMATCH" not in out.stderr and "ERROR" not in out.stderr
