"""The C ABI of libmpamd.so as a list of names: the defined dynamic symbols that begin with mpa_, mp_ or ns_ (`nm -D --defined-only`)
equal tests/golden/abi_symbols.txt, which was recorded from the build of the commit BEFORE the device code was split into one
translation unit per stage (dev_ctx / seed_run / refine_run / index_run / dp_exec).  A function lost between two units, or one that a
unit exports by accident, shows here without a device."""
import os
import subprocess
import miniprot_amd as mpa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_exported_symbols_are_the_recorded_ones():
    nm = subprocess.run(["nm", "-D", "--defined-only", mpa.LIB_PATH], check=True, capture_output=True, text=True).stdout
    have = sorted(s for s in (line.split()[-1] for line in nm.splitlines() if line.strip()) if s.startswith(("mpa_", "mp_", "ns_")))
    want = open(os.path.join(ROOT, "tests", "golden", "abi_symbols.txt")).read().split()
    assert want == sorted(want) and len(want) > 100                    # (the fixture itself)
    assert [s for s in have if s not in want] == [] and [s for s in want if s not in have] == []
    assert have == want
