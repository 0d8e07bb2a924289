"""csrc/frag_units.h -- the index arithmetic both protected MPEG-4 families' decrypt-gathers run on the device (the slot plan, a wave's
trip over the chunk slots with its jumps, the searches for a unit's tile and row) -- built for the CPU with AddressSanitizer and UBSan
into tests/cpp/frag_units_driver.cpp, a stand-alone program (its own main, run as a process, nothing preloaded).  The driver lists every
unit of one batch of four streams by brute force -- a stream without rows, one unit under forty slots, two tiles and three rows with
runs of empty rows, an empty tile and rows of 1, 63, 64 and 65 units, a stream without room -- and lets launches of 1, 4 and more waves
than there are slots meet them: each unit exactly once, at its stream, row and place.  The plan is held against both families' bounds,
for a context that knows its CU count and one that does not."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_unit_is_met_once_and_the_plan_is_both_families(tmp_path):
    exe = tmp_path / "frag_units_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           os.path.join(ROOT, "tests", "cpp", "frag_units_driver.cpp"), "-o", str(exe)])
    p = subprocess.run([str(exe)], capture_output=True, text=True, env=dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1"))
    assert p.returncode == 0 and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    assert "every unit met once" in p.stdout
