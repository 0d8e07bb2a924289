"""The batch states' registry and release -- csrc/api_common.h's state_events, dev_array, state_own and state_release over RunState
(csrc/ohgpu_internal.h), what FlacState ... FileState and RaopState share -- built for the CPU with AddressSanitizer and UBSan by
tests/cpp/batch_state_driver.cpp, a stand-alone program.  The two calls under them, ctx_dev_alloc and ctx_dev_free, are malloc and
free over a set of the live blocks there, an event is a heap byte: a block or an event that is never given back is LeakSanitizer's
to report, one given back twice fails a check of the driver's.  The cases: a state released fully built; with blocks that stayed
null (zero counts, a list no run grew); after a run replaced a block, as flac_reserve does; twice through the family's release
function; partly built -- no events yet, an event refused, a block refused."""
import os
import subprocess

import pytest

from ohpipeline_amd import build

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("batch_state") / "batch_state_driver"
    hip_include = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(build.hipcc()))), "include")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", "-Wno-unused-parameter", "-Wno-unknown-pragmas",
                           "-D__HIP_PLATFORM_AMD__", "-isystem", hip_include, os.path.join(ROOT, "tests", "cpp", "batch_state_driver.cpp"), "-o", str(exe)])
    return exe


def test_every_block_and_event_goes_back_exactly_once(driver):
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1", ASAN_OPTIONS="detect_leaks=1")
    p = subprocess.run([str(driver)], capture_output=True, text=True, env=env)
    assert p.returncode == 0 and p.stdout == "ok\n", p.stderr[-4000:]
    assert "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, p.stderr[-4000:]
