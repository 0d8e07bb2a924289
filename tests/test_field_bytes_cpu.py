"""The container walks' one field reader -- csrc/field_bytes.h: u8, le16 / be16, le32 / be32, le64 / be64 and fourcc, what
csrc/mp4_box_core.h, csrc/mp4_frag_core.h, csrc/iff_chunk_core.h and csrc/dsd_file_core.h read every header field with -- built for
the CPU with AddressSanitizer and UBSan by tests/cpp/field_bytes_driver.cpp, a stand-alone program, once with the byte reads and once
with the device's aligned reads (-DOHGPU_ALIGNED_READS).  Every width is read at every address mod 4 and compared with the value put
together by hand from the bytes; each read is made from a heap block that holds the dwords of the field and nothing else, so the
aligned reader's contract -- the dwords that hold the field, never one that holds none of its bytes: the "up to three bytes beyond"
of include/ohgpu.h's source arena -- is AddressSanitizer's to hold it to."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", params=[[], ["-DOHGPU_ALIGNED_READS"]], ids=["byte_reads", "the_devices_aligned_reads"])
def driver(request, tmp_path_factory):
    exe = tmp_path_factory.mktemp("field_bytes") / "field_bytes_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra", *request.param,
                           os.path.join(ROOT, "tests", "cpp", "field_bytes_driver.cpp"), "-o", str(exe)])
    return exe


def test_every_width_at_every_address_reads_the_holding_dwords_alone(driver):
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1", ASAN_OPTIONS="detect_leaks=1")
    p = subprocess.run([str(driver)], capture_output=True, text=True, env=env)
    assert p.returncode == 0 and p.stdout == "ok\n", p.stderr[-4000:]
    assert "runtime error" not in p.stderr and "Sanitizer" not in p.stderr, p.stderr[-4000:]
