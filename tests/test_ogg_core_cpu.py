"""csrc/ogg_page_core.h -- the text the Ogg page layer's four kernels run -- built for the CPU with AddressSanitizer and UBSan and
taken through find, verify, chain and gather by tests/cpp/ogg_core_driver.cpp, a stand-alone program: every named session of
tests/ogg_cases.py, the recorded sessions of tests/golden/ogg, pages of every size at which the checksum's slices change, and bytes
that overflow the candidate list.  The source arena is allocated to the byte, the destination pre-filled with 0xA5 with guard bytes
round every run; every record, every result and the whole destination arena must be the model's (tests/ogg_textbook.py), with no
sanitizer report.  Then the malformed tables, which ohgpu_ogg_batch_check must refuse with the documented codes: the device sees only
tables that passed that check."""
import os
import subprocess

import numpy as np
import pytest

import ogg_cases as GC
import ogg_textbook as OX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("ogg_core") / "ogg_core_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           os.path.join(ROOT, "tests", "cpp", "ogg_core_driver.cpp"), "-o", str(exe)])
    return exe


def check(driver, job, tmp_path, list_capacity=None):
    from ohpipeline_amd import capi
    capi.ogg_batch_check(job.descs, job.n_packets, job.src.size, job.dst0.size)      # what goes to the device later passes the library's own validation
    (tmp_path / "job.bin").write_bytes(job.driver_blob())
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1")
    extra = [] if list_capacity is None else [str(list_capacity)]
    p = subprocess.run([str(driver), str(tmp_path / "job.bin"), str(tmp_path / "out.bin")] + extra, capture_output=True, text=True, env=env)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    raw = (tmp_path / "out.bin").read_bytes()
    a = len(job.streams) * capi.OGG_STREAM_RESULT.itemsize
    b = a + job.n_packets * capi.OGG_PACKET.itemsize
    assert len(raw) == b + job.dst0.size
    results = np.frombuffer(raw[:a], dtype=capi.OGG_STREAM_RESULT)
    packets = np.frombuffer(raw[a:b], dtype=capi.OGG_PACKET)
    GC.assert_same(results, packets, raw[b:], job)
    return results, packets, raw[b:]


def test_the_named_sessions(driver, tmp_path):
    named = GC.sessions()
    job = GC.Job(list(named.values()))
    statuses = {name: m["status"] for name, m in zip(named, job.models)}
    assert set(statuses.values()) == set(range(6))
    _, _, arena = check(driver, job, tmp_path)
    assert arena[:GC.GUARD] == bytes([GC.FILL]) * GC.GUARD and job.want.tobytes() != job.dst0.tobytes()


def test_the_recorded_sessions(driver, tmp_path):
    golden = GC.load_golden()
    job = GC.Job([GC.stream(data, serial=rec["serial"], flags=OX.ANY_SEQ if rec["any_seq"] else 0) for data, rec in golden.values()])
    check(driver, job, tmp_path)


def test_pages_of_every_size_where_the_slices_change(driver, tmp_path):
    rng = GC.Lcg(9)
    sizes = list(range(27, 70)) + [1023, 1024, 1025, 1039, 1040, 1041, 1087, 1088, 1089, 4095, 4096, 4097, 65306, 65307]
    pages = [GC.page_of_size(n, 3, k, rng) for k, n in enumerate(sizes)]
    assert [len(p) for p in pages] == sizes
    pages.append(GC.page(3, len(sizes), [0, 3], b"end", OX.CONTINUED, 1))       # (the largest page's packet ends here)
    job = GC.Job([GC.stream(b"".join(pages), serial=3), GC.stream(b"".join(pages[5:]), serial=3, expect_seq=5)])
    assert all(m["status"] == OX.OK and m["pages"] > 40 for m in job.models)
    check(driver, job, tmp_path)


def test_packet_capacity_zero_and_too_small(driver, tmp_path):
    named = GC.sessions()
    job = GC.Job([dict(named["sizes"], packet_capacity=0), dict(named["three_pages"], packet_capacity=2), named["mapping"]])
    results, packets, _ = check(driver, job, tmp_path)
    assert [int(r["packets"]) for r in results] == [7, 3, 3]


def test_more_candidates_than_the_list_holds(driver, tmp_path):
    """"OggS" every four bytes and real pages behind it: the list overflows, the walk runs the checksums it was not given."""
    rng = GC.Lcg(31)
    dense = b"OggS" * 40 + bytes(300)
    body = dense + b"".join(GC.mux([rng.bytes(50)], 5))
    pages = GC.mux([body, rng.bytes(700)], 5, max_segments=2)
    job = GC.Job([GC.stream(b"".join(pages), serial=5)])
    assert job.models[0]["status"] == OX.OK and len(job.models[0]["packets"]) == 2
    check(driver, job, tmp_path, list_capacity=1)
    check(driver, job, tmp_path, list_capacity=0)
    check(driver, job, tmp_path)


def refused(descs, n_packets, src_bytes, dst_bytes):
    from ohpipeline_amd import capi
    with pytest.raises(capi.OhGpuError) as e:
        capi.ogg_batch_check(descs, n_packets, src_bytes, dst_bytes)
    return e.value.code


def test_malformed_tables_are_refused_with_the_documented_codes():
    from ohpipeline_amd import capi
    named = GC.sessions()
    job = GC.Job([named["sizes"], named["three_pages"], named["mapping"]])
    descs, sizes = job.descs, (job.src.size, job.dst0.size)
    capi.ogg_batch_check(descs, job.n_packets, *sizes)

    def broken(field, i, value, n_packets=job.n_packets):
        d = descs.copy()
        d[field][i] = value
        return refused(d, n_packets, *sizes)

    assert broken("reserved", 1, 1) == capi.ERR_INVALID                                        # non-zero reserved words
    assert broken("flags", 0, 8) == capi.ERR_INVALID                                           # unknown flags
    assert broken("src_bytes", 0, 1 << 31) == capi.ERR_INVALID
    assert broken("first_page_segment", 2, 256) == capi.ERR_INVALID
    assert broken("packet_first", 1, int(descs["packet_first"][1]) - 1) == capi.ERR_INVALID    # ranges that overlap in the table
    assert broken("packet_capacity", 2, job.n_packets) == capi.ERR_INVALID                     # ... or run past it
    assert refused(descs, job.n_packets - 1, *sizes) == capi.ERR_INVALID
    assert broken("src_offset", 2, sizes[0]) == capi.ERR_BOUNDS                                # a range outside the source arena
    assert refused(descs, job.n_packets, sizes[0] - 1, sizes[1]) == capi.ERR_BOUNDS            # (the last stream ends where the arena ends)
    assert broken("dst_offset", 2, sizes[1] - 4) == capi.ERR_BOUNDS                            # a run that ends outside the destination arena
    assert broken("dst_capacity", 0, sizes[1] + 1) == capi.ERR_BOUNDS
    assert broken("dst_capacity", 1, int(descs["dst_capacity"][1]) - 1) == capi.ERR_BOUNDS     # less room than the stream has bytes
    capi.ogg_batch_check(np.zeros(0, dtype=capi.OGG_STREAM_DESC), 0, 0, 0)                     # the empty batch is legal
