"""csrc/ts_packet_core.h -- the text the transport stream and ADTS kernels run -- built for the CPU with AddressSanitizer and UBSan and
taken through both routes by tests/cpp/ts_core_driver.cpp, a stand-alone program: every named stream of tests/ts_cases.py, the fixtures
of tests/golden/ts, every source phase to every destination phase.  The source arena is allocated to the byte, the destination
pre-filled with 0xA5 with guard bytes round every run; every record, every result and the whole destination arena must be the model's
(tests/ts_textbook.py), with no sanitizer report.  Then the malformed descriptors, which ohgpu_ts_batch_check and
ohgpu_adts_batch_check must refuse with the documented codes: the device sees only descriptors that passed those checks."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import ts_cases as TC
import ts_textbook as TX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("ts_core") / "ts_core_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           os.path.join(ROOT, "tests", "cpp", "ts_core_driver.cpp"), "-o", str(exe)])
    return exe


def run_driver(driver, mode, blob, tmp_path):
    (tmp_path / "job.bin").write_bytes(blob)
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([str(driver), mode, str(tmp_path / "job.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, env=env)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    return (tmp_path / "out.bin").read_bytes()


def check(driver, job, tmp_path):
    from ohpipeline_amd import capi
    capi.ts_batch_check(job.descs, job.n_pes, job.src.size, job.dst0.size)      # what goes to the device later passes the library's own validation
    raw = run_driver(driver, "ts", job.driver_blob(), tmp_path)
    a = len(job.streams) * capi.TS_STREAM_RESULT.itemsize
    b = a + job.n_pes * capi.TS_PES.itemsize
    assert len(raw) == b + job.dst0.size
    results, pes = np.frombuffer(raw[:a], dtype=capi.TS_STREAM_RESULT), np.frombuffer(raw[a:b], dtype=capi.TS_PES)
    TC.assert_same(results, pes, raw[b:], job)
    return results, pes, raw[b:]


def check_adts(driver, job, tmp_path):
    from ohpipeline_amd import capi
    capi.adts_batch_check(job.descs, job.n_frames, job.src.size)
    raw = run_driver(driver, "adts", job.driver_blob(), tmp_path)
    a = len(job.streams) * capi.ADTS_STREAM_RESULT.itemsize
    assert len(raw) == a + job.n_frames * capi.ADTS_FRAME.itemsize
    results, frames = np.frombuffer(raw[:a], dtype=capi.ADTS_STREAM_RESULT), np.frombuffer(raw[a:], dtype=capi.ADTS_FRAME)
    TC.assert_same_adts(results, frames, job)
    return results, frames


def test_the_named_streams(driver, tmp_path):
    job = TC.Job(list(TC.named().values()))
    assert {m["status"] for m in job.models} == set(range(5))
    _, _, arena = check(driver, job, tmp_path)
    assert arena[:TC.GUARD] == bytes([TC.FILL]) * TC.GUARD and job.want.tobytes() != job.dst0.tobytes()


def test_the_fixtures(driver, tmp_path):
    streams = []
    for name in sorted(os.listdir(os.path.join(ROOT, "tests", "golden", "ts"))):
        if name.endswith(".ts.gz"):
            with gzip.open(os.path.join(ROOT, "tests", "golden", "ts", name), "rb") as f:
                streams.append(TC.stream(f.read()))
    assert len(streams) == 2
    check(driver, TC.Job(streams), tmp_path)


def test_every_source_phase_to_every_destination_phase(driver, tmp_path):
    job = TC.phases_job()
    check(driver, job, tmp_path)


def test_the_named_adts_streams(driver, tmp_path):
    job = TC.AdtsJob(list(TC.adts_named().values()))
    assert {m["status"] for m in job.models} == {TX.ADTS_OK, TX.NOT_ADTS}
    check_adts(driver, job, tmp_path)
    check_adts(driver, TC.AdtsJob(list(TC.adts_named().values()), lead=3), tmp_path)


def test_one_header_and_the_tags_on_the_host():
    from ohpipeline_amd import capi
    rng = TC.Lcg(8)
    for kw in (dict(), dict(protection_absent=False), dict(sf_index=12, channels=7, profile=3), dict(sf_index=13), dict(layer=2), dict(blocks=2), dict(length=6)):
        frame = TC.adts_frame(rng.bytes(40), **kw)
        got, want = capi.adts_header(frame), TX.adts_header(frame)
        assert (got is None) == (want is None), kw
        if want is not None:
            assert {f: int(got[f]) for f in ("bytes", "header_bytes", "profile", "sf_index", "channel_config")} == want, kw
    assert capi.adts_header(TC.adts_frame(b"")[:6]) is None
    tag = b"ID3\x04\x00\x00" + bytes([0, 0, 1, 5]) + bytes(133)
    footed = b"ID3\x03\x00\x10" + bytes([0, 0, 0, 20]) + bytes(30)
    for data in (tag + b"\xff\xf1", tag + footed + tag[:9], footed, b"ID3\xff\x00\x00" + bytes(30), b"ID3\x04\x00\x00\x00\x00\x80\x00" + bytes(30), b"ID3", b"", tag[:10]):
        assert capi.id3v2_skip(data) == TX.id3v2_skip(data), data[:12]
    assert capi.id3v2_skip(tag + footed + b"\xff") == 183
    assert capi.ts_crc(b"123456789") == 0x0376E6E7 and capi.ts_crc(TC.pat()) == 0


def refused(call, *args):
    from ohpipeline_amd import capi
    with pytest.raises(capi.OhGpuError) as e:
        call(*args)
    return e.value.code


def test_malformed_descriptors_are_refused_with_the_documented_codes():
    from ohpipeline_amd import capi
    named = TC.named()
    job = TC.Job([named["ten_pes"], named["rich_pmt"], named["length_zero"]])
    descs, sizes = job.descs, (job.src.size, job.dst0.size)
    capi.ts_batch_check(descs, job.n_pes, *sizes)

    def broken(field, i, value, n_pes=job.n_pes):
        d = descs.copy()
        d[field][i] = value
        return refused(capi.ts_batch_check, d, n_pes, *sizes)

    assert broken("reserved", 1, 1) == capi.ERR_INVALID                                        # non-zero reserved words
    assert broken("flags", 0, 2) == capi.ERR_INVALID                                           # unknown flags
    assert broken("src_bytes", 0, 1 << 31) == capi.ERR_INVALID
    assert broken("pmt_pid", 2, 0x2000) == capi.ERR_INVALID and broken("audio_pid", 2, 0x2000) == capi.ERR_INVALID
    assert broken("pes_first", 1, int(descs["pes_first"][1]) - 1) == capi.ERR_INVALID          # ranges that overlap in the table
    assert broken("pes_capacity", 2, job.n_pes) == capi.ERR_INVALID                            # ... or run past it
    assert refused(capi.ts_batch_check, descs, job.n_pes - 1, *sizes) == capi.ERR_INVALID
    assert broken("src_offset", 2, sizes[0]) == capi.ERR_BOUNDS                                # a range outside the source arena
    assert refused(capi.ts_batch_check, descs, job.n_pes, sizes[0] - 1, sizes[1]) == capi.ERR_BOUNDS   # (the last stream ends where the arena ends)
    assert broken("dst_offset", 2, sizes[1] - 4) == capi.ERR_BOUNDS                            # a run that ends outside the destination arena
    assert broken("dst_capacity", 0, sizes[1] + 1) == capi.ERR_BOUNDS
    assert broken("dst_capacity", 1, int(descs["dst_capacity"][1]) - 1) == capi.ERR_BOUNDS     # less room than the packets can deliver
    capi.ts_batch_check(np.zeros(0, dtype=capi.TS_STREAM_DESC), 0, 0, 0)                       # the empty batch is legal

    anamed = TC.adts_named()
    ajob = TC.AdtsJob([anamed["plain"], anamed["junk_between"], anamed["recognise_at_0"]])
    capi.adts_batch_check(ajob.descs, ajob.n_frames, ajob.src.size)

    def abroken(field, i, value):
        d = ajob.descs.copy()
        d[field][i] = value
        return refused(capi.adts_batch_check, d, ajob.n_frames, ajob.src.size)

    assert abroken("reserved", 0, 1) == capi.ERR_INVALID and abroken("flags", 1, 2) == capi.ERR_INVALID and abroken("src_bytes", 0, 1 << 31) == capi.ERR_INVALID
    assert abroken("frame_first", 1, int(ajob.descs["frame_first"][1]) - 1) == capi.ERR_INVALID and abroken("frame_capacity", 2, ajob.n_frames) == capi.ERR_INVALID
    assert abroken("src_offset", 2, ajob.src.size) == capi.ERR_BOUNDS
    assert refused(capi.adts_batch_check, ajob.descs, ajob.n_frames, ajob.src.size - 1) == capi.ERR_BOUNDS
    capi.adts_batch_check(np.zeros(0, dtype=capi.ADTS_STREAM_DESC), 0, 0)
