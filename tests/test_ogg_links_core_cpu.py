"""csrc/ogg_page_core.h's walk with OHGPU_OGG_FOLLOW_LINKS built for the CPU with AddressSanitizer and UBSan and run by
tests/cpp/ogg_links_driver.cpp, a stand-alone program: every named chained session of tests/ogg_links_cases.py, rule 7's cut taken
as two streams of one job, and the plain sessions of tests/ogg_cases.py with the flag set, which have no link to find.  Every record,
every result -- `links` among them -- and the whole destination arena must be the model's (tests/ogg_links_textbook.py), with no
sanitizer report.  Then what ohgpu_ogg_batch_check says to the flag and to the magic."""
import os
import subprocess

import numpy as np
import pytest

import ogg_cases as GC
import ogg_links_cases as LC
import ogg_links_textbook as LX
import ogg_textbook as OX

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("ogg_links") / "ogg_links_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           os.path.join(ROOT, "tests", "cpp", "ogg_links_driver.cpp"), "-o", str(exe)])
    return exe


def check(driver, job, tmp_path):
    from ohpipeline_amd import capi
    capi.ogg_batch_check(job.descs, job.n_packets, job.src.size, job.dst0.size)
    (tmp_path / "job.bin").write_bytes(job.driver_blob())
    env = dict(os.environ, UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([str(driver), str(tmp_path / "job.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, env=env)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    raw = (tmp_path / "out.bin").read_bytes()
    a = len(job.streams) * capi.OGG_STREAM_RESULT.itemsize
    b = a + job.n_packets * capi.OGG_PACKET.itemsize
    assert len(raw) == b + job.dst0.size
    results = np.frombuffer(raw[:a], dtype=capi.OGG_STREAM_RESULT)
    packets = np.frombuffer(raw[a:b], dtype=capi.OGG_PACKET)
    LC.assert_same(results, packets, raw[b:], job)
    return results, packets


def test_the_named_chained_sessions(driver, tmp_path):
    named = LC.sessions()
    job = LC.Job(list(named.values()))
    assert {m["links"] for m in job.models} == {0, 1, 2} and {m["status"] for m in job.models} == {OX.OK, OX.LOST_SYNC, OX.HOLE, OX.UNSUPPORTED_MAPPING}
    results, packets = check(driver, job, tmp_path)
    i = list(named).index("small_capacity")
    assert LC.links_of(results)[i] == 2 and int(results[i]["packets"]) > int(job.descs[i]["packet_capacity"]) == 3


def test_the_plain_sessions_with_the_flag(driver, tmp_path):
    """No session of tests/ogg_cases.py has a foreign first page that a magic of "\\x01vorbis" matches: the flag changes nothing."""
    named = GC.sessions()
    streams = [LC.stream(s["data"], serial=s["serial"], expect_seq=s["expect_seq"], first_page_segment=s["first_page_segment"], flags=s["flags"],
                         packet_capacity=s["packet_capacity"]) for s in named.values()]
    job = LC.Job(streams)
    for s, m in zip(named.values(), job.models):
        assert m == dict(OX.demux(s["data"], s["serial"], s["expect_seq"], s["first_page_segment"], s["flags"]), links=0)
    check(driver, job, tmp_path)


def cut_streams(s, cuts):
    """For every cut the two streams of rule 7: [0, cut) and the rest from where the model says the first call stops."""
    out = []
    for cut in cuts:
        one = LC.stream(s["data"][:cut], magic=s["magic"], serial=s["serial"], flags=s["flags"] & ~LX.FOLLOW_LINKS)
        m = LC.model(one)
        assert m["status"] == OX.OK
        out += [one, LC.stream(s["data"][m["bytes_consumed"]:], magic=s["magic"], serial=m["serial"], expect_seq=m["next_seq"], first_page_segment=m["resume_segment"],
                               flags=s["flags"] & ~LX.FOLLOW_LINKS)]
    return out


def test_the_two_call_cut(driver, tmp_path):
    named = LC.sessions()
    streams = []
    for name in ("two_links", "open_at_boundary", "link_packet_open_then_closed", "flac_mapping"):
        s = named[name]
        streams += cut_streams(s, range(0, len(s["data"]) + 1, 7))
    job = LC.Job(streams)
    assert sum(m["links"] for m in job.models) > len(streams) // 2
    check(driver, job, tmp_path)


def code_of(descs, job):
    from ohpipeline_amd import capi
    with pytest.raises(capi.OhGpuError) as e:
        capi.ogg_batch_check(descs, job.n_packets, job.src.size, job.dst0.size)
    return e.value.code


def test_what_the_check_says_to_the_flag_and_the_magic():
    from ohpipeline_amd import capi
    assert (capi.OGG_FOLLOW_LINKS, capi.OGG_PACKET_LINK) == (16, 8)
    named = LC.sessions()
    job = LC.Job([named["two_links"], named["flac_mapping"], named["magic_length_0"]])
    capi.ogg_batch_check(job.descs, job.n_packets, job.src.size, job.dst0.size)          # flag 16, magics of 7, 5 and 0 bytes
    assert [int(x) for x in job.descs.view(capi.OGG_STREAM_DESC_LINKS)["link_magic_bytes"]] == [7, 5, 0] and [int(x) for x in job.descs["reserved"][0]] == [7, 0x726F7601, 0x00736962]

    def broken(**fields):
        d = job.descs.copy()
        for f, v in fields.items():
            d.view(capi.OGG_STREAM_DESC_LINKS)[f][0] = v
        return code_of(d, job)

    assert broken(flags=0) == capi.ERR_INVALID                                            # the flag's reserved words without the flag
    assert broken(flags=8) == capi.ERR_INVALID and broken(flags=16 | 8) == capi.ERR_INVALID
    assert broken(link_magic_bytes=9) == capi.ERR_INVALID
    assert broken(link_magic_bytes=6) == capi.ERR_INVALID                                 # a byte beyond the length
    assert broken(link_magic=(1, 118, 111, 114, 98, 105, 115, 1)) == capi.ERR_INVALID
    d = job.descs.copy()
    d.view(capi.OGG_STREAM_DESC_LINKS)["link_magic_bytes"][0], d.view(capi.OGG_STREAM_DESC_LINKS)["link_magic"][0] = 8, (1, 118, 111, 114, 98, 105, 115, 0)
    capi.ogg_batch_check(d, job.n_packets, job.src.size, job.dst0.size)                   # eight bytes, the last of them zero
