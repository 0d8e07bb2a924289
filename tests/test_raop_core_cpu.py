"""csrc/raop_aes_core.h -- the text the decrypt kernel runs -- built for the CPU with AddressSanitizer and UBSan and taken through the
key schedule, the block function and the piece plan by tests/cpp/raop_core_driver.cpp, a stand-alone program: every length 0..96,
1008..1040, 1456..1460, 2048 and 2064, source offsets 0, 4, 8 and 12 mod 16, several streams under different keys back to back, into
the destination (the plaintext form) and into the plaintext scratch (the decoding form).  The whole destination arena, pre-filled
with 0xA5, must be the model's (tests/raop_textbook.py), so must the scratch with its layout, with no sanitizer report.  Then the
malformed tables -- overlap, misalignment, out of range -- which ohgpu_raop_batch_check must refuse with the documented codes: this
is where odd input is explored; the device sees only tables that passed that check."""
import os
import struct
import subprocess

import numpy as np
import pytest

import alac_cases as AC
import alac_textbook as T
import raop_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = list(range(0, 97)) + list(range(1008, 1041)) + list(range(1456, 1461)) + [2048, 2064]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("raop_core") / "raop_core_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           os.path.join(ROOT, "tests", "cpp", "raop_core_driver.cpp"), "-o", str(exe)])
    return exe


def check(driver, job, tmp_path):
    from ohpipeline_amd import capi
    capi.raop_batch_check(*RC.capi_tables(job), len(job.src), len(job.dst0))          # what goes to the device later passes the library's own validation
    (tmp_path / "job.bin").write_bytes(job.driver_blob())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([str(driver), str(tmp_path / "job.bin"), str(tmp_path / "out.bin")], capture_output=True, text=True, env=env)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    raw = (tmp_path / "out.bin").read_bytes()
    n, = struct.unpack_from("<Q", raw, 0)
    scratch, arena = raw[8:8 + n], raw[8 + n:]
    assert len(arena) == len(job.dst0)
    return scratch, arena


def first_difference(a, b):
    return next((i for i in range(min(len(a), len(b))) if a[i] != b[i]), min(len(a), len(b)))


def cut(lengths, parts):
    return [lengths[k::parts] for k in range(parts)]


def test_every_length_at_every_alignment_into_the_destination(driver, tmp_path):
    """twenty streams under twenty keys, their packets interleaved in the arena: every length at every source alignment"""
    rng = AC.Lcg(31)
    streams = [RC.stream(RC.rand_bytes(rng, 16), RC.rand_bytes(rng, 16), [RC.rand_bytes(rng, n) for n in mine], align=align)
               for mine in cut(LENGTHS, 5) for align in (0, 4, 8, 12)]
    job = RC.Job(streams)
    assert {(size, off % 16) for off, size in job.table} == {(n, a) for n in LENGTHS for a in (0, 4, 8, 12)}
    scratch, arena = check(driver, job, tmp_path)
    assert scratch == b"" and arena == job.want, "the arena differs from byte %d on" % first_difference(arena, job.want)
    assert arena[:RC.GUARD] == bytes([RC.FILL]) * RC.GUARD and arena != job.dst0


def test_every_length_into_the_scratch_with_its_layout(driver, tmp_path):
    """the decoding form: nothing reaches the destination here (the Apple Lossless phases over random bytes are not this test's
    business, and tests/test_alac_core_cpu.py's on the CPU), every packet's plaintext starts at a 16-byte boundary of the scratch, in
    the table's order"""
    rng = AC.Lcg(32)
    big = dict(RC.sessions()[0]["cfg"], frame_length=4096)            # (room for the 2064-byte packet within Apple Lossless's packet limit)
    streams = [RC.stream(RC.rand_bytes(rng, 16), RC.rand_bytes(rng, 16), [RC.rand_bytes(rng, n) for n in mine], T.PACKED_LE, big) for mine in cut(LENGTHS, 3)]
    job = RC.Job(streams, decode=False)
    assert len(job.want_scratch) == sum((n + 15) // 16 * 16 for n in LENGTHS)
    scratch, arena = check(driver, job, tmp_path)
    assert arena == job.dst0
    assert len(scratch) == len(job.want_scratch) and scratch == job.want_scratch, "the scratch differs from byte %d on" % first_difference(scratch, job.want_scratch)


def test_the_committed_sessions_mixed_with_plaintext_streams(driver, tmp_path):
    rng = AC.Lcg(33)
    streams = [RC.session_stream(s, form) for s, form in zip(RC.sessions(), (T.PLANAR, T.PACKED_LE, T.PACKED_BE, T.PLANAR))]
    streams.insert(1, RC.stream(RC.rand_bytes(rng, 16), RC.rand_bytes(rng, 16), [RC.rand_bytes(rng, n) for n in (33, 0, 1040, 5)]))
    streams.append(RC.session_stream(RC.sessions()[0], RC.PLAINTEXT))
    job = RC.Job(streams)
    scratch, arena = check(driver, job, tmp_path)
    assert scratch == job.want_scratch
    # of the destination the driver writes the plaintext streams' share; the last of them is a fixture's packets in the clear
    window = RC.GUARD + len(job.src)
    assert arena[:window] == job.want[:window] and arena[window:] == job.dst0[window:]
    last = job.streams[-1]
    assert all(arena[last["dst_offset"] + off - job.table[last["first_packet"]][0]:][:size] == p
               for (off, size), p in zip(job.table[last["first_packet"]:], RC.sessions()[0]["fx"]["packets"]))


def test_wrong_key_bytes_go_through_the_sanitised_apple_lossless_core(tmp_path):
    """what tests/test_gpu_raop_textbook.py later gives the device under a wrong key: the committed sessions decrypted under keys with
    one bit flipped, through the CPU build of csrc/alac_packet_core.h on both routes, ending as the model says -- the nine streams of
    tests/raop_cases.wrong_key_streams, of which the last holds datagrams that were encrypted under another session's key
    (tests/test_raop_host_cpp.py)"""
    import test_alac_core_cpu as AlacCpu
    exe = tmp_path / "alac_core_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           os.path.join(ROOT, "tests", "cpp", "alac_core_driver.cpp"), "-o", str(exe)])
    wrong = RC.wrong_key_streams(lambda k: AC.FORMS[k // 2 % 3] if k < 8 else T.PACKED_LE)
    assert len(wrong) == 9
    job = AC.Job([(s["cfg"], RC.clear_packets(s), s["form"]) for s in wrong])
    assert T.CORRUPT in {st for st, _ in job.want_packets}
    for route in AlacCpu.ROUTES:
        AlacCpu.check(exe, job, tmp_path, route)


def refused(descs, packets, src_bytes, dst_bytes):
    from ohpipeline_amd import capi
    with pytest.raises(capi.OhGpuError) as e:
        capi.raop_batch_check(descs, packets, src_bytes, dst_bytes)
    return e.value.code


def test_malformed_tables_are_refused_with_the_documented_codes():
    from ohpipeline_amd import capi
    rng = AC.Lcg(34)
    s = RC.sessions()[0]
    job = RC.Job([RC.stream(RC.rand_bytes(rng, 16), RC.rand_bytes(rng, 16), [RC.rand_bytes(rng, n) for n in (48, 20, 64)]), RC.session_stream(s, T.PACKED_BE)], aligns=(0,))
    descs, packets = RC.capi_tables(job)
    sizes = (len(job.src), len(job.dst0))
    capi.raop_batch_check(descs, packets, *sizes)

    def broken(change):
        d, p = descs.copy(), packets.copy()
        change(d, p)
        return refused(d, p, *sizes)

    def put(array, i, field, value):
        array[field][i] = value

    assert broken(lambda d, p: put(p, 1, "src_offset", p["src_offset"][1] + 2)) == capi.ERR_INVALID          # a source offset that is no multiple of 4
    assert broken(lambda d, p: put(p, 4, "src_offset", p["src_offset"][4] + 1)) == capi.ERR_INVALID          # ... of a decoding stream
    assert broken(lambda d, p: put(p, 1, "src_offset", p["src_offset"][0] + 44)) == capi.ERR_INVALID         # plaintext: a packet that starts inside its predecessor
    assert broken(lambda d, p: put(p, 1, "src_offset", 0)) == capi.ERR_INVALID                               # plaintext: packets that do not ascend
    assert broken(lambda d, p: put(d, 0, "dst_offset", d["dst_offset"][0] + 2)) == capi.ERR_INVALID          # plaintext: dst_offset no multiple of 4
    assert broken(lambda d, p: put(d, 0, "dst_plane_stride", 64)) == capi.ERR_INVALID
    assert broken(lambda d, p: put(d, 0, "flags", RC.PLAINTEXT | 1)) == capi.ERR_INVALID                     # the plaintext flag with an output form
    assert broken(lambda d, p: put(d, 1, "flags", 8)) == capi.ERR_INVALID
    assert broken(lambda d, p: put(p, 2, "reserved", 1)) == capi.ERR_INVALID
    assert broken(lambda d, p: put(d, 1, "first_packet", 2)) == capi.ERR_INVALID                             # ranges that overlap in the table
    assert broken(lambda d, p: put(d, 1, "n_packets", 2)) == capi.ERR_INVALID                                # ... or leave part of it out
    assert broken(lambda d, p: put(p, 2, "bytes", len(job.src))) == capi.ERR_BOUNDS                          # out of the source arena
    assert broken(lambda d, p: put(p, 2, "src_offset", len(job.src) + 16)) == capi.ERR_BOUNDS
    assert broken(lambda d, p: put(p, 5, "src_offset", (len(job.src) + 3) // 4 * 4)) == capi.ERR_BOUNDS
    assert broken(lambda d, p: put(d, 0, "dst_offset", len(job.dst0) - 64)) == capi.ERR_BOUNDS               # the moved layout ends behind the destination arena
    assert broken(lambda d, p: put(d, 1, "dst_offset", len(job.dst0) - 64)) == capi.ERR_BOUNDS
    assert broken(lambda d, p: put(d, 1, "channels", 9)) == capi.ERR_INVALID                                 # Apple Lossless's limits hold for a decoding stream
    assert broken(lambda d, p: put(d, 1, "bit_depth", 12)) == capi.ERR_UNSUPPORTED
    assert refused(descs, packets, sizes[0] - 1, sizes[1]) == capi.ERR_BOUNDS and refused(descs, packets, sizes[0], sizes[1] - RC.GUARD - 4) == capi.ERR_BOUNDS
    assert refused(descs, packets[:-1], *sizes) == capi.ERR_INVALID
    # a plaintext stream's configuration is not read, and no Apple Lossless packet limit applies to it
    d, p = descs.copy(), packets.copy()
    d["frame_length"][0], d["channels"][0], d["bit_depth"][0] = 0, 0, 0
    capi.raop_batch_check(d, p, *sizes)
    capi.raop_batch_check(np.zeros(0, dtype=capi.RAOP_STREAM_DESC), np.zeros(0, dtype=capi.ALAC_PACKET), 0, 0)
