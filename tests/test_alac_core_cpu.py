"""csrc/alac_packet_core.h -- the text the device kernels run -- built for the CPU with AddressSanitizer and UBSan and taken through
the three phases over the transposed scratch and through the plain route by tests/cpp/alac_core_driver.cpp: over every fixture and
handmade packet in every output form, over the named malformed packets, and over a fixed-seed set of more than 2 000 damaged packets.
Every packet must end in the model's (tests/alac_textbook.py) status and sample count, and the whole destination arena must be the
model's, with no sanitizer report.  This is where malformed input is explored first.  The device takes the named handful
(tests/test_gpu_alac_textbook.py) and a fixed selection of the damage (tests/alac_cases.device_mutations: every 16th cut, every bit
flip, the splices within the library's packet limit; tests/test_gpu_alac_damage.py), whose exact jobs pass here on both routes
before; the full set of more than 7 000 packets, most of a minute of model time, runs only here."""
import os
import struct
import subprocess

import pytest

import alac_cases as AC
import alac_textbook as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROUTES = ("fused", "plain")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    exe = tmp_path_factory.mktemp("alac_core") / "alac_core_driver"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Wextra",
                           os.path.join(ROOT, "tests", "cpp", "alac_core_driver.cpp"), "-o", str(exe)])
    return exe


def check(driver, job, tmp_path, route, within_limits=True):
    if within_limits:                                      # what goes to the device later passes the library's own validation
        from ohpipeline_amd import capi
        capi.alac_batch_check(*AC.capi_tables(job), len(job.src), len(job.dst0))
    (tmp_path / "job.bin").write_bytes(job.driver_blob())
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=0", UBSAN_OPTIONS="print_stacktrace=1")
    p = subprocess.run([str(driver), str(tmp_path / "job.bin"), str(tmp_path / "out.bin"), route], capture_output=True, text=True, env=env)
    assert p.returncode == 0 and "runtime error" not in p.stderr and "AddressSanitizer" not in p.stderr, p.stderr[-4000:]
    raw = (tmp_path / "out.bin").read_bytes()
    n = len(job.table)
    got = [struct.unpack_from("<II", raw, 8 * i) for i in range(n)]
    assert got == [tuple(w) for w in job.want_packets], [(i, g, w) for i, (g, w) in enumerate(zip(got, job.want_packets)) if g != tuple(w)][:5]
    arena = raw[8 * n:]
    assert len(arena) == len(job.want)
    if arena != job.want:
        first = next(i for i in range(len(arena)) if arena[i] != job.want[i])
        raise AssertionError("the arena differs from byte %d on (%s route)" % (first, route))
    return {st for st, _ in got}


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("form", AC.FORMS)
def test_every_fixture_and_handmade_packet(driver, tmp_path, route, form):
    job = AC.Job(AC.fixture_streams(form) + AC.handmade_streams(form))
    assert check(driver, job, tmp_path, route) == {T.OK}


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("form", AC.FORMS)
def test_malformed_packets_between_good_neighbours(driver, tmp_path, route, form):
    job = AC.Job(AC.sandwiches(form))
    assert check(driver, job, tmp_path, route) == {T.OK, T.CORRUPT, T.UNSUPPORTED}
    want = [st for _, _, st in AC.malformed().values()]
    assert [job.want_packets[3 * i + 1][0] for i in range(len(want))] == want
    assert all(job.want_packets[3 * i][0] == T.OK and job.want_packets[3 * i + 2][0] == T.OK for i in range(len(want)) if want[i] != T.UNSUPPORTED)


@pytest.mark.parametrize("route", ROUTES)
def test_mutations_end_in_the_models_status(driver, tmp_path, route):
    cases = AC.mutations()
    assert len(cases) >= 2000
    job = AC.Job([(cfg, packets, AC.FORMS[k % 3]) for k, (cfg, packets) in enumerate(cases)])
    statuses = check(driver, job, tmp_path, route, within_limits=False)      # (a spliced packet can be longer than its stream allows)
    assert {T.OK, T.CORRUPT} <= statuses                   # the set reaches the outcomes it is there for
    assert sum(1 for st, _ in job.want_packets if st == T.OK) > 50       # ... and some damage still decodes, to other samples


def test_the_selection_that_goes_to_the_device_drops_no_cut_no_flip_and_few_splices():
    picked = AC.device_mutations()
    kinds = [kind for kind, _, _ in picked]
    n_cuts = len(AC.mutations()) - 900 - 300
    assert kinds.count("cut") == (n_cuts + 15) // 16 and kinds.count("flip") == 900 and 270 <= kinds.count("splice") <= 300
    assert kinds == sorted(kinds)                                     # (cuts, flips, splices: the order of mutations())
    assert all(len(packet) <= AC.packet_limit(cfg) for _, cfg, packet in picked)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("job", ["a_packet_a_stream", "a_stream_a_configuration"])
def test_the_damage_that_goes_to_the_device(driver, tmp_path, route, job):
    """the exact jobs of tests/test_gpu_alac_damage.py, which pass the library's own validation"""
    job = AC.damage_job() if job == "a_packet_a_stream" else AC.damage_job_by_configuration()
    assert len(job.table) == len(AC.device_mutations())
    assert {T.OK, T.CORRUPT} <= check(driver, job, tmp_path, route, within_limits=True)
