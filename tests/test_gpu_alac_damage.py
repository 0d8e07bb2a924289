"""The Apple Lossless decoder's fixed-seed damage on the device: tests/alac_cases.device_mutations -- every 16th cut, every bit flip
and the splices within the library's packet limit, about 1 600 packets over every fixture's and handmade stream's configuration --
against the plain-Python model (tests/alac_textbook.py) on both routes, each first asserted through ohgpu_batch_paths_info.  Every
packet's status and sample count, every stream's result and the whole destination arena with its guard bytes are compared.

Two jobs.  A packet a stream: a group of 64 rows of the transposed scratch then holds rows of many streams of different frame
lengths, depths and channel counts, a corrupt packet's stale records and half-written rows beside good packets of OTHER
configurations -- which the named sandwiches of tests/test_gpu_alac_textbook.py, a bad packet between two good ones of its own
stream, never produce.  And the same packets as one stream per configuration, so that damaged and good packets of one stream share
a group and a destination span.  Both jobs have passed the sanitised CPU build of the same core (tests/test_alac_core_cpu.py) on
both routes first; what the CPU cannot show is whether the kernels of csrc/alac_packet_kernel.hip agree with the model on them.
The full set of more than 7 000 packets stays on the CPU.  Nothing here is random."""
import collections

import pytest

import alac_cases as AC
import alac_textbook as T
from ohpipeline_amd import capi
from test_gpu_alac_textbook import check

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module", params=[0, 1], ids=["fused", "plain"])
def vctx(ctx, request):
    ctx.set_kernel_variant(request.param)
    ctx.alac_route = capi.ALAC_ROUTE_PLAIN if request.param else capi.ALAC_ROUTE_FUSED
    yield ctx
    ctx.set_kernel_variant(0)


@pytest.fixture(scope="module")
def jobs():
    return AC.damage_job(), AC.damage_job_by_configuration()


def assert_reaches(job):
    """by the model alone, before anything runs: each kind of damage ends both ways, and the configurations are mixed"""
    kinds = [kind for kind, _, _ in AC.device_mutations()]
    assert len(job.table) == len(kinds) == len(job.streams)
    mix = collections.Counter((kind, st) for kind, (st, _) in zip(kinds, job.want_packets))
    for kind in ("cut", "flip", "splice"):
        assert mix[(kind, T.OK)] and mix[(kind, T.CORRUPT)], mix
    assert {s["cfg"]["frame_length"] for s in job.streams} >= {64, 256, 1024, 4096}
    assert {s["cfg"]["channels"] for s in job.streams} >= {1, 2, 3, 4, 6}
    return mix


def test_a_damaged_packet_a_stream(vctx, jobs):
    job = jobs[0]
    assert_reaches(job)
    check(vctx, job)


def test_the_same_packets_a_stream_a_configuration(vctx, jobs):
    job = jobs[1]
    assert len(job.table) == len(AC.device_mutations()) and len(job.streams) < len(job.table) // 10
    per_stream = [{st for st, _ in job.want_packets[s["first_packet"]:s["first_packet"] + s["n_packets"]]} for s in job.streams]
    assert sum(1 for mine in per_stream if {T.OK, T.CORRUPT} <= mine) >= len(job.streams) // 2        # damaged beside good in one stream
    check(vctx, job)
