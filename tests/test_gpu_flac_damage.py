"""The FLAC decoder's fixed-seed damage on the device: all 2 142 streams of tests/flac_cases.device_mutations (bit flips, a cut at
every byte, splices of frames and of arbitrary slices) as ONE batch, a descriptor each, against the plain-Python model
(tests/flac_textbook.py) on both routes.  Every result is compared field by field and the whole destination arena byte for byte.

What this reaches that the named handful of tests/test_gpu_flac_textbook.py does not is the text that exists only on the device
(csrc/flac_frame_kernel.hip): a candidate list that does not fit its first size and is scanned again, the host's sort and the
rows it hands out per stream when most of a stream's candidates are rejected, scratch sized by candidates x channels x blocksize,
the store kernel's grid over all candidates, the predictor in place over rows whose candidates overlap in the source -- and the
device compile of the core itself.  Every one of these streams has ended in the model's status under AddressSanitizer and UBSan
in tests/test_flac_core_cpu.py first; the conditions the set is there for are asserted from the models before anything runs.
Nothing here is random."""
import collections

import numpy as np
import pytest

import flac_cases as FC
from ohpipeline_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.fixture(scope="module", params=[0, 1], ids=["tuned", "v1"])
def vctx(ctx, request):
    ctx.set_kernel_variant(request.param)
    yield ctx
    ctx.set_kernel_variant(0)


@pytest.fixture(scope="module")
def layout():
    return FC.damage_layout()


def assert_reaches(layout):
    """by the models alone, before anything runs: every status, a good share of streams that still deliver frames, more candidates
    than the scan's first list holds (so the run scans twice), and most of them rejected"""
    cases = layout.cases
    assert len(cases) == 2142
    mix = collections.Counter(FC.model(c)[0].status for c in cases)
    assert mix[capi.FLAC_OK] and mix[capi.FLAC_CORRUPT] and mix[capi.FLAC_OVERFLOW], mix
    assert sum(1 for c in cases if len(FC.model(c)[0].frames) > 0) > len(cases) // 3
    candidates = sum(FC.model(c)[0].candidates for c in cases)
    assert candidates > FC.first_list(layout.src.size), (candidates, layout.src.size)
    assert 2 * sum(FC.model(c)[0].candidates_rejected for c in cases) > candidates


def test_every_mutation_in_one_batch_twice_without_allocating(vctx, layout):
    assert_reaches(layout)
    layout.check(vctx, times=2)
    assert layout.allocs[1] == layout.allocs[0], layout.allocs


def test_process_host_writes_only_what_was_decoded(ctx):
    cases = list(FC.device_mutations())[::10]
    lay = FC.Layout(cases, seed=17)
    dst = lay.dst0.copy()
    res = ctx.flac_process_host(lay.descs, lay.src, dst)
    assert np.array_equal(dst, lay.want)
    for c, r in zip(cases, res):
        mine = (int(r["status"]), int(r["frames"]), int(r["samples"]), int(r["first_sample_decoded"]), int(r["bytes_consumed"]),
                int(r["candidates"]), int(r["candidates_rejected"]))
        assert mine == FC.result_tuple(FC.model(c)[0]), (c.label, mine)
