"""FLAC frames decoded on the device (ohgpu_flac_batch_create / _run / _results, csrc/flac_frame_kernel.hip) against the plain-Python
model (tests/flac_textbook.py), on both routes: the tuned one (probe into scratch, restore per row, coalesced store) and, under kernel
variant 1, the plain one (a thread per accepted frame, straight from the bytes).

Conventions, as the other textbook tests: arenas allocated to the byte, the destination pre-filled with a pattern, the WHOLE
destination arena compared with the model's, the results (status, frames, samples, first sample, bytes consumed, candidates,
rejected) compared field by field, and for whole streams the MD5 of the device's samples compared with the stream's own STREAMINFO.
Malformed input here is the named handful of tests/flac_cases.device_cases; the fixed-seed mutations go to the device as one batch
in tests/test_gpu_flac_damage.py.  Every one of either tests/test_flac_core_cpu.py has already taken through the sanitised CPU
build of the same core; nothing here is random."""
import numpy as np
import pytest

import flac_cases as FC
from flac_cases import Layout, device_md5        # (shared with the far-offset and far-position tests)
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


@pytest.mark.parametrize("packed", [False, True], ids=["planes", "packed_be"])
@pytest.mark.parametrize("name", FC.fixture_names())
def test_fixture(vctx, name, packed):
    fx = FC.fixture(name)
    case = FC.whole(fx, packed)
    lay = Layout([case])
    res, got = lay.check(vctx)
    assert int(res[0]["status"]) == capi.FLAC_OK and int(res[0]["samples"]) == fx.samples
    assert device_md5(got[:FC.arena_bytes(case)], case) == fx.info["md5"]


def test_a_batch_of_64_mixed_descriptors_twice_without_allocating(vctx):
    cases = FC.mixed_cases()
    assert len(cases) == 64 and len({c.first_sample for c in cases}) > 4 and {fx.name for fx in FC.fixtures()} <= {c.label.split("@")[0] for c in cases}
    lay = Layout(cases, seed=7)
    assert len({int(o) % 2 for o in lay.descs["src_offset"]}) == 2           # odd source offsets among them
    lay.check(vctx, times=2)
    assert lay.allocs[1] == lay.allocs[0], lay.allocs


DEVICE_CASES = {c.label: c for c in FC.device_cases()}


def neighbours(case):
    tiny = FC.fixture("tiny_s16_stereo_44k1_b16")
    forms = FC.fixture("forms_s16_mono_11k_b16")
    return [FC.whole(tiny, packed=True, label="before"), case, FC.whole(forms, label="after")]


def run_device_case(ctx, label):
    lay = Layout(neighbours(DEVICE_CASES[label]), seed=3)
    res, _ = lay.check(ctx)                                    # (the whole arena: the neighbours' shares and every untouched byte)
    assert int(res[0]["status"]) == int(res[2]["status"]) == capi.FLAC_OK and int(res[0]["frames"]) == 6 and int(res[2]["frames"]) == 8
    return res[1]


def test_false_candidate_is_rejected(vctx):
    r = run_device_case(vctx, "false_candidate")
    assert int(r["status"]) == capi.FLAC_OK and int(r["candidates_rejected"]) >= 1 and int(r["frames"]) == 3


def test_start_inside_frame_2_delivers_frames_from_3_on(vctx):
    r = run_device_case(vctx, "mid_stream")
    assert (int(r["status"]), int(r["frames"]), int(r["first_sample_decoded"])) == (capi.FLAC_OK, 3, 48)
    r = run_device_case(vctx, "mid_stream_false_candidate")
    assert (int(r["status"]), int(r["frames"]), int(r["first_sample_decoded"])) == (capi.FLAC_OK, 1, 1152) and int(r["candidates_rejected"]) >= 1


@pytest.mark.parametrize("label", ["cut_in_last_frame", "cut_in_last_frame_s16"])
def test_cut_inside_the_last_frame_is_ok_and_says_where_to_resume(vctx, label):
    r = run_device_case(vctx, label)
    c = DEVICE_CASES[label]
    last = FC.frame_spans("tiny_s16_stereo_44k1_b16" if label == "cut_in_last_frame" else "s16_stereo_44k1_b1152_l5")[-1][0]
    assert int(r["status"]) == capi.FLAC_OK and int(r["bytes_consumed"]) == last - c.offset


def test_flipped_bit_in_frame_3_of_6_is_corrupt_after_three_frames(vctx):
    r = run_device_case(vctx, "flipped_bit")
    assert (int(r["status"]), int(r["frames"]), int(r["samples"])) == (capi.FLAC_CORRUPT, 3, 48)


@pytest.mark.parametrize("label", ["overflow", "overflow_packed"])
def test_too_small_max_samples_is_overflow(vctx, label):
    r = run_device_case(vctx, label)
    assert int(r["status"]) == capi.FLAC_OVERFLOW and int(r["frames"]) == DEVICE_CASES[label].max_samples // 16


def test_process_host_writes_only_what_was_decoded(ctx):
    cases = neighbours(DEVICE_CASES["cut_in_last_frame"])
    lay = Layout(cases, seed=5)
    dst = lay.dst0.copy()
    res = ctx.flac_process_host(lay.descs, lay.src, dst)
    assert np.array_equal(dst, lay.want)
    assert [int(r["frames"]) for r in res] == [6, 5, 8]
