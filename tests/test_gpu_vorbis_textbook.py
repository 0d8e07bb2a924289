"""The Vorbis decoder on the device against the independent model (tests/vorbis_textbook.py), on both routes (the FFT transform, and the
plain route under kernel variant 1, each first asserted through ohgpu_batch_paths_info): every packet record equal, every spectrum
BIT-IDENTICAL, every PCM sample within 1 LSB -- the model transforms in float64 by the direct form, the product in float32 through an FFT
whose error on a full-scale block is near 2e-7 (tests/test_vorbis_core_cpu.py measures it) where an LSB is 3e-5, and two values less than
half an LSB apart round at most one apart -- and not a byte of the destination beyond what max_samples allows.  Shapes: tests/vorbis_cases.py.
Then damage, the resume rule, a second run that allocates nothing, the host-buffer call, and more streams than a wave of the scan holds."""
import numpy as np
import pytest

import vorbis_cases as VC
import vorbis_frames as VF
import vorbis_textbook as TB
from ohpipeline_amd import capi
from vorbis_device import FILL, check_records, run_batch, stream_pcm

pytestmark = pytest.mark.gpu

ROUTES = [pytest.param(0, id="fft"), pytest.param(1, id="plain")]


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.set_kernel_variant(0)
    c.close()


@pytest.mark.parametrize("variant", ROUTES)
@pytest.mark.parametrize("name", sorted(VC.SHAPES))
def test_records_spectrum_and_pcm(ctx, name, variant):
    st = VC.stream(name)
    total = sum(r[3] for r in VC.expected(name)[0])
    cut = total - 7                                                  # (the last packet is cut short: V4)
    recs, spectra, pcm = VC.expected(name, cut)
    res, pres, got, descs, spec = run_batch(ctx, variant, [st], max_samples=[cut], spectra=True)
    check_records(pres, recs)
    assert int(res["packets_ok"][0]) == len(st.packets) and int(res["first_bad_status"][0]) == 0 and int(res["samples"][0]) == cut
    for p, rows in enumerate(spectra):
        for c in range(st.model.channels):
            assert spec[(p, c)].tobytes() == rows[c].tobytes(), (p, c)
    mine, rest = stream_pcm(got, descs[0], st.model.channels, cut)
    worst = int(np.abs(mine - pcm).max())
    print(f"{name}: {cut} samples, largest PCM difference {worst} LSB, {int((mine != pcm).sum())} samples differ")
    assert worst <= 1
    assert (got[int(descs[0]['dst_offset']) + cut * st.model.channels * 2:] == FILL).all()


@pytest.mark.parametrize("variant", ROUTES)
def test_planes(ctx, variant):
    name = "six_128_512"
    st = VC.stream(name)
    recs, _, pcm = VC.expected(name)
    total = pcm.shape[1]
    res, pres, got, descs, _ = run_batch(ctx, variant, [st], planar=True, max_samples=[total + 3])
    mine, _ = stream_pcm(got, descs[0], 6, total, planar=True)
    assert int(np.abs(mine - pcm).max()) <= 1 and int(res["samples"][0]) == total
    stride = int(descs[0]["dst_plane_stride"])
    for c in range(6):
        assert (got[c * stride + total * 4:(c + 1) * stride] == FILL).all()


@pytest.mark.parametrize("variant", ROUTES)
def test_damage(ctx, variant):
    """Truncated packets decode as far as they go (V2); a bad mode, an empty packet and a header packet are passed over."""
    name = "six_128_512"
    st = VC.stream(name)
    hurt = VF.Stream(st.ident, st.setup, VC.damaged(name))
    recs, spectra, pcm = TB.decode_stream(hurt.model, hurt.packets)
    res, pres, got, descs, spec = run_batch(ctx, variant, [hurt], spectra=True)
    check_records(pres, recs)
    assert int(res["packets_ok"][0]) == 4 and int(res["first_bad_status"][0]) == capi.VORBIS_CORRUPT and int(res["samples"][0]) == pcm.shape[1]
    for p, rows in enumerate(spectra):
        for c in range(6):
            if rows is not None:
                assert spec[(p, c)].tobytes() == rows[c].tobytes(), (p, c)
    mine, _ = stream_pcm(got, descs[0], 6, pcm.shape[1])
    assert int(np.abs(mine - pcm).max()) <= 1


@pytest.mark.parametrize("variant", ROUTES)
def test_resume_with_the_priming_packet_equals_one_call(ctx, variant):
    """V3: [0, k) then [k - 1, n) -- the last packet of the first call sent again -- write what one call over [0, n) writes."""
    name = "stereo_256_2048"
    st = VC.stream(name)
    n, k = len(st.packets), 31
    _, _, whole, dw, _ = run_batch(ctx, variant, [st])
    res, _, parts, dp, _ = run_batch(ctx, variant, [st, st], ranges=[(0, k), (k - 1, n - k + 1)])
    total = VC.expected(name)[2].shape[1]
    a, b = int(res["samples"][0]), int(res["samples"][1])
    assert a + b == total
    frame = 2 * 2                                                    # two channels of 16 bits
    one = whole[int(dw[0]["dst_offset"]):][:total * frame]
    two = np.concatenate([parts[int(dp[0]["dst_offset"]):][:a * frame], parts[int(dp[1]["dst_offset"]):][:b * frame]])
    assert np.array_equal(one, two)


def test_a_second_run_allocates_nothing_and_writes_the_same(ctx):
    st = VC.stream("mono_64_128")
    blob, descs, packets, src, dst_bytes, _ = VF.batch_tables(capi, [st])
    b = ctx.vorbis_batch(descs, packets, blob, src.size, dst_bytes)
    d_src, d_dst = ctx.upload(src), ctx.malloc(dst_bytes)
    ctx.vorbis_run(b, d_src, d_dst)
    first = ctx.download(d_dst, dst_bytes)
    before = ctx.device_allocations()
    ctx.memset(d_dst, FILL, dst_bytes)
    ctx.vorbis_run(b, d_src, d_dst)
    ctx.vorbis_results(b, 1, packets.size)
    assert ctx.device_allocations() == before
    written = VC.expected("mono_64_128")[2].shape[1] * 2
    second = ctx.download(d_dst, dst_bytes)
    assert np.array_equal(second[:written], first[:written]) and (second[written:] == FILL).all()
    assert all(ms >= 0 for ms in ctx.vorbis_phase_ms(b))
    ctx.batch_destroy(b)
    ctx.free(d_src)
    ctx.free(d_dst)


def test_host_buffers_equal_the_device_arenas(ctx):
    names = ["mono_64_128", "eight_64_256"]
    streams = [VC.stream(n) for n in names]
    res, pres, got, descs, _ = run_batch(ctx, 0, streams)
    blob, descs2, packets, src, dst_bytes, _ = VF.batch_tables(capi, streams)
    dst = np.full(dst_bytes, 0x5A, dtype=np.uint8)
    hres, hpres = ctx.vorbis_process_host(descs2, packets, blob, src, dst)
    assert hres.tobytes() == res.tobytes() and hpres.tobytes() == pres.tobytes()
    for i, name in enumerate(names):
        ch, samples = streams[i].model.channels, int(res["samples"][i])
        at = int(descs[i]["dst_offset"])
        assert samples == VC.expected(name)[2].shape[1]
        assert np.array_equal(dst[at:at + samples * ch * 2], got[at:at + samples * ch * 2])
        end = int(descs[i + 1]["dst_offset"]) if i + 1 < len(names) else dst_bytes
        assert (dst[at + samples * ch * 2:end] == 0x5A).all()                # only what was written came back


@pytest.mark.parametrize("variant", ROUTES)
def test_more_streams_than_a_wave(ctx, variant):
    """70 streams -- the scan is a lane a stream, 64 to a workgroup -- of ranges that begin at different packets of one stream."""
    name = "mono_64_128"
    st = VC.stream(name)
    ranges = [(i % 50, 8 + i % 7) for i in range(70)]
    res, pres, got, descs, _ = run_batch(ctx, variant, [st] * 70, ranges=ranges)
    for i, (first, count) in enumerate(ranges):
        recs, _, pcm = TB.decode_stream(st.model, st.packets[first:first + count])
        check_records(pres[int(descs[i]["first_packet"]):][:count], recs)
        mine, _ = stream_pcm(got, descs[i], 1, pcm.shape[1])
        assert int(res["samples"][i]) == pcm.shape[1] and int(np.abs(mine - pcm).max()) <= 1, i
