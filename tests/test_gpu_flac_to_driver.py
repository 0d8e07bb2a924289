"""File bytes to driver bytes with no host pass over the audio: FLAC streams decoded ON THE DEVICE into TInt32 planes
(ohgpu_flac_batch_run), and the planar resampler batch (OHGPU_FLAG_SRC_PLANAR32) run on those planes where they lie -- 44.1 -> 48 kHz,
ramped, S24 big-endian.  Expected: the oracle's pack-then-resample on the PCM the plain-Python model (tests/flac_textbook.py) decodes,
bit for bit; and the resampler batch is the workgroup matrix kernel's."""
import numpy as np
import pytest

import flac_cases as FC
import flac_workload as FW
import oracle_lib as O
import workloads as W
from ohpipeline_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("name", ["s24_stereo_44k1_b4096_l8", "s16_stereo_44k1_b1152_l5"])
def test_flac_bytes_to_resampled_ramped_s24(ctx, name):
    fx = FC.fixture(name)
    ch, bits, n_in, n_streams = fx.info["channels"], fx.info["bits"], fx.samples, 16
    res = FC.model(FC.whole(fx))[0]
    pcm = np.concatenate([np.array(f.planes, dtype=np.int32) for f in res.frames], axis=1).T          # [frame][channel]
    packed_ref = np.tile(FW.pack_be(pcm, bits), n_streams)
    # the decoder's batch: every stream its own copy of the file's audio bytes, at ragged offsets; planes [stream][channel][frame]
    audio = fx.data[fx.audio:]
    fd = np.zeros(n_streams, dtype=capi.FLAC_STREAM_DESC)
    src = bytearray()
    for s in range(n_streams):
        src += bytes(s % 5)
        fd[s]["src_offset"], fd[s]["src_bytes"] = len(src), len(audio)
        src += audio
        fd[s]["dst_offset"], fd[s]["dst_plane_stride"] = s * ch * n_in * 4, n_in * 4
    fd["max_samples"], fd["sample_rate"], fd["blocksize"], fd["max_blocksize"] = n_in, 44100, fx.blocksize, fx.info["max_blocksize"]
    fd["channels"], fd["bits"], fd["flags"] = ch, bits, capi.FLAC_FLAG_AT_FRAME
    src = np.frombuffer(bytes(src), dtype=np.uint8)
    planes_bytes = n_streams * ch * n_in * 4
    # the resampler's batch over those planes
    L, M, coef = capi.src_design(44100, 48000, 32, 9.0, 20000.0)
    ref = O.Src(44100, 48000, 32, 9.0, 20000.0)
    h = ctx.src_create(L, M, 32, coef)
    out_total = ref.out_frames(n_in)
    n_msgs = (out_total + 239) // 240
    sched = W.ramp_schedule(n_msgs, 240 * 1176, 20 * O.JIFFIES_PER_MS, 40 * O.JIFFIES_PER_MS)
    descs, sbytes, dbytes, _, _ = W.src_stream_descs(n_streams, n_in, L, M, 240, ch, bits, O.ENDIAN_BIG, 24, O.ENDIAN_BIG, sched)
    assert sbytes == packed_ref.size
    want = np.zeros(dbytes, dtype=np.uint8)
    assert ref.process_batch(descs, packed_ref, want) == 0
    fused = descs.copy().view(capi.SRC_MSG_DESC)
    per_packed, per_planes = n_in * ch * (bits // 8), ch * n_in * 4
    fused["src_offset"] = (descs["src_offset"] // per_packed) * per_planes
    fused["src_plane_stride"] = n_in * 4
    fused["flags"] |= capi.FLAG_SRC_PLANAR32
    d_bytes, d_planes, d_out = ctx.upload(src), ctx.malloc(planes_bytes), ctx.malloc(dbytes)
    fb = ctx.flac_batch(fd, src.size, planes_bytes)
    sb = ctx.src_batch(h, fused, planes_bytes, dbytes)
    try:
        assert ctx.src_kernel_name(sb) == "src_mfma_wg_kernel"
        ctx.flac_run(fb, d_bytes, d_planes)
        ctx.src_run(sb, d_planes, d_out)                                   # (the same stream: it queues behind the decoder)
        got = ctx.download(d_out, dbytes)
        r = ctx.flac_results(fb, n_streams)
    finally:
        ctx.batch_destroy(sb); ctx.batch_destroy(fb); ctx.src_destroy(h)
        ctx.free(d_bytes); ctx.free(d_planes); ctx.free(d_out)
    assert (r["status"] == capi.FLAC_OK).all() and (r["samples"] == n_in).all() and (r["frames"] == len(res.frames)).all()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (int(bad.size), int(bad[0]))
