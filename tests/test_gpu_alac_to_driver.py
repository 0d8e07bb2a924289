"""Packets to driver bytes with no host pass over the audio: Apple Lossless streams decoded ON THE DEVICE into TInt32 planes
(ohgpu_alac_batch_run), and the planar resampler batch (OHGPU_FLAG_SRC_PLANAR32) run on those planes where they lie -- 44.1 -> 48 kHz,
ramped, S24 big-endian.  Expected: the oracle's pack-then-resample on the PCM the fixture's packets were encoded from, bit for bit;
and the resampler batch is the workgroup matrix kernel's."""
import numpy as np
import pytest

import alac_cases as AC
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


@pytest.mark.parametrize("name", ["stereo24_fl1024", "stereo16_fl4096"])
def test_alac_packets_to_resampled_ramped_s24(ctx, name):
    fx = AC.load_fixture(name)
    cfg, meta = fx["cfg"], fx["meta"]
    ch, bits, n_in, fl, n_streams = meta["channels"], meta["bits"], meta["frames"], meta["frame_length"], 16
    assert meta["rate"] == 44100
    pcm = np.array(fx["samples"], dtype=np.int32)                                         # [frame][channel]: what was encoded
    packed_ref = np.tile(FW.pack_be(pcm, bits), n_streams)
    # the decoder's batch: every stream its own copy of the packets, at ragged offsets; planes [stream][channel][packets x frame length]
    n_packets = len(fx["packets"])
    plane = n_packets * fl * 4
    ad = np.zeros(n_streams, dtype=capi.ALAC_STREAM_DESC)
    ap = np.zeros(n_streams * n_packets, dtype=capi.ALAC_PACKET)
    src = bytearray()
    for s in range(n_streams):
        for k in ("frame_length", "bit_depth", "pb", "mb", "kb", "channels", "max_run", "sample_rate"):
            ad[s][k] = cfg[k]
        ad[s]["first_packet"], ad[s]["n_packets"], ad[s]["dst_offset"], ad[s]["dst_plane_stride"] = s * n_packets, n_packets, s * ch * plane, plane
        for k, packet in enumerate(fx["packets"]):
            src += bytes(s % 5)
            ap[s * n_packets + k]["src_offset"], ap[s * n_packets + k]["bytes"] = len(src), len(packet)
            src += packet
    src = np.frombuffer(bytes(src), dtype=np.uint8)
    planes_bytes = n_streams * ch * plane
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
    per_packed, per_planes = n_in * ch * (bits // 8), ch * plane
    fused["src_offset"] = (descs["src_offset"] // per_packed) * per_planes
    fused["src_plane_stride"] = plane
    fused["flags"] |= capi.FLAG_SRC_PLANAR32
    d_bytes, d_planes, d_out = ctx.upload(src), ctx.malloc(planes_bytes), ctx.malloc(dbytes)
    ab = ctx.alac_batch(ad, ap, src.size, planes_bytes)
    sb = ctx.src_batch(h, fused, planes_bytes, dbytes)
    try:
        assert ctx.batch_paths(ab)["alac_route"] == capi.ALAC_ROUTE_FUSED
        assert ctx.src_kernel_name(sb) == "src_mfma_wg_kernel"
        ctx.alac_run(ab, d_bytes, d_planes)
        ctx.src_run(sb, d_planes, d_out)                                   # (the same stream: it queues behind the decoder)
        got = ctx.download(d_out, dbytes)
        sres, pres = ctx.alac_results(ab, n_streams, n_streams * n_packets)
    finally:
        ctx.batch_destroy(sb); ctx.batch_destroy(ab); ctx.src_destroy(h)
        ctx.free(d_bytes); ctx.free(d_planes); ctx.free(d_out)
    assert (pres["status"] == capi.ALAC_OK).all() and (sres["samples"] == n_in).all() and (sres["packets_ok"] == n_packets).all()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (int(bad.size), int(bad[0]))
