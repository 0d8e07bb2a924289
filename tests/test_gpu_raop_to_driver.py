"""The AirPlay path end to end with no host pass over the audio: 16 RAOP sessions, each under its own key, whose datagrams lie in the
source arena whole (12 header bytes, then the encrypted payload), are decrypted and decoded ON THE DEVICE into packed big-endian S16
(ohgpu_raop_batch_run), and the PCM message batch runs over those bytes where they lie -- attenuation 128 (row a6, which exists for
RAOP alone) and a ramp down over the stream, to S16.  Expected: the oracle's message path on the PCM the fixture's packets were
encoded from, bit for bit."""
import numpy as np
import pytest

import alac_cases as AC
import flac_workload as FW
import oracle_lib as O
import raop_cases as RC
import raop_textbook as R
import workloads as W
from ohpipeline_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def test_raop_datagrams_to_attenuated_ramped_s16(ctx):
    session = RC.session("stereo16_noise_fl256")
    fx, cfg = session["fx"], session["cfg"]
    meta = fx["meta"]
    ch, bits, n_in, fl, n_streams = meta["channels"], meta["bits"], meta["frames"], meta["frame_length"], 16
    assert (ch, bits) == (2, 16) and len({len(p) for p in fx["packets"]}) > 1
    n_packets = len(fx["packets"])
    # the sessions: the committed one, and fifteen more of the same packets under fixed-seed keys (encrypted by the model, which
    # tests/test_raop_textbook.py holds to libcrypto); every datagram at a multiple of 4, so its payload is at one too
    rng = AC.Lcg(61)
    rd = np.zeros(n_streams, dtype=capi.RAOP_STREAM_DESC)
    rp = np.zeros(n_streams * n_packets, dtype=capi.ALAC_PACKET)
    block = n_packets * fl * ch * 2                                                    # a stream's share of the decoded arena
    src = bytearray()
    for s in range(n_streams):
        key, iv = (session["key"], session["iv"]) if s == 0 else (RC.rand_bytes(rng, 16), RC.rand_bytes(rng, 16))
        for k in ("frame_length", "bit_depth", "pb", "mb", "kb", "channels", "max_run", "sample_rate"):
            rd[s][k] = cfg[k]
        rd[s]["first_packet"], rd[s]["n_packets"], rd[s]["dst_offset"], rd[s]["flags"] = s * n_packets, n_packets, s * block, capi.ALAC_OUT_PACKED_BE
        rd[s]["aes_key"], rd[s]["aes_iv"] = list(key), list(iv)
        for k, packet in enumerate(fx["packets"]):
            datagram = session["datagrams"][k] if s == 0 else R.make_datagram(100 * s + k, k * fl, s, R.encrypt_packet(key, iv, packet))
            src += bytes(-len(src) % 4)
            rp[s * n_packets + k]["src_offset"], rp[s * n_packets + k]["bytes"] = len(src) + 12, len(datagram) - 12
            src += datagram
    src = np.frombuffer(bytes(src), dtype=np.uint8)
    decoded_bytes = n_streams * block
    # the message batch over the decoded bytes: messages of 240 frames, the whole stream one ramp down, half volume
    pcm = np.array(fx["samples"], dtype=np.int32)                                         # [frame][channel]: what was encoded
    packed_ref = np.tile(FW.pack_be(pcm, bits), n_streams)
    sizes = [min(240, n_in - at) for at in range(0, n_in, 240)]
    per_frame = O.JIFFIES_PER_SEC // meta["rate"]
    sched = W.ramp_schedule(len(sizes), [n * per_frame for n in sizes], 0, n_in * per_frame)
    assert all(on for on, _, _ in sched) and sched[0][1] == O.RAMP_MAX and sched[-1][2] < sched[0][1]
    descs, sbytes, dbytes = W.pcm_stream_descs(n_streams, n_in, 240, ch, bits, O.ENDIAN_BIG, 16, O.ENDIAN_BIG, sched)
    descs["attenuation"] = 128
    assert sbytes == packed_ref.size
    want = np.full(dbytes, 0xa5, dtype=np.uint8)
    assert O.msg_process_batch(descs, packed_ref, want) == 0
    on_device = descs.copy()
    on_device["src_offset"] = (descs["src_offset"] // (n_in * ch * 2)) * block + descs["src_offset"] % (n_in * ch * 2)
    d_src, d_decoded, d_out = ctx.upload(src), ctx.malloc(decoded_bytes), ctx.malloc(dbytes)
    ctx.memset(d_out, 0xa5, dbytes)
    rb = ctx.raop_batch(rd, rp, src.size, decoded_bytes)
    pb = ctx.pcm_batch(on_device, decoded_bytes, dbytes)
    try:
        assert ctx.batch_paths(rb)["alac_route"] == capi.ALAC_ROUTE_FUSED
        ctx.raop_run(rb, d_src, d_decoded)
        ctx.pcm_run(pb, d_decoded, d_out)                                  # (the same stream: it queues behind the decoder)
        got = ctx.download(d_out, dbytes)
        sres, pres = ctx.raop_results(rb, n_streams, n_streams * n_packets)
    finally:
        ctx.batch_destroy(pb); ctx.batch_destroy(rb)
        ctx.free(d_src); ctx.free(d_decoded); ctx.free(d_out)
    assert (pres["status"] == capi.ALAC_OK).all() and (sres["samples"] == n_in).all() and (sres["packets_ok"] == n_packets).all()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (int(bad.size), int(bad[0]))
    assert not np.array_equal(want, packed_ref)                             # (the attenuation and the ramp did something)
