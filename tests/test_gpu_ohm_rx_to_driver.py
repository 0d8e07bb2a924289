"""From received datagrams to what a driver reads, with no host pass over the audio.

  * The gathered run goes, without leaving the device, into ohgpu_pcm_batch_run as ITS source arena: big-endian stereo S16 off the
    wire -> ramped S24 messages.  The result must be the oracle's message path (ohp_msg_process_batch) over the MODEL's gathered
    bytes (tests/ohm_rx_textbook.py).
  * Through the host element: the scripted lanes of tests/test_ohm_rx_host_cpp.py, tick by tick, through OhmReceiver::Flush ->
    CodecController -> MsgAudioPcm -> playable -> ProcessorPcmBufTest.  The report (streams, delays, the 5 ms cuts of OutputAudioPcm and
    their track offsets, halt, stops, resend requests, what stays queued) and the bytes that reach the processors must be the model's."""
import numpy as np
import pytest

import ohm_rx_cases as RC
import ohm_rx_textbook as RX
import ohm_textbook as OT
import oracle_lib as O
import test_ohm_rx_host_cpp as HOST
from ohpipeline_amd import capi

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def test_the_gathered_run_is_the_message_paths_source_arena(ctx):
    rng = RC.Lcg(95)
    frames = RC.window_shuffle(list(range(24)), rng, reach=6)
    grams = [RC.audio_gram(100 + j, rng.bytes(4 * 220)) for j in frames]
    job = RC.Job([RC.stream(grams)], dst_lead=32)
    _, res, pcm = RX.receive(RX.new_state(), grams)
    assert res["n_output"] == 24 and len(pcm) == 24 * 880
    # messages of 240 frames over the run, ramped, S16 big-endian -> S24 big-endian
    n_msgs = len(pcm) // 4 // 240
    descs = np.zeros(n_msgs, dtype=O.MSG_DESC)
    for k in range(n_msgs):
        d = descs[k]
        d["src_offset"], d["dst_offset"], d["n_frames"] = 32 + k * 960, k * 1440, 240
        d["ramp_start"], d["ramp_end"] = (O.RAMP_MAX, 0) if k % 2 else (0, O.RAMP_MAX)
        d["attenuation"] = 256
        d["channels"], d["src_bits"], d["src_endian"], d["dst_bits"], d["dst_endian"], d["flags"] = 2, 16, O.ENDIAN_BIG, 24, O.ENDIAN_BIG, O.FLAG_RAMP
    arena = np.frombuffer(job.want, dtype=np.uint8)                         # the model's gathered arena
    want = np.zeros(n_msgs * 1440, dtype=np.uint8)
    assert O.msg_process_batch(descs, arena, want) == 0
    src, dst0 = np.frombuffer(job.src, dtype=np.uint8), np.frombuffer(job.dst0, dtype=np.uint8)
    d_src, d_mid, d_out = ctx.upload(src), ctx.upload(dst0), ctx.malloc(want.size)
    rx = ctx.ohm_rx_batch(job.d_streams, job.d_grams, src.size, dst0.size)
    pcm_batch = ctx.pcm_batch(descs, dst0.size, want.size)
    try:
        ctx.ohm_rx_run(rx, d_src, d_mid)
        ctx.pcm_run(pcm_batch, d_mid, d_out)                                # (the same stream: queued behind the gather, no host in between)
        got = ctx.download(d_out, want.size)
    finally:
        ctx.batch_destroy(rx)
        ctx.batch_destroy(pcm_batch)
        for p in (d_src, d_mid, d_out):
            ctx.free(p)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%d bytes differ, the first at %d" % (bad.size, bad[0])


def test_lanes_from_datagrams_to_processor_through_the_gpu(tmp_path):
    lanes = HOST.scripted_lanes()
    want_lines, want_bytes = HOST.expected(lanes)
    got_lines = HOST.run("gpu", tmp_path, lanes)
    assert got_lines == want_lines, next(("line %d: got %r, want %r" % (k, g, w) for k, (g, w) in enumerate(zip(got_lines, want_lines)) if g != w),
                                         "lengths %d, %d" % (len(got_lines), len(want_lines)))
    got = (tmp_path / "bytes.bin").read_bytes()
    assert got == b"".join(want_bytes) and len(got) > 40 * 880
