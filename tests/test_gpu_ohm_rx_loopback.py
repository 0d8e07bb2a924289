"""Songcast sent and received on the device: ohgpu_ohm_batch_run (the sender) writes datagrams for stereo S16, stereo S24, mono S24
and a six-channel S24 source (two channels on the wire); the datagram table is derived from ohgpu_ohm_frame_layout; a seeded
window-bounded shuffle reorders every stream's datagrams; ohgpu_ohm_rx_batch_run reads them where the sender left them.  The
receiver's output arena must be tests/ohm_textbook.sender_audio of what the sender was given, under any such reordering, and the parsed
frame numbers, sample starts and formats must be the sender's.  Nothing of the datagrams passes through the host."""
import ctypes as C

import numpy as np
import pytest

import ohm_rx_cases as RC
import ohm_textbook as OT
from ohpipeline_amd import capi

pytestmark = pytest.mark.gpu

FILL = 0xA5
# (rate, bits, channels, codec): frames of 5 ms -- 220 / 240 samples -- and a short last one
SOURCES = [(44100, 16, 2, b"PCM"), (48000, 24, 2, b"FLAC"), (48000, 24, 1, b""), (44100, 24, 6, b"ALAC!")]
FRAMES = 37


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def frame_layout(stream_row, samples):
    header, total = C.c_uint32(0), C.c_uint32(0)
    capi.check(capi.lib().ohgpu_ohm_frame_layout(stream_row.ctypes.data_as(C.c_void_p), samples, C.byref(header), C.byref(total)))
    return int(header.value), int(total.value)


@pytest.mark.parametrize("seed,first_frame", [(1, 0), (2, 0xfffffff0)])
def test_what_the_sender_wrote_comes_back_as_the_audio_that_went_in(ctx, seed, first_frame):
    rng = np.random.default_rng(9000 + seed)
    lcg = RC.Lcg(seed)
    streams = np.zeros(len(SOURCES), dtype=capi.OHM_STREAM)
    frames = np.zeros(len(SOURCES) * FRAMES, dtype=capi.OHM_FRAME_DESC)
    fragments = np.zeros(frames.size, dtype=capi.OHM_FRAGMENT)
    pcm, sizes, streams_audio, sp, tp = [], [], [], 0, 0
    for i, (rate, bits, ch, codec) in enumerate(SOURCES):
        s = streams[i]
        s["samples_total"], s["sample_rate"], s["bit_rate"] = 10 ** 7 + i, rate, rate * bits * ch
        s["src_channels"], s["src_bits"], s["codec_bytes"], s["src_endian"] = ch, bits, len(codec), capi.ENDIAN_BIG
        s["codec"][:len(codec)] = np.frombuffer(codec, dtype=np.uint8)
        per_frame, start, mine = rate * 5 // 1000, 1000 * i, []
        for k in range(FRAMES):
            n = per_frame if k < FRAMES - 1 else 7 + i
            q = i * FRAMES + k
            audio = rng.integers(0, 256, n * ch * bits // 8, dtype=np.uint8)
            sp += int(rng.integers(0, 5))
            fragments[q]["src_offset"], fragments[q]["n_frames"], fragments[q]["attenuation"] = sp, n, capi.UNITY_ATTENUATION
            fragments[q]["ramp_start"] = fragments[q]["ramp_end"] = capi.RAMP_MAX
            pcm.append((sp, audio))
            sp += audio.size
            mine.append(audio)
            f = frames[q]
            tp = (tp + 3) // 4 * 4                                            # the receiver takes datagrams at multiples of 4
            f["dst_offset"], f["sample_start"], f["stream"], f["frame"] = tp, start, i, (first_frame + k) & 0xffffffff
            f["network_timestamp"], f["media_latency"], f["first_fragment"], f["n_fragments"], f["flags"] = q, 4410 + i, q, 1, capi.OHM_FLAG_LOSSLESS
            header, total = frame_layout(streams[i:i + 1], n)
            assert header == 58 + len(codec) and total == header + n * min(ch, 2) * min(bits, 24) // 8
            sizes.append((tp, total))
            tp += total
            start += n
        s_audio = OT.sender_audio(b"".join(a.tobytes() for a in mine), ch, bits)
        streams_audio.append(s_audio)
    src = np.zeros(sp, dtype=np.uint8)
    for off, a in pcm:
        src[off:off + a.size] = a
    wire_bytes = tp                                                          # the datagram arena, to the byte
    # the receiver's tables: every stream's datagrams in a shuffled arrival order, its first frame in place
    rx_streams = np.zeros(len(SOURCES), dtype=capi.OHM_RX_STREAM)
    rx_grams = np.zeros(frames.size, dtype=capi.OHM_RX_DATAGRAM)
    at, order_of = 16 + 5, []
    for i in range(len(SOURCES)):
        order = RC.window_shuffle(list(range(FRAMES)), lcg, reach=(2, 9, 30, 199)[i])
        order_of.append(order)
        for k, j in enumerate(order):
            rx_grams[i * FRAMES + k]["src_offset"], rx_grams[i * FRAMES + k]["bytes"] = sizes[i * FRAMES + j]
        r = rx_streams[i]
        r["first_datagram"], r["n_datagrams"], r["dst_offset"] = i * FRAMES, FRAMES, at
        r["dst_capacity"] = sum(sizes[i * FRAMES + j][1] - 58 for j in range(FRAMES))
        r["last_sample_start"], r["stream_msg_due"] = 0xffffffff, 1
        at += int(r["dst_capacity"]) + 16 + i
    out_bytes = at
    capi.ohm_rx_batch_check(rx_streams, rx_grams, wire_bytes, out_bytes)
    want = np.full(out_bytes, FILL, dtype=np.uint8)
    for i, audio in enumerate(streams_audio):
        o = int(rx_streams[i]["dst_offset"])
        want[o:o + len(audio)] = np.frombuffer(audio, dtype=np.uint8)

    d_src, d_wire, d_out = ctx.upload(src), ctx.malloc(wire_bytes), ctx.malloc(out_bytes)
    tx = rx = None
    try:
        ctx.memset(d_wire, FILL, wire_bytes)
        ctx.memset(d_out, FILL, out_bytes)
        tx = ctx.ohm_batch(streams, frames, fragments, src.size, wire_bytes)
        rx = ctx.ohm_rx_batch(rx_streams, rx_grams, wire_bytes, out_bytes)
        ctx.ohm_run(tx, d_src, d_wire)
        ctx.ohm_rx_run(rx, d_wire, d_out)                                    # (the same stream: it queues behind the sender)
        sres, recs = ctx.ohm_rx_results(rx, len(SOURCES), frames.size)
        got = ctx.download(d_out, out_bytes)
    finally:
        for b in (tx, rx):
            if b is not None:
                ctx.batch_destroy(b)
        for p in (d_src, d_wire, d_out):
            ctx.free(p)
    assert all(int(r["status"]) == capi.OHM_RX_OK and int(r["disposition"]) == capi.OHM_RX_OUTPUT for r in recs)
    for i, (rate, bits, ch, codec) in enumerate(SOURCES):
        for k, j in enumerate(order_of[i]):
            r, f = recs[i * FRAMES + k], frames[i * FRAMES + j]
            assert (int(r["frame"]), int(r["sample_start"]), int(r["order"])) == (int(f["frame"]), int(f["sample_start"]), j)
            assert (int(r["sample_rate"]), int(r["bit_depth"]), int(r["channels"]), int(r["media_latency"])) == (rate, min(bits, 24), min(ch, 2), 4410 + i)
            assert bytes(r["codec"][:int(r["codec_bytes"])]) == codec and int(r["samples_total"]) == 10 ** 7 + i
            assert int(r["events"]) == (3 if j == 0 else 0)
        assert int(sres[i]["n_output"]) == FRAMES and int(sres[i]["n_pending"]) == 0 and int(sres[i]["out_bytes"]) == len(streams_audio[i])
        assert int(sres[i]["frame"]) == (first_frame + FRAMES - 1) & 0xffffffff
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, "%d bytes differ, the first at %d" % (bad.size, bad[0])
