"""tests/ohm_textbook.py (one Songcast audio datagram by struct.pack, the sender's channel selection and 24-bit cap, the 5 ms
packetiser's cut points) held to test_oracle_songcast.py's hand-assembled datagram and to the oracle, for every (rate, bits,
channels) the GPU tests use plus 7350 Hz and 384 kHz, timestamped or not, with and without a halt.

Readings of the reference recorded here:
  * OhmMsg.cpp:203-223 (ReinitialiseFields): a timestamping sender sets kFlagTimestamped2 as well, and iMediaTimestamp is always 0.
  * OhmMsg.cpp:368-372, Ohm.cpp:16-20: the header's length field counts the 8 bytes of the OhmHeader itself.
  * Sender.cpp:351-377: mono sends ONE channel (the second copy of the reference's loop is overwritten by the next frame and, at the
    end, lies beyond the bytes counted); ten channels and more send channels 8 and 9.
No disagreement between model and oracle was met.
"""
import ctypes as C
import itertools

import numpy as np
import pytest

import ohm_textbook as OT
import oracle_lib as O
from test_oracle_songcast import hand_built_frame

FORMATS = [(48000, 24, 2), (44100, 16, 2), (96000, 32, 2), (44100, 24, 1), (192000, 24, 2), (48000, 8, 2), (48000, 24, 6), (44100, 16, 6),
           (48000, 32, 8), (44100, 24, 4), (48000, 16, 3), (48000, 24, 10), (7350, 16, 2), (384000, 24, 2), (7350, 8, 1), (384000, 32, 10)]


def test_model_equals_the_hand_assembled_datagram():
    audio = bytes(range(1, 1 + 36))
    sh = OT.stream_header(123456789012, 48000, 2304000, -3, 24, 2, b"FLAC")
    got = OT.audio_frame(OT.FLAG_LOSSLESS | OT.FLAG_HALT, 6, 0x01020304, 0xa0b0c0d0, 0x00112233, 0x0102030405060708, sh, audio)
    want = hand_built_frame(0x03, 6, 0x01020304, 0xa0b0c0d0, 0x00112233, 0x0102030405060708, 123456789012, 48000, 2304000, -3,
                            24, 2, b"FLAC", audio)
    assert got == want and len(got) == 8 + 28 + 26 + 36
    assert got[:12] == b"Ohm \x01\x03" + bytes([0, 98]) + b"\x32\x03\x00\x06"


@pytest.mark.parametrize("rate,bits,ch", FORMATS)
def test_model_equals_oracle_frame(rate, bits, ch):
    rng = np.random.default_rng(rate + bits + ch)
    wire_ch, wire_bits = OT.wire_format(ch, bits)
    per_packet = min(rate * 5 // 1000, OT.MAX_SAMPLE_BYTES // (wire_ch * wire_bits // 8))
    for timestamped, halt, samples, codec in itertools.product((0, 1), (0, 1), (0, 1, per_packet), (b"", b"PCM", b"x" * 29)):
        flags = OT.FLAG_LOSSLESS | (OT.FLAG_TIMESTAMPED if timestamped else 0) | (OT.FLAG_HALT if halt else 0) | (OT.FLAG_RESENT if samples == 1 else 0)
        total, start = int(rng.integers(0, 2 ** 62)), int(rng.integers(0, 2 ** 62))
        frame, net, lat = (int(v) for v in rng.integers(0, 2 ** 32, 3))
        vol = int(rng.integers(-32768, 32768))
        audio = bytes(rng.integers(0, 256, samples * wire_ch * wire_bits // 8, dtype=np.uint8))
        n, sh = O.ohm_stream_header(total, rate, rate * bits * ch, vol, wire_bits, wire_ch, codec)
        mine = OT.stream_header(total, rate, rate * bits * ch, vol, wire_bits, wire_ch, codec)
        assert n == len(mine) and bytes(sh) == mine
        n, gram = O.ohm_audio_frame(flags, samples, frame, net, lat, start, sh, audio)
        want = OT.audio_frame(flags, samples, frame, net, lat, start, mine, audio)
        assert n == len(want) and bytes(gram) == want, (timestamped, halt, samples, codec)


@pytest.mark.parametrize("ch,nbytes", list(itertools.product(range(1, 11), (1, 2, 3, 4))))
def test_sender_audio_equals_oracle(ch, nbytes):
    rng = np.random.default_rng(ch * 8 + nbytes)
    for frames in (1, 2, 5, 240):
        pcm = rng.integers(0, 256, frames * ch * nbytes, dtype=np.uint8)
        packed, nb = np.zeros(pcm.size, dtype=np.uint8), C.c_uint32(0)
        assert O.lib().ohp_sender_pack(O._ptr(pcm), pcm.size, ch, nbytes, O._ptr(packed), C.byref(nb)) == 0
        assert OT.sender_audio(pcm.tobytes(), ch, nbytes * 8) == packed[:nb.value].tobytes()


@pytest.mark.parametrize("rate", [7350, 44100, 48000, 96000, 192000, 384000])
def test_packet_cut_points_equal_oracle(rate):
    rng = np.random.default_rng(rate)
    jps = O.lib().ohp_jiffies_per_sample(rate)
    for trial in range(20):
        frames = [int(v) for v in rng.integers(1, max(3, rate // (20 if trial % 2 else 120)), size=int(rng.integers(1, 30)))]
        if trial == 0:
            frames = [rate * 5 // 1000] * 3 + [1, rate // 100, 2]                # exactly one packet, several packets in one message
        msgs = []
        for f in frames:
            m = O.MsgAudio()
            assert O.lib().ohp_msg_audio_init_pcm(m, f * 2 * 2, 2, rate, 16) == 0
            msgs.append(m)
        err, frags, packs = O.sender_packetise(msgs, flush=True)
        assert err == 0
        want = [[(f.msg, f.playable.jiffies) for f in frags[p.first_fragment:p.first_fragment + p.n_fragments]] for p in packs]
        got = OT.packet_cuts([f * jps for f in frames], flush=True)
        assert [p for p in got if p] == [p for p in want if p], (trial, frames)
