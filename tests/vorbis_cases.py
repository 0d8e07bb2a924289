"""The Vorbis streams the CPU and the GPU tests share (tests/vorbis_frames.py writes them, tests/vorbis_textbook.py decodes them), each
made once a session: the shapes at which the decoder can go wrong -- the smallest blocks and the largest, both sizes in one stream with
all four neighbour pairs, 1 / 2 / 6 / 8 channels, coupling and submaps, 70 and more packets so that a wave of packets is crossed, and one
stream whose PCM clips."""
import functools

import numpy as np

import vorbis_frames as VF
import vorbis_textbook as TB

#        name            seed channels e0 e1 packets coupling submaps peak
SHAPES = {
    "mono_64_128":      (11, 1, 6, 7, 72, 0, 1, 0.45),
    "stereo_256_2048":  (12, 2, 8, 11, 70, 1, 1, 0.45),
    "mono_8192":        (13, 1, 11, 13, 6, 0, 1, 0.45),
    "six_128_512":      (14, 6, 7, 9, 16, 2, 2, 0.45),
    "eight_64_256":     (15, 8, 6, 8, 12, 3, 3, 0.45),
    "stereo_clips":     (16, 2, 6, 7, 20, 1, 1, 3.0),
    "encoder_256":      None,          # (not random: see ENCODER)
}
# The streams held against Tremor (tests/test_vorbis_tremor.py).  They keep to what an encoder writes where Tremor and the specification
# part: (1) the floors' end amplitudes are drawn from the lower 45 % of their range, so that the floor carries the
# level and the residue's value vectors are of the size of whole numbers -- Tremor keeps the residue in fixed point, eight bits behind the
# point; (2) a residue has as many classes as its class book's entries decompose into -- Tremor ends the residue at a class word out of
# range, the specification takes it modulo; (3) the long block is twice the short one, so that every floor's last post stands at or
# beyond the block's half -- behind the last post Tremor multiplies by the curve's level itself, not by the table's value of it; (4) a
# type 2 residue's partition size is a multiple of its submap's channel count -- Tremor begins the round of the channels anew at every
# partition, the specification deinterleaves the vector as a whole (the six-channel stream's seed is chosen for bundles of 2 and 4).
TREMOR_SHAPES = {
    "tremor_mono_64_128":      (21, 1, 6, 7, 40, 0, 1, 0.45),
    "tremor_stereo_1024_2048": (22, 2, 10, 11, 12, 1, 1, 0.45),
    "tremor_six_128_256":      (24, 6, 7, 8, 16, 2, 2, 0.45),
}


ENCODER = "encoder_256"            # the minimal encoder's stream (tests/vorbis_frames.encode of a sine sweep), a shape like the others


def sweep():
    t = np.arange(256 * 24)
    return 0.5 * np.sin(2 * np.pi * (0.01 + 0.00002 * t) * t)


@functools.lru_cache(maxsize=None)
def stream(name):
    if name == ENCODER:
        return VF.encode(sweep())
    if name in TREMOR_SHAPES:
        seed, ch, e0, e1, n, coupling, submaps, peak = TREMOR_SHAPES[name]
        return VF.random_stream(seed, ch, e0, e1, n, coupling, submaps, peak, floor_cap=0.45, one_entry=1, strict=True)
    seed, ch, e0, e1, n, coupling, submaps, peak = SHAPES[name]
    return VF.random_stream(seed, ch, e0, e1, n, coupling, submaps, peak)


@functools.lru_cache(maxsize=None)
def expected(name, max_samples=None):
    """(records, spectra, pcm) of the whole stream by the model; the arrays are shared: do not write to them."""
    st = stream(name)
    return TB.decode_stream(st.model, st.packets, max_samples)


def pcm_s16be(pcm):
    """int32 [channels][samples] -> the interleaved big-endian bytes"""
    return pcm.T.astype(">i2").tobytes()


BAD_MODE = bytes([0b110])          # an audio packet whose mode number is 3 where the streams have three modes


def damaged(name):
    """The stream's packets with every fifth cut short (at a third of its bytes) and two replaced by a bad mode and an empty packet."""
    st = stream(name)
    packets = list(st.packets)
    for k in range(2, len(packets), 5):
        packets[k] = packets[k][:max(1, len(packets[k]) // 3)]
    packets[4] = BAD_MODE
    packets[7] = b""
    packets[9] = b"\x05vorbis"
    return packets


def granules(name):
    """Per audio packet, the samples delivered up to and with it: the granule positions of the stream's Ogg pages."""
    return [r[4] + r[3] for r in expected(name)[0]]


@functools.lru_cache(maxsize=None)
def ogg(name):
    return VF.ogg_file(stream(name), granules(name))
