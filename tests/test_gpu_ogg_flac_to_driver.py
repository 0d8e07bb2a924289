"""Ogg FLAC end to end on the device (ohgpu_ogg_flac_process_host): the committed FLAC fixtures -- encoded by the reference's libFLAC,
each with the MD5 of its PCM in STREAMINFO -- wrapped in pages by the tests' own muxer (tests/ogg_cases.py), demuxed into a
device-only middle arena and decoded from there.  The PCM must have the stream's MD5 and be the bytes the native stream decodes to
(ohgpu_flac_process_host on the same frames); ticks cut anywhere -- inside a page header, a lacing table, a body -- give the same PCM
as one call; every audio packet of the table is one decoded frame; a corrupt lane among healthy ones delivers what precedes the
break while the others decode whole."""
import hashlib

import numpy as np
import pytest

import flac_cases as FC
import ogg_cases as GC
from ohpipeline_amd import capi

pytestmark = pytest.mark.gpu

ENCODED = ["s16_stereo_44k1_b1152_l5", "s24_stereo_44k1_b576_l0", "s8_mono_8k_b256_l2", "s24_stereo_44k1_b4096_l8", "s24_6ch_48k_b4608_l3"]


@pytest.fixture(scope="module")
def ctx():
    c = capi.Context(0)
    yield c
    c.close()


def frame_bytes(fx):
    return fx.info["channels"] * (fx.info["bits"] // 8)


def md5_of_packed_be(pcm, fx):
    """STREAMINFO's MD5 is over the interleaved samples, little-endian: the packed big-endian output with every sample reversed."""
    w = fx.info["bits"] // 8
    return hashlib.md5(np.frombuffer(pcm, dtype=np.uint8).reshape(-1, w)[:, ::-1].tobytes()).digest()


def native_pcm(ctx, fx):
    case = FC.whole(fx, packed=True)
    d = np.zeros(1, dtype=capi.FLAC_STREAM_DESC)
    d["src_offset"], d["src_bytes"], d["max_samples"], d["sample_rate"] = case.offset, case.src_bytes, case.max_samples, case.rate
    d["blocksize"], d["max_blocksize"], d["channels"], d["bits"], d["flags"] = case.blocksize, case.max_blocksize, case.channels, case.bits, case.flags
    dst = np.zeros(case.max_samples * frame_bytes(fx), dtype=np.uint8)
    res = ctx.flac_process_host(d, np.frombuffer(fx.data, dtype=np.uint8), dst)
    assert int(res[0]["status"]) == capi.FLAC_OK and int(res[0]["samples"]) == fx.samples
    return dst.tobytes()


class Tick:
    """Lanes of Ogg bytes -> the descriptors of one fused call."""

    def __init__(self, lanes):
        # lanes: (fixture, bytes, serial, expect_seq, first_page_segment, first_sample)
        n = len(lanes)
        self.lanes = lanes
        self.ogg, self.flac = np.zeros(n, dtype=capi.OGG_STREAM_DESC), np.zeros(n, dtype=capi.FLAC_STREAM_DESC)
        src, mid, dst, pk = bytearray(), 0, 0, 0
        self.pk_cap = []
        for i, (fx, data, serial, seq, seg, first_sample) in enumerate(lanes):
            src += bytes(i % 3)                                           # (lanes at different alignments)
            o, f = self.ogg[i], self.flac[i]
            cap = len(data) // 28 + 1
            o["src_offset"], o["src_bytes"], o["dst_offset"], o["dst_capacity"] = len(src), len(data), mid, len(data)
            o["serial"], o["expect_seq"], o["first_page_segment"], o["flags"] = serial, seq, seg, capi.OGG_FLAC_MAPPING
            o["packet_first"], o["packet_capacity"] = pk, cap
            left = fx.samples - first_sample
            f["src_offset"], f["dst_offset"], f["first_sample"], f["max_samples"] = mid, dst, first_sample, left
            f["sample_rate"], f["blocksize"], f["max_blocksize"] = fx.info["sample_rate"], fx.blocksize, fx.info["max_blocksize"]
            f["channels"], f["bits"], f["flags"] = fx.info["channels"], fx.info["bits"], capi.FLAC_FLAG_AT_FRAME | capi.FLAC_OUT_PACKED_BE
            src += data
            mid += len(data) + 5 + i
            dst += (left * frame_bytes(fx) + 3) // 4 * 4
            pk += cap
            self.pk_cap.append(cap)
        self.src, self.mid_bytes, self.n_packets = np.frombuffer(bytes(src), dtype=np.uint8), mid, pk
        self.dst = np.full(dst, 0xA5, dtype=np.uint8)

    def run(self, ctx, frames_capacity=4096):
        self.ores, self.packets, self.fres, self.frames = ctx.ogg_flac_process_host(self.ogg, self.flac, self.n_packets, self.src, self.mid_bytes, self.dst,
                                                                                    frames_capacity)
        return self

    def pcm(self, i):
        a, fx = int(self.flac[i]["dst_offset"]), self.lanes[i][0]
        return self.dst[a:a + int(self.fres[i]["samples"]) * frame_bytes(fx)].tobytes()


def audio_lane(fx, max_segments):
    data, _, _ = GC.ogg_flac(fx, max_segments=max_segments)
    info, serial, off, seg, seq = capi.ogg_flac_head(data)
    assert bytes(info["md5"]) == bytes(fx.info["md5"])
    return (fx, data[off:], serial, seq, seg, 0)


def test_every_encoded_fixture_has_its_md5_and_its_native_pcm(ctx):
    fxs = [FC.fixture(n) for n in ENCODED]
    tick = Tick([audio_lane(fx, (3, 255, 1, 17, 40)[i]) for i, fx in enumerate(fxs)]).run(ctx)
    for i, fx in enumerate(fxs):
        assert int(tick.ores[i]["status"]) == capi.OGG_OK and int(tick.ores[i]["eos_seen"]) == 1, fx.name
        assert int(tick.fres[i]["status"]) == capi.FLAC_OK and int(tick.fres[i]["samples"]) == fx.samples, fx.name
        assert int(tick.fres[i]["bytes_consumed"]) == int(tick.ores[i]["bytes_delivered"]) == len(fx.data) - fx.audio, fx.name
        pcm = tick.pcm(i)
        assert md5_of_packed_be(pcm, fx) == bytes(fx.info["md5"]), fx.name
        assert pcm == native_pcm(ctx, fx), fx.name
        # every audio packet of the table is one decoded frame
        first = int(tick.ogg[i]["packet_first"])
        mine = tick.packets[first:first + int(tick.ores[i]["packets"])]
        frames = tick.frames[tick.frames["stream"] == i]
        assert len(mine) == len(frames) == len(FC.frame_spans(fx.name)), fx.name
        assert [(int(k["run_pos"]), int(k["run_pos"]) + int(k["bytes"])) for k in mine] == [(int(f["src_pos"]), int(f["src_end"])) for f in frames], fx.name
        assert int(mine[-1]["granule"]) == fx.samples and int(tick.ores[i]["last_granule"]) == fx.samples
    assert (tick.dst[-1] == 0xA5) or tick.dst.size % 4 == 0


def test_ticks_cut_anywhere_give_the_pcm_of_one_call(ctx):
    fx = FC.fixture("s16_stereo_44k1_b1152_l5")
    lane = audio_lane(fx, 5)
    data = lane[1]
    whole = native_pcm(ctx, fx)
    # the page that starts nearest the middle: cut inside its header, inside its lacing table, inside its body, and at its start
    starts, p = [], 0
    while p < len(data):
        starts.append(p)
        n = data[p + 26]
        p += 27 + n + sum(data[p + 27:p + 27 + n])
    mid = min(starts, key=lambda s: abs(s - len(data) // 2))
    cuts = [mid, mid + 10, mid + 28, mid + 27 + data[mid + 26] + 100, 1, len(data) - 1]
    first = Tick([(fx, data[:c], lane[2], lane[3], lane[4], 0) for c in cuts]).run(ctx)
    second = []
    for i, c in enumerate(cuts):
        o, f = first.ores[i], first.fres[i]
        assert int(o["status"]) == capi.OGG_OK and int(f["status"]) == capi.FLAC_OK and int(f["bytes_consumed"]) == int(o["bytes_delivered"]), c
        second.append((fx, data[int(o["bytes_consumed"]):], int(o["serial"]), int(o["next_seq"]), int(o["resume_segment"]), int(f["samples"])))
    then = Tick(second).run(ctx)
    for i, c in enumerate(cuts):
        assert int(then.ores[i]["status"]) == capi.OGG_OK and int(then.fres[i]["status"]) == capi.FLAC_OK, c
        assert int(first.fres[i]["samples"]) + int(then.fres[i]["samples"]) == fx.samples, c
        assert first.pcm(i) + then.pcm(i) == whole, c
    assert len({int(r["samples"]) for r in first.fres}) > 2                     # (the cuts are not all the same cut)


def test_a_corrupt_lane_among_healthy_ones(ctx):
    fx, small = FC.fixture("s24_stereo_44k1_b576_l0"), FC.fixture("s8_mono_8k_b256_l2")
    good = audio_lane(fx, 9)
    bad = bytearray(good[1])
    bad[len(bad) * 2 // 3] ^= 0x40
    gap = audio_lane(small, 2)
    starts, p = [], 0
    while p < len(gap[1]):
        starts.append(p)
        n = gap[1][p + 26]
        p += 27 + n + sum(gap[1][p + 27:p + 27 + n])
    holed = gap[1][:starts[3]] + gap[1][starts[4]:]                               # the fourth page is missing
    tick = Tick([good, (fx, bytes(bad)) + good[2:], audio_lane(small, 255), (small, holed) + gap[2:]]).run(ctx)
    assert [int(r["status"]) for r in tick.ores] == [capi.OGG_OK, capi.OGG_LOST_SYNC, capi.OGG_OK, capi.OGG_HOLE]
    whole, whole_small = native_pcm(ctx, fx), native_pcm(ctx, small)
    assert tick.pcm(0) == whole and tick.pcm(2) == whole_small
    for i, ref in ((1, whole), (3, whole_small)):
        got = tick.pcm(i)
        assert 0 < len(got) < len(ref) and got == ref[:len(got)], i
        assert int(tick.fres[i]["status"]) == capi.FLAC_OK and int(tick.fres[i]["bytes_consumed"]) == int(tick.ores[i]["bytes_delivered"]), i
        assert int(tick.ores[i]["bytes_consumed"]) < len(tick.lanes[i][1])
