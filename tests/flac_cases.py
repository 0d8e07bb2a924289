"""What the FLAC decoder's tests share: the fixtures (encoder-made under golden/flac, handmade under golden/flac_decode), a Case =
one stream descriptor over a byte buffer, the model's answer for a case (tests/flac_textbook.py: results and the whole destination
arena), the named malformed cases and the fixed-seed mutations that also run on the device -- each of which
tests/test_flac_core_cpu.py first takes through the sanitised CPU build -- and the layout of cases into the device's two arenas.
TEST INFRASTRUCTURE ONLY."""
import collections
import functools
import hashlib
import json
import os
import random

import numpy as np

import flac_textbook as T
from ohpipeline_amd import capi

HERE = os.path.dirname(os.path.abspath(__file__))
OLD_DIR = os.path.join(HERE, "golden", "flac")
NEW_DIR = os.path.join(HERE, "golden", "flac_decode")

AT_FRAME, PACKED_BE = 1, 2

Fixture = collections.namedtuple("Fixture", "name data info audio blocksize first_sample samples")
Case = collections.namedtuple("Case", "label data offset src_bytes channels bits rate blocksize max_blocksize max_samples first_sample flags")


@functools.lru_cache(maxsize=None)
def fixtures():
    out = []
    for name, item in sorted(json.load(open(os.path.join(OLD_DIR, "index.json"))).items()):
        data = open(os.path.join(OLD_DIR, name + ".flac"), "rb").read()
        info, audio = T.streaminfo(data)
        out.append(Fixture(name, data, info, audio, item["blocksize"], 0, info["total_samples"]))
    for name, item in sorted(json.load(open(os.path.join(NEW_DIR, "index.json"))).items()):
        data = open(os.path.join(NEW_DIR, name + ".flac"), "rb").read()
        info, audio = T.streaminfo(data)
        out.append(Fixture(name, data, info, audio, item["blocksize"], item["first_sample"], item["samples"]))
    return tuple(out)


def fixture(name):
    return next(f for f in fixtures() if f.name == name)


def fixture_names():
    return [f.name for f in fixtures()]


def whole(fx, packed=False, label=None):
    """The fixture's audio bytes as one case, the first frame at the range's start."""
    return Case(label or fx.name, fx.data, fx.audio, len(fx.data) - fx.audio, fx.info["channels"], fx.info["bits"], fx.info["sample_rate"],
                fx.blocksize, fx.info["max_blocksize"], fx.samples, fx.first_sample, AT_FRAME | (PACKED_BE if packed else 0))


def arena_bytes(case):
    if case.flags & PACKED_BE:
        return case.max_samples * case.channels * (case.bits // 8)
    return case.max_samples * 4 * case.channels


def pattern(n, seed=0):
    """What a destination arena holds before a run: any byte still there afterwards was not written."""
    return ((np.arange(n, dtype=np.uint64) * 37 + 11 + seed) & 0xff).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _decode(data, offset, src_bytes, channels, bits, rate, blocksize, max_blocksize, max_samples, first_sample, at_frame):
    return T.decode_range(data, offset, src_bytes, channels=channels, bits=bits, sample_rate=rate, max_blocksize=max_blocksize,
                          max_samples=max_samples, blocksize=blocksize, first_sample=first_sample, at_frame=at_frame)


@functools.lru_cache(maxsize=None)
def model(case):
    """(Result, arena): the arena a run leaves when it starts as pattern(arena_bytes(case)), the stream's output at offset 0, its
    planes max_samples * 4 bytes apart."""
    res = _decode(case.data, case.offset, case.src_bytes, case.channels, case.bits, case.rate, case.blocksize, case.max_blocksize,
                  case.max_samples, case.first_sample, bool(case.flags & AT_FRAME))
    arena = bytearray(pattern(arena_bytes(case)).tobytes())
    T.render(res, arena, dst_offset=0, channels=case.channels, bits=case.bits, packed=bool(case.flags & PACKED_BE),
             dst_plane_stride=case.max_samples * 4)
    return res, np.frombuffer(bytes(arena), dtype=np.uint8)


def result_tuple(res):
    return (res.status, len(res.frames), res.samples, res.first_sample_decoded, res.bytes_consumed, res.candidates, res.candidates_rejected)


@functools.lru_cache(maxsize=None)
def frame_spans(name):
    """[(start, end)] of the fixture's frames, as offsets into its file."""
    fx = fixture(name)
    res, _ = model(whole(fx))
    return [(fx.audio + f.pos, fx.audio + f.end) for f in res.frames]


def device_cases():
    """The malformed and awkward inputs that also run on the device (label -> Case)."""
    out = []
    fc = fixture("false_candidate_s16_stereo_44k1_b576")
    out.append(whole(fc, label="false_candidate"))
    # starting at a byte inside frame 2 of the tiny stream's six (frames count from 0): frames from 3 on
    tiny = fixture("tiny_s16_stereo_44k1_b16")
    spans = frame_spans(tiny.name)
    inside = spans[2][0] + 5
    out.append(Case("mid_stream", tiny.data, inside, len(tiny.data) - inside, 2, 16, 44100, 16, 16, 16 * 3, 16 * 3, 0))
    # the same for the false-candidate stream, whose planted header lies inside frame 1: the scan meets it first
    spans_fc = frame_spans(fc.name)
    inside = spans_fc[1][0] + 3
    out.append(Case("mid_stream_false_candidate", fc.data, inside, len(fc.data) - inside, 2, 16, 44100, 576, 576, 576, 576 * 2, PACKED_BE))
    # cut inside the last frame
    end = spans[5][0] + 9
    out.append(Case("cut_in_last_frame", tiny.data[:end], tiny.audio, end - tiny.audio, 2, 16, 44100, 16, 16, 96, 0, AT_FRAME))
    s16 = fixture("s16_stereo_44k1_b1152_l5")
    sp = frame_spans(s16.name)
    end = sp[-1][0] + 100
    out.append(Case("cut_in_last_frame_s16", s16.data[:end], s16.audio, end - s16.audio, 2, 16, 44100, 1152, 1152, s16.samples, 0, AT_FRAME | PACKED_BE))
    # one flipped bit in frame 3 of 6
    bad = bytearray(tiny.data)
    bad[spans[3][0] + 12] ^= 0x10
    out.append(Case("flipped_bit", bytes(bad), tiny.audio, len(bad) - tiny.audio, 2, 16, 44100, 16, 16, 96, 0, AT_FRAME))
    # max_samples too small for the stream's fourth frame
    out.append(Case("overflow", tiny.data, tiny.audio, len(tiny.data) - tiny.audio, 2, 16, 44100, 16, 16, 50, 0, AT_FRAME))
    out.append(Case("overflow_packed", tiny.data, tiny.audio, len(tiny.data) - tiny.audio, 2, 16, 44100, 16, 16, 47, 0, AT_FRAME | PACKED_BE))
    return out


def mixed_cases():
    """64 descriptors over every fixture: whole streams and streams entered at a later frame (another first_sample), planes and packed."""
    big = {"s16_stereo_44k1_b1152_l5", "s24_6ch_48k_b4608_l3", "s24_stereo_44k1_b4096_l8", "s24_stereo_44k1_b576_l0"}
    out, k = [], 0
    while len(out) < 64:
        for fx in fixtures():
            packed = bool((k + len(out)) % 2)
            if fx.name in big or fx.first_sample or k % 3 == 0:       # (a stream that does not start at sample 0: whole, at its own first_sample)
                out.append(whole(fx, packed))
            else:
                # from frame j on: another first_sample, the range starting at that frame
                spans = frame_spans(fx.name)
                j = 1 + k % (len(spans) - 1)
                res = model(whole(fx))[0]
                s0 = sum(f.header.blocksize for f in res.frames[:j])
                out.append(Case("%s@%d" % (fx.name, j), fx.data, spans[j][0], len(fx.data) - spans[j][0], fx.info["channels"], fx.info["bits"],
                                   fx.info["sample_rate"], fx.blocksize, fx.info["max_blocksize"], fx.samples - s0 + 3 * (k % 2), s0,
                                   AT_FRAME * (k % 2) | (PACKED_BE if packed else 0)))
            if len(out) == 64:
                break
        k += 1
    return out


def mutations(seed=20240611):
    """A fixed-seed set of malformed streams made from short fixtures: single and double bit flips, a cut at every byte, splices of
    frames and of arbitrary slices.  Cases over small buffers, so that the model answers each in milliseconds."""
    rnd = random.Random(seed)
    tiny = fixture("tiny_s16_stereo_44k1_b16")
    forms = fixture("forms_s16_mono_11k_b16")
    out = []

    def case(label, fx, audio_bytes, **over):
        base = dict(offset=0, src_bytes=len(audio_bytes), channels=fx.info["channels"], bits=fx.info["bits"], rate=fx.info["sample_rate"],
                    blocksize=fx.blocksize, max_blocksize=fx.info["max_blocksize"], max_samples=fx.samples, first_sample=0,
                    flags=rnd.choice((0, AT_FRAME, PACKED_BE, AT_FRAME | PACKED_BE)))
        base.update(over)
        out.append(Case(label, bytes(audio_bytes), **base))

    for fx, flips in ((tiny, 900), (forms, 500)):
        audio = fx.data[fx.audio:]
        for k in range(flips):
            b = bytearray(audio)
            for _ in range(1 if k % 3 else 2):
                at = rnd.randrange(len(b) * 8)
                b[at >> 3] ^= 0x80 >> (at & 7)
            case("flip:%s:%d" % (fx.name, k), fx, b)
    audio = tiny.data[tiny.audio:]
    for end in range(len(audio) + 1):
        case("cut:%d" % end, tiny, audio[:end], flags=AT_FRAME if end % 2 else 0)
    spans = [(a - tiny.audio, b - tiny.audio) for a, b in frame_spans(tiny.name)]
    for k in range(450):
        kind = k % 3
        if kind == 0:                      # frames dropped, repeated or reordered
            pick = [rnd.randrange(6) for _ in range(rnd.randint(1, 7))]
            b = b"".join(audio[spans[i][0]:spans[i][1]] for i in pick)
        elif kind == 1:                    # a slice removed
            lo = rnd.randrange(len(audio))
            b = audio[:lo] + audio[lo + rnd.randint(1, 40):]
        else:                              # junk or a slice of the stream inserted
            lo = rnd.randrange(len(audio))
            ins = bytes(rnd.randrange(256) for _ in range(rnd.randint(1, 12))) if k % 2 else audio[rnd.randrange(len(audio)):][:rnd.randint(1, 30)]
            b = audio[:lo] + ins + audio[lo:]
        case("splice:%d" % k, tiny, b, max_samples=rnd.choice((96, 96, 200, 40)), first_sample=rnd.choice((0, 0, 16)))
    return out


@functools.lru_cache(maxsize=None)
def device_mutations():
    """The damaged streams that also run on the device: all of mutations().  tests/test_flac_core_cpu.py takes every one of them
    through the sanitised CPU build of the core first."""
    return tuple(mutations())


@functools.lru_cache(maxsize=None)
def damage_layout():
    """One Layout of device_mutations(), built once: every damaged stream in one source arena, one descriptor each."""
    return Layout(list(device_mutations()), seed=13)


def first_list(src_bytes):
    """The entries of the scan's first candidate list: csrc/flac_frame_kernel.hip's flac_run asks for S / 512 + 256, and its
    allocator hands out half as much again plus 32 (tests/many_trips_cases.flac_first_list restates the same sizing)."""
    return 1.5 * (src_bytes / 512 + 256) + 32


# ---------------------------------------------------------------- on the device
class Layout:
    """Cases laid into one source arena (ragged offsets, junk between the ranges) and one destination arena (each case's share
    starts as pattern from its own index 0, so that the expected arena is the model's arenas side by side)."""

    def __init__(self, cases, seed=1):
        rng = np.random.default_rng(seed)
        src, dst0, want = bytearray(), [], []
        self.descs = np.zeros(len(cases), dtype=capi.FLAC_STREAM_DESC)
        self.cases = cases
        at = 0
        for i, c in enumerate(cases):
            junk = bytes(rng.integers(0, 256, (i * 7 + 1) % 13, dtype=np.uint8)) + (b"\xff\xf8" if i % 3 == 0 else b"")
            src += junk
            d = self.descs[i]
            d["src_offset"], d["src_bytes"] = len(src), c.src_bytes
            src += c.data[c.offset:c.offset + c.src_bytes]
            d["dst_offset"] = at
            d["dst_plane_stride"] = 0 if c.flags & PACKED_BE else c.max_samples * 4
            d["first_sample"], d["max_samples"], d["sample_rate"] = c.first_sample, c.max_samples, c.rate
            d["blocksize"], d["max_blocksize"], d["channels"], d["bits"], d["flags"] = c.blocksize, c.max_blocksize, c.channels, c.bits, c.flags
            n = arena_bytes(c)
            pad = -n % 4 + 4 * (i % 2)
            dst0 += [pattern(n), np.full(pad, 0xEE, dtype=np.uint8)]
            want += [model(c)[1], np.full(pad, 0xEE, dtype=np.uint8)]
            at += n + pad
        src += b"\xff"
        self.src = np.frombuffer(bytes(src), dtype=np.uint8)
        self.dst0 = np.concatenate(dst0) if dst0 else np.zeros(0, dtype=np.uint8)
        self.want = np.concatenate(want) if want else np.zeros(0, dtype=np.uint8)

    def run(self, ctx, times=1):
        d_src, d_dst = ctx.upload(self.src), ctx.upload(self.dst0)
        b = ctx.flac_batch(self.descs, self.src.size, self.dst0.size)
        allocs = []
        for _ in range(times):
            ctx.flac_run(b, d_src, d_dst)
            res = ctx.flac_results(b, len(self.cases))
            allocs.append(ctx.device_allocations())
        got = ctx.download(d_dst, self.dst0.size)
        ctx.batch_destroy(b)
        ctx.free(d_src)
        ctx.free(d_dst)
        self.allocs = allocs
        return res, got

    def check(self, ctx, times=1):
        res, got = self.run(ctx, times)
        for i, c in enumerate(self.cases):
            r = res[i]
            mine = (int(r["status"]), int(r["frames"]), int(r["samples"]), int(r["first_sample_decoded"]), int(r["bytes_consumed"]),
                    int(r["candidates"]), int(r["candidates_rejected"]))
            assert mine == result_tuple(model(c)[0]), (c.label, mine, result_tuple(model(c)[0]))
        bad = np.flatnonzero(got != self.want)
        assert bad.size == 0, f"{bad.size} bytes differ, the first at {bad[0]}"
        return res, got


def device_md5(arena, case):
    """The MD5 STREAMINFO carries, of what the device wrote for a whole stream."""
    nb = case.bits // 8
    if case.flags & PACKED_BE:
        le = arena.reshape(-1, nb)[:, ::-1]
    else:
        planes = arena.view("<i4").reshape(case.channels, case.max_samples)
        le = np.ascontiguousarray(planes.T).view(np.uint8).reshape(-1, 4)[:, :nb]
    return hashlib.md5(np.ascontiguousarray(le).tobytes()).digest()
