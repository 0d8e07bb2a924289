"""What the Apple Lossless tests share: the committed encoder-made fixtures (tests/golden/alac/), the PCM they were made from
(regenerated from a seed by integer arithmetic), the handmade packets (tests/alac_frames.py) and the malformed ones."""
import hashlib
import json
import os
import struct

import alac_frames as F
import alac_textbook as T

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "alac")

# name: (bits, channels, rate, frame_length, frames, kind, seed, fast)
FIXTURES = {
    "mono16_fl256":          (16, 1, 44100, 256, 3 * 256 + 100, "tone", 1, False),
    "stereo16_fl1024":       (16, 2, 44100, 1024, 3 * 1024 + 300, "tone", 2, False),
    "stereo24_fl1024":       (24, 2, 44100, 1024, 3 * 1024 + 77, "tone", 3, False),
    "stereo32_fl256":        (32, 2, 96000, 256, 3 * 256 + 31, "tone", 4, False),
    "stereo16_silence_fl256": (16, 2, 44100, 256, 3 * 256 + 200, "silence", 5, False),
    "stereo16_uncorr_fl1024": (16, 2, 44100, 1024, 3 * 1024 + 1, "walk", 6, False),
    "six16_fl256":           (16, 6, 48000, 256, 3 * 256 + 255, "tone", 7, False),
    "stereo16_fast_fl1024":  (16, 2, 44100, 1024, 3 * 1024 + 512, "tone", 8, True),
    "stereo16_noise_fl256":  (16, 2, 44100, 256, 3 * 256 + 9, "noise", 9, False),
    "mono24_noise_fl256":    (24, 1, 48000, 256, 3 * 256 + 128, "noise", 10, False),
    "stereo16_fl4096":       (16, 2, 44100, 4096, 3 * 4096 + 1000, "tone", 11, False),
}


class Lcg:
    def __init__(self, seed):
        self.x = (seed * 2654435761 + 12345) & 0x7fffffff

    def next(self):
        self.x = (self.x * 1103515245 + 12345) & 0x7fffffff
        return self.x >> 8                      # 23 bits

    def small(self, spread):
        return self.next() % (2 * spread + 1) - spread


def triangle(phase, amp):
    """a triangle wave of period 1024 in `phase`, peak `amp`"""
    p = phase & 1023
    q = p if p < 512 else 1024 - p              # 0 .. 512
    return (q - 256) * amp // 256


def fixture_samples(name):
    """-> frames x channels of signed numbers at the fixture's depth, by integer arithmetic only"""
    bits, channels, _, _, frames, kind, seed, _ = FIXTURES[name]
    rng = Lcg(seed)
    full = (1 << (bits - 1)) - 1
    amp = full // 3
    out = []
    walk = [0] * channels
    for i in range(frames):
        row = []
        for c in range(channels):
            if kind == "noise":
                v = (rng.next() * 517 + rng.next()) % (2 * full + 2) - full - 1
            elif kind == "walk":
                walk[c] = max(-full, min(full, walk[c] + rng.small(full // 300)))
                v = walk[c]
            else:
                base = triangle(i * (7 + 2 * (c // 2)), amp) + triangle(i * 23 + 100, amp // 5)
                v = base - (base >> 3) * (c % 2) + rng.small(1 + (full >> 13))
                if kind == "silence" and 150 <= i < 650:
                    v = 0
            row.append(v)
        out.append(row)
    return out


def pcm_bytes(samples, bits):
    """interleaved little-endian, `bits` / 8 bytes a sample: the reference decoder's own output buffer"""
    size = bits // 8
    out = bytearray()
    for row in samples:
        for v in row:
            out += (v & ((1 << bits) - 1)).to_bytes(size, "little")
    return bytes(out)


_cache = {}


def load_fixture(name):
    """-> dict(name, meta, cookie, cfg, packets, samples, pcm)"""
    if name not in _cache:
        with open(os.path.join(GOLDEN, name + ".json")) as f:
            meta = json.load(f)
        with open(os.path.join(GOLDEN, name + ".bin"), "rb") as f:
            blob = f.read()
        packets, at = [], 0
        for size in meta["packet_sizes"]:
            packets.append(blob[at:at + size])
            at += size
        assert at == len(blob)
        cookie = bytes.fromhex(meta["cookie"])
        samples = fixture_samples(name)
        _cache[name] = dict(name=name, meta=meta, cookie=cookie, cfg=T.parse_config(cookie), packets=packets, samples=samples,
                            pcm=pcm_bytes(samples, meta["bits"]))
    return _cache[name]


def fixtures():
    return [load_fixture(n) for n in FIXTURES]


def sha256(b):
    return hashlib.sha256(b).hexdigest()


# ---- handmade packets.  Every stream here: frame length 64, pb 40, mb 10, kb 14 unless said otherwise. ----
FL = 64


def _cfg(depth, fl=FL):
    return (fl, depth, 40, 10, 14)


def _res(seed, n, spread):
    rng = Lcg(seed)
    return [rng.small(spread) for _ in range(n)]


def _packet(build):
    w = F.BitWriter()
    build(w)
    return w.bytes()


def _mono(depth, ch, **kw):
    def build(w):
        F.audio(w, _cfg(depth), F.SCE, [ch], **kw)
        F.end(w)
    return _packet(build)


def _pair(depth, a, b, **kw):
    def build(w):
        F.audio(w, _cfg(depth), F.CPE, [a, b], **kw)
        F.end(w)
    return _packet(build)


HAND_MONO8 = dict(res=[3, -1, 2, 0, 0, -4, 1, 5], expect=[[3, 2, 4, 4, 4, 0, 1, 6]])
HAND_STEREO8 = dict(u=[4, 8, -3, 0, 7, -8, 1, 2], v=[2, -4, 6, 0, -1, 3, 8, -5],
                    expect=[[6, 5, 2, 0, 7, -5, 7, -1], [4, 9, -4, 0, 8, -8, -1, 4]])


def handmade():
    """-> {name: (cookie, [packets])}: streams of handmade packets, all of them decodable"""
    out = {}
    mono16, stereo16 = F.cookie(FL, 16, 1), F.cookie(FL, 16, 2)
    out["hand_mono8"] = (mono16, [_mono(16, F.channel(HAND_MONO8["res"], order=31, coef=[0] * 31), partial=8)])
    out["hand_stereo8"] = (stereo16, [_pair(16, F.channel(HAND_STEREO8["u"]), F.channel(HAND_STEREO8["v"]), partial=8, mix_bits=2, mix_res=1)])
    # predictor orders, one packet each (order 31 reads its 31 coefficients and ignores them)
    packets = []
    for k, order in enumerate((0, 1, 2, 3, 4, 5, 8, 16, 30, 31)):
        coef = [Lcg(100 + k).small(1500) for _ in range(order)]
        packets.append(_mono(16, F.channel(_res(200 + k, FL, 40), order=order, coef=coef)))
    out["orders"] = (mono16, packets)
    out["mode_nonzero"] = (stereo16, [_pair(16, F.channel(_res(300, FL, 3), order=4, coef=[160, -190, 170, -130], mode=1),
                                            F.channel(_res(301, FL, 3), order=31, coef=[0] * 31, mode=15), mix_bits=2, mix_res=0)])
    out["factors"] = (mono16, [_mono(16, F.channel(_res(310 + f, FL, 300), order=2, coef=[500, -200], factor=f)) for f in (0, 1, 3, 5, 7)])
    out["den_shifts"] = (mono16, [_mono(16, F.channel(_res(320 + d, FL, 60), order=4, coef=[3, -2, 1, 1] if d < 2 else [900, -700, 300, 100], den_shift=d))
                                  for d in (0, 1, 15)])
    out["long_escape"] = (mono16, [_mono(16, F.channel(_res(330, FL, 20) + [], order=0, escape_at=(0, 5, 63)) ),
                                   _mono(16, F.channel([30000, -30000] + _res(331, FL - 2, 5), order=0))])
    zeros = [5] + [0] * 50 + _res(332, FL - 51, 2)
    out["zero_runs"] = (mono16, [_mono(16, F.channel(zeros, order=0)), _mono(16, F.channel([0] * FL, order=0)),
                                 _mono(16, F.channel([1] + [0] * 20 + [3] * (FL - 21), order=0, run_escape_at=(1,)))])

    def fil_dse(w):
        F.fil(w, 3)
        F.dse(w, 5, False)
        F.audio(w, _cfg(16), F.SCE, [F.channel(_res(340, FL, 9), order=1, coef=[700])])
        F.fil(w, 20)
        F.dse(w, 2, True)
        F.dse(w, 260, True)
        F.audio(w, _cfg(16), F.SCE, [F.channel(_res(341, FL, 9), order=0)], instance=1)
        F.end(w)
    out["fil_dse"] = (stereo16, [_packet(fil_dse)])

    def lfe(w):
        F.audio(w, _cfg(16), F.SCE, [F.channel(_res(350, FL, 9))])
        F.audio(w, _cfg(16), F.CPE, [F.channel(_res(351, FL, 9)), F.channel(_res(352, FL, 9))], mix_bits=3, mix_res=-5)
        F.audio(w, _cfg(16), F.LFE, [F.channel(_res(353, FL, 9), order=2, coef=[100, 50])])
    out["lfe"] = (F.cookie(FL, 16, 4), [_packet(lfe)])

    def early_end(w):
        F.audio(w, _cfg(16), F.SCE, [F.channel(_res(360, FL, 9))])
        F.end(w)
    out["early_end"] = (F.cookie(FL, 16, 3), [_packet(early_end), _packet(lambda w: F.end(w))])

    def pair_beyond(w):
        F.audio(w, _cfg(16), F.CPE, [F.channel(_res(370, FL, 9)), F.channel(_res(371, FL, 9))], mix_bits=1, mix_res=1)
        F.audio(w, _cfg(16), F.CPE, [F.channel(_res(372, FL, 9)), F.channel(_res(373, FL, 9))])
    out["pair_beyond"] = (F.cookie(FL, 16, 3), [_packet(pair_beyond)])

    raw24 = [[Lcg(380).next() - (1 << 22) for _ in range(FL)], [-(1 << 23)] + [(1 << 23) - 1] * (FL - 1)]

    def escape_shift(w):
        F.audio(w, _cfg(24), F.CPE, None, raw=raw24, shifted=1)
        F.end(w)
    out["escape_with_shift"] = (F.cookie(FL, 24, 2), [_packet(escape_shift)])
    low = [[Lcg(390 + c).next() & 0xff for _ in range(FL)] for c in range(2)]
    out["shifted"] = (F.cookie(FL, 24, 2), [
        _pair(24, F.channel(_res(391, FL, 30), order=4, coef=[640, -300, 100, 5]), F.channel(_res(392, FL, 30)), shifted=1, low=low, mix_bits=2, mix_res=3),
        _pair(24, F.channel(_res(393, FL, 3)), F.channel(_res(394, FL, 3)), shifted=2, mix_bits=40, mix_res=-128,
              low=[[Lcg(395 + c).next() & 0xffff for _ in range(FL)] for c in range(2)])])
    out["shifted_mono32"] = (F.cookie(FL, 32, 1), [
        _mono(32, F.channel(_res(396, FL, 1000), order=8, coef=[300, -200, 100, -50, 25, -12, 6, -3]), shifted=2, low=[[Lcg(397).next() & 0xffff for _ in range(FL)]]),
        _mono(32, F.channel([(1 << 31) - 1, -(1 << 31)] + _res(398, FL - 2, 1 << 20), order=1, coef=[32767]))])
    # coefficients at the edge of 16 bits: the adaptation pushes them over
    out["coef_wrap"] = (mono16, [_mono(16, F.channel([7, -3] * (FL // 2), order=2, coef=[32767, -32768], den_shift=15)),
                                 _mono(16, F.channel([-7, 3] * (FL // 2), order=3, coef=[-32768, 32767, -32768], den_shift=1))])
    out["partial"] = (stereo16, [_pair(16, F.channel(_res(400, 5, 9), order=16, coef=[10] * 16), F.channel(_res(401, 5, 9), order=4, coef=[1, 2, 3, 4]), partial=5),
                                 _pair(16, F.channel([]), F.channel([]), partial=0),
                                 _pair(16, F.channel(_res(402, 1, 9), order=31, coef=[0] * 31), F.channel(_res(403, 1, 9), order=8, coef=[0] * 8), partial=1)])
    return out


def _header_only(shifted):
    """a single-channel element's header with `shifted` bytes shifted, then zeros enough for anything"""
    w = F.BitWriter()
    w.put(F.SCE, 3); w.put(0, 4); w.put(0, 12); w.put(0, 1); w.put(shifted, 2); w.put(0, 1)
    for _ in range(FL * 4):
        w.put(0, 8)
    return w.bytes()


def malformed():
    """-> {name: (cookie, packet, status)}: one bad packet each"""
    mono16, stereo16 = F.cookie(FL, 16, 1), F.cookie(FL, 16, 2)
    good = F.channel(_res(500, FL, 9), order=1, coef=[500])
    out = {}
    out["empty"] = (mono16, b"", T.CORRUPT)
    out["tag_cce"] = (mono16, bytes([2 << 5, 0, 0, 0]), T.CORRUPT)
    out["tag_pce"] = (mono16, bytes([5 << 5, 0, 0, 0]), T.CORRUPT)
    out["unused_bits"] = (mono16, _mono(16, good, unused=0x800), T.CORRUPT)
    out["three_bytes_shifted"] = (mono16, _header_only(shifted=3), T.CORRUPT)
    out["count_above_frame_length"] = (mono16, _mono(16, F.channel(_res(501, FL + 1, 9)), partial=FL + 1), T.CORRUPT)
    out["count_huge"] = (mono16, _mono(16, good, partial=0xffffffff), T.CORRUPT)

    def disagree(w):
        F.audio(w, _cfg(16), F.SCE, [F.channel(_res(502, FL, 9))])
        F.audio(w, _cfg(16), F.SCE, [F.channel(_res(503, 10, 9))], partial=10)
    out["counts_disagree"] = (stereo16, _packet(disagree), T.CORRUPT)
    whole = _mono(16, F.channel(_res(504, FL, 200), order=2, coef=[100, 100]))
    out["cut_short"] = (mono16, whole[:len(whole) // 2], T.CORRUPT)
    out["cut_in_header"] = (mono16, whole[:2], T.CORRUPT)
    # a run of zeros longer than what is left: the writer's run count, patched up by hand
    w = F.BitWriter()
    w.put(F.SCE, 3); w.put(0, 4); w.put(0, 12); w.put(1, 1); w.put(0, 2); w.put(0, 1); w.put(4, 32)
    w.put(0, 8); w.put(0, 8); w.put(0, 4); w.put(9, 4); w.put(4, 3); w.put(0, 5)
    w.put(0, 1)                             # residual 0 (k = 1 at the start): a lone zero bit; the mean stays below 128
    w.ones(9); w.put(10, 16)                # a run of 10 with 3 samples to go
    w.put(0, 64)
    out["run_beyond_count"] = (mono16, w.bytes(), T.CORRUPT)
    out["width_33"] = (F.cookie(FL, 32, 2), _pair(32, F.channel(_res(505, FL, 9)), F.channel(_res(506, FL, 9))), T.CORRUPT)
    out["width_0"] = (mono16, _header_only(shifted=2), T.CORRUPT)
    out["depth_20"] = (F.cookie(FL, 20, 1), _mono(20, good), T.UNSUPPORTED)
    return out


# ---- batches: what the C ABI (or the CPU driver) is given, and what the model says must come of it ----
_decoded = {}


def decode_cached(cfg, data):
    key = (tuple(sorted(cfg.items())), bytes(data))
    if key not in _decoded:
        st, n, chans = T.decode_packet(cfg, data)
        _decoded[key] = (st, n, chans)
    return _decoded[key]


GUARD = 64
FILL = 0xa5


class Job:
    """streams: [(cfg, packets, form)].  Lays the packets out back to back (three stray bytes between them, none behind the last) and
    every stream's destination with GUARD bytes of FILL around each plane / block; `want` is the model's arena, `want_packets` its
    (status, samples) per packet."""

    def __init__(self, streams):
        self.streams, self.table = [], []
        src = bytearray()
        at = GUARD
        for cfg, packets, form in streams:
            first = len(self.table)
            for k, p in enumerate(packets):
                if self.table:
                    src += b"\xee" * 3
                self.table.append((len(src), len(p)))
                src += p
            span = len(packets) * cfg["frame_length"]
            if form == T.PLANAR:
                stride = span * 4 + GUARD
                size = cfg["channels"] * stride
            else:
                stride = 0
                size = (span * cfg["channels"] * (cfg["bit_depth"] // 8) + 3) // 4 * 4 + GUARD
            self.streams.append(dict(cfg=cfg, packets=list(packets), form=form, first_packet=first, n_packets=len(packets), dst_offset=at, plane_stride=stride))
            at += size
        self.src = bytes(src)
        self.dst0 = bytes([FILL]) * at
        want = bytearray(self.dst0)
        self.want_packets = []
        for s in self.streams:
            self.want_packets += T.render(s["cfg"], s["packets"], s["form"], want, s["dst_offset"], s["plane_stride"], decode_packet=decode_cached)
        self.want = bytes(want)

    def want_streams(self):
        """per stream: (leading OK packets, samples in them, first bad status or 0)"""
        out, at = [], 0
        for s in self.streams:
            res = self.want_packets[at:at + s["n_packets"]]
            at += s["n_packets"]
            ok = 0
            while ok < len(res) and res[ok][0] == T.OK:
                ok += 1
            out.append((ok, sum(n for _, n in res[:ok]), res[ok][0] if ok < len(res) else 0))
        return out

    def driver_blob(self):
        """the job file of tests/cpp/alac_core_driver.cpp"""
        out = [struct.pack("<IIQQ", len(self.streams), len(self.table), len(self.src), len(self.dst0))]
        for s in self.streams:
            c = s["cfg"]
            out.append(struct.pack("<QQIIIIHBBBBBBQ", s["dst_offset"], s["plane_stride"], s["first_packet"], s["n_packets"], c["frame_length"],
                                   c["sample_rate"], c["max_run"], c["bit_depth"], c["pb"], c["mb"], c["kb"], c["channels"], s["form"], 0))
        for i, s in enumerate(self.streams):
            for k in range(s["n_packets"]):
                off, size = self.table[s["first_packet"] + k]
                out.append(struct.pack("<QIIIIQ", off, size, i, k, 0, 0))
        out += [self.src, self.dst0]
        return b"".join(out)


FORMS = (T.PLANAR, T.PACKED_LE, T.PACKED_BE)


def fixture_streams(form):
    return [(fx["cfg"], fx["packets"], form) for fx in fixtures()]


def handmade_streams(form):
    return [(T.parse_config(cookie), packets, form) for cookie, packets in handmade().values()]


def sandwiches(form):
    """each malformed packet between two good neighbours of its own stream"""
    out = []
    for cookie, packet, _ in malformed().values():
        cfg = T.parse_config(cookie)
        good = _good_packet(cfg)
        out.append((cfg, [good, packet, good], form))
    return out


def _good_packet(cfg):
    depth, nch = cfg["bit_depth"], cfg["channels"]
    def build(w):
        for c in range(nch):
            F.audio(w, (cfg["frame_length"], depth, cfg["pb"], cfg["mb"], cfg["kb"]), F.SCE, [F.channel(_res(600 + c, cfg["frame_length"], 50), order=1, coef=[400])], instance=c)
        F.end(w)
    return _packet(build)


def mutations():
    """-> [(cfg, [packet])]: fixed-seed damage -- a cut at every byte of one packet (the shortest) of every fixture, bit flips, and
    packets spliced from two"""
    rng = Lcg(4242)
    out = []
    pools = []
    for fx in fixtures():
        short = min(fx["packets"], key=len)
        pools.append((fx["cfg"], fx["packets"]))
        for cut in range(len(short)):
            out.append((fx["cfg"], [short[:cut]]))
    for cookie, packets in handmade().values():
        pools.append((T.parse_config(cookie), packets))
    small = [(cfg, p) for cfg, ps in pools for p in ps if len(p) <= 1600]
    for k in range(900):
        cfg, p = small[rng.next() % len(small)]
        b = bytearray(p)
        for _ in range(1 + rng.next() % 3):
            if b:
                bit = rng.next() % (8 * len(b)) if k % 3 else rng.next() % min(8 * len(b), 96)      # a third of them in the headers
                b[bit >> 3] ^= 0x80 >> (bit & 7)
        out.append((cfg, [bytes(b)]))
    for k in range(300):
        cfg, p = small[rng.next() % len(small)]
        _, q = small[rng.next() % len(small)]
        a, b = rng.next() % (len(p) + 1), rng.next() % (len(q) + 1)
        out.append((cfg, [p[:a] + q[b:]]))
    return out


def packet_limit(cfg):
    """the longest packet the library takes for a stream of this configuration (ohgpu_alac_batch_check)"""
    return cfg["frame_length"] * cfg["channels"] * 5 + 64


_device = {}


def device_mutations():
    """-> [(kind, cfg, packet)], kind of "cut", "flip", "splice": the part of mutations() that also runs on the device -- every 16th
    of the cuts, every bit flip, and the splices that are no longer than packet_limit() of their stream (a longer one the library
    refuses before anything runs).  The whole of mutations() stays with tests/test_alac_core_cpu.py: its model time is most of a
    minute."""
    if "picked" not in _device:
        cases = mutations()
        n_cuts = len(cases) - 900 - 300
        kinds = ["cut"] * n_cuts + ["flip"] * 900 + ["splice"] * 300
        picked = [(kind, cfg, packets[0]) for k, (kind, (cfg, packets)) in enumerate(zip(kinds, cases))
                  if (kind != "cut" or k % 16 == 0) and (kind != "splice" or len(packets[0]) <= packet_limit(cfg))]
        assert all(len(p) <= packet_limit(cfg) for _, cfg, p in picked)
        _device["picked"] = picked
    return _device["picked"]


def damage_job():
    """device_mutations() as one Job, a packet a stream, the forms in turn as tests/test_alac_core_cpu.py lays out mutations()"""
    if "job" not in _device:
        _device["job"] = Job([(cfg, [packet], FORMS[k % 3]) for k, (_, cfg, packet) in enumerate(device_mutations())])
    return _device["job"]


def damage_job_by_configuration():
    """the same packets as one stream per configuration, in the same order: damaged and good packets of one stream side by side in
    a group of rows and in one destination span"""
    if "grouped" not in _device:
        streams = {}
        for _, cfg, packet in device_mutations():
            streams.setdefault(tuple(sorted(cfg.items())), (cfg, []))[1].append(packet)
        _device["grouped"] = Job([(cfg, packets, FORMS[k % 3]) for k, (cfg, packets) in enumerate(streams.values())])
    return _device["grouped"]


def capi_tables(job):
    """a Job as ohpipeline_amd.capi's (ALAC_STREAM_DESC array, ALAC_PACKET array)"""
    import numpy as np
    from ohpipeline_amd import capi
    descs = np.zeros(len(job.streams), dtype=capi.ALAC_STREAM_DESC)
    for d, s in zip(descs, job.streams):
        for k in ("frame_length", "bit_depth", "pb", "mb", "kb", "channels", "max_run", "max_frame_bytes", "avg_bit_rate", "sample_rate"):
            d[k] = s["cfg"][k]
        d["first_packet"], d["n_packets"], d["dst_offset"], d["dst_plane_stride"], d["flags"] = s["first_packet"], s["n_packets"], s["dst_offset"], s["plane_stride"], s["form"]
    packets = np.zeros(len(job.table), dtype=capi.ALAC_PACKET)
    for p, (off, size) in zip(packets, job.table):
        p["src_offset"], p["bytes"] = off, size
    return descs, packets
